// femasm — vertex-graph kernels (included at the end of femasm_eval.hip: one translation unit).
//
// fa_vertex_spread  the reference's damage smoothing (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:315-475,
//                   MFEM/mechanic2d/asym_elasto_damage_model.cc:1159-1315) on one process: `iterations` times a
//                   gated and a full Jacobi pass of d(v) <- max(r(v) * sum of d over the neighbours of v, d(v))
//                   on the CSR vertex graph.
//
// One lane per vertex walks its row with plain loads: rows are short (6-7 entries on triangles, about 14 on
// tetrahedra) and the neighbours' values sit in cache. The sum starts at 0.0 and adds the row in its stored
// order, the product with the stored reciprocal is followed by a compare only (nothing an FMA could form
// from), and a pass reads one buffer and writes the other: the result is the sequential loop's, bit for
// bit, run to run. No LDS, no atomics, no cross-lane operation. An index outside [0, nverts) is skipped,
// never dereferenced. All index arithmetic is 64-bit.

template <bool GATED>
__global__ __launch_bounds__(256) void k_spread_pass(int64_t nverts, const int64_t* __restrict__ indptr,
                                                     const int32_t* __restrict__ indices,
                                                     const double* __restrict__ inv_deg, double threshold,
                                                     const double* __restrict__ in, double* __restrict__ out) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nverts; v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t k0 = indptr[v], k1 = indptr[v + 1];
    const double r = inv_deg[v], dv = in[v];
    double s = 0.0;
    if (!GATED || dv < threshold) {
      for (int64_t k = k0; k < k1; ++k) {
        const int64_t w = indices[k];
        if (w < 0 || w >= nverts) continue;
        s += in[w];
      }
    }
    const double a = s * r;
    out[v] = a > dv ? a : dv;
  }
}

extern "C" int fa_vertex_spread(int64_t nverts, const int64_t* indptr, const int32_t* indices, const double* inv_deg,
                                double* d, double* tmp, int32_t iterations, double threshold, void* stream) {
  if (nverts < 0) return fail(FA_E_ARG, "fa_vertex_spread: nverts %lld", (long long)nverts);
  if (iterations < 0) return fail(FA_E_ARG, "fa_vertex_spread: iterations %d", iterations);
  if (nverts > INT32_MAX) return fail(FA_E_CAPACITY, "fa_vertex_spread: vertex indices are int32");
  if (nverts == 0) return FA_OK;  // empty arrays have no address
  if (!indptr || !indices || !inv_deg || !d || !tmp)
    return fail(FA_E_ARG, "fa_vertex_spread: null indptr, indices, inv_deg, d or tmp");
  if (iterations == 0) return FA_OK;  // d is the result already; a launch of nothing is an error to HIP
  hipStream_t s = (hipStream_t)stream;
  const int grid = grid_for(nverts);
  for (int32_t it = 0; it < iterations; ++it) {
    k_spread_pass<true><<<grid, 256, 0, s>>>(nverts, indptr, indices, inv_deg, threshold, d, tmp);
    k_spread_pass<false><<<grid, 256, 0, s>>>(nverts, indptr, indices, inv_deg, threshold, tmp, d);
  }
  LAUNCH_CHECK();
  return FA_OK;
}
