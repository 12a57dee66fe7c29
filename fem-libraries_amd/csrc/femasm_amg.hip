// femasm — smoothed-aggregation algebraic multigrid kernels (included at the end of femasm_eval.hip: one
// translation unit).
//
// fa_bcsr_mult     y (+)= B x for a block-CSR matrix with rectangular row-major blocks [br][bc]: the
//                  prolongator P, its stored transpose (the restriction as a gather) and the coarse
//                  matrices with 6-dof nodes.
// fa_bcsr_product  the numeric phase of a block SpGEMM on an inverted product list: output block s is
//                  the sum of X[xa[q]] * Y[yb[q]] over its list range (A*T, A*P and P^T*(A P)).
// fa_cheb_step6    fa_cheb_step for 6-dof nodes.
// fa_csr_row_max   out[i] = free[i] ? max over row i of in[indices] : 0, the one graph primitive of the
//                  MIS(2) aggregation.
//
// All four gather in a fixed order and use no atomics: results are bit-identical run to run. A group of
// lanes shares an output row / block, its lanes stride the row's blocks / the block's products, and the
// partial sums meet in an xor butterfly. Every lane of the group computes the same tree (a + b == b + a
// exactly), so all of them end with the same bits. Indices outside the operand are skipped, never
// dereferenced. All index arithmetic is 64-bit.

constexpr int kBcsrMultLanes = 8;  // lanes per block row of fa_bcsr_mult

template <int N>
__device__ __forceinline__ double amg_pick(const double (&v)[N], int r) {
  double o = v[0];  // select without indexing the register array dynamically
#pragma unroll
  for (int q = 1; q < N; ++q) o = r == q ? v[q] : o;
  return o;
}

template <int BR, int BC>
__global__ __launch_bounds__(256) void k_bcsr_mult(int64_t nrows, int64_t ncols, const int64_t* __restrict__ indptr,
                                                   const int32_t* __restrict__ indices,
                                                   const double* __restrict__ data, const double* __restrict__ x,
                                                   int add, double* __restrict__ y) {
  constexpr int G = kBcsrMultLanes;
  static_assert(BR <= G, "one lane per row of the block writes");
  const int lane = threadIdx.x & (G - 1);
  const int64_t ngroups = (int64_t)gridDim.x * (blockDim.x / G);
  for (int64_t row = blockIdx.x * (int64_t)(blockDim.x / G) + threadIdx.x / G; row < nrows; row += ngroups) {
    const int64_t k1 = indptr[row + 1];
    double acc[BR];
#pragma unroll
    for (int r = 0; r < BR; ++r) acc[r] = 0.0;
    for (int64_t k = indptr[row] + lane; k < k1; k += G) {
      const int64_t col = indices[k];
      if (col < 0 || col >= ncols) continue;
      const double* __restrict__ B = data + k * (BR * BC);
      double xv[BC];
#pragma unroll
      for (int c = 0; c < BC; ++c) xv[c] = x[col * BC + c];
#pragma unroll
      for (int r = 0; r < BR; ++r)
#pragma unroll
        for (int c = 0; c < BC; ++c) acc[r] += B[r * BC + c] * xv[c];
    }
#pragma unroll
    for (int off = 1; off < G; off <<= 1)
#pragma unroll
      for (int r = 0; r < BR; ++r) acc[r] += __shfl_xor(acc[r], off, 64);
    if (lane < BR) {  // one 8-byte store per lane
      const int64_t i = row * BR + lane;
      const double v = amg_pick(acc, lane);
      y[i] = add ? y[i] + v : v;
    }
  }
}

// G lanes per output block: lane t is row i = t % R2 of the block and strides the list from p = t / R2.
template <int R, int K, int C, int G>
__global__ __launch_bounds__(256) void k_bcsr_product(int64_t nout, int64_t nprod, const int64_t* __restrict__ optr,
                                                      const int32_t* __restrict__ xa, const int32_t* __restrict__ yb,
                                                      const double* __restrict__ X, int64_t nx,
                                                      const double* __restrict__ Y, int64_t ny,
                                                      double* __restrict__ out) {
  constexpr int R2 = R <= 2 ? 2 : R <= 4 ? 4 : 8;
  constexpr int NP = G / R2;
  static_assert(G % R2 == 0 && NP >= 1, "group shape");
  const int t = threadIdx.x & (G - 1);
  const int i = t & (R2 - 1), p = t / R2;
  const int64_t ngroups = (int64_t)gridDim.x * (blockDim.x / G);
  for (int64_t s = blockIdx.x * (int64_t)(blockDim.x / G) + threadIdx.x / G; s < nout; s += ngroups) {
    int64_t q0 = optr[s], q1 = optr[s + 1];
    if (q0 < 0) q0 = 0;
    if (q1 > nprod) q1 = nprod;
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.0;
    if (i < R) {
      for (int64_t q = q0 + p; q < q1; q += NP) {
        const int64_t a = xa[q], b = yb[q];
        if (a < 0 || a >= nx || b < 0 || b >= ny) continue;
        const double* __restrict__ xr = X + (a * R + i) * K;
        const double* __restrict__ yk = Y + b * (K * C);
        double xv[K];
#pragma unroll
        for (int k = 0; k < K; ++k) xv[k] = xr[k];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] += xv[k] * yk[k * C + c];
      }
    }
#pragma unroll
    for (int off = R2; off < G; off <<= 1)
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += __shfl_xor(acc[c], off, 64);
    if (p == 0 && i < R) {
      double* __restrict__ o = out + (s * R + i) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) o[c] = acc[c];
      store_fence(acc);  // the next block of the grid-stride loop rewrites the stores' data registers
    }
  }
}

__global__ __launch_bounds__(256) void k_csr_row_max(int64_t nrows, const int64_t* __restrict__ indptr,
                                                     const int32_t* __restrict__ indices,
                                                     const int8_t* __restrict__ free_, const int64_t* __restrict__ in,
                                                     int64_t nin, int64_t* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nrows; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t m = 0;
    if (!free_ || free_[i]) {
      const int64_t k1 = indptr[i + 1];
      bool first = true;
      for (int64_t k = indptr[i]; k < k1; ++k) {
        const int64_t j = indices[k];
        if (j < 0 || j >= nin) continue;
        const int64_t v = in[j];
        m = (first || v > m) ? v : m;
        first = false;
      }
    }
    out[i] = m;
  }
}

template <int BR, int BC>
static void bcsr_mult_launch(int64_t nrows, int64_t ncols, const int64_t* indptr, const int32_t* indices,
                             const double* data, const double* x, int add, double* y, hipStream_t s) {
  k_bcsr_mult<BR, BC><<<grid_for(nrows * kBcsrMultLanes), 256, 0, s>>>(nrows, ncols, indptr, indices, data, x, add, y);
}

extern "C" int fa_bcsr_mult(int64_t nrows, int64_t ncols, int32_t br, int32_t bc, const int64_t* indptr,
                            const int32_t* indices, const double* data, const double* x, int32_t add, double* y,
                            void* stream) {
  if (nrows < 0 || ncols < 0) return fail(FA_E_ARG, "fa_bcsr_mult: negative size (%lld x %lld)", (long long)nrows, (long long)ncols);
  if (ncols > INT32_MAX) return fail(FA_E_CAPACITY, "fa_bcsr_mult: column indices are int32");
  const int shape = br * 10 + bc;
  if (br < 1 || bc < 1 || br > 6 || bc > 6 ||
      (shape != 23 && shape != 32 && shape != 33 && shape != 36 && shape != 63 && shape != 66))
    return fail(FA_E_UNSUPPORTED, "fa_bcsr_mult: blocks %d x %d ((2,3), (3,2), (3,3), (3,6), (6,3), (6,6))", br, bc);
  if (nrows == 0) return FA_OK;
  if (!indptr || !x || !y) return fail(FA_E_ARG, "fa_bcsr_mult: null indptr, x or y");
  hipStream_t s = (hipStream_t)stream;
  switch (shape) {
    case 23: bcsr_mult_launch<2, 3>(nrows, ncols, indptr, indices, data, x, add, y, s); break;
    case 32: bcsr_mult_launch<3, 2>(nrows, ncols, indptr, indices, data, x, add, y, s); break;
    case 33: bcsr_mult_launch<3, 3>(nrows, ncols, indptr, indices, data, x, add, y, s); break;
    case 36: bcsr_mult_launch<3, 6>(nrows, ncols, indptr, indices, data, x, add, y, s); break;
    case 63: bcsr_mult_launch<6, 3>(nrows, ncols, indptr, indices, data, x, add, y, s); break;
    default: bcsr_mult_launch<6, 6>(nrows, ncols, indptr, indices, data, x, add, y, s); break;
  }
  LAUNCH_CHECK();
  return FA_OK;
}

// a wave per output block when the lists are long on average, a quarter wave when they are short (the
// choice depends on the arguments only, so a call's summation order is fixed)
template <int R, int K, int C>
static void bcsr_product_launch(int64_t nout, int64_t nprod, const int64_t* optr, const int32_t* xa, const int32_t* yb,
                                const double* X, int64_t nx, const double* Y, int64_t ny, double* out, hipStream_t s) {
  if (nprod > 8 * nout)
    k_bcsr_product<R, K, C, 64><<<grid_for(nout * 64), 256, 0, s>>>(nout, nprod, optr, xa, yb, X, nx, Y, ny, out);
  else
    k_bcsr_product<R, K, C, 16><<<grid_for(nout * 16), 256, 0, s>>>(nout, nprod, optr, xa, yb, X, nx, Y, ny, out);
}

extern "C" int fa_bcsr_product(int64_t nout, int32_t r, int32_t k, int32_t c, const int64_t* optr, int64_t nprod,
                               const int32_t* xa, const int32_t* yb, const double* X, int64_t nx, const double* Y,
                               int64_t ny, double* out, void* stream) {
  if (nout < 0 || nprod < 0 || nx < 0 || ny < 0)
    return fail(FA_E_ARG, "fa_bcsr_product: negative count (nout %lld, nprod %lld, nx %lld, ny %lld)", (long long)nout,
                (long long)nprod, (long long)nx, (long long)ny);
  if (nx > INT32_MAX || ny > INT32_MAX) return fail(FA_E_CAPACITY, "fa_bcsr_product: block slots are int32");
  const int shape = (r >= 1 && r <= 6 && k >= 1 && k <= 6 && c >= 1 && c <= 6) ? r * 100 + k * 10 + c : 0;
  if (shape != 223 && shape != 333 && shape != 336 && shape != 666 && shape != 323 && shape != 636)
    return fail(FA_E_UNSUPPORTED, "fa_bcsr_product: blocks [%d][%d] x [%d][%d] ((2,2,3), (3,3,3), (3,3,6), (6,6,6), "
                "(3,2,3), (6,3,6))", r, k, k, c);
  if (nout == 0) return FA_OK;
  if (!optr || !out) return fail(FA_E_ARG, "fa_bcsr_product: null optr or out");
  if (nprod > 0 && (!xa || !yb || !X || !Y)) return fail(FA_E_ARG, "fa_bcsr_product: null xa, yb, X or Y");
  hipStream_t s = (hipStream_t)stream;
  switch (shape) {
    case 223: bcsr_product_launch<2, 2, 3>(nout, nprod, optr, xa, yb, X, nx, Y, ny, out, s); break;
    case 333: bcsr_product_launch<3, 3, 3>(nout, nprod, optr, xa, yb, X, nx, Y, ny, out, s); break;
    case 336: bcsr_product_launch<3, 3, 6>(nout, nprod, optr, xa, yb, X, nx, Y, ny, out, s); break;
    case 666: bcsr_product_launch<6, 6, 6>(nout, nprod, optr, xa, yb, X, nx, Y, ny, out, s); break;
    case 323: bcsr_product_launch<3, 2, 3>(nout, nprod, optr, xa, yb, X, nx, Y, ny, out, s); break;
    default: bcsr_product_launch<6, 3, 6>(nout, nprod, optr, xa, yb, X, nx, Y, ny, out, s); break;
  }
  LAUNCH_CHECK();
  return FA_OK;
}

extern "C" int fa_cheb_step6(int64_t nnodes, const double* Dinv, const double* b, const double* Ax, double c_d,
                             double c_r, double* d, double* x, void* stream) {
  if (nnodes < 0) return fail(FA_E_ARG, "fa_cheb_step6: nnodes %lld", (long long)nnodes);
  if (!Dinv || !b || !d || !x) return fail(FA_E_ARG, "fa_cheb_step6: null Dinv, b, d or x");
  if (nnodes == 0) return FA_OK;
  const int64_t ndofs = nnodes * 6;
  k_cheb_step<6><<<grid_for(ndofs), 256, 0, (hipStream_t)stream>>>(ndofs, Dinv, b, Ax, c_d, c_r, d, x);
  LAUNCH_CHECK();
  return FA_OK;
}

extern "C" int fa_csr_row_max(int64_t nrows, const int64_t* indptr, const int32_t* indices, const int8_t* free_nodes,
                              const int64_t* in, int64_t nin, int64_t* out, void* stream) {
  if (nrows < 0 || nin < 0) return fail(FA_E_ARG, "fa_csr_row_max: negative count (nrows %lld, nin %lld)",
                                        (long long)nrows, (long long)nin);
  if (nin > INT32_MAX) return fail(FA_E_CAPACITY, "fa_csr_row_max: column indices are int32");
  if (nrows == 0) return FA_OK;
  if (!indptr || !in || !out) return fail(FA_E_ARG, "fa_csr_row_max: null indptr, in or out");
  k_csr_row_max<<<grid_for(nrows), 256, 0, (hipStream_t)stream>>>(nrows, indptr, indices, free_nodes, in, nin, out);
  LAUNCH_CHECK();
  return FA_OK;
}
