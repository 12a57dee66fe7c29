// femasm — scalar functionals: one number integrated over the mesh (included at the end of
// femasm_eval.hip: one translation unit). The counterpart of dolfinx.fem.assemble_scalar for the
// integrands the library's forms define:
//
//   FA_FUNC_MEASURE        int 1 dx
//   FA_FUNC_STRAIN_ENERGY  int psi(grad u) dx of the form's law: the potential whose first derivative is
//                          fa_assemble_vector's sigma term and whose second is the assembled tangent
//   FA_FUNC_L2             int |w - g|^2 dx
//   FA_FUNC_H1             int |grad w - G|^2 dx
//
// k_functional_cells visits every cell exactly once (one lane per cell) and writes the cell's integral;
// k_functional_reduce sums 256-cell tiles in a fixed tree order and then the tile partials in a fixed order.
// No atomics: the total is bit-identical run to run and independent of the grid.
// The device laws and the geometry are femasm.hip's (cell_geometry_q, phys_grad, cell_lame,
// deformation_gradient, neo_psi, damage_potential): nothing is restated here.

// kernel kinds: the public FA_FUNC_* values, the strain energy split by law
constexpr int FK_MEASURE = 0, FK_LIN = 1, FK_L2 = 2, FK_H1 = 3, FK_NEO = 4, FK_DAMAGE = 5;
constexpr int kFuncTile = 256;  // cells per partial

// One lane per cell. The tables are indexed by wave-uniform values (scalar loads); the nodal values are
// read inside the node loop, so no per-lane array is indexed by a runtime value (no scratch at any nn).
// fld: the nodal field, form->u (energies) or w (norms), [nnodes][GD]. gq: g [ncells][nq][GD] (FK_L2) or
// G [ncells][nq][GD][GD] (FK_H1), or NULL.
template <int GD, int NV, int KIND>
__global__ __launch_bounds__(256) void k_functional_cells(MeshView M, FormView F, DevTables T,
                                                          const double* __restrict__ fld,
                                                          const double* __restrict__ gq,
                                                          double* __restrict__ cell_out) {
  const int nn = M.nn, nq = T.nq;
  for (int64_t c = blockIdx.x * (int64_t)256 + threadIdx.x; c < M.ncells; c += (int64_t)gridDim.x * 256) {
    const int32_t* cn = M.cells + c * nn;
    [[maybe_unused]] double lam = 0.0, mu = 0.0;
    if constexpr (KIND == FK_LIN || KIND == FK_NEO || KIND == FK_DAMAGE) cell_lame(F, c, lam, mu);
    double Ji[GD][GD];
    double dj = 0.0;
    if constexpr (NV == GD + 1) dj = cell_geometry_q<GD, NV>(M, c, T.gdphi, Ji);  // affine: once per cell
    double acc = 0.0;
    for (int q = 0; q < nq; ++q) {
      if constexpr (NV != GD + 1) dj = cell_geometry_q<GD, NV>(M, c, T.gdphi + (size_t)q * NV * GD, Ji);
      const double wd = T.wq[q] * dj;
      if constexpr (KIND == FK_MEASURE) {
        acc += wd;
      } else if constexpr (KIND == FK_L2) {
        double v[GD];
#pragma unroll
        for (int i = 0; i < GD; ++i) v[i] = 0.0;
        for (int b = 0; b < nn; ++b) {
          const double ph = T.phi[(size_t)q * nn + b];
          const int64_t n = cn[b];
#pragma unroll
          for (int i = 0; i < GD; ++i) v[i] += fld[n * GD + i] * ph;
        }
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < GD; ++i) {
          const double d = gq ? v[i] - gq[(c * nq + q) * GD + i] : v[i];
          s += d * d;
        }
        acc += wd * s;
      } else if constexpr (KIND == FK_NEO) {
        double Fq[GD * GD];
        deformation_gradient<GD>(fld, cn, nn, T.dphi + (size_t)q * nn * GD, Ji, Fq);
        acc += wd * neo_psi<GD, double>(Fq, lam, mu);  // J <= 0: NaN / inf, passed through
      } else {
        double gu[GD][GD];
#pragma unroll
        for (int i = 0; i < GD; ++i)
#pragma unroll
          for (int k = 0; k < GD; ++k) gu[i][k] = 0.0;
        [[maybe_unused]] double dq = 0.0;
        for (int b = 0; b < nn; ++b) {
          double gb[GD];
          phys_grad<GD>(T.dphi + ((size_t)q * nn + b) * GD, Ji, gb);
          const int64_t n = cn[b];
#pragma unroll
          for (int i = 0; i < GD; ++i) {
            const double ui = fld[n * GD + i];
#pragma unroll
            for (int k = 0; k < GD; ++k) gu[i][k] += ui * gb[k];
          }
          if constexpr (KIND == FK_DAMAGE)
            if (F.d) dq += F.d[n];
        }
        if constexpr (KIND == FK_H1) {
          double s = 0.0;
#pragma unroll
          for (int i = 0; i < GD; ++i)
#pragma unroll
            for (int k = 0; k < GD; ++k) {
              const double d = gq ? gu[i][k] - gq[((c * nq + q) * GD + i) * GD + k] : gu[i][k];
              s += d * d;
            }
          acc += wd * s;
        } else {
          // small strain: 1/2 lam tr(eps)^2 + mu eps:eps, or the damage potential for d > 0
          double psi = 0.0;
          bool linear = true;
          if constexpr (KIND == FK_DAMAGE) {
            if constexpr (GD == 2) {
              const double d = dq * (1.0 / 3.0);  // the mean nodal damage, unclamped (as damage_stress_ad)
              if (d > 0.0) {
                const double s01 = 0.5 * (gu[0][1] + gu[1][0]);
                const double st[4] = {gu[0][0], s01, s01, gu[1][1]};
                psi = damage_potential<double>(st, lam, mu, d);
                linear = false;
              }
            }
          }
          if (linear) {
            double tr = 0.0, ee = 0.0;
#pragma unroll
            for (int i = 0; i < GD; ++i) {
              tr += gu[i][i];
              ee += gu[i][i] * gu[i][i];
            }
#pragma unroll
            for (int i = 0; i < GD; ++i)
#pragma unroll
              for (int k = i + 1; k < GD; ++k) {
                const double e = 0.5 * (gu[i][k] + gu[k][i]);
                ee += 2.0 * (e * e);
              }
            psi = 0.5 * lam * (tr * tr) + mu * ee;
          }
          acc += wd * psi;
        }
      }
    }
    double o[1] = {acc};
    cell_out[c] = o[0];
    store_fence(o);  // (as k_vector: the grid-stride loop's next cell rewrites the store's data register)
  }
}

// Fixed-order sums. stage 0: out[t] = the sum of in[256 t .. 256 t + 255] (entries past n count as +0.0),
// one workgroup per tile in a grid-stride loop: lane i holds entry i, then a binary tree over the lanes
// (strides 128, 64, .. 1). stage 1, ONE workgroup: lane i adds in[i], in[i + 256], in[i + 512], .. in that
// order, then the same tree; out[0] = the total. Neither depends on the grid size.
__global__ __launch_bounds__(256) void k_functional_reduce(const double* __restrict__ in, int64_t n,
                                                           double* __restrict__ out, int stage) {
  __shared__ double sh[kFuncTile];
  const int t = threadIdx.x;
  if (stage == 0) {
    const int64_t ntiles = (n + kFuncTile - 1) / kFuncTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const int64_t i = tile * kFuncTile + t;
      sh[t] = i < n ? in[i] : 0.0;
      __syncthreads();
#pragma unroll
      for (int s = kFuncTile / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
      }
      if (t == 0) out[tile] = sh[0];
      __syncthreads();  // sh is rewritten by the next tile
    }
  } else {
    if (blockIdx.x != 0) return;
    double a = 0.0;
    for (int64_t i = t; i < n; i += kFuncTile) a += in[i];
    sh[t] = a;
    __syncthreads();
#pragma unroll
    for (int s = kFuncTile / 2; s > 0; s >>= 1) {
      if (t < s) sh[t] += sh[t + s];
      __syncthreads();
    }
    if (t == 0) out[0] = sh[0];
  }
}

// workspace layout: cell values [ncells] (used when the caller passes no cell_out), then the tile partials
static int64_t functional_cell_bytes(int64_t ncells) { return align256(ncells * (int64_t)sizeof(double)); }
static int64_t functional_ntiles(int64_t ncells) { return (ncells + kFuncTile - 1) / kFuncTile; }

extern "C" int fa_quadrature(int32_t cell_type, int32_t qdeg, int32_t* nq, double* pts, double* wts) {
  if (cell_type != FA_TRIANGLE && cell_type != FA_QUADRILATERAL && cell_type != FA_TETRAHEDRON &&
      cell_type != FA_HEXAHEDRON)
    return fail(FA_E_UNSUPPORTED, "fa_quadrature: cell type %d", cell_type);
  if (qdeg < 0 || qdeg > 12) return fail(FA_E_UNSUPPORTED, "fa_quadrature: degree %d outside 0 .. 12", qdeg);
  if (!nq) return fail(FA_E_ARG, "fa_quadrature: null nq");
  const Quadrature Q = make_quadrature(cell_type, qdeg);
  const int n = Q.size();
  if (pts || wts) {
    if (*nq < n) return fail(FA_E_ARG, "fa_quadrature: capacity *nq = %d, the rule has %d points", *nq, n);
    if (pts) std::copy(Q.pts.begin(), Q.pts.end(), pts);
    if (wts) std::copy(Q.wts.begin(), Q.wts.end(), wts);
  }
  *nq = n;
  return FA_OK;
}

extern "C" int fa_functional_work_bytes(const fa_mesh* mesh, int64_t* bytes) {
  if (!mesh || !bytes) return fail(FA_E_ARG, "fa_functional_work_bytes: null argument");
  if (mesh->ncells < 0) return fail(FA_E_ARG, "negative sizes");
  *bytes = functional_cell_bytes(mesh->ncells) + align256(functional_ntiles(mesh->ncells) * (int64_t)sizeof(double)) + 256;
  return FA_OK;
}

extern "C" int fa_assemble_scalar(const fa_mesh* mesh, const fa_form* form, int32_t kind, const double* w,
                                  const double* g, int32_t qdeg, double* cell_out, void* work, int64_t work_bytes,
                                  double* total, void* stream) {
  if (!mesh) return fail(FA_E_ARG, "mesh has null arrays");
  if (kind != FA_FUNC_MEASURE && kind != FA_FUNC_STRAIN_ENERGY && kind != FA_FUNC_L2 && kind != FA_FUNC_H1)
    return fail(FA_E_ARG, "fa_assemble_scalar: kind %d (FA_FUNC_*)", kind);
  if (!cell_out && !total && mesh->ncells != 0)
    return fail(FA_E_ARG, "fa_assemble_scalar: no output (cell_out and total are NULL)");
  if (mesh->ncells == 0) {  // an empty mesh (its arrays may be null): +0.0, no cell launch
    if (total) HIP_TRY(hipMemsetAsync(total, 0, sizeof(double), (hipStream_t)stream));
    return FA_OK;
  }
  int rc = check_mesh(mesh);
  if (rc) return rc;
  if (qdeg > 12) return fail(FA_E_UNSUPPORTED, "quadrature degree %d > 12", qdeg);
  const int ct = mesh->cell_type, p = mesh->degree;
  const int64_t nc = mesh->ncells;
  int64_t need = 0;
  if ((rc = fa_functional_work_bytes(mesh, &need))) return rc;
  if (total && (!work || work_bytes < need))
    return fail(FA_E_ARG, "fa_assemble_scalar: workspace of %lld bytes, %lld needed (fa_functional_work_bytes)",
                (long long)(work ? work_bytes : 0), (long long)need);
  if (!cell_out && (reinterpret_cast<uintptr_t>(work) & 7u)) return fail(FA_E_ARG, "fa_assemble_scalar: work not 8-byte aligned");
  FormView F{};
  int fk = kind;
  const double* fld = w;
  int qd = qdeg;
  if (kind == FA_FUNC_STRAIN_ENERGY) {
    if ((rc = form_view(mesh, form, F))) return rc;
    if (!F.u) return fail(FA_E_ARG, "FA_FUNC_STRAIN_ENERGY needs the state u (form->u is NULL)");
    fk = F.kind == FA_NEO_HOOKEAN ? FK_NEO : F.kind == FA_ASYM_DAMAGE ? FK_DAMAGE : FK_LIN;
    fld = F.u;
    if (qd < 0 || fk == FK_DAMAGE) qd = fk == FK_DAMAGE ? 1 : form->qdeg;  // the rule of k_vector's sigma term
    if (qd < 0) qd = estimated_qdeg(ct, p);
  } else if (kind == FA_FUNC_MEASURE) {
    if (qd < 0) qd = std::max(1, estimated_qdeg(ct, p));
  } else {
    if (!w) return fail(FA_E_ARG, "fa_assemble_scalar: FA_FUNC_L2 / FA_FUNC_H1 need the nodal field w");
    if (qd < 0) qd = 2 * p;
  }
  hipStream_t s = (hipStream_t)stream;
  DevTables T;
  if ((rc = get_tables(ct, p, qd, &T))) return rc;
  double* cells_buf = cell_out ? cell_out : reinterpret_cast<double*>(work);
  double* partials = total ? reinterpret_cast<double*>(reinterpret_cast<char*>(work) + functional_cell_bytes(nc)) : nullptr;
  MeshView M{mesh->cells, mesh->geom, mesh->x, mesh->ncells, mesh->nnodes, mesh->nn, mesh->nv, mesh->gdim};
  const int grid = grid_for(nc);
#define FN(GD_, NV_, K_) k_functional_cells<GD_, NV_, K_><<<grid, 256, 0, s>>>(M, F, T, fld, g, cells_buf)
#define FN_CELL(GD_, NV_)                    \
  switch (fk) {                              \
    case FK_MEASURE: FN(GD_, NV_, FK_MEASURE); break; \
    case FK_LIN: FN(GD_, NV_, FK_LIN); break;         \
    case FK_L2: FN(GD_, NV_, FK_L2); break;           \
    case FK_H1: FN(GD_, NV_, FK_H1); break;           \
    case FK_NEO: FN(GD_, NV_, FK_NEO); break;         \
    default: return fail(FA_E_UNSUPPORTED, "fa_assemble_scalar: kind %d on cell type %d", fk, ct); \
  }
  switch (ct) {
    case FA_TRIANGLE:
      if (fk == FK_DAMAGE) FN(2, 3, FK_DAMAGE);  // (form_view admits the damage kinds on P1 triangles only)
      else FN_CELL(2, 3);
      break;
    case FA_QUADRILATERAL: FN_CELL(2, 4); break;
    case FA_TETRAHEDRON: FN_CELL(3, 4); break;
    case FA_HEXAHEDRON: FN_CELL(3, 8); break;
    default: return fail(FA_E_UNSUPPORTED, "fa_assemble_scalar: cell type %d", ct);
  }
#undef FN_CELL
#undef FN
  LAUNCH_CHECK();
  if (total) {
    const int64_t nt = functional_ntiles(nc);
    k_functional_reduce<<<grid_for(nt, 1), kFuncTile, 0, s>>>(cells_buf, nc, partials, 0);
    LAUNCH_CHECK();
    k_functional_reduce<<<1, kFuncTile, 0, s>>>(partials, nt, total, 1);
    LAUNCH_CHECK();
  }
  return FA_OK;
}
