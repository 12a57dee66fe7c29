// femasm — point location and evaluation of a finite-element field at arbitrary points (included at the
// end of femasm_eval.hip: one translation unit). The counterpart of dolfinx.geometry.bb_tree +
// compute_colliding_cells and of Function.eval: what carries a solution to another mesh and what feeds
// the error norms of femasm_scalar.hip with a solution computed on a different mesh (the reference
// compares its two codes' displacements by matching dof coordinates,
// FEniCSx/mechanic2d/asym_elasto_damage_model.cc, IN_COMP; that needs meshes that share their nodes).
//
//   k_locate_points  one lane per point: the point's bin of a uniform grid (a host-built plan), the bin's
//                    cells in stored (ascending) order, the first cell that accepts the point.
//   k_eval_points    one lane per point: the space's Lagrange basis at the point's own reference
//                    coordinates, evaluated on the device, contracted with the nodal values.
//
// Neither uses atomics or allocates (k_eval_points caches a small table per element on the first call);
// both are grid-stride with 64-bit index arithmetic. No per-lane array is indexed by a runtime value:
// every loop over vertices, axes and lattice positions is unrolled over compile-time bounds.

constexpr int kLocateNewtonCap = 12;         // Newton steps per (point, cell) on quadrilaterals / hexahedra
constexpr double kLocateNewtonStop = 1e-12;  // converged when |dX|_inf of a step is at most this

struct GridView {
  int dims[3];
  double lo[3], inv_h[3];
  const int64_t* bin_ptr;
  const int32_t* bin_cells;
};

// det and adjugate of a GD x GD matrix (A^-1 = adj / det: the cofactor form, valid for either sign of det)
template <int GD>
__device__ __forceinline__ double pt_adjugate(const double (&A)[GD][GD], double (&C)[GD][GD]) {
  if constexpr (GD == 2) {
    C[0][0] = A[1][1];
    C[0][1] = -A[0][1];
    C[1][0] = -A[1][0];
    C[1][1] = A[0][0];
    return A[0][0] * A[1][1] - A[0][1] * A[1][0];
  } else {
    C[0][0] = A[1][1] * A[2][2] - A[1][2] * A[2][1];
    C[0][1] = A[0][2] * A[2][1] - A[0][1] * A[2][2];
    C[0][2] = A[0][1] * A[1][2] - A[0][2] * A[1][1];
    C[1][0] = A[1][2] * A[2][0] - A[1][0] * A[2][2];
    C[1][1] = A[0][0] * A[2][2] - A[0][2] * A[2][0];
    C[1][2] = A[0][2] * A[1][0] - A[0][0] * A[1][2];
    C[2][0] = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    C[2][1] = A[0][1] * A[2][0] - A[0][0] * A[2][1];
    C[2][2] = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    return A[0][0] * C[0][0] + A[0][1] * C[1][0] + A[0][2] * C[2][0];
  }
}

// Q1 geometry basis and reference gradients at X: vertex v = i + 2 j + 4 k (basix tensor order)
template <int GD>
__device__ __forceinline__ void pt_q1(const double (&X)[GD], double (&psi)[1 << GD], double (&dpsi)[1 << GD][GD]) {
#pragma unroll
  for (int v = 0; v < (1 << GD); ++v) {
    double f[GD], s[GD];
#pragma unroll
    for (int d = 0; d < GD; ++d) {
      const bool up = (v >> d) & 1;
      f[d] = up ? X[d] : 1.0 - X[d];
      s[d] = up ? 1.0 : -1.0;
    }
    double p = f[0];
#pragma unroll
    for (int d = 1; d < GD; ++d) p *= f[d];
    psi[v] = p;
#pragma unroll
    for (int k = 0; k < GD; ++k) {
      double g = s[k];
#pragma unroll
      for (int d = 0; d < GD; ++d)
        if (d != k) g *= f[d];
      dpsi[v][k] = g;
    }
  }
}

// The acceptance rule (include/femasm.h states it; femasm.geometry's host path restates it in torch).
// e[v] = x_v - x_v0 (e[0] is not read), dx = x - x_v0. Returns whether the cell holds the point; X is the
// point's reference position when it does.
template <int GD, int NV>
__device__ __forceinline__ bool pt_accept(const double (&e)[NV][GD], const double (&dx)[GD], double tol, double (&X)[GD]) {
  if constexpr (NV == GD + 1) {
    double J[GD][GD], C[GD][GD];
#pragma unroll
    for (int i = 0; i < GD; ++i)
#pragma unroll
      for (int k = 0; k < GD; ++k) J[i][k] = e[k + 1][i];
    const double det = pt_adjugate<GD>(J, C);
    double l0 = 1.0;
    bool in = true;
#pragma unroll
    for (int k = 0; k < GD; ++k) {
      double s = C[k][0] * dx[0];
#pragma unroll
      for (int i = 1; i < GD; ++i) s += C[k][i] * dx[i];
      X[k] = s / det;
      l0 -= X[k];
      in = in && X[k] >= -tol;
    }
    return in && l0 >= -tol;  // (a NaN fails every comparison: a degenerate cell holds nothing)
  } else {
#pragma unroll
    for (int d = 0; d < GD; ++d) X[d] = 0.5;
    double sign = 0.0;
    bool live = true, conv = false;
    for (int it = 0; it < kLocateNewtonCap && live && !conv; ++it) {
      double psi[NV], dpsi[NV][GD];
      pt_q1<GD>(X, psi, dpsi);
      double r[GD], J[GD][GD], C[GD][GD];
#pragma unroll
      for (int i = 0; i < GD; ++i) {
        r[i] = -dx[i];
#pragma unroll
        for (int k = 0; k < GD; ++k) J[i][k] = 0.0;
      }
#pragma unroll
      for (int v = 1; v < NV; ++v)
#pragma unroll
        for (int i = 0; i < GD; ++i) {
          r[i] += psi[v] * e[v][i];
#pragma unroll
          for (int k = 0; k < GD; ++k) J[i][k] += e[v][i] * dpsi[v][k];
        }
      const double det = pt_adjugate<GD>(J, C);
      if (it == 0) sign = det;  // the cell's orientation: det J at its centre
      const bool okdet = det * sign > 0.0;
      double step = 0.0;
      bool inbox = true;
      double Xn[GD];
#pragma unroll
      for (int k = 0; k < GD; ++k) {
        double s = C[k][0] * r[0];
#pragma unroll
        for (int i = 1; i < GD; ++i) s += C[k][i] * r[i];
        const double dX = -s / det;
        Xn[k] = X[k] + dX;
        step = fmax(step, fabs(dX));
        inbox = inbox && Xn[k] >= -1.0 && Xn[k] <= 2.0;
      }
      live = okdet && inbox;  // a step that leaves [-1, 2]^tdim or flips det J rejects the cell
      if (live) {
#pragma unroll
        for (int k = 0; k < GD; ++k) X[k] = Xn[k];
        conv = step <= kLocateNewtonStop;
      }
    }
    bool in = live && conv;
#pragma unroll
    for (int k = 0; k < GD; ++k) in = in && X[k] >= -tol && X[k] <= 1.0 + tol;
    return in;
  }
}

template <int GD, int NV>
__global__ __launch_bounds__(256) void k_locate_points(const int32_t* __restrict__ geom, const double* __restrict__ xv,
                                                       int64_t ncells, GridView G, int64_t npts,
                                                       const double* __restrict__ x, double tol,
                                                       int32_t* __restrict__ cell, double* __restrict__ Xout) {
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < npts; i += (int64_t)gridDim.x * 256) {
    double xp[GD];
    int64_t bin = 0;
    bool inside = true;
#pragma unroll
    for (int d = GD - 1; d >= 0; --d) {
      xp[d] = x[i * GD + d];
      const double t = (xp[d] - G.lo[d]) * G.inv_h[d];
      inside = inside && t >= 0.0 && t <= (double)G.dims[d];  // NaN and inf fail
      int b = inside ? (int)t : 0;                            // (t >= 0: truncation is the floor)
      b = b > G.dims[d] - 1 ? G.dims[d] - 1 : b;
      bin = bin * G.dims[d] + b;
    }
    int32_t found = -1;
    double Xf[GD];
#pragma unroll
    for (int d = 0; d < GD; ++d) Xf[d] = qnan;
    if (inside) {
      const int64_t j1 = G.bin_ptr[bin + 1];
      for (int64_t j = G.bin_ptr[bin]; j < j1; ++j) {
        const int64_t c = G.bin_cells[j];
        if (c < 0 || c >= ncells) continue;  // (never dereferenced)
        const int32_t* gv = geom + c * NV;
        double x0[GD], e[NV][GD], dx[GD];
        const int64_t v0 = gv[0];
#pragma unroll
        for (int d = 0; d < GD; ++d) {
          x0[d] = xv[v0 * GD + d];
          dx[d] = xp[d] - x0[d];
          e[0][d] = 0.0;
        }
#pragma unroll
        for (int v = 1; v < NV; ++v) {
          const int64_t vv = gv[v];
#pragma unroll
          for (int d = 0; d < GD; ++d) e[v][d] = xv[vv * GD + d] - x0[d];
        }
        double Xc[GD];
        if (pt_accept<GD, NV>(e, dx, tol, Xc)) {
          found = (int32_t)c;
#pragma unroll
          for (int d = 0; d < GD; ++d) Xf[d] = Xc[d];
          break;
        }
      }
    }
    cell[i] = found;
#pragma unroll
    for (int d = 0; d < GD; ++d) eval_store(Xout + i * GD + d, Xf[d]);
    store_fence(Xf);  // (as k_vector: the grid-stride loop's next point rewrites the stores' data registers)
  }
}

extern "C" int fa_locate_points(const fa_mesh* mesh, const fa_cell_grid* grid, int64_t npts, const double* x, double tol,
                                int32_t* cell, double* X, void* stream) {
  int rc = check_mesh(mesh);
  if (rc) return rc;
  if (!grid || !grid->bin_ptr || !grid->bin_cells) return fail(FA_E_ARG, "fa_locate_points: null grid arrays");
  if (npts < 0) return fail(FA_E_ARG, "fa_locate_points: npts %lld < 0", (long long)npts);
  if (!(tol >= 0.0)) return fail(FA_E_ARG, "fa_locate_points: tol must be >= 0");
  const int gd = mesh->gdim;
  int64_t nbins = 1;
  GridView G;
  for (int d = 0; d < 3; ++d) {
    if (grid->dims[d] < 1 || (d >= gd && grid->dims[d] != 1) || (nbins *= grid->dims[d]) >= (1ll << 31))
      return fail(FA_E_ARG, "fa_locate_points: grid dims %d x %d x %d (each >= 1, 1 beyond gdim, fewer than 2^31 bins)",
                  grid->dims[0], grid->dims[1], grid->dims[2]);
    G.dims[d] = grid->dims[d];
    G.lo[d] = grid->lo[d];
    G.inv_h[d] = grid->inv_h[d];
    if (d < gd && !(std::isfinite(G.lo[d]) && std::isfinite(G.inv_h[d]) && G.inv_h[d] > 0.0))
      return fail(FA_E_ARG, "fa_locate_points: grid axis %d has lo %g, inv_h %g", d, G.lo[d], G.inv_h[d]);
  }
  if (npts == 0) return FA_OK;
  if (!x || !cell || !X) return fail(FA_E_ARG, "fa_locate_points: null point arrays");
  G.bin_ptr = grid->bin_ptr;
  G.bin_cells = grid->bin_cells;
  hipStream_t s = (hipStream_t)stream;
  const int g = grid_for(npts);
#define LOC(GD_, NV_) \
  k_locate_points<GD_, NV_><<<g, 256, 0, s>>>(mesh->geom, mesh->x, mesh->ncells, G, npts, x, tol, cell, X)
  switch (mesh->cell_type) {
    case FA_TRIANGLE: LOC(2, 3); break;
    case FA_QUADRILATERAL: LOC(2, 4); break;
    case FA_TETRAHEDRON: LOC(3, 4); break;
    case FA_HEXAHEDRON: LOC(3, 8); break;
    default: return fail(FA_E_UNSUPPORTED, "fa_locate_points: cell type %d", mesh->cell_type);
  }
#undef LOC
  LAUNCH_CHECK();
  return FA_OK;
}

// ------------------------------------------------------------------------------------ evaluation
// Per-element table of the tensor elements, from the host definition (elements.h): the 1-D node positions
// r [P + 1] and, per lattice position (k * (P + 1) + j) * (P + 1) + i, the basix local node that sits there
// (tensor_node_lattice inverted). Simplices need none: their basis is closed-form in the barycentrics.
struct PointTable {
  const double* r;
  const int32_t* node;
};
static std::mutex g_point_mu;
static std::map<std::tuple<int, int, int>, PointTable> g_point_tabs;

static int get_point_table(int ct, int p, PointTable* out) {
  *out = PointTable{nullptr, nullptr};
  if (is_simplex(ct)) return FA_OK;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_point_mu);
  const auto key = std::make_tuple(dev, ct, p);
  auto it = g_point_tabs.find(key);
  if (it == g_point_tabs.end()) {
    const std::vector<double> r = line_points(p);
    const std::vector<int> L = tensor_node_lattice(ct, p);
    const int n1 = p + 1, nn = num_nodes(ct, p);
    std::vector<int32_t> node((size_t)n1 * n1 * n1, 0);
    for (int a = 0; a < nn; ++a) node[(L[3 * a + 2] * n1 + L[3 * a + 1]) * n1 + L[3 * a]] = a;
    // one allocation: the doubles first (8-byte aligned), then the ints
    const size_t rb = (size_t)n1 * sizeof(double), nb = node.size() * sizeof(int32_t);
    char* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, rb + nb));
    HIP_TRY(hipMemcpy(d, r.data(), rb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + rb, node.data(), nb, hipMemcpyHostToDevice));
    it = g_point_tabs.emplace(key, PointTable{reinterpret_cast<const double*>(d), reinterpret_cast<const int32_t*>(d + rb)}).first;
  }
  *out = it->second;
  return FA_OK;
}

// basix's edge order as local vertex pairs (elements.h: TRI_E, TET_E)
template <int GD>
__device__ __forceinline__ constexpr int pt_edge(int e, int end) {
  if constexpr (GD == 2) {
    constexpr int E[3][2] = {{1, 2}, {0, 2}, {0, 1}};
    return E[e][end];
  } else {
    constexpr int E[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
    return E[e][end];
  }
}

// One node's contribution: val[i] += phi w_a[i], R[i][k] += w_a[i] dphi[k] (rows i >= bs stay zero).
template <int GD>
__device__ __forceinline__ void pt_add(const double* __restrict__ w, int64_t node, int bs, double phi,
                                       const double (&dphi)[GD], double (&val)[3], double (&R)[3][GD]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    if (i < bs) {
      const double wi = w[node * bs + i];
      val[i] += phi * wi;
#pragma unroll
      for (int k = 0; k < GD; ++k) R[i][k] += wi * dphi[k];
    }
}

// P: the space's degree. Simplices (NV == GD + 1): P in {1, 2}; tensor cells: P in {1, 2, 3}.
template <int GD, int NV, int P>
__global__ __launch_bounds__(256) void k_eval_points(MeshView M, PointTable T, const double* __restrict__ w, int bs,
                                                     int64_t npts, const int32_t* __restrict__ cell,
                                                     const double* __restrict__ Xin, double* __restrict__ val_out,
                                                     double* __restrict__ grad_out) {
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const int nn = M.nn;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < npts; i += (int64_t)gridDim.x * 256) {
    const int64_t c = cell[i];
    double val[3] = {qnan, qnan, qnan}, g[3][GD];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < GD; ++k) g[r][k] = qnan;
    if (c >= 0 && c < M.ncells) {  // rows with cell < 0 (or out of range) read nothing
      double X[GD];
#pragma unroll
      for (int d = 0; d < GD; ++d) X[d] = Xin[i * GD + d];
      const int32_t* cn = M.cells + c * nn;
      const int32_t* gv = M.geom + c * NV;
      double R[3][GD];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        val[r] = 0.0;
#pragma unroll
        for (int k = 0; k < GD; ++k) R[r][k] = 0.0;
      }
      // the geometry Jacobian J[i][k] = sum_v x_v[i] d psi_v / d X_k at X, from edge vectors at vertex 0
      double J[GD][GD], C[GD][GD];
      {
        double x0[GD];
        const int64_t v0 = gv[0];
#pragma unroll
        for (int d = 0; d < GD; ++d) x0[d] = M.x[v0 * GD + d];
        if constexpr (NV == GD + 1) {
#pragma unroll
          for (int k = 0; k < GD; ++k) {
            const int64_t vv = gv[k + 1];
#pragma unroll
            for (int d = 0; d < GD; ++d) J[d][k] = M.x[vv * GD + d] - x0[d];
          }
        } else {
          double psi[NV], dpsi[NV][GD];
          pt_q1<GD>(X, psi, dpsi);
#pragma unroll
          for (int d = 0; d < GD; ++d)
#pragma unroll
            for (int k = 0; k < GD; ++k) J[d][k] = 0.0;
#pragma unroll
          for (int v = 1; v < NV; ++v) {
            const int64_t vv = gv[v];
#pragma unroll
            for (int d = 0; d < GD; ++d) {
              const double ev = M.x[vv * GD + d] - x0[d];
#pragma unroll
              for (int k = 0; k < GD; ++k) J[d][k] += ev * dpsi[v][k];
            }
          }
        }
      }
      const double det = pt_adjugate<GD>(J, C);
      if constexpr (NV == GD + 1) {
        double lam[NV];
        lam[0] = 1.0;
#pragma unroll
        for (int d = 0; d < GD; ++d) {
          lam[d + 1] = X[d];
          lam[0] -= X[d];
        }
#pragma unroll
        for (int a = 0; a < NV; ++a) {  // grad lambda_0 = -1, grad lambda_k = e_(k-1)
          double dp[GD];
          const double f = P == 1 ? 1.0 : 4.0 * lam[a] - 1.0;
#pragma unroll
          for (int k = 0; k < GD; ++k) dp[k] = a == 0 ? -f : (a == k + 1 ? f : 0.0);
          pt_add<GD>(w, cn[a], bs, P == 1 ? lam[a] : lam[a] * (2.0 * lam[a] - 1.0), dp, val, R);
        }
        if constexpr (P == 2) {
#pragma unroll
          for (int ed = 0; ed < GD * (GD + 1) / 2; ++ed) {
            const int a = pt_edge<GD>(ed, 0), b = pt_edge<GD>(ed, 1);
            double dp[GD];
#pragma unroll
            for (int k = 0; k < GD; ++k) {
              const double ga = a == 0 ? -1.0 : (a == k + 1 ? 1.0 : 0.0);
              const double gb = b == 0 ? -1.0 : (b == k + 1 ? 1.0 : 0.0);
              dp[k] = 4.0 * (lam[a] * gb + lam[b] * ga);
            }
            pt_add<GD>(w, cn[NV + ed], bs, 4.0 * lam[a] * lam[b], dp, val, R);
          }
        }
      } else {
        // 1-D Lagrange polynomials on the element's nodes (elements.h lagrange_1d), per axis
        constexpr int N1 = P + 1;
        double rr[N1], l[GD][N1], dl[GD][N1];
#pragma unroll
        for (int m = 0; m < N1; ++m) rr[m] = T.r[m];
#pragma unroll
        for (int d = 0; d < GD; ++d)
#pragma unroll
          for (int a = 0; a < N1; ++a) {
            double v = 1.0, dv = 0.0;
#pragma unroll
            for (int m = 0; m < N1; ++m)
              if (m != a) {
                const double inv = 1.0 / (rr[a] - rr[m]);  // wave-uniform
                const double f = (X[d] - rr[m]) * inv;
                dv = dv * f + v * inv;
                v *= f;
              }
            l[d][a] = v;
            dl[d][a] = dv;
          }
#pragma unroll
        for (int kk = 0; kk < (GD == 3 ? N1 : 1); ++kk)
#pragma unroll
          for (int jj = 0; jj < N1; ++jj)
#pragma unroll
            for (int ii = 0; ii < N1; ++ii) {
              const int a = T.node[(kk * N1 + jj) * N1 + ii];  // wave-uniform (scalar load)
              double dp[GD], phi;
              if constexpr (GD == 2) {
                phi = l[0][ii] * l[1][jj];
                dp[0] = dl[0][ii] * l[1][jj];
                dp[1] = l[0][ii] * dl[1][jj];
              } else {
                phi = l[0][ii] * l[1][jj] * l[2][kk];
                dp[0] = dl[0][ii] * l[1][jj] * l[2][kk];
                dp[1] = l[0][ii] * dl[1][jj] * l[2][kk];
                dp[2] = l[0][ii] * l[1][jj] * dl[2][kk];
              }
              pt_add<GD>(w, cn[a], bs, phi, dp, val, R);
            }
      }
      // grad[r][j] = sum_k R[r][k] Jinv[k][j], Jinv = adj / det
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int j = 0; j < GD; ++j) {
          double s = R[r][0] * C[0][j];
#pragma unroll
          for (int k = 1; k < GD; ++k) s += R[r][k] * C[k][j];
          g[r][j] = s / det;
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (r < bs) {
        if (val_out) eval_store(val_out + i * bs + r, val[r]);
        if (grad_out)
#pragma unroll
          for (int j = 0; j < GD; ++j) eval_store(grad_out + (i * bs + r) * GD + j, g[r][j]);
      }
    store_fence(val);
    store_fence(g);
  }
}

extern "C" int fa_eval_points(const fa_mesh* mesh, const double* w, int32_t bs, int64_t npts, const int32_t* cell,
                              const double* X, double* val, double* grad, void* stream) {
  int rc = check_mesh(mesh);
  if (rc) return rc;
  if (bs < 1 || bs > 3) return fail(FA_E_ARG, "fa_eval_points: block size %d outside 1 .. 3", bs);
  if (npts < 0) return fail(FA_E_ARG, "fa_eval_points: npts %lld < 0", (long long)npts);
  if (!w) return fail(FA_E_ARG, "fa_eval_points: null nodal field w");
  if (!val && !grad) return fail(FA_E_ARG, "fa_eval_points: no output requested (val and grad are NULL)");
  if (npts == 0) return FA_OK;
  if (!cell || !X) return fail(FA_E_ARG, "fa_eval_points: null cell / X");
  const int ct = mesh->cell_type, p = mesh->degree;
  PointTable T;
  if ((rc = get_point_table(ct, p, &T))) return rc;
  hipStream_t s = (hipStream_t)stream;
  MeshView M{mesh->cells, mesh->geom, mesh->x, mesh->ncells, mesh->nnodes, mesh->nn, mesh->nv, mesh->gdim};
  const int g = grid_for(npts);
#define EP(GD_, NV_, P_) k_eval_points<GD_, NV_, P_><<<g, 256, 0, s>>>(M, T, w, bs, npts, cell, X, val, grad)
#define EP_SIMPLEX(GD_)                       \
  if (p == 1) EP(GD_, GD_ + 1, 1);            \
  else EP(GD_, GD_ + 1, 2)
#define EP_TENSOR(GD_)                        \
  if (p == 1) EP(GD_, 1 << GD_, 1);           \
  else if (p == 2) EP(GD_, 1 << GD_, 2);      \
  else EP(GD_, 1 << GD_, 3)
  switch (ct) {
    case FA_TRIANGLE: EP_SIMPLEX(2); break;
    case FA_TETRAHEDRON: EP_SIMPLEX(3); break;
    case FA_QUADRILATERAL: EP_TENSOR(2); break;
    case FA_HEXAHEDRON: EP_TENSOR(3); break;
    default: return fail(FA_E_UNSUPPORTED, "fa_eval_points: cell type %d", ct);
  }
#undef EP_TENSOR
#undef EP_SIMPLEX
#undef EP
  LAUNCH_CHECK();
  return FA_OK;
}
