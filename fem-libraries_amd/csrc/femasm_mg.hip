// femasm — geometric multigrid kernels (included at the end of femasm_eval.hip: one translation unit).
//
// fa_prolong / fa_restrict: the linear-interpolation transfer between a coarse lattice of nc[d] + 1
// points per axis and the fine lattice of 2 nc[d] + 1 points (lattice index 0 fastest, the numbering of
// the structured meshes' degree-1 and degree-2 nodes). The degree-2 nodes of an n mesh and the degree-1
// nodes of a 2n mesh are the same lattice, and the right-diagonal triangle / Kuhn tetrahedron mesh of 2n
// refines that of n, so this one stencil is both the P2 -> P1 transfer on one mesh and the P1(h) ->
// P1(2h) transfer. A fine point I with odd mask o = I & 1:
//   simplices     x_f(I) = 1/2 x_c((I - o) / 2) + 1/2 x_c((I + o) / 2)   (o is an edge direction)
//   tensor cells  the mean of the 2^|o| coarse points (I +- o) / 2 over the odd axes
// Both kernels gather (one thread per output dof, fixed summation order, no atomics), so the restriction
// is the exact transpose of the prolongation and bit-reproducible.
//
// fa_cheb_step: one fused pass of the Chebyshev / block-Jacobi smoother.
//
// Threads map to (dof within a lattice row, row, plane) through the launch grid: no integer division by
// a lattice extent, and every offset is 64-bit (config E's P2 lattice has 6.8e7 nodes, 2.0e8 dofs).

struct MgLattice {
  int simplex;
  int64_t pc[3];  // coarse points per axis (nc + 1; 1 on an unused axis)
  int64_t pf[3];  // fine points per axis (2 nc + 1; 1 on an unused axis)
};

template <int BS>
__global__ __launch_bounds__(256) void k_mg_prolong(MgLattice T, const double* __restrict__ xc,
                                                    const int8_t* __restrict__ bc_c, const int8_t* __restrict__ bc_f,
                                                    int add, double* __restrict__ xf) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= T.pf[0] * BS) return;
  const int64_t I = t / BS;
  const int c = (int)(t - I * BS);
  const int64_t sc1 = T.pc[0], sc2 = T.pc[0] * T.pc[1];
  const int o0 = (int)(I & 1);
  for (int64_t K = blockIdx.z; K < T.pf[2]; K += gridDim.z) {
    const int o2 = (int)(K & 1);
    for (int64_t J = blockIdx.y * (int64_t)blockDim.y + threadIdx.y; J < T.pf[1]; J += (int64_t)gridDim.y * blockDim.y) {
      const int o1 = (int)(J & 1);
      const int64_t fd = (I + T.pf[0] * (J + T.pf[1] * K)) * BS + c;
      const int64_t na = (I >> 1) + sc1 * (J >> 1) + sc2 * (K >> 1);
      double v = 0.0;
      if (!(bc_f && bc_f[fd])) {
        if (T.simplex) {
          const int64_t nb = na + o0 + o1 * sc1 + o2 * sc2;
          const int64_t da = na * BS + c, db = nb * BS + c;
          const double va = (bc_c && bc_c[da]) ? 0.0 : xc[da];
          if (nb == na) {
            v = va;
          } else {
            const double vb = (bc_c && bc_c[db]) ? 0.0 : xc[db];
            v = 0.5 * va + 0.5 * vb;
          }
        } else {
          double s = 0.0;
          for (int s2 = 0; s2 <= o2; ++s2)
            for (int s1 = 0; s1 <= o1; ++s1)
              for (int s0 = 0; s0 <= o0; ++s0) {
                const int64_t dc = (na + s0 + s1 * sc1 + s2 * sc2) * BS + c;
                s += (bc_c && bc_c[dc]) ? 0.0 : xc[dc];
              }
          const int k = o0 + o1 + o2;
          v = s * (k == 0 ? 1.0 : k == 1 ? 0.5 : k == 2 ? 0.25 : 0.125);
        }
      }
      if (!add) xf[fd] = v;
      else if (!(bc_f && bc_f[fd])) xf[fd] += v;  // a masked fine dof receives nothing
    }
  }
}

template <int BS>
__global__ __launch_bounds__(256) void k_mg_restrict(MgLattice T, const double* __restrict__ rf,
                                                     const int8_t* __restrict__ bc_f, const int8_t* __restrict__ bc_c,
                                                     double* __restrict__ rc) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= T.pc[0] * BS) return;
  const int64_t I = t / BS;
  const int c = (int)(t - I * BS);
  const int64_t sf1 = T.pf[0], sf2 = T.pf[0] * T.pf[1];
  for (int64_t K = blockIdx.z; K < T.pc[2]; K += gridDim.z) {
    for (int64_t J = blockIdx.y * (int64_t)blockDim.y + threadIdx.y; J < T.pc[1]; J += (int64_t)gridDim.y * blockDim.y) {
      const int64_t cd = (I + T.pc[0] * (J + T.pc[1] * K)) * BS + c;
      double s = 0.0;
      if (!(bc_c && bc_c[cd])) {
        const int64_t F0 = 2 * I, F1 = 2 * J, F2 = 2 * K;
        for (int e2 = -1; e2 <= 1; ++e2) {
          if (F2 + e2 < 0 || F2 + e2 >= T.pf[2]) continue;
          for (int e1 = -1; e1 <= 1; ++e1) {
            if (F1 + e1 < 0 || F1 + e1 >= T.pf[1]) continue;
            for (int e0 = -1; e0 <= 1; ++e0) {
              if (F0 + e0 < 0 || F0 + e0 >= T.pf[0]) continue;
              // simplices: the neighbour is +o or -o for a 0/1 vector o (no mixed signs)
              const bool pos = e0 > 0 || e1 > 0 || e2 > 0, neg = e0 < 0 || e1 < 0 || e2 < 0;
              if (T.simplex && pos && neg) continue;
              const int k = (e0 != 0) + (e1 != 0) + (e2 != 0);
              const double w = k == 0 ? 1.0 : (T.simplex || k == 1) ? 0.5 : k == 2 ? 0.25 : 0.125;
              const int64_t fd = ((F0 + e0) + sf1 * (F1 + e1) + sf2 * (F2 + e2)) * BS + c;
              if (!(bc_f && bc_f[fd])) s += w * rf[fd];
            }
          }
        }
      }
      rc[cd] = s;
    }
  }
}

// d <- c_d d + c_r Dinv (b - Ax), x <- x + d; one thread per dof (row r of its node's block). c_d == 0
// (the first step of a polynomial) does not read d; Ax == NULL is A x = 0 (a zero initial guess).
template <int BS>
__global__ __launch_bounds__(256) void k_cheb_step(int64_t ndofs, const double* __restrict__ Dinv,
                                                   const double* __restrict__ b, const double* __restrict__ Ax,
                                                   double c_d, double c_r, double* __restrict__ d,
                                                   double* __restrict__ x) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < ndofs; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n0 = (i / BS) * BS;
    const double* __restrict__ Di = Dinv + i * BS;
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < BS; ++c) s += Di[c] * (Ax ? b[n0 + c] - Ax[n0 + c] : b[n0 + c]);
    double dn = c_r * s;
    if (c_d != 0.0) dn += c_d * d[i];
    d[i] = dn;
    x[i] += dn;
  }
}

static int mg_lattice(const fa_transfer* t, MgLattice& T) {
  if (!t) return fail(FA_E_ARG, "null transfer descriptor");
  if (t->tdim != 2 && t->tdim != 3) return fail(FA_E_ARG, "fa_transfer: tdim %d (2 or 3)", t->tdim);
  if (t->simplex != 0 && t->simplex != 1) return fail(FA_E_ARG, "fa_transfer: simplex %d (0 or 1)", t->simplex);
  if (t->bs < 1 || t->bs > 3) return fail(FA_E_UNSUPPORTED, "fa_transfer: block size %d (1 to 3)", t->bs);
  T.simplex = t->simplex;
  double total = (double)t->bs;
  for (int d = 0; d < 3; ++d) {
    const int64_t n = d < t->tdim ? t->nc[d] : 0;
    if (d < t->tdim && (n < 1 || n > (int64_t)1 << 30))
      return fail(FA_E_ARG, "fa_transfer: nc[%d] = %lld (at least 1)", d, (long long)t->nc[d]);
    T.pc[d] = n + 1;
    T.pf[d] = 2 * n + 1;
    total *= (double)T.pf[d];
  }
  if (total >= 9.0e18) return fail(FA_E_CAPACITY, "fa_transfer: the fine lattice has more than 2^63 dofs");
  return FA_OK;
}

// (row dofs, rows, planes) -> block (bx, 256 / bx) and grid; rows and planes beyond the grid limits are
// looped over in the kernels
static void mg_launch_shape(int64_t rowdofs, int64_t rows, int64_t planes, dim3& grid, dim3& block) {
  const int bx = rowdofs <= 64 ? 64 : rowdofs <= 128 ? 128 : 256;
  const int by = 256 / bx;
  block = dim3(bx, by, 1);
  grid = dim3((unsigned)((rowdofs + bx - 1) / bx), (unsigned)std::min<int64_t>((rows + by - 1) / by, 65535),
              (unsigned)std::min<int64_t>(planes, 65535));
}

extern "C" int fa_prolong(const fa_transfer* t, const double* xc, const int8_t* bc_c, const int8_t* bc_f, int32_t add,
                          double* xf, void* stream) {
  MgLattice T;
  int rc = mg_lattice(t, T);
  if (rc) return rc;
  if (!xc || !xf) return fail(FA_E_ARG, "fa_prolong: null xc or xf");
  dim3 grid, block;
  mg_launch_shape(T.pf[0] * t->bs, T.pf[1], T.pf[2], grid, block);
  hipStream_t s = (hipStream_t)stream;
  switch (t->bs) {
    case 1: k_mg_prolong<1><<<grid, block, 0, s>>>(T, xc, bc_c, bc_f, add, xf); break;
    case 2: k_mg_prolong<2><<<grid, block, 0, s>>>(T, xc, bc_c, bc_f, add, xf); break;
    default: k_mg_prolong<3><<<grid, block, 0, s>>>(T, xc, bc_c, bc_f, add, xf); break;
  }
  LAUNCH_CHECK();
  return FA_OK;
}

extern "C" int fa_restrict(const fa_transfer* t, const double* rf, const int8_t* bc_f, const int8_t* bc_c, double* rc_out,
                           void* stream) {
  MgLattice T;
  int rc = mg_lattice(t, T);
  if (rc) return rc;
  if (!rf || !rc_out) return fail(FA_E_ARG, "fa_restrict: null rf or rc");
  dim3 grid, block;
  mg_launch_shape(T.pc[0] * t->bs, T.pc[1], T.pc[2], grid, block);
  hipStream_t s = (hipStream_t)stream;
  switch (t->bs) {
    case 1: k_mg_restrict<1><<<grid, block, 0, s>>>(T, rf, bc_f, bc_c, rc_out); break;
    case 2: k_mg_restrict<2><<<grid, block, 0, s>>>(T, rf, bc_f, bc_c, rc_out); break;
    default: k_mg_restrict<3><<<grid, block, 0, s>>>(T, rf, bc_f, bc_c, rc_out); break;
  }
  LAUNCH_CHECK();
  return FA_OK;
}

extern "C" int fa_cheb_step(int64_t nnodes, int32_t bs, const double* Dinv, const double* b, const double* Ax, double c_d,
                            double c_r, double* d, double* x, void* stream) {
  if (nnodes < 0) return fail(FA_E_ARG, "fa_cheb_step: nnodes %lld", (long long)nnodes);
  if (bs < 1 || bs > 3) return fail(FA_E_UNSUPPORTED, "fa_cheb_step: block size %d (1 to 3)", bs);
  if (!Dinv || !b || !d || !x) return fail(FA_E_ARG, "fa_cheb_step: null Dinv, b, d or x");
  if (nnodes == 0) return FA_OK;
  const int64_t ndofs = nnodes * bs;
  const int grid = grid_for(ndofs);
  hipStream_t s = (hipStream_t)stream;
  switch (bs) {
    case 1: k_cheb_step<1><<<grid, 256, 0, s>>>(ndofs, Dinv, b, Ax, c_d, c_r, d, x); break;
    case 2: k_cheb_step<2><<<grid, 256, 0, s>>>(ndofs, Dinv, b, Ax, c_d, c_r, d, x); break;
    default: k_cheb_step<3><<<grid, 256, 0, s>>>(ndofs, Dinv, b, Ax, c_d, c_r, d, x); break;
  }
  LAUNCH_CHECK();
  return FA_OK;
}
