// femasm — the library's translation unit: femasm.hip (assembly kernels and their C ABI, kept
// byte-identical so the traffic records keyed on its hash stay valid) plus per-cell expression
// evaluation, fa_eval_cells: grad u, strain, stress and energy density at reference points of every
// cell, the reference's post-processing step (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:909-942:
// create_expression + interpolate into a DG0 space; MFEM strainTensor / stressTensor coefficients,
// MFEM/mechanic2d/asym_elasto_damage_model.cc:332-457). One translation unit: the file-static helpers
// and the device laws of femasm.hip (damage_stress, damage_stress_ad, neo_stress_ad, the geometry) are
// used here, not copied.
//
// fa_version is this file's (101: fa_eval_cells present; 102: the matrix-free Jacobian action of
// femasm_apply.hip, included at the end of this file; 103: the multigrid transfers and smoother step of
// femasm_mg.hip, included after it; 104: mesh refinement and the edge transfers of femasm_refine.hip,
// included after that; 105: the prepared cell state of femasm.hip, fa_prepare_cells .. fa_gather_rows_prepared;
// 106: the exterior-facet loads of femasm_facet.hip; 107: the scalar functionals of femasm_scalar.hip,
// included after it; 108: point location and evaluation, femasm_points.hip; 109: the smoothed-aggregation
// multigrid kernels of femasm_amg.hip; 110: the vertex-graph spread of femasm_graph.hip, included last); femasm.hip's own definition is compiled under another,
// hidden name.
#include "../../include/femasm.h"
#define fa_version __attribute__((visibility("hidden"))) fa_version_assembly
#include "femasm.hip"
#undef fa_version

extern "C" int fa_version(void) { return 110; }

// ------------------------------------------------------------------------------------ expressions
constexpr int EV_LIN = 0, EV_DAMAGE = 1, EV_NEO = 2;
constexpr int kEvalStagedRow = 16;    // doubles per cell and quantity the staged store takes
constexpr int kEvalStagedTotal = 24;  // doubles per cell over all quantities (LDS: 4 waves x 64 x 24 x 8 = 48 KiB)

// Reduced (symmetric) components of a GD x GD tensor in row-major upper-triangle order:
// 2-D (xx, xy, yy), 3-D (xx, xy, xz, yy, yz, zz).
template <int GD>
__device__ __forceinline__ void eval_reduce(const double (&t)[GD][GD], double (&r)[GD * (GD + 1) / 2]) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < GD; ++i)
#pragma unroll
    for (int j = i; j < GD; ++j) r[k++] = t[i][j];
}

__device__ __forceinline__ void eval_store(double* p, double v) { *reinterpret_cast<volatile double*>(p) = v; }

// A wave's run of `len` doubles from wave-private LDS to `g` with 16 B per lane. `g` is only 8-B
// aligned and `len` may be odd (value sizes 1 and 3): an 8-B head brings the run to a 16-B boundary,
// an 8-B tail ends it.
__device__ __forceinline__ void eval_drain(const double* s, double* g, int len, int lane) {
  const int head = (int)((reinterpret_cast<uintptr_t>(g) >> 3) & 1u);
  if (lane == 0 && head) g[0] = s[0];
  const int npair = (len - head) >> 1;
  for (int t = lane; t < npair; t += 64) {
    fa_dv2 w;
    w.x = s[head + 2 * t];
    w.y = s[head + 2 * t + 1];
    *reinterpret_cast<fa_dv2*>(g + head + 2 * t) = w;
    store_guard1(w);  // the next pass's LDS reads return into these registers
  }
  if (lane == 0 && ((len - head) & 1)) g[len - 1] = s[len - 1];
}

// One lane per output cell (position k holds cell cells[k]), looping over the npts points. The
// tables at the points, tab = dphi[npts][nn][GD] | gdphi[npts][NV][GD] | phi[npts][nn], are indexed
// by wave-uniform values only (scalar loads). Requested outputs (out_* non-NULL), each
// [n][npts][value size]: grad u (row-major), reduced strain, the law's stress at w = 1 (reduced
// Cauchy stress; EV_NEO: first Piola stress, row-major) and energy = eps : sigma.
// STAGED (npts x value size <= 16 for every requested quantity, which covers every DG0 case): as
// k_cell_records_staged, a wave's 64 cells are one contiguous run of each output; the lanes write
// their values to wave-private LDS (quantity i's rows at 64 * off_i) and the wave stores each run
// with 16 B per lane. Otherwise the slow path: every lane stores its own values.
template <int GD, int NV, int LAW, bool STAGED>
__global__ __launch_bounds__(256) void k_eval_cells(MeshView M, FormView F, const double* __restrict__ tab,
                                                    const int32_t* __restrict__ cells, int64_t n, int npts,
                                                    double* __restrict__ out_grad, double* __restrict__ out_strain,
                                                    double* __restrict__ out_stress, double* __restrict__ out_energy) {
  constexpr int VG = GD * GD, VS = GD * (GD + 1) / 2, VT = LAW == EV_NEO ? VG : VS;
  extern __shared__ __attribute__((aligned(16))) double ev_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nn = M.nn;
  const double* __restrict__ t_dphi = tab;
  const double* __restrict__ t_gdphi = t_dphi + (size_t)npts * nn * GD;
  const double* __restrict__ t_phi = t_gdphi + (size_t)npts * NV * GD;
  // row lengths and LDS row offsets of the requested quantities
  const int rl_g = out_grad ? npts * VG : 0, rl_s = out_strain ? npts * VS : 0;
  const int rl_t = out_stress ? npts * VT : 0, rl_e = out_energy ? npts : 0;
  const int of_s = rl_g, of_t = of_s + rl_s, of_e = of_t + rl_t, total = of_e + rl_e;
  double* sb = ev_lds + (STAGED ? (size_t)wave * 64 * total : 0);
  for (int64_t kb = (int64_t)blockIdx.x * 256 + wave * 64; kb < n; kb += (int64_t)gridDim.x * 256) {
    const int64_t k = kb + lane;
    const bool valid = k < n;
    const int64_t kk = valid ? k : n - 1;
    const int64_t c = cells ? (int64_t)cells[kk] : kk;
    const int32_t* cn = M.cells + c * nn;
    double lam, mu;
    cell_lame(F, c, lam, mu);
    double Ji[GD][GD];
    [[maybe_unused]] double xv[NV][GD];
    if constexpr (NV == GD + 1) {
      simplex_geometry<GD>(M, c, Ji);  // affine: one Jacobian per cell
    } else {
      const int32_t* gv = M.geom + c * NV;
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int i = 0; i < GD; ++i) xv[v][i] = M.x[(int64_t)gv[v] * GD + i];
    }
    for (int q = 0; q < npts; ++q) {
      if constexpr (NV != GD + 1) tensor_geometry<GD, NV>(xv, t_gdphi + (size_t)q * NV * GD, Ji);
      // reference gradient R[i][k] = sum_a u_a[i] dphi_a[k], then grad u = R Ji
      double R[GD][GD];
#pragma unroll
      for (int i = 0; i < GD; ++i)
#pragma unroll
        for (int j = 0; j < GD; ++j) R[i][j] = 0.0;
      [[maybe_unused]] double dq = 0.0;
      const double* dp = t_dphi + (size_t)q * nn * GD;
      for (int a = 0; a < nn; ++a) {
        const int64_t nd = cn[a];
#pragma unroll
        for (int i = 0; i < GD; ++i) {
          const double ui = F.u[nd * GD + i];
#pragma unroll
          for (int j = 0; j < GD; ++j) R[i][j] += ui * dp[a * GD + j];
        }
        if constexpr (LAW == EV_DAMAGE)
          if (F.d) dq += t_phi[(size_t)q * nn + a] * F.d[nd];
      }
      double gu[GD][GD];
#pragma unroll
      for (int i = 0; i < GD; ++i)
#pragma unroll
        for (int j = 0; j < GD; ++j) {
          double s = 0.0;
#pragma unroll
          for (int l = 0; l < GD; ++l) s += R[i][l] * Ji[l][j];
          gu[i][j] = s;
        }
      double eps[GD][GD];
#pragma unroll
      for (int i = 0; i < GD; ++i)
#pragma unroll
        for (int j = 0; j < GD; ++j) eps[i][j] = i == j ? gu[i][i] : 0.5 * (gu[i][j] + gu[j][i]);
      double vg[VG], vs[VS], vt[VT], ve[1];
#pragma unroll
      for (int i = 0; i < GD; ++i)
#pragma unroll
        for (int j = 0; j < GD; ++j) vg[i * GD + j] = gu[i][j];
      eval_reduce<GD>(eps, vs);
      ve[0] = 0.0;
      if (out_stress || out_energy) {
        if constexpr (LAW == EV_NEO) {
          double Fq[VG];
#pragma unroll
          for (int i = 0; i < GD; ++i)
#pragma unroll
            for (int j = 0; j < GD; ++j) Fq[i * GD + j] = gu[i][j] + (i == j ? 1.0 : 0.0);
          neo_stress_ad<GD>(Fq, lam, mu, vt);
        } else {
          double sig[GD][GD];
          if constexpr (LAW == EV_DAMAGE) {
            if (F.ad) damage_stress_ad(eps[0][0], eps[1][1], eps[0][1], lam, mu, dq, 1.0, sig);
            else damage_stress(eps[0][0], eps[1][1], eps[0][1], lam, mu, dq, 1.0, sig);
          } else {
            double tr = 0.0;
#pragma unroll
            for (int i = 0; i < GD; ++i) tr += gu[i][i];
#pragma unroll
            for (int i = 0; i < GD; ++i)
#pragma unroll
              for (int j = 0; j < GD; ++j) sig[i][j] = 2.0 * mu * eps[i][j] + (i == j ? lam * tr : 0.0);
          }
          eval_reduce<GD>(sig, vt);
          double e = 0.0;
#pragma unroll
          for (int i = 0; i < GD; ++i)
#pragma unroll
            for (int j = 0; j < GD; ++j) e += eps[i][j] * sig[i][j];
          ve[0] = e;
        }
      }
      if constexpr (STAGED) {
        if (out_grad)
#pragma unroll
          for (int j = 0; j < VG; ++j) sb[lane * rl_g + q * VG + j] = vg[j];
        if (out_strain)
#pragma unroll
          for (int j = 0; j < VS; ++j) sb[64 * of_s + lane * rl_s + q * VS + j] = vs[j];
        if (out_stress)
#pragma unroll
          for (int j = 0; j < VT; ++j) sb[64 * of_t + lane * rl_t + q * VT + j] = vt[j];
        if (out_energy) sb[64 * of_e + lane * rl_e + q] = ve[0];
      } else if (valid) {
        // the slow path: a lane's stores touch one cache line per lane and instruction. 8-B stores
        // through a volatile pointer: merged into 16-B ones they would be subject to the store-data
        // hazard (the next value's arithmetic rewrites their data registers)
        const int64_t r = k * npts + q;
        if (out_grad)
#pragma unroll
          for (int j = 0; j < VG; ++j) eval_store(out_grad + r * VG + j, vg[j]);
        if (out_strain)
#pragma unroll
          for (int j = 0; j < VS; ++j) eval_store(out_strain + r * VS + j, vs[j]);
        if (out_stress)
#pragma unroll
          for (int j = 0; j < VT; ++j) eval_store(out_stress + r * VT + j, vt[j]);
        if (out_energy) eval_store(out_energy + r, ve[0]);
      }
    }
    if constexpr (STAGED) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int cnt = (int)min<int64_t>(64, n - kb);
      if (out_grad) eval_drain(sb, out_grad + kb * rl_g, cnt * rl_g, lane);
      if (out_strain) eval_drain(sb + 64 * of_s, out_strain + kb * rl_s, cnt * rl_s, lane);
      if (out_stress) eval_drain(sb + 64 * of_t, out_stress + kb * rl_t, cnt * rl_t, lane);
      if (out_energy) eval_drain(sb + 64 * of_e, out_energy + kb * rl_e, cnt * rl_e, lane);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

// Tables at the default (DG0 interpolation) point, cached per (device, cell, degree) like g_tabs: a
// steady-state call at that point allocates and copies nothing.
static std::mutex g_eval_mu;
static std::map<std::tuple<int, int, int>, const double*> g_eval_tabs;

static void eval_host_tables(int ct, int p, int npts, const double* X, std::vector<double>& h) {
  Quadrature Q;
  Q.tdim = cell_tdim(ct);
  Q.pts.assign(X, X + (size_t)npts * Q.tdim);
  Q.wts.assign(npts, 0.0);
  std::vector<double> phi, dphi, gphi, gdphi;
  tabulate(ct, p, Q, phi, dphi);
  tabulate(ct, 1, Q, gphi, gdphi);
  h.clear();
  h.insert(h.end(), dphi.begin(), dphi.end());
  h.insert(h.end(), gdphi.begin(), gdphi.end());
  h.insert(h.end(), phi.begin(), phi.end());
}

static bool eval_default_point(int ct, int npts, const double* X) {
  if (npts != 1) return false;
  const int td = cell_tdim(ct);
  const double m = is_simplex(ct) ? 1.0 / (td + 1) : 0.5;
  for (int d = 0; d < td; ++d)
    if (X[d] != m) return false;
  return true;
}

template <int GD, int NV, int LAW>
static int launch_eval(bool staged, size_t lds, int grid, hipStream_t s, const MeshView& M, const FormView& F,
                       const double* tab, const int32_t* cells, int64_t n, int npts, double* grad, double* strain,
                       double* stress, double* energy) {
  if (staged) k_eval_cells<GD, NV, LAW, true><<<grid, 256, lds, s>>>(M, F, tab, cells, n, npts, grad, strain, stress, energy);
  else k_eval_cells<GD, NV, LAW, false><<<grid, 256, 0, s>>>(M, F, tab, cells, n, npts, grad, strain, stress, energy);
  LAUNCH_CHECK();
  return FA_OK;
}

extern "C" int fa_eval_cells(const fa_mesh* mesh, const fa_form* form, int32_t npts, const double* X,
                             const int32_t* cells, int64_t ncells_out, double* grad, double* strain, double* stress,
                             double* energy, void* stream) {
  int rc = check_mesh(mesh);
  if (rc) return rc;
  FormView F;
  if ((rc = form_view(mesh, form, F))) return rc;
  if (!F.u) return fail(FA_E_ARG, "fa_eval_cells needs the state u (form->u is NULL)");
  if (npts < 1 || !X) return fail(FA_E_ARG, "fa_eval_cells needs npts >= 1 reference points X");
  if (ncells_out < 0 || (!cells && ncells_out > mesh->ncells))
    return fail(FA_E_ARG, "ncells_out %lld outside [0, ncells = %lld]", (long long)ncells_out, (long long)mesh->ncells);
  const int flags = (grad ? FA_EVAL_GRAD : 0) | (strain ? FA_EVAL_STRAIN : 0) | (stress ? FA_EVAL_STRESS : 0) |
                    (energy ? FA_EVAL_ENERGY : 0);
  if (!flags) return fail(FA_E_ARG, "fa_eval_cells: no output requested");
  const int law = F.kind == FA_NEO_HOOKEAN ? EV_NEO : F.kind == FA_ASYM_DAMAGE ? EV_DAMAGE : EV_LIN;
  if (law == EV_NEO && (flags & FA_EVAL_ENERGY))
    return fail(FA_E_UNSUPPORTED, "FA_EVAL_ENERGY is inner(eps, sigma) of the small-strain laws: not defined for FA_NEO_HOOKEAN");
  if (ncells_out == 0) return FA_OK;
  const int ct = mesh->cell_type, gd = mesh->gdim;
  const int vg = gd * gd, vs = gd * (gd + 1) / 2, vt = law == EV_NEO ? vg : vs;
  if ((int64_t)npts * vg >= (1 << 20)) return fail(FA_E_CAPACITY, "npts %d too large", npts);
  hipStream_t s = (hipStream_t)stream;
  // tables at X: cached for the default point, else uploaded for this call (the upload waits for
  // the stream: the host copy must not outlive this call)
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  const double* tab = nullptr;
  double* tmp = nullptr;
  if (eval_default_point(ct, npts, X)) {
    std::lock_guard<std::mutex> lock(g_eval_mu);
    auto key = std::make_tuple(dev, ct, (int)mesh->degree);
    auto it = g_eval_tabs.find(key);
    if (it == g_eval_tabs.end()) {
      std::vector<double> h;
      eval_host_tables(ct, mesh->degree, npts, X, h);
      double* d = nullptr;
      HIP_TRY(hipMalloc(&d, h.size() * sizeof(double)));
      HIP_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
      it = g_eval_tabs.emplace(key, d).first;
    }
    tab = it->second;
  } else {
    std::vector<double> h;
    eval_host_tables(ct, mesh->degree, npts, X, h);
    if ((rc = scratch_alloc((void**)&tmp, h.size() * sizeof(double), s))) return rc;
    HIP_TRY(hipMemcpyWithStream(tmp, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, s));
    tab = tmp;
  }
  const int rows[4] = {grad ? npts * vg : 0, strain ? npts * vs : 0, stress ? npts * vt : 0, energy ? npts : 0};
  const int total = rows[0] + rows[1] + rows[2] + rows[3];
  const bool staged = *std::max_element(rows, rows + 4) <= kEvalStagedRow && total <= kEvalStagedTotal;
  const size_t lds = staged ? (size_t)4 * 64 * total * sizeof(double) : 0;
  const int grid = grid_for(ncells_out);
  MeshView M{mesh->cells, mesh->geom, mesh->x, mesh->ncells, mesh->nnodes, mesh->nn, mesh->nv, mesh->gdim};
#define EV(GD_, NV_, LAW_) \
  rc = launch_eval<GD_, NV_, LAW_>(staged, lds, grid, s, M, F, tab, cells, ncells_out, npts, grad, strain, stress, energy)
  switch (ct) {
    case FA_TRIANGLE:
      if (law == EV_DAMAGE) EV(2, 3, EV_DAMAGE);
      else if (law == EV_NEO) EV(2, 3, EV_NEO);
      else EV(2, 3, EV_LIN);
      break;
    case FA_QUADRILATERAL:
      if (law == EV_NEO) EV(2, 4, EV_NEO);
      else EV(2, 4, EV_LIN);
      break;
    case FA_TETRAHEDRON:
      if (law == EV_NEO) EV(3, 4, EV_NEO);
      else EV(3, 4, EV_LIN);
      break;
    case FA_HEXAHEDRON:
      if (law == EV_NEO) EV(3, 8, EV_NEO);
      else EV(3, 8, EV_LIN);
      break;
  }
#undef EV
  if (tmp) HIP_TRY(hipFreeAsync(tmp, s));
  return rc;
}

// ------------------------------------------------------------------------------------ matrix-free Jacobian action
#include "femasm_apply.hip"

// ------------------------------------------------------------------------------------ geometric multigrid
#include "femasm_mg.hip"

// ------------------------------------------------------------------------------------ refinement, edge transfers
#include "femasm_refine.hip"

// ------------------------------------------------------------------------------------ exterior-facet loads
#include "femasm_facet.hip"

// ------------------------------------------------------------------------------------ scalar functionals
#include "femasm_scalar.hip"

// ------------------------------------------------------------------------------------ point location, evaluation
#include "femasm_points.hip"

// ------------------------------------------------------------------------------------ algebraic multigrid
#include "femasm_amg.hip"

// ------------------------------------------------------------------------------------ vertex graph: damage spread
#include "femasm_graph.hip"
