// femasm — matrix-free Jacobian action, included by femasm_eval.hip (the library's translation unit)
// after its own content: y = J(u) x and the diagonal blocks of J(u) with no assembled matrix, from the
// device laws, element tables and geometry of femasm.hip (used here, not copied).
//
//   fa_apply_jacobian      y = A x, A = the matrix fa_assemble_matrix would hold at form->u
//   fa_jacobian_block_diag the block-Jacobi preconditioner of that A
//   fa_apply_plan(_bytes)  the apply plan of the planned kernel (P1/P2 triangles and tetrahedra)
//
// Two kernels compute the action. k_apply_generic is node-parallel through the adjacency (the shape
// of k_vector): every cell type and degree, affine or not; a cell's gradients are recomputed once
// per node of the cell. k_apply_planned removes that redundancy: one workgroup per chunk of
// consecutive rows; phase 1 computes y_e = K_e(u) x_e once per distinct cell of the chunk (one lane
// per cell) into an LDS tile, phase 2 sums each row's entries from the tile in adjacency order.
// Both are deterministic: no atomics, every dof written exactly once.

// ------------------------------------------------------------------------------------ shared device code
constexpr int kApplyTile = 256;    // distinct cells per chunk: phase-1 lanes of a workgroup, 8-bit tile slots
constexpr int kApplySeg = 2048;    // rows per planning segment (a chunk never crosses a segment)
constexpr int kApplyGrid = 2048;   // workgroups of the planned launch (256 CUs x 8), looping over the chunks
constexpr int kApplyMaxNN = 10;    // nodes per cell of the planned elements (P2 tetrahedron)
constexpr int64_t kApplyMagic = 0x66615f6170706c00ll;  // "fa_appl\0"; the header adds nn

// x_j seen by the cells: constrained columns contribute nothing
__device__ __forceinline__ double apply_col(const double* __restrict__ x, const int8_t* __restrict__ bc, int64_t dof) {
  const double v = x[dof];
  return (bc && bc[dof]) ? 0.0 : v;
}

// dP[(iJ)] = sum_(kL) d2 psi / dF_iJ dF_kL H_kL: the neo-Hookean AD tangent contracted with H, in the
// form the assembly uses (neo_energy_coeffs: forward-over-forward AD of W(I1, J), then the closed
// contraction with F and C = cof F), without forming the GD^2 x GD^2 tangent:
//   dP = (co0 F:H + co1 C:H) F + (co1 F:H + co2 C:H) C + co4 H - co3 C H^T C.
template <int GD>
__device__ __forceinline__ void neo_tangent_dir(const double (&Fq)[GD * GD], const double (&H)[GD * GD], double lam,
                                                double mu, double (&dP)[GD * GD]) {
  constexpr int N = GD * GD;
  double I1 = GD == 2 ? 1.0 : 0.0, J;
#pragma unroll
  for (int m = 0; m < N; ++m) I1 = fma(Fq[m], Fq[m], I1);
  if constexpr (GD == 2) J = Fq[0] * Fq[3] - Fq[1] * Fq[2];
  else J = Fq[0] * (Fq[4] * Fq[8] - Fq[5] * Fq[7]) - Fq[1] * (Fq[3] * Fq[8] - Fq[5] * Fq[6]) +
           Fq[2] * (Fq[3] * Fq[7] - Fq[4] * Fq[6]);
  double co[5], C[GD][GD];
  neo_energy_coeffs(I1, J, lam, mu, co);
  cofactor<GD>(Fq, C);
  double fh = 0.0, ch = 0.0;
#pragma unroll
  for (int i = 0; i < GD; ++i)
#pragma unroll
    for (int k = 0; k < GD; ++k) {
      fh += Fq[i * GD + k] * H[i * GD + k];
      ch += C[i][k] * H[i * GD + k];
    }
  const double cf = co[0] * fh + co[1] * ch, cc = co[1] * fh + co[2] * ch;
  double HtC[GD][GD];  // (H^T C)[L][j] = sum_k H[k][L] C[k][j]
#pragma unroll
  for (int l = 0; l < GD; ++l)
#pragma unroll
    for (int j = 0; j < GD; ++j) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < GD; ++k) t += H[k * GD + l] * C[k][j];
      HtC[l][j] = t;
    }
#pragma unroll
  for (int i = 0; i < GD; ++i)
#pragma unroll
    for (int j = 0; j < GD; ++j) {
      double t = 0.0;
#pragma unroll
      for (int l = 0; l < GD; ++l) t += C[i][l] * HtC[l][j];
      dP[i * GD + j] = cf * Fq[i * GD + j] + cc * C[i][j] + co[4] * H[i * GD + j] - co[3] * t;
    }
}

// sigma(H) of the Lame law for a displacement gradient H (row-major)
template <int GD>
__device__ __forceinline__ void lin_stress_dir(const double (&H)[GD * GD], double lam, double mu, double (&S)[GD * GD]) {
  double tr = H[0];
#pragma unroll
  for (int i = 1; i < GD; ++i) tr += H[i * GD + i];
#pragma unroll
  for (int i = 0; i < GD; ++i)
#pragma unroll
    for (int k = 0; k < GD; ++k) S[i * GD + k] = mu * (H[i * GD + k] + H[k * GD + i]) + (i == k ? lam * tr : 0.0);
}

// damage_cell with the AD hook taken inline: damage_hook_ad is a call (its 3 x 3 result would live in
// scratch); here its ten hyper-dual passes are unrolled, same operations in the same order, so H is
// the tangent damage_cell gives and the kernels below use no scratch.
__device__ __forceinline__ void apply_damage_cell(const MeshView& M, const FormView& F, int64_t c, double (&g)[3][2],
                                                  double& w, double (&H)[3][3]) {
  if (!F.ad) {
    damage_cell(M, F, c, g, w, H);
    return;
  }
  FormView Fh = F;
  Fh.ad = 0;
  Fh.d = nullptr;  // geometry and weight only: the hand hook's linear branch, overwritten below
  damage_cell(M, Fh, c, g, w, H);
  double l, m;
  cell_lame(F, c, l, m);
  const int32_t* nd = M.cells + c * 3;
  double gr[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, d = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int64_t n = nd[a];
    const double u0 = F.u ? F.u[n * 2 + 0] : 0.0, u1 = F.u ? F.u[n * 2 + 1] : 0.0;
    gr[0][0] += u0 * g[a][0]; gr[0][1] += u0 * g[a][1];
    gr[1][0] += u1 * g[a][0]; gr[1][1] += u1 * g[a][1];
    if (F.d) d += F.d[n];
  }
  d *= (1.0 / 3.0);
  if (!(d > 0.0)) return;  // H is the linear hook already
  d = fmin(d, 1.0 - 1.e-12);
  const double s01 = 0.5 * (gr[0][1] + gr[1][0]);
  const double st[4] = {gr[0][0], s01, s01, gr[1][1]};
  using DD = Dual<Dual<double>>;
  double hs[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      DD xx[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) xx[k] = DD{{st[k], k == i ? 1.0 : 0.0}, {k == j ? 1.0 : 0.0, 0.0}};
      const double h = damage_potential<DD>(xx, l, m, d).d.d;
      hs[i][j] = h;
      hs[j][i] = h;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) H[i][j] = hs[i + 2 * (i % 2)][j + 2 * (j % 2)];
  H[2][2] = 0.5 * (H[2][2] + hs[1][2]);
}

// ------------------------------------------------------------------------------------ generic kernel
// One thread per node a: y_a = sum over the cells of a of sum_q w_q |J| C(u)[grad x] g_a, with
// grad x = sum_b x_b (x) g_b over free columns. Constrained rows: y = diag * x.
template <int GD, int NV, int MAT>
__global__ __launch_bounds__(256) void k_apply_generic(MeshView M, FormView F, DevTables T,
                                                       const int64_t* __restrict__ adj_ptr,
                                                       const int32_t* __restrict__ adj_idx,
                                                       const int8_t* __restrict__ bc, double diag,
                                                       const double* __restrict__ x, double* __restrict__ y) {
  const int nn = M.nn;
  for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a < M.nnodes; a += (int64_t)gridDim.x * blockDim.x) {
    double r[GD];
#pragma unroll
    for (int i = 0; i < GD; ++i) r[i] = 0.0;
    for (int64_t j = adj_ptr[a]; j < adj_ptr[a + 1]; ++j) {
      const int32_t p = adj_idx[j];
      const int64_t c = p / nn;
      const int aloc = p % nn;
      const int32_t* cn = M.cells + c * nn;
      if constexpr (MAT == FA_ASYM_DAMAGE) {
        if constexpr (GD == 2) {
          double g[3][2], w, H[3][3];
          apply_damage_cell(M, F, c, g, w, H);
          double e[3] = {0.0, 0.0, 0.0};  // B x: (xx, yy, engineering xy)
#pragma unroll
          for (int bb = 0; bb < 3; ++bb) {
            const int64_t n = cn[bb];
            const double x0 = apply_col(x, bc, n * 2), x1 = apply_col(x, bc, n * 2 + 1);
            e[0] += x0 * g[bb][0];
            e[1] += x1 * g[bb][1];
            e[2] += x0 * g[bb][1] + x1 * g[bb][0];
          }
          double s[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) s[k] = H[k][0] * e[0] + H[k][1] * e[1] + H[k][2] * e[2];
          r[0] += w * (g[aloc][0] * s[0] + g[aloc][1] * s[2]);
          r[1] += w * (g[aloc][1] * s[1] + g[aloc][0] * s[2]);
        }
      } else {
        double lam, mu;
        cell_lame(F, c, lam, mu);
        const bool neo = F.kind == FA_NEO_HOOKEAN;
        for (int q = 0; q < T.nq; ++q) {
          double Ji[GD][GD];
          const double wd = T.wq[q] * cell_geometry_q<GD, NV>(M, c, T.gdphi + (size_t)q * NV * GD, Ji);
          double gx[GD * GD], gu[GD * GD], ga[GD];
#pragma unroll
          for (int i = 0; i < GD * GD; ++i) gx[i] = gu[i] = 0.0;
#pragma unroll
          for (int k = 0; k < GD; ++k) ga[k] = 0.0;
          for (int bb = 0; bb < nn; ++bb) {
            double gb[GD];
            phys_grad<GD>(T.dphi + ((size_t)q * nn + bb) * GD, Ji, gb);
            if (bb == aloc)
#pragma unroll
              for (int k = 0; k < GD; ++k) ga[k] = gb[k];
            const int64_t n = cn[bb];
#pragma unroll
            for (int i = 0; i < GD; ++i) {
              const double xi = apply_col(x, bc, n * GD + i);
#pragma unroll
              for (int k = 0; k < GD; ++k) gx[i * GD + k] += xi * gb[k];
              if (neo) {
                const double ui = F.u[n * GD + i];
#pragma unroll
                for (int k = 0; k < GD; ++k) gu[i * GD + k] += ui * gb[k];
              }
            }
          }
          double S[GD * GD];
          if (neo) {
#pragma unroll
            for (int i = 0; i < GD; ++i) gu[i * GD + i] += 1.0;  // F = I + grad u
            neo_tangent_dir<GD>(gu, gx, lam, mu, S);
          } else {
            lin_stress_dir<GD>(gx, lam, mu, S);
          }
#pragma unroll
          for (int i = 0; i < GD; ++i) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < GD; ++k) s += S[i * GD + k] * ga[k];
            r[i] += wd * s;
          }
        }
      }
    }
    double o[GD];
#pragma unroll
    for (int i = 0; i < GD; ++i) {
      const double xi = x[a * GD + i];
      o[i] = (bc && bc[a * GD + i]) ? diag * xi : r[i];
    }
#pragma unroll
    for (int i = 0; i < GD; ++i) y[a * GD + i] = o[i];
    store_fence(o);  // the grid-stride loop's next node would rewrite the store's data registers
  }
}

// ------------------------------------------------------------------------------------ block diagonal
// out[a] = sum over the cells of a of K_e[a, a], bc rows / columns of the block zeroed, `diag` on
// constrained diagonal entries: k_lifting's block computation with the column node fixed to the row
// node. The neo-Hookean block is taken column by column with neo_tangent_dir (direction e_k (x) g_a):
// no GD^2 x GD^2 tangent array, no scratch.
template <int GD, int NV, int MAT>
__global__ __launch_bounds__(256) void k_apply_block_diag(MeshView M, FormView F, DevTables T,
                                                          const int64_t* __restrict__ adj_ptr,
                                                          const int32_t* __restrict__ adj_idx,
                                                          const int8_t* __restrict__ bc, double diag,
                                                          double* __restrict__ out) {
  const int nn = M.nn;
  for (int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; a < M.nnodes; a += (int64_t)gridDim.x * blockDim.x) {
    double D[GD][GD];
#pragma unroll
    for (int i = 0; i < GD; ++i)
#pragma unroll
      for (int k = 0; k < GD; ++k) D[i][k] = 0.0;
    for (int64_t j = adj_ptr[a]; j < adj_ptr[a + 1]; ++j) {
      const int32_t p = adj_idx[j];
      const int64_t c = p / nn;
      const int aloc = p % nn;
      double K[GD][GD];
      if constexpr (MAT == FA_ASYM_DAMAGE) {
        if constexpr (GD == 2) {
          double gg[3][2], w, H[3][3];
          apply_damage_cell(M, F, c, gg, w, H);
          const double ga[2] = {gg[aloc][0], gg[aloc][1]};
          damage_block(ga, ga, w, H, K);
        }
      } else {
        double lam, mu;
        cell_lame(F, c, lam, mu);
        const bool neo = F.kind == FA_NEO_HOOKEAN;
        double G[GD][GD];
#pragma unroll
        for (int i = 0; i < GD; ++i)
#pragma unroll
          for (int k = 0; k < GD; ++k) G[i][k] = K[i][k] = 0.0;
        for (int q = 0; q < T.nq; ++q) {
          double Ji[GD][GD];
          const double wd = T.wq[q] * cell_geometry_q<GD, NV>(M, c, T.gdphi + (size_t)q * NV * GD, Ji);
          double ga[GD];
          phys_grad<GD>(T.dphi + ((size_t)q * nn + aloc) * GD, Ji, ga);
          if (neo) {
            double Fq[GD * GD];
            deformation_gradient<GD>(F.u, M.cells + c * nn, nn, T.dphi + (size_t)q * nn * GD, Ji, Fq);
#pragma unroll
            for (int k = 0; k < GD; ++k) {
              double H[GD * GD], dP[GD * GD];
#pragma unroll
              for (int m = 0; m < GD * GD; ++m) H[m] = (m / GD == k) ? ga[m % GD] : 0.0;
              neo_tangent_dir<GD>(Fq, H, lam, mu, dP);
#pragma unroll
              for (int i = 0; i < GD; ++i) {
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < GD; ++l) s += dP[i * GD + l] * ga[l];
                K[i][k] += wd * s;
              }
            }
          } else {
#pragma unroll
            for (int i = 0; i < GD; ++i)
#pragma unroll
              for (int k = 0; k < GD; ++k) G[i][k] += wd * ga[i] * ga[k];
          }
        }
        if (!neo) lin_block<GD>(G, lam, mu, K);
      }
#pragma unroll
      for (int i = 0; i < GD; ++i)
#pragma unroll
        for (int k = 0; k < GD; ++k) D[i][k] += K[i][k];
    }
    double o[GD][GD];
#pragma unroll
    for (int i = 0; i < GD; ++i) {
      const bool ri = bc && bc[a * GD + i];
#pragma unroll
      for (int k = 0; k < GD; ++k) {
        const bool ck = bc && bc[a * GD + k];
        o[i][k] = (ri || ck) ? ((i == k) ? diag : 0.0) : D[i][k];
      }
    }
#pragma unroll
    for (int i = 0; i < GD; ++i)
#pragma unroll
      for (int k = 0; k < GD; ++k) out[(a * GD + i) * GD + k] = o[i][k];
    store_fence(o);  // (as k_vector)
  }
}

// ------------------------------------------------------------------------------------ apply plan
// Plan buffer (device, 8-B aligned), for nch chunks, V cell visits and E = ncells * nn adjacency entries:
//   int64 header[4] = {kApplyMagic + nn, nch, E, V}
//   int64 row_start[nch + 1]   rows of chunk k: [row_start[k], row_start[k + 1])
//   int64 cell_off[nch + 1]    its distinct cells: cells[cell_off[k] .. cell_off[k + 1]), at most kApplyTile
//   int32 cells[V]  (padded to 8 B)   in order of first appearance along the chunk's adjacency entries
//   uint16 pos[E]   (padded to 8 B)   per adjacency entry: tile slot of its cell | local node << 8
// 32 + 16 (nch + 1) + 4 V + 2 E (+ padding) bytes; V <= E (a visited cell holds a row of the chunk), so
// at most 6 B per entry + 16 B per chunk + 64.
// A cell is NEW at row r of a chunk starting at row f when none of its nodes lies in [f, r): a test
// on the dofmap alone, so the cut kernel (sequential per segment) and the fill kernel (parallel per
// chunk) agree on every chunk's cell list without sharing state.
struct ApplyPlanLayout {
  int64_t off_rows, off_coff, off_cells, off_pos, bytes;
};
static ApplyPlanLayout apply_plan_layout(int64_t nch, int64_t visits, int64_t entries) {
  ApplyPlanLayout Lo;
  Lo.off_rows = 32;
  Lo.off_coff = Lo.off_rows + 8 * (nch + 1);
  Lo.off_cells = Lo.off_coff + 8 * (nch + 1);
  Lo.off_pos = Lo.off_cells + ((4 * visits + 7) & ~int64_t(7));
  Lo.bytes = Lo.off_pos + ((2 * entries + 7) & ~int64_t(7));
  return Lo;
}

__device__ __forceinline__ bool apply_cell_new(const int32_t* __restrict__ cn, int nn, int64_t f, int64_t r) {
  bool isnew = true;
  for (int b = 0; b < nn; ++b) {
    const int64_t n = cn[b];
    isnew &= !(n >= f && n < r);
  }
  return isnew;
}

// One thread per segment of kApplySeg rows, greedy: a chunk is closed before the row whose new cells
// would overflow the tile. PASS 0 counts: seg[2 s] = chunks, seg[2 s + 1] = cell visits of segment s,
// *maxval = the largest valence met. PASS 1 (seg = exclusive scans of those) writes row_start / cell_off.
template <int PASS>
__global__ __launch_bounds__(64) void k_apply_cut(const int32_t* __restrict__ cells, int nn, int64_t nnodes,
                                                  const int64_t* __restrict__ adj_ptr,
                                                  const int32_t* __restrict__ adj_idx, int64_t nseg,
                                                  int64_t* __restrict__ seg, int* __restrict__ maxval,
                                                  int64_t* __restrict__ row_start, int64_t* __restrict__ cell_off) {
  const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  const int64_t rb = s * kApplySeg, re = min(nnodes, rb + kApplySeg);
  int64_t f = rb, nch = 0, vis = 0;
  int cur = 0, mv = 0;
  [[maybe_unused]] int64_t kb = 0, vb = 0;
  if constexpr (PASS == 1) {
    kb = seg[2 * s];
    vb = seg[2 * s + 1];
    row_start[kb] = rb;
    cell_off[kb] = vb;
  }
  for (int64_t r = rb; r < re; ++r) {
    const int64_t j0 = adj_ptr[r], j1 = adj_ptr[r + 1];
    const int val = (int)min<int64_t>(j1 - j0, INT32_MAX);
    mv = max(mv, val);
    int nw = 0;
    for (int64_t j = j0; j < j1; ++j) nw += apply_cell_new(cells + (int64_t)(adj_idx[j] / nn) * nn, nn, f, r) ? 1 : 0;
    if (cur + nw > kApplyTile) {  // close [f, r); every cell of r is new to the chunk that starts at r
      ++nch;
      vis += cur;
      f = r;
      cur = val;
      if constexpr (PASS == 1) {
        row_start[kb + nch] = r;
        cell_off[kb + nch] = vb + vis;
      }
    } else {
      cur += nw;
    }
  }
  ++nch;
  vis += cur;
  if constexpr (PASS == 0) {
    seg[2 * s] = nch;
    seg[2 * s + 1] = vis;
    if (mv > kApplyTile) atomicMax(maxval, mv);
  } else if (s == nseg - 1) {
    row_start[kb + nch] = nnodes;
    cell_off[kb + nch] = vb + vis;
  }
}

// One workgroup per chunk: the chunk's adjacency entries (at most kApplyTile * nn) in order; the new
// ones are ranked by a ballot scan (= tile slot, and the cell list), every other entry finds its
// cell's slot at the entry that introduced it (row = the cell's first node in the chunk; that row's
// adjacency is sorted by dofmap position: binary search).
__global__ __launch_bounds__(256) void k_apply_fill(const int32_t* __restrict__ cells, int nn,
                                                    const int64_t* __restrict__ adj_ptr,
                                                    const int32_t* __restrict__ adj_idx, int64_t nchunks,
                                                    const int64_t* __restrict__ row_start,
                                                    const int64_t* __restrict__ cell_off, int32_t* __restrict__ clist,
                                                    uint16_t* __restrict__ pos) {
  __shared__ uint16_t rank[kApplyTile * kApplyMaxNN];  // bit 15: the entry is new
  const int tid = threadIdx.x, lane = tid & 63;
  for (int64_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const int64_t r0 = row_start[k], r1 = row_start[k + 1];
    const int64_t e0 = adj_ptr[r0], c0 = cell_off[k], c1 = cell_off[k + 1];
    const int ne = (int)min<int64_t>(adj_ptr[r1] - e0, kApplyTile * kApplyMaxNN);
    for (int e = tid; e < ne; e += 256) {
      const int32_t p = adj_idx[e0 + e];
      rank[e] = apply_cell_new(cells + (int64_t)(p / nn) * nn, nn, r0, cells[p]) ? 0x8000 : 0;
    }
    __syncthreads();
    if (tid < 64) {
      int running = 0;
      for (int b = 0; b < ne; b += 64) {
        const bool nw = b + lane < ne && (rank[b + lane] & 0x8000);
        const uint64_t m = __ballot(nw);
        if (b + lane < ne) rank[b + lane] = (uint16_t)((nw ? 0x8000 : 0) | (running + __popcll(m & ((1ull << lane) - 1))));
        running += __popcll(m);
      }
    }
    __syncthreads();
    for (int e = tid; e < ne; e += 256) {
      const int32_t p = adj_idx[e0 + e];
      const int32_t c = p / nn;
      const int aloc = p - c * nn;
      int slot;
      if (rank[e] & 0x8000) {
        slot = rank[e] & 0x7FFF;
        if (c0 + slot < c1) clist[c0 + slot] = c;
      } else {
        // the cell's first node in the chunk, and the adjacency entry of that (node, cell)
        const int32_t* cn = cells + (int64_t)c * nn;
        int64_t rf = INT64_MAX;
        int bf = 0;
        for (int b = 0; b < nn; ++b) {
          const int64_t n = cn[b];
          if (n >= r0 && n < rf) {
            rf = n;
            bf = b;
          }
        }
        const int32_t want = c * nn + bf;
        int64_t lo = adj_ptr[rf], hi = adj_ptr[rf + 1] - 1;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (adj_idx[mid] < want) lo = mid + 1;
          else hi = mid;
        }
        const int64_t ef = min<int64_t>(max<int64_t>(lo - e0, 0), ne - 1);
        slot = rank[ef] & 0x7FFF;
      }
      pos[e0 + e] = (uint16_t)((slot & 0xFF) | (aloc << 8));
    }
    __syncthreads();
  }
}

static bool apply_plan_element(const fa_mesh* m) {
  return (m->cell_type == FA_TRIANGLE || m->cell_type == FA_TETRAHEDRON) && (m->degree == 1 || m->degree == 2);
}

// Cut pass 0 and its sums: nchunks, visits and (optionally) the per-segment counts on the host.
static int apply_plan_count(const fa_mesh* mesh, const fa_adjacency* adj, hipStream_t s, int64_t* nchunks,
                            int64_t* visits, std::vector<int64_t>* seg_out) {
  const int64_t nseg = (mesh->nnodes + kApplySeg - 1) / kApplySeg;
  *nchunks = *visits = 0;
  if (nseg == 0) return FA_OK;
  int64_t* seg = nullptr;
  int rc = scratch_alloc((void**)&seg, sizeof(int64_t) * (2 * nseg + 1), s);
  if (rc) return rc;
  int* maxval = reinterpret_cast<int*>(seg + 2 * nseg);
  HIP_TRY(hipMemsetAsync(maxval, 0, sizeof(int64_t), s));
  k_apply_cut<0><<<grid_for(nseg, 64), 64, 0, s>>>(mesh->cells, mesh->nn, mesh->nnodes, adj->ptr, adj->idx, nseg, seg,
                                                  maxval, nullptr, nullptr);
  LAUNCH_CHECK();
  std::vector<int64_t> h(2 * nseg + 1);
  HIP_TRY(hipMemcpyAsync(h.data(), seg, sizeof(int64_t) * h.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipFreeAsync(seg, s));
  int mv = 0;
  std::memcpy(&mv, &h[2 * nseg], sizeof(int));
  if (mv > kApplyTile)
    return fail(FA_E_CAPACITY, "apply plan: a node has %d cells, more than the %d-cell tile of a chunk (use the generic kernel)",
                mv, kApplyTile);
  for (int64_t i = 0; i < nseg; ++i) {
    *nchunks += h[2 * i];
    *visits += h[2 * i + 1];
  }
  if (seg_out) {
    h.pop_back();
    seg_out->swap(h);
  }
  return FA_OK;
}

static int apply_plan_args(const fa_mesh* mesh, const fa_adjacency* adj) {
  int rc = check_mesh(mesh);
  if (rc) return rc;
  if (!adj || !adj->ptr || !adj->idx) return fail(FA_E_ARG, "null adjacency");
  if (!apply_plan_element(mesh))
    return fail(FA_E_UNSUPPORTED, "apply plan: P1 / P2 triangles and tetrahedra only (cell %d degree %d takes the generic kernel)",
                mesh->cell_type, mesh->degree);
  return FA_OK;
}

extern "C" int fa_apply_plan_bytes(const fa_mesh* mesh, const fa_adjacency* adj, int64_t* bytes, int64_t* nchunks,
                                   void* stream) {
  int rc = apply_plan_args(mesh, adj);
  if (rc) return rc;
  if (!bytes) return fail(FA_E_ARG, "null output");
  int64_t nch = 0, vis = 0;
  if ((rc = apply_plan_count(mesh, adj, (hipStream_t)stream, &nch, &vis, nullptr))) return rc;
  *bytes = apply_plan_layout(nch, vis, mesh->ncells * mesh->nn).bytes;
  if (nchunks) *nchunks = nch;
  return FA_OK;
}

extern "C" int fa_apply_plan(const fa_mesh* mesh, const fa_adjacency* adj, void* buf, int64_t bytes, void* stream) {
  int rc = apply_plan_args(mesh, adj);
  if (rc) return rc;
  if (!buf || (reinterpret_cast<uintptr_t>(buf) & 7)) return fail(FA_E_ARG, "apply plan buffer null or not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int64_t nch = 0, vis = 0;
  std::vector<int64_t> seg;
  if ((rc = apply_plan_count(mesh, adj, s, &nch, &vis, &seg))) return rc;
  const int64_t entries = mesh->ncells * mesh->nn;
  const ApplyPlanLayout Lo = apply_plan_layout(nch, vis, entries);
  if (bytes < Lo.bytes) return fail(FA_E_ARG, "apply plan buffer of %lld bytes, %lld needed", (long long)bytes, (long long)Lo.bytes);
  char* base = static_cast<char*>(buf);
  const int64_t hdr[4] = {kApplyMagic + mesh->nn, nch, entries, vis};
  HIP_TRY(hipMemcpyAsync(base, hdr, sizeof hdr, hipMemcpyHostToDevice, s));
  const int64_t nseg = (int64_t)seg.size() / 2;
  if (nseg > 0) {
    int64_t k = 0, v = 0;  // exclusive scans of the segments' counts
    for (int64_t i = 0; i < nseg; ++i) {
      const int64_t dk = seg[2 * i], dv = seg[2 * i + 1];
      seg[2 * i] = k;
      seg[2 * i + 1] = v;
      k += dk;
      v += dv;
    }
    int64_t* dseg = nullptr;
    if ((rc = scratch_alloc((void**)&dseg, sizeof(int64_t) * seg.size(), s))) return rc;
    HIP_TRY(hipMemcpyAsync(dseg, seg.data(), sizeof(int64_t) * seg.size(), hipMemcpyHostToDevice, s));
    int64_t* row_start = reinterpret_cast<int64_t*>(base + Lo.off_rows);
    int64_t* cell_off = reinterpret_cast<int64_t*>(base + Lo.off_coff);
    k_apply_cut<1><<<grid_for(nseg, 64), 64, 0, s>>>(mesh->cells, mesh->nn, mesh->nnodes, adj->ptr, adj->idx, nseg, dseg,
                                                    nullptr, row_start, cell_off);
    LAUNCH_CHECK();
    k_apply_fill<<<(int)std::min<int64_t>(nch, kMaxBlocks), 256, 0, s>>>(
        mesh->cells, mesh->nn, adj->ptr, adj->idx, nch, row_start, cell_off,
        reinterpret_cast<int32_t*>(base + Lo.off_cells), reinterpret_cast<uint16_t*>(base + Lo.off_pos));
    LAUNCH_CHECK();
    HIP_TRY(hipFreeAsync(dseg, s));
  } else {
    const int64_t zero2[2] = {0, 0};  // no rows: row_start[0] = cell_off[0] = 0
    HIP_TRY(hipMemcpyAsync(base + Lo.off_rows, zero2, 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(base + Lo.off_coff, zero2, 8, hipMemcpyHostToDevice, s));
  }
  HIP_TRY(hipStreamSynchronize(s));  // the host buffers above must outlive their copies
  return FA_OK;
}

// ------------------------------------------------------------------------------------ planned kernel
// y_e = K_e(u) x_e of one affine simplex cell, written to the lane's tile slot: value (a, i) at
// ys[(a * GD + i) * kApplyTile] (lanes = consecutive slots: conflict-free LDS stores). x_e (and u_e)
// stay in registers; y_e is accumulated over the quadrature points in LDS, not in registers.
// Per point: R = sum_b x_b (x) dphi_b (reference gradient), H = R Ji, S = law(H), then
// y_a += (w |J| S Ji^T) dphi_a: the tables are read with wave-uniform indices (scalar loads).
template <int GD, int NN, int LAW>
__device__ __forceinline__ void apply_cell(const MeshView& M, const FormView& F, const DevTables& T, int64_t c,
                                           const int8_t* __restrict__ bc, const double* __restrict__ x,
                                           double* __restrict__ ys) {
  const int32_t* cn = M.cells + c * NN;
  double xe[NN][GD];
  [[maybe_unused]] double ue[NN][GD];
#pragma unroll
  for (int b = 0; b < NN; ++b) {
    const int64_t n = cn[b];
#pragma unroll
    for (int i = 0; i < GD; ++i) {
      xe[b][i] = apply_col(x, bc, n * GD + i);
      if constexpr (LAW == EV_NEO) ue[b][i] = F.u[n * GD + i];
    }
  }
  if constexpr (LAW == EV_DAMAGE) {
    if constexpr (GD == 2 && NN == 3) {
      double g[3][2], w, H[3][3];
      apply_damage_cell(M, F, c, g, w, H);
      double e[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        e[0] += xe[b][0] * g[b][0];
        e[1] += xe[b][1] * g[b][1];
        e[2] += xe[b][0] * g[b][1] + xe[b][1] * g[b][0];
      }
      double s[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] = H[k][0] * e[0] + H[k][1] * e[1] + H[k][2] * e[2];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        ys[(a * 2 + 0) * kApplyTile] = w * (g[a][0] * s[0] + g[a][1] * s[2]);
        ys[(a * 2 + 1) * kApplyTile] = w * (g[a][1] * s[1] + g[a][0] * s[2]);
      }
    }
  } else {
    double Ji[GD][GD];
    const double det = fabs(simplex_geometry<GD>(M, c, Ji));
    double lam, mu;
    cell_lame(F, c, lam, mu);
    for (int q = 0; q < T.nq; ++q) {
      const double* __restrict__ dp = T.dphi + (size_t)q * NN * GD;
      double R[GD * GD], H[GD * GD], S[GD * GD];
#pragma unroll
      for (int i = 0; i < GD * GD; ++i) R[i] = 0.0;
#pragma unroll
      for (int b = 0; b < NN; ++b)
#pragma unroll
        for (int i = 0; i < GD; ++i)
#pragma unroll
          for (int k = 0; k < GD; ++k) R[i * GD + k] += xe[b][i] * dp[b * GD + k];
#pragma unroll
      for (int i = 0; i < GD; ++i)
#pragma unroll
        for (int d = 0; d < GD; ++d) {
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < GD; ++k) s += R[i * GD + k] * Ji[k][d];
          H[i * GD + d] = s;
        }
      if constexpr (LAW == EV_NEO) {
        double Ru[GD * GD], Fq[GD * GD];
#pragma unroll
        for (int i = 0; i < GD * GD; ++i) Ru[i] = 0.0;
#pragma unroll
        for (int b = 0; b < NN; ++b)
#pragma unroll
          for (int i = 0; i < GD; ++i)
#pragma unroll
            for (int k = 0; k < GD; ++k) Ru[i * GD + k] += ue[b][i] * dp[b * GD + k];
#pragma unroll
        for (int i = 0; i < GD; ++i)
#pragma unroll
          for (int d = 0; d < GD; ++d) {
            double s = (i == d) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < GD; ++k) s += Ru[i * GD + k] * Ji[k][d];
            Fq[i * GD + d] = s;
          }
        neo_tangent_dir<GD>(Fq, H, lam, mu, S);
      } else {
        lin_stress_dir<GD>(H, lam, mu, S);
      }
      // back to reference coordinates: St[i][k] = w |J| sum_d S[i][d] Ji[k][d]
      const double wd = T.wq[q] * det;
      double St[GD * GD];
#pragma unroll
      for (int i = 0; i < GD; ++i)
#pragma unroll
        for (int k = 0; k < GD; ++k) {
          double s = 0.0;
#pragma unroll
          for (int d = 0; d < GD; ++d) s += S[i * GD + d] * Ji[k][d];
          St[i * GD + k] = wd * s;
        }
#pragma unroll
      for (int a = 0; a < NN; ++a)
#pragma unroll
        for (int i = 0; i < GD; ++i) {
          double v = 0.0;
#pragma unroll
          for (int k = 0; k < GD; ++k) v += St[i * GD + k] * dp[a * GD + k];
          double* slot = ys + (a * GD + i) * kApplyTile;
          *slot = q == 0 ? v : *slot + v;
        }
    }
  }
}

// (No occupancy bound: asking for 2 waves per SIMD spills the P2-tetrahedron neo-Hookean instantiation to
// 488 B of scratch per lane; unbounded it takes 256 VGPRs + 124 AGPRs, no scratch, 1 wave per SIMD.)
template <int GD, int NN, int LAW>
__global__ __launch_bounds__(256) void k_apply_planned(MeshView M, FormView F, DevTables T,
                                                       const int64_t* __restrict__ plan,
                                                       const int64_t* __restrict__ adj_ptr,
                                                       const int8_t* __restrict__ bc, double diag,
                                                       const double* __restrict__ x, double* __restrict__ y) {
  __shared__ double tile[NN * GD * kApplyTile];
  // a buffer that is not this mesh's plan writes nothing (the header is device memory: no host check)
  const int64_t nchunks = plan[1], visits = plan[3];
  if (plan[0] != kApplyMagic + NN || plan[2] != M.ncells * NN || nchunks < 0) return;
  const int64_t* __restrict__ row_start = plan + 4;
  const int64_t* __restrict__ cell_off = row_start + nchunks + 1;
  const int32_t* __restrict__ clist = reinterpret_cast<const int32_t*>(cell_off + nchunks + 1);
  const uint16_t* __restrict__ pos = reinterpret_cast<const uint16_t*>(clist + ((visits + 1) & ~int64_t(1)));
  if (row_start[nchunks] != M.nnodes) return;
  const int tid = threadIdx.x;
  for (int64_t k = blockIdx.x; k < nchunks; k += gridDim.x) {
    const int64_t r0 = row_start[k], r1 = row_start[k + 1];
    const int64_t c0 = cell_off[k];
    const int nc = (int)min<int64_t>(cell_off[k + 1] - c0, kApplyTile);
    if (tid < nc) {
      const int64_t c = clist[c0 + tid];
      if (c >= 0 && c < M.ncells) apply_cell<GD, NN, LAW>(M, F, T, c, bc, x, tile + tid);
    }
    __syncthreads();
    for (int64_t r = r0 + tid; r < r1; r += 256) {
      double acc[GD];
#pragma unroll
      for (int i = 0; i < GD; ++i) acc[i] = 0.0;
      for (int64_t j = adj_ptr[r]; j < adj_ptr[r + 1]; ++j) {
        const int pj = pos[j];
        const int slot = pj & 0xFF, aloc = min(pj >> 8, NN - 1);
#pragma unroll
        for (int i = 0; i < GD; ++i) acc[i] += tile[(aloc * GD + i) * kApplyTile + slot];
      }
      double o[GD];
#pragma unroll
      for (int i = 0; i < GD; ++i) {
        const double xi = x[r * GD + i];
        o[i] = (bc && bc[r * GD + i]) ? diag * xi : acc[i];
      }
#pragma unroll
      for (int i = 0; i < GD; ++i) y[r * GD + i] = o[i];
      store_fence(o);  // the next row / chunk would rewrite the store's data registers
    }
    __syncthreads();
  }
}

template <int GD, int NN, int LAW>
static int launch_apply_planned(const MeshView& M, const FormView& F, const DevTables& T, const void* plan,
                                const fa_adjacency* adj, const int8_t* bc, double diag, const double* x, double* y,
                                hipStream_t s) {
  const int grid = (int)std::min<int64_t>(std::max<int64_t>(M.nnodes, 1), kApplyGrid);
  k_apply_planned<GD, NN, LAW><<<grid, 256, 0, s>>>(M, F, T, static_cast<const int64_t*>(plan), adj->ptr, bc, diag, x, y);
  LAUNCH_CHECK();
  return FA_OK;
}

// ------------------------------------------------------------------------------------ C ABI
static int apply_common(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj, FormView& F) {
  int rc = check_mesh(mesh);
  if (rc) return rc;
  if (!adj || !adj->ptr || !adj->idx) return fail(FA_E_ARG, "null adjacency");
  if ((rc = form_view(mesh, form, F))) return rc;
  return FA_OK;
}

extern "C" int fa_apply_jacobian(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj, const void* plan,
                                 const int8_t* bc, double diag, const double* x, double* y, void* stream) {
  FormView F;
  DevTables T;
  int rc = apply_common(mesh, form, adj, F);
  if (rc) return rc;
  if (!x || !y) return fail(FA_E_ARG, "fa_apply_jacobian: null x or y");
  const int64_t ndofs = mesh->nnodes * mesh->gdim;
  const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y);
  if (xa < ya + 8 * (uintptr_t)ndofs && ya < xa + 8 * (uintptr_t)ndofs)
    return fail(FA_E_ARG, "fa_apply_jacobian: x and y must not alias (y is written while x is read)");
  if (plan && !apply_plan_element(mesh))
    return fail(FA_E_UNSUPPORTED, "apply plan: P1 / P2 triangles and tetrahedra only (cell %d degree %d: pass plan = NULL)",
                mesh->cell_type, mesh->degree);
  if (plan && (reinterpret_cast<uintptr_t>(plan) & 7)) return fail(FA_E_ARG, "apply plan not 8-byte aligned");
  if (mesh->nnodes == 0) return FA_OK;
  if ((rc = get_tables(mesh->cell_type, mesh->degree, form->qdeg, &T))) return rc;
  hipStream_t s = (hipStream_t)stream;
  MeshView M{mesh->cells, mesh->geom, mesh->x, mesh->ncells, mesh->nnodes, mesh->nn, mesh->nv, mesh->gdim};
  if (!plan) {
    FA_VEC_DISPATCH(k_apply_generic, M, F, T, adj->ptr, adj->idx, bc, diag, x, y);
    return FA_OK;
  }
  const int law = F.kind == FA_NEO_HOOKEAN ? EV_NEO : F.kind == FA_ASYM_DAMAGE ? EV_DAMAGE : EV_LIN;
#define AP(GD_, NN_, LAW_) return launch_apply_planned<GD_, NN_, LAW_>(M, F, T, plan, adj, bc, diag, x, y, s)
#define AP_LAWS(GD_, NN_)        \
  if (law == EV_NEO) AP(GD_, NN_, EV_NEO); \
  AP(GD_, NN_, EV_LIN)
  if (mesh->cell_type == FA_TRIANGLE) {
    if (mesh->degree == 1) {
      if (law == EV_DAMAGE) AP(2, 3, EV_DAMAGE);
      AP_LAWS(2, 3);
    }
    AP_LAWS(2, 6);
  }
  if (mesh->degree == 1) {
    AP_LAWS(3, 4);
  }
  AP_LAWS(3, 10);
#undef AP_LAWS
#undef AP
}

extern "C" int fa_jacobian_block_diag(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj,
                                      const int8_t* bc, double diag, double* out, void* stream) {
  FormView F;
  DevTables T;
  int rc = apply_common(mesh, form, adj, F);
  if (rc) return rc;
  if (!out) return fail(FA_E_ARG, "fa_jacobian_block_diag: null output");
  if (mesh->nnodes == 0) return FA_OK;
  if ((rc = get_tables(mesh->cell_type, mesh->degree, form->qdeg, &T))) return rc;
  hipStream_t s = (hipStream_t)stream;
  MeshView M{mesh->cells, mesh->geom, mesh->x, mesh->ncells, mesh->nnodes, mesh->nn, mesh->nv, mesh->gdim};
  FA_VEC_DISPATCH(k_apply_block_diag, M, F, T, adj->ptr, adj->idx, bc, diag, out);
  return FA_OK;
}
