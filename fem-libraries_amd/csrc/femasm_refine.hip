// femasm — uniform ("red") refinement of simplex meshes and the multigrid transfers over the refined
// hierarchy (included at the end of femasm_eval.hip: one translation unit).
//
// Numbering (mesh.refine): the parent's vertices keep their indices, the midpoint of edge e of
// mesh.entities(m, 1) is vertex nverts + e, the children of cell c are cells c * 2^tdim + k. This is the
// numbering of the parent's degree-2 nodes (fem._generic_dofmap), so the P1 space on the refined mesh
// and the P2 space on the parent share their nodes, and one edge stencil (an edge node takes half of
// each end vertex) is both the P2 -> P1 transfer on one mesh and the P1(h) -> P1(2h) transfer.
//
// Local vertex codes of a parent cell: 0 .. nv - 1 its vertices, then the midpoints m01, m02, (m03,)
// m12, (m13, m23). With basix's edge order (triangle (1,2),(0,2),(0,1); tetrahedron (2,3),(1,3),(1,2),
// (0,3),(0,2),(0,1)) code nv + k is local edge nedges_local - 1 - k.

__constant__ int8_t kRefineTri[4][3] = {{0, 3, 4}, {3, 1, 5}, {4, 5, 2}, {3, 5, 4}};
// corner children, then per diagonal (m01-m23, m02-m13, m03-m12) the four children around it, each
// ordered so that it keeps the parent's orientation sign
__constant__ int8_t kRefineTetCorner[4][4] = {{0, 4, 5, 6}, {4, 1, 7, 8}, {5, 7, 2, 9}, {6, 8, 9, 3}};
__constant__ int8_t kRefineTetInner[3][4][4] = {
    {{4, 5, 6, 9}, {4, 6, 8, 9}, {4, 7, 9, 8}, {4, 5, 9, 7}},
    {{4, 5, 6, 8}, {4, 5, 8, 7}, {5, 6, 8, 9}, {5, 7, 9, 8}},
    {{4, 5, 6, 7}, {5, 6, 7, 9}, {6, 7, 9, 8}, {4, 6, 8, 7}},
};

__global__ __launch_bounds__(256) void k_refine_tri(int64_t ncells, int64_t nverts, const int32_t* __restrict__ cells,
                                                    const int32_t* __restrict__ cell_edges,
                                                    const int32_t* __restrict__ tags, int32_t* __restrict__ children,
                                                    int32_t* __restrict__ child_tags) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < ncells; c += (int64_t)gridDim.x * blockDim.x) {
    int32_t L[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      L[k] = cells[c * 3 + k];
      L[3 + k] = (int32_t)(nverts + cell_edges[c * 3 + (2 - k)]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int32_t v[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) children[(c * 4 + j) * 3 + k] = v[k] = L[kRefineTri[j][k]];
      if (tags) child_tags[c * 4 + j] = tags[c];
      store_guard3(v[0], v[1], v[2]);  // a 12-byte store: its data registers stay live until it has read them
    }
  }
}

// squared distance of the midpoints of two opposite edges (a, b) and (p, q), each product and sum
// rounded on its own (no fused multiply-add): the host path computes the same bits, so both pick the same
// diagonal also where two lengths differ in the last place only
__device__ __forceinline__ double diagonal_length2(const double (*X)[3], int a, int b, int p, int q) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double m0 = 0.5 * (X[a][d] + X[b][d]);
    const double m1 = 0.5 * (X[p][d] + X[q][d]);
    const double df = m0 - m1;
    const double sq = df * df;
    s = d == 0 ? sq : s + sq;
  }
  return s;
}

__global__ __launch_bounds__(256) void k_refine_tet(int64_t ncells, int64_t nverts, const int32_t* __restrict__ cells,
                                                    const int32_t* __restrict__ cell_edges,
                                                    const double* __restrict__ x, const int32_t* __restrict__ tags,
                                                    int32_t* __restrict__ children, int32_t* __restrict__ child_tags) {
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < ncells; c += (int64_t)gridDim.x * blockDim.x) {
    int32_t L[10];
    double X[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      L[k] = cells[c * 4 + k];
#pragma unroll
      for (int d = 0; d < 3; ++d) X[k][d] = x[(int64_t)L[k] * 3 + d];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) L[4 + k] = (int32_t)(nverts + cell_edges[c * 6 + (5 - k)]);
    // shortest diagonal of the inner octahedron, ties to the first
    const double l0 = diagonal_length2(X, 0, 1, 2, 3);
    const double l1 = diagonal_length2(X, 0, 2, 1, 3);
    const double l2 = diagonal_length2(X, 0, 3, 1, 2);
    int g = 0;
    double lb = l0;
    if (l1 < lb) { g = 1; lb = l1; }
    if (l2 < lb) g = 2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int32_t child[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int code = j < 4 ? kRefineTetCorner[j][k] : kRefineTetInner[g][j - 4][k];
        int32_t v = L[0];  // select without indexing the register array dynamically
#pragma unroll
        for (int q = 1; q < 10; ++q) v = code == q ? L[q] : v;
        child[k] = v;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) children[(c * 8 + j) * 4 + k] = child[k];
      if (tags) child_tags[c * 8 + j] = tags[c];
      // a 16-byte store: its data registers stay live until it has read them
      store_guard4(child[0], child[1], child[2], child[3]);
    }
  }
}

// one thread per edge and component: xm[e][d] = 0.5 * (x[a][d] + x[b][d])
__global__ __launch_bounds__(256) void k_edge_midpoints(int64_t n, int gdim, const int32_t* __restrict__ edge_verts,
                                                        const double* __restrict__ x, double* __restrict__ xm) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = i / gdim;
    const int d = (int)(i - e * gdim);
    const int64_t a = edge_verts[2 * e], b = edge_verts[2 * e + 1];
    xm[i] = 0.5 * (x[a * gdim + d] + x[b * gdim + d]);
  }
}

extern "C" int fa_refine_cells(int32_t cell_type, int64_t ncells, int64_t nverts, const int32_t* cells,
                               const int32_t* cell_edges, const double* x, const int32_t* tags, int32_t* children,
                               int32_t* child_tags, void* stream) {
  if (cell_type != kTriangle && cell_type != kTetrahedron)
    return fail(FA_E_UNSUPPORTED, "fa_refine_cells: cell type %d (triangles and tetrahedra)", cell_type);
  if (ncells < 0 || nverts < 0) return fail(FA_E_ARG, "fa_refine_cells: negative count");
  const int64_t nchild = cell_type == kTriangle ? 4 : 8;
  if (ncells > (int64_t)INT32_MAX / nchild) return fail(FA_E_CAPACITY, "fa_refine_cells: the child cells exceed int32");
  if (ncells == 0) return FA_OK;
  if (!cells || !cell_edges || !children) return fail(FA_E_ARG, "fa_refine_cells: null cells, cell_edges or children");
  if (cell_type == kTetrahedron && !x) return fail(FA_E_ARG, "fa_refine_cells: null x (tetrahedra)");
  if ((tags == nullptr) != (child_tags == nullptr))
    return fail(FA_E_ARG, "fa_refine_cells: tags and child_tags go together");
  hipStream_t s = (hipStream_t)stream;
  if (cell_type == kTriangle)
    k_refine_tri<<<grid_for(ncells), 256, 0, s>>>(ncells, nverts, cells, cell_edges, tags, children, child_tags);
  else
    k_refine_tet<<<grid_for(ncells), 256, 0, s>>>(ncells, nverts, cells, cell_edges, x, tags, children, child_tags);
  LAUNCH_CHECK();
  return FA_OK;
}

extern "C" int fa_edge_midpoints(int64_t nedges, int32_t gdim, const int32_t* edge_verts, const double* x, double* xm,
                                 void* stream) {
  if (nedges < 0) return fail(FA_E_ARG, "fa_edge_midpoints: nedges %lld", (long long)nedges);
  if (gdim < 1 || gdim > 3) return fail(FA_E_ARG, "fa_edge_midpoints: gdim %d (1 to 3)", gdim);
  if (nedges == 0) return FA_OK;
  if (!edge_verts || !x || !xm) return fail(FA_E_ARG, "fa_edge_midpoints: null edge_verts, x or xm");
  const int64_t n = nedges * gdim;
  k_edge_midpoints<<<grid_for(n), 256, 0, (hipStream_t)stream>>>(n, gdim, edge_verts, x, xm);
  LAUNCH_CHECK();
  return FA_OK;
}

// ------------------------------------------------------------------------------------ edge transfers
// Fine nodes = the ncoarse coarse nodes, then one node per edge; P is the identity on the first and
// 1/2, 1/2 on an edge node. Both kernels gather: one thread per output dof, fixed summation order.

template <int BS>
__global__ __launch_bounds__(256) void k_prolong_edges(int64_t ncoarse, int64_t nedges,
                                                       const int32_t* __restrict__ edge_verts,
                                                       const double* __restrict__ xc, const int8_t* __restrict__ bc_c,
                                                       const int8_t* __restrict__ bc_f, int add,
                                                       double* __restrict__ xf) {
  const int64_t nf = (ncoarse + nedges) * BS, ncd = ncoarse * BS;
  for (int64_t fd = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; fd < nf; fd += (int64_t)gridDim.x * blockDim.x) {
    const bool masked = bc_f && bc_f[fd];
    double v = 0.0;
    if (!masked) {
      if (fd < ncd) {
        v = (bc_c && bc_c[fd]) ? 0.0 : xc[fd];
      } else {
        const int64_t e = (fd - ncd) / BS;
        const int c = (int)(fd - ncd - e * BS);
        const int64_t da = (int64_t)edge_verts[2 * e] * BS + c, db = (int64_t)edge_verts[2 * e + 1] * BS + c;
        const double va = (bc_c && bc_c[da]) ? 0.0 : xc[da];
        const double vb = (bc_c && bc_c[db]) ? 0.0 : xc[db];
        v = 0.5 * va + 0.5 * vb;
      }
    }
    if (!add) xf[fd] = v;
    else if (!masked) xf[fd] += v;  // a masked fine dof receives nothing
  }
}

// one thread per coarse dof: its own fine dof, then half of each of its node's edge dofs in vedges
// order (any valence: the loop runs over the node's CSR row)
template <int BS>
__global__ __launch_bounds__(256) void k_restrict_edges(int64_t ncoarse, const int64_t* __restrict__ vptr,
                                                        const int32_t* __restrict__ vedges,
                                                        const double* __restrict__ rf, const int8_t* __restrict__ bc_f,
                                                        const int8_t* __restrict__ bc_c, double* __restrict__ rc) {
  const int64_t ncd = ncoarse * BS;
  for (int64_t cd = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; cd < ncd; cd += (int64_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    if (!(bc_c && bc_c[cd])) {
      const int64_t v = cd / BS;
      const int c = (int)(cd - v * BS);
      if (!(bc_f && bc_f[cd])) s = rf[cd];
      const int64_t k1 = vptr[v + 1];
      for (int64_t k = vptr[v]; k < k1; ++k) {
        const int64_t fd = (ncoarse + (int64_t)vedges[k]) * BS + c;
        if (!(bc_f && bc_f[fd])) s += 0.5 * rf[fd];
      }
    }
    rc[cd] = s;
  }
}

static int edge_transfer_check(const fa_edge_transfer* t, const char* who) {
  if (!t) return fail(FA_E_ARG, "%s: null transfer descriptor", who);
  if (t->bs < 1 || t->bs > 3) return fail(FA_E_UNSUPPORTED, "%s: block size %d (1 to 3)", who, t->bs);
  if (t->ncoarse < 0 || t->nedges < 0)
    return fail(FA_E_ARG, "%s: negative count (ncoarse %lld, nedges %lld)", who, (long long)t->ncoarse,
                (long long)t->nedges);
  if (t->ncoarse > INT32_MAX || t->nedges > INT32_MAX)
    return fail(FA_E_CAPACITY, "%s: node and edge indices are int32", who);
  if (t->nedges > 0 && (!t->edge_verts || !t->vptr || !t->vedges))
    return fail(FA_E_ARG, "%s: null edge_verts, vptr or vedges", who);
  return FA_OK;
}

extern "C" int fa_prolong_edges(const fa_edge_transfer* t, const double* xc, const int8_t* bc_c, const int8_t* bc_f,
                                int32_t add, double* xf, void* stream) {
  int rc = edge_transfer_check(t, "fa_prolong_edges");
  if (rc) return rc;
  if (!xc || !xf) return fail(FA_E_ARG, "fa_prolong_edges: null xc or xf");
  const int64_t nf = (t->ncoarse + t->nedges) * t->bs;
  if (nf == 0) return FA_OK;
  const int grid = grid_for(nf);
  hipStream_t s = (hipStream_t)stream;
  switch (t->bs) {
    case 1: k_prolong_edges<1><<<grid, 256, 0, s>>>(t->ncoarse, t->nedges, t->edge_verts, xc, bc_c, bc_f, add, xf); break;
    case 2: k_prolong_edges<2><<<grid, 256, 0, s>>>(t->ncoarse, t->nedges, t->edge_verts, xc, bc_c, bc_f, add, xf); break;
    default: k_prolong_edges<3><<<grid, 256, 0, s>>>(t->ncoarse, t->nedges, t->edge_verts, xc, bc_c, bc_f, add, xf); break;
  }
  LAUNCH_CHECK();
  return FA_OK;
}

extern "C" int fa_restrict_edges(const fa_edge_transfer* t, const double* rf, const int8_t* bc_f, const int8_t* bc_c,
                                 double* rc_out, void* stream) {
  int rc = edge_transfer_check(t, "fa_restrict_edges");
  if (rc) return rc;
  if (!rf || !rc_out) return fail(FA_E_ARG, "fa_restrict_edges: null rf or rc");
  if (!t->vptr) return fail(FA_E_ARG, "fa_restrict_edges: null vptr");
  const int64_t ncd = t->ncoarse * t->bs;
  if (ncd == 0) return FA_OK;
  const int grid = grid_for(ncd);
  hipStream_t s = (hipStream_t)stream;
  switch (t->bs) {
    case 1: k_restrict_edges<1><<<grid, 256, 0, s>>>(t->ncoarse, t->vptr, t->vedges, rf, bc_f, bc_c, rc_out); break;
    case 2: k_restrict_edges<2><<<grid, 256, 0, s>>>(t->ncoarse, t->vptr, t->vedges, rf, bc_f, bc_c, rc_out); break;
    default: k_restrict_edges<3><<<grid, 256, 0, s>>>(t->ncoarse, t->vptr, t->vedges, rf, bc_f, bc_c, rc_out); break;
  }
  LAUNCH_CHECK();
  return FA_OK;
}
