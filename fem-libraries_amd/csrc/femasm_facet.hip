// femasm — exterior-facet loads: surface tractions and pressure in the residual (included at the end of
// femasm_eval.hip: one translation unit).
//
//   b[a, i] += alpha * sum over the loaded facets F of node a of  int_F (t_i - p n_i) phi_a dS
//
// on the reference configuration (dead loads). The facet points are cell reference points: a rule on the
// reference facet (Gauss on [0, 1]; make_quadrature(triangle | quadrilateral)) mapped through the local
// facet's reference vertices, X = V0 + xi (V1 - V0) + eta (V2 - V0), so tabulate() gives the space's phi
// and the geometry gradients there. With J = sum_v x_v (x) gdphi_v at the point, Nanson's formula
//   n dS = sign(det J) cof(J) N_ref dS_ref
// needs no inverse and is outward for either cell orientation; N_ref dS_ref is the (outward) normal of the
// reference facet scaled by the parametrisation: (V1 - V0) rotated by -90 degrees, or (V1 - V0) x (V2 - V0).

// basix local facets as reference vertices (facet rule coordinates run along V0 -> V1 and V0 -> V2)
static const int kFacetVerts[4][6][3] = {
    {{1, 2, -1}, {0, 2, -1}, {0, 1, -1}},                                     // triangle
    {{0, 1, -1}, {0, 2, -1}, {1, 3, -1}, {2, 3, -1}},                         // quadrilateral
    {{1, 2, 3}, {0, 2, 3}, {0, 1, 3}, {0, 1, 2}},                             // tetrahedron
    {{0, 1, 2}, {0, 1, 4}, {0, 2, 4}, {1, 3, 5}, {2, 3, 6}, {4, 5, 6}},       // hexahedron (V3 = V1 + V2 - V0)
};
static int facet_cell_row(int ct) { return ct == kTriangle ? 0 : ct == kQuadrilateral ? 1 : ct == kTetrahedron ? 2 : 3; }
static int cell_nfacets(int ct) { return ct == kTriangle ? 3 : ct == kQuadrilateral ? 4 : ct == kTetrahedron ? 4 : 6; }
static void ref_vertex(int ct, int v, double* X) {
  const int td = cell_tdim(ct);
  for (int d = 0; d < td; ++d) X[d] = is_simplex(ct) ? (v == d + 1 ? 1.0 : 0.0) : (double)((v >> d) & 1);
}
static int facet_closure_size(int ct, int p) {
  switch (ct) {
    case kTriangle:
    case kQuadrilateral: return p + 1;
    case kTetrahedron: return (p + 1) * (p + 2) / 2;
  }
  return (p + 1) * (p + 1);
}

struct FacetTables {
  int nl, nk, nq, nn, nv;
  const double* wq;        // [nq]
  const double* phi;       // [nl][nq][nn]
  const double* gdphi;     // [nl][nq][nv][td]
  const double* nref;      // [nl][td]  N_ref dS_ref
  const int32_t* closure;  // [nl][nk]  local nodes of each local facet's closure, ascending
};

static std::mutex g_facet_mu;
static std::map<std::tuple<int, int, int, int>, FacetTables> g_facet_tabs;

// local nodes (basix order) lying on local facet lf, ascending
static std::vector<int> facet_closure(int ct, int p, int lf) {
  std::vector<int> out;
  const int nn = num_nodes(ct, p), td = cell_tdim(ct);
  if (is_simplex(ct)) {
    // facet lf is opposite vertex lf: vertex nodes other than lf, then (p = 2) the edges without lf
    const int TRI_E[3][2] = {{1, 2}, {0, 2}, {0, 1}};
    const int TET_E[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};
    const int nvx = td + 1;
    for (int a = 0; a < nvx; ++a)
      if (a != lf) out.push_back(a);
    if (p == 2)
      for (int e = 0; e < nn - nvx; ++e) {
        const int i = td == 2 ? TRI_E[e][0] : TET_E[e][0], j = td == 2 ? TRI_E[e][1] : TET_E[e][1];
        if (i != lf && j != lf) out.push_back(nvx + e);
      }
    return out;
  }
  // tensor cells: the facet is the coordinate plane its reference vertices share
  const int* fv = kFacetVerts[facet_cell_row(ct)][lf];
  int dir = -1, side = 0;
  for (int d = 0; d < td; ++d) {
    const int b0 = (fv[0] >> d) & 1, b1 = (fv[1] >> d) & 1, b2 = td == 3 ? (fv[2] >> d) & 1 : b0;
    if (b0 == b1 && b0 == b2) { dir = d; side = b0; }
  }
  const std::vector<int> L = tensor_node_lattice(ct, p);
  for (int a = 0; a < nn; ++a)
    if (L[3 * a + dir] == side * p) out.push_back(a);
  return out;
}

static int get_facet_tables(int ct, int p, int qdeg, FacetTables* out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (!supported(ct, p)) return fail(FA_E_UNSUPPORTED, "unsupported element: cell %d degree %d", ct, p);
  const int qd = qdeg < 0 ? 2 * p : qdeg;
  if (qd < 1 || qd > 12) return fail(FA_E_UNSUPPORTED, "facet quadrature degree %d outside 1 .. 12", qd);
  std::lock_guard<std::mutex> lock(g_facet_mu);
  const auto key = std::make_tuple(dev, ct, p, qd);
  auto it = g_facet_tabs.find(key);
  if (it != g_facet_tabs.end()) {
    *out = it->second;
    return FA_OK;
  }
  const int td = cell_tdim(ct), nn = num_nodes(ct, p), nv = cell_nverts(ct), nl = cell_nfacets(ct);
  const int nk = facet_closure_size(ct, p);
  // the rule on the reference facet
  Quadrature R;
  if (td == 2) {
    R.tdim = 1;
    gauss_legendre_01((qd + 2) / 2, R.pts, R.wts);
  } else {
    R = make_quadrature(ct == kTetrahedron ? (int)kTriangle : (int)kQuadrilateral, qd);
  }
  const int nq = R.size();
  std::vector<double> h(R.wts), phi_all, gd_all, nref_all;
  std::vector<int32_t> closure;
  double cen[3] = {0, 0, 0};  // the reference cell's centroid
  for (int v = 0; v < nv; ++v) {
    double X[3] = {0, 0, 0};
    ref_vertex(ct, v, X);
    for (int d = 0; d < td; ++d) cen[d] += X[d] / nv;
  }
  for (int lf = 0; lf < nl; ++lf) {
    const int* fv = kFacetVerts[facet_cell_row(ct)][lf];
    double V0[3] = {0, 0, 0}, A[3] = {0, 0, 0}, B[3] = {0, 0, 0};
    ref_vertex(ct, fv[0], V0);
    ref_vertex(ct, fv[1], A);
    if (td == 3) ref_vertex(ct, fv[2], B);
    for (int d = 0; d < td; ++d) {
      A[d] -= V0[d];
      if (td == 3) B[d] -= V0[d];
    }
    Quadrature Q;
    Q.tdim = td;
    Q.wts = R.wts;
    double mid[3] = {0, 0, 0};  // a point of the facet: the mean of its rule's points
    for (int q = 0; q < nq; ++q)
      for (int d = 0; d < td; ++d) {
        const double X = V0[d] + R.pts[q * (td - 1)] * A[d] + (td == 3 ? R.pts[q * 2 + 1] * B[d] : 0.0);
        Q.pts.push_back(X);
        mid[d] += X / nq;
      }
    std::vector<double> phi, dphi, gphi, gdphi;
    if (!tabulate(ct, p, Q, phi, dphi) || !tabulate(ct, 1, Q, gphi, gdphi))
      return fail(FA_E_UNSUPPORTED, "element tables failed for cell %d degree %d", ct, p);
    phi_all.insert(phi_all.end(), phi.begin(), phi.end());
    gd_all.insert(gd_all.end(), gdphi.begin(), gdphi.end());
    double N[3];
    if (td == 2) {
      N[0] = A[1];
      N[1] = -A[0];
    } else {
      N[0] = A[1] * B[2] - A[2] * B[1];
      N[1] = A[2] * B[0] - A[0] * B[2];
      N[2] = A[0] * B[1] - A[1] * B[0];
    }
    double out_dot = 0.0;
    for (int d = 0; d < td; ++d) out_dot += N[d] * (mid[d] - cen[d]);
    for (int d = 0; d < td; ++d) nref_all.push_back(out_dot < 0.0 ? -N[d] : N[d]);
    const std::vector<int> cl = facet_closure(ct, p, lf);
    if ((int)cl.size() != nk)
      return fail(FA_E_UNSUPPORTED, "facet closure of cell %d degree %d: %d nodes, not %d", ct, p, (int)cl.size(), nk);
    closure.insert(closure.end(), cl.begin(), cl.end());
  }
  const size_t off_phi = h.size();
  h.insert(h.end(), phi_all.begin(), phi_all.end());
  const size_t off_gd = h.size();
  h.insert(h.end(), gd_all.begin(), gd_all.end());
  const size_t off_n = h.size();
  h.insert(h.end(), nref_all.begin(), nref_all.end());
  double* d = nullptr;
  int32_t* dc = nullptr;
  HIP_TRY(hipMalloc(&d, h.size() * sizeof(double)));
  HIP_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMalloc(&dc, closure.size() * sizeof(int32_t)));
  HIP_TRY(hipMemcpy(dc, closure.data(), closure.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  FacetTables T{nl, nk, nq, nn, nv, d, d + off_phi, d + off_gd, d + off_n, dc};
  g_facet_tabs[key] = T;
  *out = T;
  return FA_OK;
}

struct FacetLoadView {
  int64_t nfacets, nloaded, nvalues;
  const int32_t* facet_cell;
  const int32_t* facet_local;
  const int32_t* facet_value;
  const int32_t* nodes;
  const int64_t* node_ptr;
  const int32_t* entries;
  int tmode, pmode;
  const double* traction;
  const double* pressure;
};

// n dS at one facet point: sign(det J) cof(J) N with J[i][k] = sum_v x_v[i] gdphi_v[k]
template <int GD, int NV>
__device__ __forceinline__ void facet_normal(const double (&xv)[NV][GD], const double* __restrict__ gd,
                                             const double (&N)[GD], double (&nds)[GD]) {
  double J[GD][GD];
#pragma unroll
  for (int i = 0; i < GD; ++i)
#pragma unroll
    for (int k = 0; k < GD; ++k) J[i][k] = 0.0;
#pragma unroll
  for (int v = 0; v < NV; ++v)
#pragma unroll
    for (int i = 0; i < GD; ++i)
#pragma unroll
      for (int k = 0; k < GD; ++k) J[i][k] += xv[v][i] * gd[v * GD + k];
  if constexpr (GD == 2) {
    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double sg = det < 0.0 ? -1.0 : 1.0;
    nds[0] = sg * (J[1][1] * N[0] - J[1][0] * N[1]);
    nds[1] = sg * (J[0][0] * N[1] - J[0][1] * N[0]);
  } else {
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    const double c10 = J[0][2] * J[2][1] - J[0][1] * J[2][2];
    const double c11 = J[0][0] * J[2][2] - J[0][2] * J[2][0];
    const double c12 = J[0][1] * J[2][0] - J[0][0] * J[2][1];
    const double c20 = J[0][1] * J[1][2] - J[0][2] * J[1][1];
    const double c21 = J[0][2] * J[1][0] - J[0][0] * J[1][2];
    const double c22 = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    const double sg = det < 0.0 ? -1.0 : 1.0;
    nds[0] = sg * (c00 * N[0] + c01 * N[1] + c02 * N[2]);
    nds[1] = sg * (c10 * N[0] + c11 * N[1] + c12 * N[2]);
    nds[2] = sg * (c20 * N[0] + c21 * N[1] + c22 * N[2]);
  }
}

// One thread per loaded node; its entries (slot, k) in stored order, every facet point in rule order:
// a fixed summation order and one write per dof, as k_vector.
template <int GD, int NV>
__global__ __launch_bounds__(256) void k_facet_load(MeshView M, FacetLoadView L, FacetTables T, double alpha,
                                                    double* __restrict__ b) {
  const int nn = M.nn, nk = T.nk, nq = T.nq;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < L.nloaded; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t a = L.nodes[t];
    if (a < 0 || a >= M.nnodes) continue;
    double r[GD];
#pragma unroll
    for (int i = 0; i < GD; ++i) r[i] = 0.0;
    const int64_t j1 = L.node_ptr[t + 1];
    for (int64_t j = L.node_ptr[t]; j < j1; ++j) {
      const int32_t e = L.entries[j];
      if (e < 0) continue;
      const int64_t slot = e / nk;
      const int k = e % nk;
      if (slot >= L.nfacets) continue;
      const int64_t c = L.facet_cell[slot];
      const int lf = L.facet_local[slot];
      if (c < 0 || c >= M.ncells || lf < 0 || lf >= T.nl) continue;
      int64_t row = 0;
      if (L.tmode == FA_LOAD_FACET || L.pmode == FA_LOAD_FACET) {
        row = L.facet_value[slot];
        if (row < 0 || row >= L.nvalues) continue;
      }
      const int aloc = T.closure[lf * nk + k];
      const int32_t* cn = M.cells + c * nn;
      const int32_t* gv = M.geom + c * NV;
      double xv[NV][GD];
#pragma unroll
      for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int i = 0; i < GD; ++i) xv[v][i] = M.x[(int64_t)gv[v] * GD + i];
      double N[GD];
#pragma unroll
      for (int i = 0; i < GD; ++i) N[i] = T.nref[lf * GD + i];
      // the values that do not vary over the facet
      double tq[GD], pq = 0.0;
#pragma unroll
      for (int i = 0; i < GD; ++i) tq[i] = 0.0;
      if (L.tmode == FA_LOAD_CONSTANT || L.tmode == FA_LOAD_FACET) {
        const double* tv = L.traction + (L.tmode == FA_LOAD_FACET ? row * GD : 0);
#pragma unroll
        for (int i = 0; i < GD; ++i) tq[i] = tv[i];
      }
      if (L.pmode == FA_LOAD_CONSTANT) pq = L.pressure[0];
      else if (L.pmode == FA_LOAD_FACET) pq = L.pressure[row];
      for (int q = 0; q < nq; ++q) {
        const double* ph = T.phi + ((size_t)lf * nq + q) * nn;
        double nds[GD];
        facet_normal<GD, NV>(xv, T.gdphi + ((size_t)lf * nq + q) * NV * GD, N, nds);
        if (L.tmode == FA_LOAD_NODAL || L.pmode == FA_LOAD_NODAL) {
          if (L.tmode == FA_LOAD_NODAL)
#pragma unroll
            for (int i = 0; i < GD; ++i) tq[i] = 0.0;
          if (L.pmode == FA_LOAD_NODAL) pq = 0.0;
          for (int bb = 0; bb < nn; ++bb) {
            const int64_t n = cn[bb];
            const double pb = ph[bb];
            if (L.tmode == FA_LOAD_NODAL)
#pragma unroll
              for (int i = 0; i < GD; ++i) tq[i] += pb * L.traction[n * GD + i];
            if (L.pmode == FA_LOAD_NODAL) pq += pb * L.pressure[n];
          }
        }
        double s2 = 0.0;
#pragma unroll
        for (int i = 0; i < GD; ++i) s2 += nds[i] * nds[i];
        const double dS = sqrt(s2);
        const double wa = T.wq[q] * ph[aloc];
#pragma unroll
        for (int i = 0; i < GD; ++i) r[i] += wa * (tq[i] * dS - pq * nds[i]);
      }
    }
    double o[GD];
#pragma unroll
    for (int i = 0; i < GD; ++i) o[i] = b[a * GD + i] + alpha * r[i];
#pragma unroll
    for (int i = 0; i < GD; ++i) b[a * GD + i] = o[i];
    store_fence(o);  // (as k_vector: the next node of the grid-stride loop rewrites the store's data registers)
  }
}

static bool load_mode_ok(int m) { return m == FA_LOAD_NONE || m == FA_LOAD_CONSTANT || m == FA_LOAD_FACET || m == FA_LOAD_NODAL; }

extern "C" int fa_facet_load_apply(const fa_mesh* mesh, const fa_facet_load* load, double alpha, double* b,
                                   void* stream) {
  int rc = check_mesh(mesh);
  if (rc) return rc;
  if (!load || !b) return fail(FA_E_ARG, "fa_facet_load_apply: null load or b");
  if (load->nfacets < 0 || load->nloaded < 0 || load->nvalues < 0)
    return fail(FA_E_ARG, "fa_facet_load_apply: negative count");
  if (!load_mode_ok(load->traction_mode) || !load_mode_ok(load->pressure_mode))
    return fail(FA_E_ARG, "fa_facet_load_apply: value modes %d / %d (FA_LOAD_*)", load->traction_mode, load->pressure_mode);
  if ((load->traction_mode != FA_LOAD_NONE && !load->traction) || (load->pressure_mode != FA_LOAD_NONE && !load->pressure))
    return fail(FA_E_ARG, "fa_facet_load_apply: a value mode is set and its pointer is null");
  FacetTables T;
  if ((rc = get_facet_tables(mesh->cell_type, mesh->degree, load->qdeg, &T))) return rc;
  if (load->nk != T.nk)
    return fail(FA_E_ARG, "fa_facet_load_apply: nk %d, the element's facets hold %d nodes", load->nk, T.nk);
  if (load->nfacets > INT32_MAX / T.nk) return fail(FA_E_CAPACITY, "fa_facet_load_apply: entries slot * nk + k are int32");
  if (load->nloaded == 0 || load->nfacets == 0) return FA_OK;
  if (load->traction_mode == FA_LOAD_NONE && load->pressure_mode == FA_LOAD_NONE) return FA_OK;
  if (!load->facet_cell || !load->facet_local || !load->nodes || !load->node_ptr || !load->entries)
    return fail(FA_E_ARG, "fa_facet_load_apply: null plan array");
  const bool per_facet = load->traction_mode == FA_LOAD_FACET || load->pressure_mode == FA_LOAD_FACET;
  if (per_facet && !load->facet_value) return fail(FA_E_ARG, "fa_facet_load_apply: per-facet values need facet_value");
  hipStream_t s = (hipStream_t)stream;
  MeshView M{mesh->cells, mesh->geom, mesh->x, mesh->ncells, mesh->nnodes, mesh->nn, mesh->nv, mesh->gdim};
  FacetLoadView L{load->nfacets, load->nloaded, load->nvalues, load->facet_cell, load->facet_local, load->facet_value,
                  load->nodes, load->node_ptr, load->entries, load->traction_mode, load->pressure_mode,
                  load->traction, load->pressure};
  const int grid = grid_for(load->nloaded);
  switch (mesh->cell_type) {
    case FA_TRIANGLE: k_facet_load<2, 3><<<grid, 256, 0, s>>>(M, L, T, alpha, b); break;
    case FA_QUADRILATERAL: k_facet_load<2, 4><<<grid, 256, 0, s>>>(M, L, T, alpha, b); break;
    case FA_TETRAHEDRON: k_facet_load<3, 4><<<grid, 256, 0, s>>>(M, L, T, alpha, b); break;
    case FA_HEXAHEDRON: k_facet_load<3, 8><<<grid, 256, 0, s>>>(M, L, T, alpha, b); break;
  }
  LAUNCH_CHECK();
  return FA_OK;
}
