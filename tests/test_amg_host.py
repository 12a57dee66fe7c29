"""Host side of the smoothed-aggregation multigrid (femasm.amg, mg.SmoothedAggregation), no GPU: the
aggregation against the independent restatement in tests/amg_reference.py, node for node; the rigid-body
modes through the tentative prolongator and in the null space of every coarse matrix; the symbolic product
lists against scipy's P.T @ A @ P; the dead rotations; the refusals. Matrices come from the CPU oracle or are
random SPD block matrices; the set-up runs in torch on the CPU (index_add in list order)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import amg_reference as R
import irregular_meshes as IM

RBAR = 1e-12  # the per-row bar of tests/rowparity.py


def _box(n):
    from femasm import mesh

    b = mesh.create_box((1.0, 1.0, 1.0), (n, n, n), mesh.CellType.tetrahedron)
    return mesh.Mesh(b.cell_type, b.x, b.cells, None, None)


MESHES = {"square": IM.square_msh, "fan70": lambda: IM.fan(70), "box3": lambda: _box(3),
          "delaunay": IM.delaunay_tets_n4, "square_r1": lambda: IM.square_msh(refine=1)}


def _host_matrix(oracle, m, marker=None, seed=0):
    """Linear elasticity, degree 1, E random in [1, 200] per cell, as a la.MatrixCSR on the CPU."""
    from femasm import la

    cells = m.cells.numpy()
    ip, ix = oracle.sparsity(cells, m.num_vertices)
    E = np.random.default_rng(seed).uniform(1.0, 200.0, m.num_cells)
    lam, mu = oracle.lame(E, 0.3)
    vals = oracle.assemble_elasticity(int(m.cell_type), 1, cells, cells, m.x.numpy(), lam, mu, ip, ix, bc=marker, diag=1.0)
    return la.MatrixCSR(torch.tensor(ip), torch.tensor(ix), m.gdim, data=torch.tensor(vals))


def _pattern(oracle, m):
    ip, ix = oracle.sparsity(m.cells.numpy(), m.num_vertices)
    return torch.tensor(ip), torch.tensor(ix)


def _markers(name, m, indptr, indices):
    """Constraint markers per dof for the aggregation cases: none, x = 0 clamped with one single-component
    constraint, scattered fully constrained interior nodes, and one free node whose neighbours are all
    constrained."""
    n, g = m.num_vertices, m.gdim
    x = m.x.numpy()
    out = {"none": None}
    mk = np.zeros((n, g), np.int8)
    mk[np.isclose(x[:, 0], x[:, 0].min())] = 1
    mk[np.isclose(x[:, 0], x[:, 0].max()), 0] = 1  # one component only: the node stays free
    out["sides"] = mk.reshape(-1)
    rng = np.random.default_rng(5)
    mk = np.zeros((n, g), np.int8)
    mk[rng.random(n) < 0.25] = 1
    out["scattered"] = mk.reshape(-1)
    ip, ix = indptr.numpy(), indices.numpy()
    i = int(np.argmin(np.diff(ip)))  # a node of low valence, walled in
    mk = np.zeros((n, g), np.int8)
    nb = ix[ip[i]:ip[i + 1]]
    mk[nb[nb != i]] = 1
    out["walled"] = mk.reshape(-1)
    return out, i


def _pattern_matrix(indptr, indices, n, b):
    G = sp.csr_matrix((np.ones(indices.numel()), indices.numpy(), indptr.numpy()), shape=(n, n))
    return sp.kron(G, np.ones((b, b)), format="csr")


@pytest.mark.parametrize("name", ["square", "fan70", "box3", "delaunay"])
def test_aggregation_equals_the_reference_node_for_node(oracle, name):
    from femasm import amg

    m = MESHES[name]()
    n, g = m.num_vertices, m.gdim
    indptr, indices = _pattern(oracle, m)
    markers, walled = _markers(name, m, indptr, indices)
    A = _pattern_matrix(indptr, indices, n, g)
    for case, mk in markers.items():
        free = R.free_nodes(mk, n, g)
        ref, nref = R.aggregate(R.node_graph(A, g, free), free)
        agg, nagg = amg.aggregate(indptr, indices, torch.tensor(free))
        agg = agg.numpy()
        assert nagg == nref and np.array_equal(agg, ref), (name, case)
        assert (agg[free] >= 0).all() and (agg[free] < nagg).all()  # every free node in exactly one aggregate
        assert (agg[~free] == -1).all()  # no fully constrained node in any
        assert np.array_equal(np.unique(agg[free]), np.arange(nagg))
        if case == "walled":
            assert free[walled] and (agg == agg[walled]).sum() == 1  # an aggregate of its own
        if case == "sides":
            assert 0 < (~free).sum() < (np.asarray(mk).reshape(n, g) != 0).any(1).sum()


def test_row_max_primitive_on_the_cpu():
    from femasm import amg

    indptr = torch.tensor([0, 2, 2, 5, 6])
    indices = torch.tensor([1, 3, 0, 1, 2, 3], dtype=torch.int32)
    v = torch.tensor([5, 9, -2, 7])
    assert amg.csr_row_max(indptr, indices, v).tolist() == [9, 0, 9, 7]
    free = torch.tensor([1, 1, 0, 1], dtype=torch.int8)
    assert amg.csr_row_max(indptr, indices, v, free).tolist() == [9, 0, 0, 7]
    p = amg.node_priorities(5)
    assert p.tolist() == [(((i * 2654435761) % 2 ** 32) << 31) + i + 1 for i in range(5)]


def _dinv(A, b):
    Dinv = R.block_jacobi_inverse(A, b)
    n = A.shape[0] // b
    return Dinv, torch.tensor(np.stack([Dinv[i * b:(i + 1) * b, i * b:(i + 1) * b].toarray() for i in range(n)]))


def _levels(A, x, marker, min_nodes=10):
    """femasm.amg levels on the CPU from a la matrix down, with the reference's lambda_max: [(A scipy, b, x,
    marker, Aggregation, lmax)]. Stops at min_nodes nodes, as coarse_dofs does: a level of a handful of nodes
    coarsens to one aggregate, whose unconstrained Galerkin matrix is zero up to rounding."""
    from femasm import amg

    out = []
    while A.num_block_rows > min_nodes:
        b = A.bs
        As = sp.csr_matrix(A.to_scipy())
        tr = amg.Aggregation(A, x, marker)
        Dinv_s, Dinv = _dinv(As, b)
        lmax = R.lambda_max(As, Dinv_s)
        tr.smooth(A, Dinv, lmax)
        tr.galerkin(A)
        out.append((As, b, x.numpy(), None if marker is None else marker.numpy(), tr, lmax))
        A, x, marker = tr.Ac, tr.xc, tr.marker_c
    return out


@pytest.mark.parametrize("name", ["square_r1", "delaunay", "box3"])
def test_rigid_body_modes_pass_through_every_level(oracle, name):
    """T B_c = B on the free dofs, and without bcs the modes are in the null space of every coarse matrix:
    |A_c B_c| <= 1e-10 |A_c| |B_c| (a wrong rotation sign fails this)."""
    m = MESHES[name]()
    A = _host_matrix(oracle, m)
    levels = _levels(A, m.x, None)
    assert len(levels) >= (2 if name == "square_r1" else 1)
    for As, b, x, mk, tr, _ in levels:
        assert not bool(tr.dead.any()), "the unconstrained test meshes have no dead rotations"
        xc = tr.xc.numpy()
        B, Bc = R.rigid_body_modes(x, b), R.rigid_body_modes(xc, tr.nr)
        T = sp.csr_matrix(tr.T.to_scipy())
        assert np.abs(T @ Bc - B).max() <= 1e-13 * max(1.0, np.abs(B).max())
        Ac = sp.csr_matrix(tr.Ac.to_scipy())
        assert np.abs(As @ B).max() <= 1e-10 * abs(As).max() * np.abs(B).max()  # (the fine matrix has them too)
        res = np.linalg.norm(Ac @ Bc)
        bound = 1e-10 * np.linalg.norm(Ac.toarray()) * np.linalg.norm(Bc)
        print(f"{name} level {b}->{tr.nr}: |Ac Bc| = {res:.3e}, bound {bound:.3e}")
        assert res <= bound


def test_tentative_reproduces_the_modes_on_free_dofs_with_constraints(oracle):
    m = MESHES["square"]()
    indptr, indices = _pattern(oracle, m)
    markers, _ = _markers("square", m, indptr, indices)
    mk = markers["sides"]
    A = _host_matrix(oracle, m, mk)
    (As, b, x, _, tr, _), = _levels(A, m.x, torch.tensor(mk), min_nodes=30)[:1]
    free_nodes = R.free_nodes(mk, m.num_vertices, 2)
    alive = ~np.repeat(tr.dead.numpy(), 3) | np.tile([True, True, False], tr.nagg)
    B, Bc = R.rigid_body_modes(x, b), R.rigid_body_modes(tr.xc.numpy(), 3)
    got = sp.csr_matrix(tr.T.to_scipy()) @ (Bc * alive[:, None])
    rows = np.repeat(free_nodes, 2)
    assert not tr.dead.any()
    assert np.abs(got - B)[rows].max() <= 1e-13
    assert np.abs(got[~rows]).max() == 0.0
    # M_f: the constrained dofs are zero rows of P, also on the nodes that stay free
    P = sp.csr_matrix(tr.P.to_scipy())
    assert abs(P[np.asarray(mk) != 0]).sum() == 0.0


def _random_spd(n, b, rng):
    """A random sparse SPD block matrix on a ring-plus-chords graph, la.BlockCSR-compatible, with coordinates."""
    from femasm import la

    rows, cols = [], []
    for i in range(n):
        for j in {i, (i + 1) % n, (i - 1) % n, (i * 7 + 3) % n}:
            rows += [i, j]
            cols += [j, i]
    G = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    G.sum_duplicates()
    G.sort_indices()
    blocks = rng.standard_normal((G.indices.size, b, b))
    S = sp.bsr_matrix((blocks, G.indices, G.indptr), shape=(n * b, n * b))
    S = sp.csr_matrix(S + S.T)
    S = S + sp.diags(np.asarray(abs(S).sum(1)).reshape(-1) + 1.0)
    B = sp.bsr_matrix(S, blocksize=(b, b))
    B.sort_indices()
    assert np.array_equal(B.indices, G.indices)
    return la.MatrixCSR(torch.tensor(B.indptr.astype(np.int64)), torch.tensor(B.indices.astype(np.int32)), b,
                        data=torch.tensor(B.data))


@pytest.mark.parametrize("gdim,b", [(2, 2), (2, 3), (3, 3), (3, 6)])
def test_symbolic_products_equal_scipy(gdim, b):
    """Each block shape: A T, A P and P^T Y through the product lists (torch numerics) against scipy, per row;
    P against the reference's P with the same lambda_max; the stored P^T is the exact transpose."""
    rng = np.random.default_rng(11 * gdim + b)
    n = 60
    A = _random_spd(n, b, rng)
    x = torch.tensor(rng.random((n, gdim)))
    mk = np.zeros((n, b), np.int8)
    mk[3] = 1
    mk[10, 0] = 1
    mk = mk.reshape(-1)
    (As, _, xs, _, tr, lmax), = _levels(A, x, torch.tensor(mk), min_nodes=n - 1)[:1]
    P, Pt, Ac = (sp.csr_matrix(t.to_scipy()) for t in (tr.P, tr.Pt, tr.Ac))
    assert abs(Pt - P.T).max() == 0.0
    Pref, Acref, xc, mc, agg, _, _ = R.coarsen(As, xs, mk, b, lmax)
    assert np.array_equal(tr.agg.numpy(), agg) and np.array_equal(tr.marker_c.numpy(), mc)
    assert R.row_rel_error(P, Pref) <= RBAR
    unit = sp.diags(mc.astype(float))
    assert R.row_rel_error(Ac, P.T @ As @ P + unit) <= RBAR
    assert R.row_rel_error(Ac, Acref) <= RBAR
    T = sp.csr_matrix(tr.T.to_scipy())
    AT = torch.zeros_like(tr.P.data)
    tr.AT.numeric(A.data, tr.T.data, AT)
    from femasm import la

    keep = sp.diags(np.repeat(tr.free.numpy(), b).astype(float))
    assert R.row_rel_error(la.BlockCSR(tr.P.indptr, tr.P.indices, AT, tr.nagg).to_scipy(), keep @ As @ T) <= RBAR
    # the CPU gather of the block product with a vector
    v = torch.tensor(rng.standard_normal(P.shape[1]))
    assert np.abs(tr.P.mult(v).numpy() - P @ v.numpy()).max() <= 1e-13 * abs(P).sum(1).max() * np.abs(v.numpy()).max()
    med, mx = tr.PtY.list_stats()
    assert 1 <= med <= mx == int(tr.PtY.counts.max())


@pytest.mark.parametrize("name", ["square", "delaunay", "box3"])
def test_dead_rotations_keep_the_coarse_matrix_definite(oracle, name):
    """A walled-in free node is an aggregate of one: translations only, unit diagonal on its rotation dofs,
    and the coarse matrix stays SPD (box3 without walls: the lattice's collinear aggregates, if any)."""
    m = MESHES[name]()
    indptr, indices = _pattern(oracle, m)
    markers, walled = _markers(name, m, indptr, indices)
    mk = markers["walled"]
    mk = mk.copy().reshape(m.num_vertices, m.gdim)
    mk[np.isclose(m.x.numpy()[:, 0], 0.0)] = 1
    mk[walled] = 0  # (the walled-in node itself stays free wherever it lies)
    mk = mk.reshape(-1)
    A = _host_matrix(oracle, m, mk)
    (As, b, x, _, tr, lmax), = _levels(A, m.x, torch.tensor(mk), min_nodes=m.num_vertices - 1)[:1]
    g, nr = m.gdim, tr.nr
    I = int(tr.agg[walled])
    assert bool(tr.dead[I]) and int((tr.agg == I).sum()) == 1
    Ac = sp.csr_matrix(tr.Ac.to_scipy()).toarray()
    mc = tr.marker_c.numpy()
    assert mc.reshape(-1, nr)[I, g:].all() and not mc.reshape(-1, nr)[:, :g].any()
    on = mc != 0
    assert np.array_equal(Ac[on][:, on], np.eye(on.sum())) and np.abs(Ac[on][:, ~on]).max() == 0.0
    assert np.abs(Ac - Ac.T).max() <= 1e-12 * np.abs(Ac).max()
    ev = np.linalg.eigvalsh(0.5 * (Ac + Ac.T))
    print(f"{name}: {int(tr.dead.sum())} dead of {tr.nagg} aggregates, coarse eigenvalues {ev[0]:.3e} .. {ev[-1]:.3e}")
    assert ev[0] > 0.0
    Pref, Acref, *_ = R.coarsen(As, x, mk, b, lmax)
    assert R.row_rel_error(Ac, Acref) <= RBAR


def test_unserved_spaces_raise_and_geometric_multigrid_still_refuses():
    from femasm import fem, mesh, mg

    sq = IM.square_msh()
    V1 = fem.functionspace(sq, ("Lagrange", 1, (2,)))
    with pytest.raises(ValueError, match="no parent mesh to coarsen to"):
        mg.GeometricMultigrid(fem.LinearElasticity(V1, E=1.0), coarse_dofs=10)
    M = mg.SmoothedAggregation(fem.LinearElasticity(V1, E=1.0), coarse_dofs=10)  # the same space is served
    assert M.updates == 0 and M.rebuilds == 0
    with pytest.raises(ValueError, match="bs = gdim"):
        mg.SmoothedAggregation(fem.LinearElasticity(fem.functionspace(sq, ("Lagrange", 1, (1,))), E=1.0))
    with pytest.raises(ValueError, match="degree"):
        mg.SmoothedAggregation(fem.LinearElasticity(fem.functionspace(sq, ("DG", 0, (2,))), E=1.0))
    q = mesh.create_rectangle((1.0, 1.0), (4, 4), mesh.CellType.quadrilateral)
    with pytest.raises(ValueError, match="degree"):
        mg.SmoothedAggregation(fem.LinearElasticity(fem.functionspace(q, ("Lagrange", 3, (2,))), E=1.0))
    slab = mesh.create_box((1.0, 1.0, 1.0), (2, 2, 4), mesh.CellType.tetrahedron, z_range=(0, 2))
    with pytest.raises(ValueError, match="z_range"):
        mg.SmoothedAggregation(fem.LinearElasticity(fem.functionspace(slab, ("Lagrange", 1, (3,))), E=1.0))
    qu = mesh.Mesh(q.cell_type, q.x, q.cells, None, None)
    with pytest.raises(ValueError, match="triangles or tetrahedra"):
        mg.SmoothedAggregation(fem.LinearElasticity(fem.functionspace(qu, ("Lagrange", 2, (2,))), E=1.0))
    mg.SmoothedAggregation(fem.LinearElasticity(fem.functionspace(qu, ("Lagrange", 1, (2,))), E=1.0))  # degree 1: any cell
    with pytest.raises(ValueError, match="max_levels"):
        mg.SmoothedAggregation(fem.LinearElasticity(V1, E=1.0), max_levels=0)
    with pytest.raises(ValueError, match="smoother_degree"):
        mg.SmoothedAggregation(fem.LinearElasticity(V1, E=1.0), smoother_degree=0)
