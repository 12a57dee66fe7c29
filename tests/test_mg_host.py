"""Host side of the geometric multigrid (femasm.mg), no GPU: the lattice transfer stencil against
brute-force point location in the coarse mesh (p- and h-transfers on all four cell types), the
child -> parent cell map used to average per-cell coefficients, hierarchy planning with its
ValueErrors, and the coarsening of the constraint markers."""
import numpy as np
import pytest
import torch

CASES = [(3, (2, 3)), (4, (2, 3)), (-4, (2, 1, 2)), (8, (1, 2, 2))]
LENGTHS = {2: (1.0, 1.0), 3: (1.0, 1.0, 1.0)}


def _mesh(ct, n):
    from femasm import mesh

    if len(n) == 2:
        return mesh.create_rectangle(LENGTHS[2], n, mesh.CellType(ct))
    return mesh.create_box(LENGTHS[3], n, mesh.CellType(ct))


def _cell_coordinates(m, X):
    """For points X [npts, gdim]: (cell containing each, the cell's P1 / Q1 basis values there
    [npts, nverts]) by brute force over all cells."""
    from femasm import fem

    x = m.x.numpy()
    cells = m.cells.numpy().astype(np.int64)
    simplex = fem.is_simplex(m.cell_type)
    gd = m.gdim
    found = np.full(X.shape[0], -1)
    basis = np.zeros((X.shape[0], cells.shape[1]))
    for c, vs in enumerate(cells):
        v = x[vs]
        if simplex:
            T = (v[1:] - v[0]).T  # x = v0 + T xi
            xi = np.linalg.solve(T, (X - v[0]).T).T
        else:  # axis-aligned boxes: vertex 0 is the low corner, the last one the high corner
            xi = (X - v[0]) / (v[-1] - v[0])
        phi = fem._geometry_basis(m.cell_type, xi)
        inside = (phi >= -1e-12).all(1) if simplex else ((xi >= -1e-12) & (xi <= 1 + 1e-12)).all(1)
        new = inside & (found < 0)
        found[new] = c
        basis[new] = phi[new]
    assert (found >= 0).all()
    return found, basis, gd


def _brute_force_P(mc, Xf):
    found, basis, _ = _cell_coordinates(mc, Xf)
    cells = mc.cells.numpy().astype(np.int64)
    P = np.zeros((Xf.shape[0], mc.num_vertices))
    for i in range(Xf.shape[0]):
        P[i, cells[found[i]]] = basis[i]  # continuous basis: any containing cell gives the same row
    return P


@pytest.mark.parametrize("ct,n", CASES)
@pytest.mark.parametrize("mode", ["p", "h"])
def test_transfer_matrix_is_coarse_basis_at_fine_nodes(ct, n, mode):
    from femasm import fem, mg

    mc = _mesh(ct, n)
    if mode == "p":  # the degree-2 nodes of the same mesh
        Xf = fem.functionspace(mc, ("Lagrange", 2, (1,))).tabulate_dof_coordinates().numpy()
    else:  # the vertices of the mesh with every n doubled
        Xf = _mesh(ct, tuple(2 * k for k in n)).x.numpy()
    t = mg.Transfer(len(n), fem.is_simplex(ct), 1, n)
    P = mg.transfer_matrix(t).toarray()
    ref = _brute_force_P(mc, Xf)
    assert P.shape == ref.shape
    assert np.abs(P - ref).max() <= 1e-14
    # rows sum to one and a linear field is reproduced exactly
    Xc = mc.x.numpy()
    w = np.array([2.0, -3.0, 0.5])[:len(n)]
    assert np.abs(P @ (1.0 + Xc @ w) - (1.0 + Xf @ w)).max() <= 1e-14
    # blocked dofs: node * bs + comp
    P3 = mg.transfer_matrix(mg.Transfer(len(n), fem.is_simplex(ct), 3, n)).toarray()
    for c in range(3):
        np.testing.assert_array_equal(P3[c::3, c::3], P)
    assert np.count_nonzero(P3) == 3 * np.count_nonzero(P)


@pytest.mark.parametrize("ct,n", CASES)
def test_injection_picks_the_coinciding_nodes(ct, n):
    from femasm import fem, mg

    t = mg.Transfer(len(n), fem.is_simplex(ct), 1, n)
    inj = mg.injection_nodes(t).numpy()
    Xc = _mesh(ct, n).x.numpy()
    Xf = _mesh(ct, tuple(2 * k for k in n)).x.numpy()
    np.testing.assert_allclose(Xf[inj], Xc, rtol=0, atol=1e-15)
    P = mg.transfer_matrix(t).toarray()
    np.testing.assert_array_equal(P[inj], np.eye(Xc.shape[0]))


@pytest.mark.parametrize("ct,n", CASES)
def test_parent_cells(ct, n):
    from femasm import mg

    mc = _mesh(ct, n)
    mf = _mesh(ct, tuple(2 * k for k in n))
    parent = mg.parent_cells(ct, n).numpy()
    assert parent.shape == (mf.num_cells,)
    # every coarse cell has exactly 2^d children
    np.testing.assert_array_equal(np.bincount(parent, minlength=mc.num_cells), 2 ** len(n))
    # each fine centroid has barycentric coordinates >= 0 in its parent (strictly inside, in fact)
    cent = mf.x.numpy()[mf.cells.numpy().astype(np.int64)].mean(1)
    x = mc.x.numpy()
    from femasm import fem

    for c in range(mc.num_cells):
        v = x[mc.cells.numpy()[c].astype(np.int64)]
        pts = cent[parent == c]
        if fem.is_simplex(ct):
            xi = np.linalg.solve((v[1:] - v[0]).T, (pts - v[0]).T).T
            lam = np.concatenate([1.0 - xi.sum(1, keepdims=True), xi], 1)
            assert (lam >= 1e-3).all(), (c, lam.min())
        else:
            xi = (pts - v[0]) / (v[-1] - v[0])
            assert ((xi >= 1e-3) & (xi <= 1 - 1e-3)).all()


def _space(ct, n, p, **kw):
    from femasm import fem, mesh

    if len(n) == 2:
        m = mesh.create_rectangle((1.0, 1.0), n, mesh.CellType(ct), **kw)
    else:
        m = mesh.create_box((1.0, 1.0, 1.0), n, mesh.CellType(ct), **kw)
    return fem.functionspace(m, ("Lagrange", p, (len(n),)))


def test_level_table():
    from femasm import mg

    V = _space(-4, (8, 4, 12), 2)
    assert V.num_dofs == 17 * 9 * 25 * 3
    # default coarse_dofs: the degree-1 level (1755 dofs) is small enough to factor
    assert mg.plan_hierarchy(V) == [(2, (8, 4, 12)), (1, (8, 4, 12))]
    # all the way down: (2, 1, 3) has odd entries and ends the halving
    full = [(2, (8, 4, 12)), (1, (8, 4, 12)), (1, (4, 2, 6)), (1, (2, 1, 3))]
    assert mg.plan_hierarchy(V, coarse_dofs=0) == full
    assert mg.plan_hierarchy(V, coarse_dofs=5 * 3 * 7 * 3) == full[:3]  # stops where a level fits
    assert mg.plan_hierarchy(V, coarse_dofs=0, max_levels=2) == full[:2]
    assert mg.plan_hierarchy(V, coarse_dofs=10 ** 9) == full[:1]
    assert mg.plan_hierarchy(_space(4, (8, 8), 1), coarse_dofs=0) == [(1, (8, 8)), (1, (4, 4)), (1, (2, 2)), (1, (1, 1))]


def test_unsupported_spaces_raise():
    from femasm import fem, mesh, mg

    V = _space(-4, (2, 2, 2), 1)
    m = V.mesh
    Vu = fem.functionspace(mesh.Mesh(m.cell_type, m.x, m.cells, None, None), ("Lagrange", 1, (3,)))
    with pytest.raises(ValueError, match="structured"):
        mg.plan_hierarchy(Vu)
    with pytest.raises(ValueError, match="z_range"):
        mg.plan_hierarchy(_space(-4, (2, 2, 4), 1, z_range=(0, 2)), coarse_dofs=0)
    with pytest.raises(ValueError, match="left"):
        mg.plan_hierarchy(_space(3, (4, 4), 2, diagonal="left"), coarse_dofs=0)
    with pytest.raises(ValueError, match="degree"):
        mg.plan_hierarchy(_space(4, (4, 4), 3), coarse_dofs=0)
    with pytest.raises(ValueError, match="no coarser level"):
        mg.plan_hierarchy(_space(3, (4, 5), 1), coarse_dofs=0)
    # an odd n is fine below a degree-2 level, and for a space small enough to factor
    assert mg.plan_hierarchy(_space(3, (4, 5), 2), coarse_dofs=0) == [(2, (4, 5)), (1, (4, 5))]
    assert mg.plan_hierarchy(_space(3, (4, 5), 1)) == [(1, (4, 5))]
    # the constructor raises the same errors before it touches the device
    with pytest.raises(ValueError, match="left"):
        Vl = _space(3, (4, 4), 2, diagonal="left")
        mg.GeometricMultigrid(fem.LinearElasticity(Vl, E=1.0), coarse_dofs=0)


def test_constraints_coarsen_with_the_coinciding_nodes():
    from femasm import fem, mg

    n = (4, 2, 2)
    V2 = _space(-4, n, 2)
    on_plane = lambda x: torch.isclose(x[0], torch.zeros_like(x[0]))
    bc = fem.dirichletbc(0.0, fem.locate_dofs_geometrical(V2, on_plane), V2, components=[0, 2])
    marker, _ = fem._combine_bcs(V2, [bc], with_g=False)
    for nc, Vc in (((4, 2, 2), _space(-4, (4, 2, 2), 1)), ((2, 1, 1), _space(-4, (2, 1, 1), 1))):
        marker = mg.coarsen_marker(marker, mg.Transfer(3, True, 3, nc))
        bcc = fem.dirichletbc(0.0, fem.locate_dofs_geometrical(Vc, on_plane), Vc, components=[0, 2])
        ref, _ = fem._combine_bcs(Vc, [bcc], with_g=False)
        assert marker.dtype == torch.int8 and marker.is_contiguous()
        np.testing.assert_array_equal(marker.numpy(), ref.numpy())
        assert int(marker.sum()) == 2 * (nc[1] + 1) * (nc[2] + 1)
    assert mg.coarsen_marker(None, mg.Transfer(3, True, 3, (2, 1, 1))) is None


def test_chebyshev_coefficients_damp_the_interval():
    """The smoother's error polynomial 1 - lambda p(lambda) of the (c_d, c_r) recurrence stays below
    the Chebyshev bound on [lo, hi] and equals 1 at 0."""
    from femasm import mg

    lo, hi = 0.1 * 1.7, 1.1 * 1.7
    for degree in (1, 2, 3, 8):
        lam = np.linspace(lo, hi, 401)
        x, d = np.zeros_like(lam), np.zeros_like(lam)
        for cd, cr in mg.chebyshev_coefficients(lo, hi, degree):
            d = cd * d + cr * (1.0 - lam * x)  # scalar problem lam x = 1
            x = x + d
        err = np.abs(1.0 - lam * x)
        sigma = (hi + lo) / (hi - lo)
        bound = 1.0 / np.cosh(degree * np.arccosh(sigma))
        assert err.max() <= bound * (1 + 1e-12), (degree, err.max(), bound)
