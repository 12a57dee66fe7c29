"""GPU checks of the scalar functionals (k_functional_cells / k_functional_reduce through
fem.assemble_scalar) and of the Newton energy line search.

Per-cell parity: |device - host|_c <= 1e-12 * magnitude_c, host = the torch definition on the same mesh moved
to the CPU and magnitude_c the cell integral with every product taken in absolute value
(fem.assemble_scalar_host). Totals: |total - fsum(cell values)| <= 1e-12 * sum |cell values| (the tree sum's
bound is about log2(n) eps) and bit-identical run to run.

Line search at a large load: on the 2^3 x 6 P1-tetrahedron cube with rollers, plain
Newton (max_it 25) from u = 0 survived every traction 0.05 E, 0.1 E, .. 3.2 E (10 iterations at 3.2 E), so
the committed test asserts convergence and non-increasing energies of the line search at LOAD = 3.2 E, where
it halves the first step and converges in 6 iterations."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import irregular_meshes as IM  # noqa: E402
import transformed_meshes as TM  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-12
TRI, QUAD, TET, HEX = 3, 4, -4, 8
LOAD = 3.2  # traction / E of the large-load test: the last load of the doubling, which plain Newton survived


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _rand(shape, seed, amp=1.0):
    return amp * (torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5)


def _spaces(m_host, p, dev):
    """The space on the GPU and the same space (same dofmap) on the host mesh."""
    from femasm import fem

    gd = m_host.gdim
    V = fem.functionspace(m_host.to(dev), ("Lagrange", p, (gd,)))
    Vh = fem.FunctionSpace.from_dofmap(m_host, p, gd, V.dofmap.cpu(), V.num_nodes)
    return V, Vh


def _functionals(V, u, law_kw, d=None):
    """Every functional of a space at the nodal field u (on V's device): name -> descriptor."""
    from femasm import fem

    dev_ = V.mesh.device
    nc, gd, p = V.mesh.num_cells, V.mesh.gdim, V.degree
    u = u.to(dev_)
    E = (1.0 + torch.arange(nc, dtype=torch.float64) % 7).to(dev_)
    nq = len(fem.quadrature(V.mesh.cell_type, 2 * p)[1])
    g = _rand((nc, nq, gd), 21, 0.2).to(dev_)
    G = _rand((nc, nq, gd, gd), 22, 0.5).to(dev_)
    out = {
        "measure": fem.Measure(V),
        "lin": fem.StrainEnergy(fem.LinearElasticity(V, E=E, nu=0.3, u=u, **law_kw)),
        "neo": fem.StrainEnergy(fem.NeoHookean(V, E=E, nu=0.3, u=u, **law_kw)),
        "l2": fem.L2Norm2(u, V=V), "l2-g": fem.L2Norm2(u, g=g, V=V),
        "h1": fem.H1Semi2(u, V=V), "h1-G": fem.H1Semi2(u, G=G, V=V),
        "l2-q": fem.L2Norm2(u, V=V, qdeg=2 * p + 1),
    }
    if d is not None:
        for t in ("hand", "ad"):
            out["damage-" + t] = fem.StrainEnergy(fem.AsymDamage(V, E=E, nu=0.3, u=u, d=d.to(dev_), tangent=t))
    return out


def _state(Vh, n_axis):
    xn = Vh.tabulate_dof_coordinates()
    xs = (xn - xn.min(0).values) / (xn.max(0).values - xn.min(0).values)
    h = 1.0 / (n_axis * Vh.degree)
    return (0.05 * torch.sin(torch.pi * xs).reshape(-1) + _rand(Vh.num_dofs, 11, 0.05 * h)).contiguous()


def _check_parity(V, Vh, u, what, law_kw=None, d=None):
    from femasm import fem

    dev_fn = _functionals(V, u, law_kw or {}, d)
    host_fn = _functionals(Vh, u, law_kw or {}, d)
    for name, M in dev_fn.items():
        out = torch.full((V.mesh.num_cells,), math.nan, dtype=torch.float64, device=V.mesh.device)
        got = fem.assemble_scalar(M, cellwise=True, out=out)
        assert got is out
        got = got.cpu().numpy()
        want, mag = (t.numpy() for t in fem.assemble_scalar_host(host_fn[name]))
        assert np.isfinite(got).all(), f"{what} {name}: a cell was not written"
        ratio = np.abs(got - want) / mag
        print(f"{what} {name}: max |dev - host| / magnitude = {ratio.max():.2e}")
        assert (np.abs(got - want) <= RTOL * mag).all(), f"{what} {name}: worst ratio {ratio.max():.3e}"
        assert np.array_equal(fem.assemble_scalar(M, cellwise=True).cpu().numpy(), got)  # run to run


# ------------------------------------------------------------------------------------ 6. per-cell parity
STRUCTURED = [(ct, p, n) for ct, n in ((TRI, (3, 3)), (QUAD, (3, 3)), (TET, (3, 3, 3)), (HEX, (3, 3, 3))) for p in (1, 2)]
STRUCTURED += [(HEX, 3, (2, 2, 2))]


@pytest.mark.parametrize("ct,p,n", STRUCTURED)
def test_cellwise_matches_host_on_structured_meshes(dev, ct, p, n):
    from femasm import mesh

    m = mesh.create_unit_square(*n, cell_type=ct) if len(n) == 2 else mesh.create_unit_cube(*n, cell_type=ct)
    V, Vh = _spaces(m, p, dev)
    _check_parity(V, Vh, _state(Vh, max(n)), f"cell {ct} P{p}", law_kw=dict(quadrature_degree=None))


@pytest.mark.parametrize("family,tr", [("tri-P2", "shear"), ("tet-P2", "shear"), ("quad-Q2", "shear"),
                                       ("hex-Q1", "shear"), ("tri-P1", "shear")]
                         + [(f, None) for f in TM.WARPED])
def test_cellwise_matches_host_on_transformed_meshes(dev, family, tr):
    ct, p, n, _ = TM.FAMILIES[family]
    m = TM.base_mesh(family)
    V0, _ = _spaces(m, p, dev)
    u = _state(fem_space_on_host(m, p, V0), max(n))  # the state of the untransformed nodes
    if tr is not None:
        m = TM.apply(m, tr)
    V, Vh = _spaces(m, p, dev)
    _check_parity(V, Vh, u, f"{family} {tr}")


def fem_space_on_host(m, p, V):
    from femasm import fem

    return fem.FunctionSpace.from_dofmap(m, p, m.gdim, V.dofmap.cpu(), V.num_nodes)


@pytest.mark.parametrize("p", [1, 2])
def test_cellwise_matches_host_on_a_delaunay_mesh(dev, p):
    m = IM.delaunay_tets_n4()
    V, Vh = _spaces(m, p, dev)
    _check_parity(V, Vh, _state(Vh, 4), f"delaunay P{p}")


def test_cellwise_damage_kinds_on_square_msh(dev):
    m = IM.square_msh()
    V, Vh = _spaces(m, 1, dev)
    xn = Vh.tabulate_dof_coordinates()
    A = torch.tensor([[2e-2, 1e-2], [0.0, -5e-3]], dtype=torch.float64)
    u = (xn @ A.T + 2e-3 * torch.stack([torch.sin(3 * xn[:, 0] + 2 * xn[:, 1]),
                                        torch.cos(2 * xn[:, 0] - 3 * xn[:, 1])], 1)).reshape(-1).contiguous()
    r = torch.rand(V.num_nodes, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
    d = torch.where(r < 0.6, 1.2 * r, torch.zeros_like(r))  # damaged, undamaged and mixed cells
    _check_parity(V, Vh, u, "square.msh", d=d)
    _check_parity(V, Vh, -u, "square.msh (compression)", d=d)


# ------------------------------------------------------------------------------------ 7. totals
@pytest.fixture(scope="module")
def big(dev):
    """36^3 x 6 P1 tetrahedra with a linear strain energy: 279 936 cells, 1094 tile partials."""
    from femasm import fem, mesh

    m = mesh.create_unit_cube(36, 36, 36, device=dev)
    V = fem.functionspace(m, ("Lagrange", 1, (3,)))
    u = _rand(V.num_dofs, 3, 1e-2).to(dev)
    E = (1.0 + torch.arange(m.num_cells, dtype=torch.float64) % 7).to(dev)
    return fem.StrainEnergy(fem.LinearElasticity(V, E=E, nu=0.3, u=u))


def _check_total(M, what):
    from femasm import fem

    t1, t2 = fem.assemble_scalar(M), fem.assemble_scalar(M)
    assert t1.shape == () and t1.dtype == torch.float64 and t1.device == M.V.mesh.device
    cells = fem.assemble_scalar(M, cellwise=True).cpu().numpy()
    t3 = fem.assemble_scalar(M)
    a, b, c = float(t1), float(t2), float(t3)
    assert a == b == c, f"{what}: totals differ run to run"
    ref, scale = math.fsum(cells), math.fsum(np.abs(cells))
    print(f"{what}: {cells.size} cells, total {a:.12e}, |total - fsum| / sum|c| = {abs(a - ref) / max(scale, 1e-300):.2e}")
    assert abs(a - ref) <= RTOL * scale
    return a


@pytest.mark.parametrize("nc", [0, 1, 63, 257, 1260])
def test_totals_of_cell_subsets(dev, nc):
    from femasm import fem, mesh

    full = mesh.create_unit_cube(7, 6, 5)
    assert full.num_cells == 1260
    m = mesh.Mesh(full.cell_type, full.x, full.cells[:nc].contiguous()).to(dev)
    V = fem.functionspace(m, ("Lagrange", 1, (3,)))
    u = _rand(V.num_dofs, 3, 1e-2).to(dev)
    E = (1.0 + torch.arange(nc, dtype=torch.float64) % 7).to(dev)
    for name, M in (("measure", fem.Measure(V)), ("lin", fem.StrainEnergy(fem.LinearElasticity(V, E=E, nu=0.3, u=u))),
                    ("h1", fem.H1Semi2(u, V=V))):
        total = _check_total(M, f"{name} nc={nc}")
        if nc == 0:
            assert total == 0.0 and math.copysign(1.0, total) == 1.0
    if nc == 1260:
        vol = float(fem.assemble_scalar(fem.Measure(V)))
        assert abs(vol - 1.0) <= 1e-13


def test_total_with_more_than_1024_partials(dev, big):
    assert big.V.mesh.num_cells == 279936
    _check_total(big, "36^3 x 6 P1 tets")


# ------------------------------------------------------------------------------------ 8. an inverted cell
def test_neo_hookean_energy_of_an_inverted_cell_is_not_finite(dev):
    from femasm import fem, mesh

    m = mesh.create_unit_cube(2, 2, 2)
    X = m.x[m.cells[0].to(torch.int64)]
    u = torch.zeros_like(m.x)
    u[int(m.cells[0, 0])] = 2.5 * (X[1:].mean(0) - X[0])  # vertex 0 of cell 0 pushed through its opposite face
    V = fem.functionspace(m.to(dev), ("Lagrange", 1, (3,)))
    M = fem.StrainEnergy(fem.NeoHookean(V, E=1.0, nu=0.3, u=u.reshape(-1).to(dev)))
    cells = fem.assemble_scalar(M, cellwise=True).cpu().numpy()
    assert not np.isfinite(cells[0]) and np.isfinite(cells).sum() > 0
    assert not math.isfinite(float(fem.assemble_scalar(M)))
    ok = fem.StrainEnergy(fem.NeoHookean(V, E=1.0, nu=0.3, u=torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)))
    assert float(fem.assemble_scalar(ok)) == 0.0


# ------------------------------------------------------------------------------------ 9. Newton end to end
def _cube_solve(dev, matrix_free, line_search, load=0.05, max_it=50, error=True, tape=None, replay=False):
    """tape (assembled only): a list the problem's J appends every assembled matrix's values to, or, with
    replay, takes them from instead of assembling."""
    from femasm import fem, nls
    from test_gpu_facet_load import NEO, _on_plane, _rollers

    class Problem(nls.NonlinearProblem):
        def J(self, x, A):
            if tape is None:
                return super().J(x, A)
            if replay:
                for (_, _, d), s in zip(A.parts, tape.pop(0)):
                    d.copy_(s)
            else:
                super().J(x, A)
                tape.append([d.clone() for _, _, d in A.parts])

    m = mesh_cube(dev)
    V = fem.functionspace(m, ("Lagrange", 1, (3,)))
    ld = fem.SurfaceLoad(V, _on_plane(m, 0, 1.0), traction=[load * NEO["E"], 0.0, 0.0])
    u = fem.Function(V)
    F = fem.NeoHookean(V, u=u, loads=[ld], **NEO)
    problem = Problem(F, u, bcs=_rollers(V, m, dev), matrix_free=matrix_free)
    solver = nls.NewtonSolver(None, problem)
    solver.line_search, solver.max_it, solver.error_on_nonconvergence = line_search, max_it, error
    its, converged = solver.solve(u)
    return solver, u, its, converged


def mesh_cube(dev):
    from femasm import mesh

    return mesh.create_unit_cube(2, 2, 2, cell_type=mesh.CellType.tetrahedron, device=dev)


@pytest.mark.parametrize("matrix_free", [False, True])
def test_line_search_takes_full_steps_at_a_small_load(dev, matrix_free):
    """Every step is 1 and the iterates are bit-identical to the plain solver's, assembled and matrix-free.
    The matrix-free operator is bit-reproducible, so two independent solves are compared. The assembled
    neo-Hookean matrix is not (its row gather adds with LDS atomics from four waves, DESIGN.md section 3.2:
    two PLAIN solves already differ in the last bits, residuals 4.5464012e-12 and 4.5464008e-12 measured),
    so there the line-search solve is given the very matrices the plain solve assembled, and everything
    else (residuals, CG, updates, the energy evaluations in between) must reproduce the plain iterates."""
    tape = None if matrix_free else []
    plain, u0, its0, conv0 = _cube_solve(dev, matrix_free, None, tape=tape)
    ls, u1, its1, conv1 = _cube_solve(dev, matrix_free, "energy", tape=tape, replay=True)
    assert not tape  # every recorded matrix was used
    print(f"matrix_free={matrix_free}: {its1} iterations, steps {ls.steps}, energies {ls.energies}")
    assert conv0 and conv1 and its0 == its1 > 0
    assert ls.steps == [1.0] * its1 and len(ls.energies) == its1 + 1
    assert torch.equal(u0.x, u1.x) and plain.history == ls.history  # bit-identical iterates
    assert all(b <= a for a, b in zip(ls.energies, ls.energies[1:]))


# ------------------------------------------------------------------------------------ 10. a large load
@pytest.mark.parametrize("matrix_free", [False, True])
def test_line_search_converges_at_a_large_load(dev, matrix_free):
    ls, u, its, conv = _cube_solve(dev, matrix_free, "energy", load=LOAD, max_it=25)
    print(f"matrix_free={matrix_free}: load {LOAD} E, {its} iterations, steps {ls.steps}, energies {ls.energies}")
    assert conv and bool(torch.isfinite(u.x).all())
    assert all(b <= a for a, b in zip(ls.energies, ls.energies[1:]))
