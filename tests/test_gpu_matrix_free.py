"""Matrix-free Jacobian action (fem.JacobianOperator: fa_apply_jacobian / fa_jacobian_block_diag) against
the assembled matrix of the unchanged fem.assemble_matrix(a, bcs, diagonal), which the existing suite
pins to the oracle.

Bar, per scalar row i: |y - S x|_i <= 1e-12 * (|S| |x|)_i (tests/rowparity.RTOL); a row with
(|S| |x|)_i = 0 must be reproduced exactly. x is seeded random with nonzero entries on constrained
dofs, y is pre-filled with NaN (every dof must be written), diagonal = 2.5.

Neo-Hookean states: u = 0.05 sin(pi x) plus white noise of amplitude 0.05 x the node spacing. Plain
white noise of amplitude 0.05 inverts cells on these meshes (node spacing 1/12 .. 1/40): the CPU
oracle's tangent at such a state has non-finite entries (det F < 0 under the logarithm), so there is
no reference to compare with; the noise is therefore scaled to the node spacing, which keeps every
cell's own random strain state while det F stays positive.
"""
import os

import numpy as np
import pytest
import torch

from irregular_meshes import fan
from rowparity import RTOL

pytestmark = pytest.mark.gpu

DIAG = 2.5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t):
    return t.detach().cpu().numpy()


def _mesh(ct, n, dev, perturb=0.0):
    from femasm import mesh

    m = mesh.create_unit_square(*n, cell_type=ct, device=dev) if len(n) == 2 else \
        mesh.create_unit_cube(*n, cell_type=ct, device=dev)
    if perturb:  # interior vertices moved: non-affine tensor cells
        g = torch.Generator().manual_seed(3)
        x = m.x.cpu()
        interior = ((x > 1e-9) & (x < 1 - 1e-9)).all(1)
        x[interior] += perturb / max(n) * (torch.rand(x[interior].shape, generator=g, dtype=torch.float64) - 0.5)
        m.x = x.to(dev)
    return m


def _E(oracle, m):
    return torch.tensor(oracle.e_range()[np.arange(m.num_cells) % 200], dtype=torch.float64, device=m.device)


def _rand(n, seed, dev, amp=1.0):
    g = torch.Generator().manual_seed(seed)
    return (amp * (torch.rand(n, generator=g, dtype=torch.float64) - 0.5)).to(dev)


def _form(oracle, V, kind, h):
    """kind: lin | neo | dam-hand | dam-ad. h: node spacing (scales the neo-Hookean noise)."""
    from femasm import fem

    m = V.mesh
    E = _E(oracle, m)
    if kind == "lin":
        return fem.LinearElasticity(V, E=E, nu=0.3)
    xn = V.tabulate_dof_coordinates()
    if kind == "neo":
        u = (0.05 * torch.sin(torch.pi * xn).reshape(-1) + _rand(V.num_dofs, 11, m.device, 0.05 * h)).contiguous()
        return fem.NeoHookean(V, E=E, nu=0.3, u=u)
    # damage: d > 0 on a band; u puts cells in tension (right half) and in compression (left half), with noise
    u = torch.zeros((V.num_nodes, 2), dtype=torch.float64, device=m.device)
    xc = xn[:, 0] - xn[:, 0].mean()
    u[:, 0] = 2e-3 * xc ** 2 * torch.sign(xc)
    u[:, 1] = 1e-3 * torch.sin(3.0 * xn[:, 0]) * xn[:, 1]
    u = (u.reshape(-1) + _rand(V.num_dofs, 5, m.device, 1e-4)).contiguous()
    t = (xn - xn.min(0).values) / (xn.max(0).values - xn.min(0).values)  # position in the bounding box
    d = torch.where((t[:, 1] > 0.3) & (t[:, 1] < 0.7), 0.2 + 0.6 * t[:, 0], torch.zeros_like(t[:, 0])).contiguous()
    assert float(d.max()) > 0 and float(d.min()) == 0
    return fem.AsymDamage(V, E=E, nu=0.3, u=u, d=d, tangent="hand" if kind == "dam-hand" else "ad")


def _bcs(V, which):
    """none | mixed (a plane fully constrained + one component of another plane: mixed blocks) | all."""
    from femasm import fem

    if which == "none":
        return []
    if which == "all":
        return [fem.dirichletbc(0.0, torch.arange(V.num_nodes, device=V.mesh.device), V)]
    xn = V.tabulate_dof_coordinates()
    lo, hi = float(xn[:, 0].min()), float(xn[:, 0].max())
    left = torch.nonzero(torch.isclose(xn[:, 0], torch.full_like(xn[:, 0], lo)), as_tuple=False).reshape(-1)
    right = torch.nonzero(torch.isclose(xn[:, 0], torch.full_like(xn[:, 0], hi)), as_tuple=False).reshape(-1)
    assert left.numel() > 0 and right.numel() > 0
    return [fem.dirichletbc(0.0, left, V), fem.dirichletbc(0.0, right, V, components=[0])]


def _assembled(a, bcs):
    from femasm import fem

    return fem.assemble_matrix(a, bcs=bcs, diagonal=DIAG).to_scipy().tocsr()


def _check_mult(op, S, dev, what, seed=1):
    n = S.shape[0]
    x = _rand(n, seed, dev, 2.0)
    assert float(x.abs().min()) > 0.0
    y = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    out = op.mult(x, y)
    assert out.data_ptr() == y.data_ptr()
    yn, xh = _np(y), _np(x)
    assert np.isfinite(yn).all(), f"{what}: dofs not written or not finite"
    ref = S @ xh
    scale = abs(S) @ np.abs(xh)
    zero = scale == 0.0
    np.testing.assert_array_equal(yn[zero], ref[zero])
    rel = np.abs(yn - ref)[~zero] / scale[~zero]
    worst = float(rel.max()) if rel.size else 0.0
    print(f"{what}: worst row |y - Sx| / (|S||x|) = {worst:.3e}")
    assert worst <= RTOL, f"{what}: per-row parity {worst:.3e} > {RTOL:g}"
    return x, y


def _check_block_diag(op, S, what):
    bs = op.bs
    D = _np(op.block_diagonal())
    nn = S.shape[0] // bs
    assert D.shape == (nn, bs, bs)
    rowmax = np.asarray(abs(S).max(axis=1).todense()).reshape(nn, bs)
    nodes = np.arange(nn)
    worst = 0.0
    for i in range(bs):
        for k in range(bs):
            ref = np.asarray(S[nodes * bs + i, nodes * bs + k]).reshape(-1)
            err = np.abs(D[:, i, k] - ref)
            zero = rowmax[:, i] == 0.0
            assert not np.any(err[zero] > 0.0), what
            worst = max(worst, float((err[~zero] / rowmax[:, i][~zero]).max(initial=0.0)))
    print(f"{what}: block diagonal, worst entry error / row max = {worst:.3e}")
    assert worst <= RTOL, f"{what}: block diagonal {worst:.3e} > {RTOL:g}"


# id: cell, degree, n, form kinds. The meshes are just large enough for >= 3 chunks of the 256-cell tile.
PLANNED = {
    "p1tri": (3, 1, (24, 20), ("lin", "neo", "dam-hand", "dam-ad")),
    "p2tri": (3, 2, (20, 16), ("lin", "neo")),
    "p1tet": (-4, 1, (6, 5, 4), ("lin", "neo")),
    "p2tet": (-4, 2, (6, 5, 4), ("lin", "neo")),
}
_cache = {}


def _planned_case(oracle, dev, name, kind, bc="mixed"):
    """(V, form, bcs, assembled S) of a multi-chunk case, built once per module."""
    from femasm import fem

    key = (name, kind, bc)
    if key not in _cache:
        ct, p, n, _ = PLANNED[name]
        vkey = ("V", name)
        if vkey not in _cache:
            m = _mesh(ct, n, dev)
            _cache[vkey] = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
        V = _cache[vkey]
        a = _form(oracle, V, kind, 1.0 / (p * max(n)))
        bcs = _bcs(V, bc)
        _cache[key] = (V, a, bcs, _assembled(a, bcs))
    return _cache[key]


@pytest.mark.parametrize("ct,p,n", [(3, 1, (1, 1)), (-4, 2, (1, 1, 1))])
def test_fewer_cells_than_a_wave(oracle, dev, ct, p, n):
    """Two triangles / six tetrahedra: corner nodes have one cell, one chunk, most lanes idle."""
    from femasm import fem

    m = _mesh(ct, n, dev)
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    a = _form(oracle, V, "lin", 1.0)
    for bc in ("none", "mixed"):
        bcs = _bcs(V, bc)
        S = _assembled(a, bcs)
        op = fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method="planned")
        assert op.num_chunks == 1 and op.redundancy == 1.0
        assert op.shape == S.shape and op.bs == m.gdim
        _check_mult(op, S, dev, f"tiny {ct} P{p} bc={bc}")
        _check_block_diag(op, S, f"tiny {ct} P{p} bc={bc}")


@pytest.mark.parametrize("name,kind", [(nm, k) for nm, c in PLANNED.items() for k in c[3]])
def test_planned_multi_chunk(oracle, dev, name, kind):
    from femasm import fem

    V, a, bcs, S = _planned_case(oracle, dev, name, kind)
    op = fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method="planned")
    # a later plan change must not quietly make the case single-chunk
    assert op.num_chunks >= 3 and op.redundancy > 1.0, (op.num_chunks, op.redundancy)
    ne = V.mesh.num_cells * V.nn
    assert 0 < op.plan_bytes <= 16 * ne + 64 * op.num_chunks
    _check_mult(op, S, dev, f"{name} {kind} planned")
    _check_block_diag(op, S, f"{name} {kind}")


@pytest.mark.parametrize("bc", ["none", "all"])
@pytest.mark.parametrize("name", ["p1tri", "p2tet"])
def test_boundary_conditions(oracle, dev, name, bc):
    from femasm import fem

    V, a, bcs, S = _planned_case(oracle, dev, name, "lin", bc)
    for method in ("planned", "generic"):
        op = fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method=method)
        x, y = _check_mult(op, S, dev, f"{name} bc={bc} {method}")
        if bc == "all":  # every dof constrained: exactly diagonal * x
            assert torch.equal(y, DIAG * x)
    _check_block_diag(op, S, f"{name} bc={bc}")


@pytest.mark.parametrize("kind", ["lin", "neo"])
def test_generic_kernel_on_planned_element(oracle, dev, kind):
    from femasm import fem

    V, a, bcs, S = _planned_case(oracle, dev, "p2tet", kind)
    op = fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method="generic")
    assert op.num_chunks == 0 and op.plan_bytes == 0 and op.redundancy == V.nn
    _check_mult(op, S, dev, f"p2tet {kind} generic")


@pytest.mark.parametrize("tangent", ["dam-hand", "dam-ad"])
def test_reference_square_msh(oracle, dev, tangent):
    """The reference's own unstructured mesh (62 nodes / 98 triangles) with both damage tangents."""
    from femasm import fem, mesh

    m = mesh.read_gmsh(os.path.join(GOLDEN, "square.msh"), gdim=2, device=dev)
    V = fem.functionspace(m, ("Lagrange", 1, (2,)))
    a = _form(oracle, V, tangent, 1.0)
    bcs = _bcs(V, "mixed")
    S = _assembled(a, bcs)
    for method in ("auto", "generic"):
        op = fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method=method)
        _check_mult(op, S, dev, f"square.msh {tangent} {method}")
    _check_block_diag(op, S, f"square.msh {tangent}")


@pytest.mark.parametrize("name", ["p1tri", "p1tet"])
def test_permuted_node_numbering(oracle, dev, name):
    """FunctionSpace.from_dofmap with a random node permutation: a chunk's rows hold scattered cells."""
    from femasm import fem

    ct, p, n, _ = PLANNED[name]
    m = _mesh(ct, n, dev)
    nv = m.num_vertices
    perm = torch.randperm(nv, generator=torch.Generator().manual_seed(7)).to(dev)
    V = fem.FunctionSpace.from_dofmap(m, 1, m.gdim, perm[m.cells.to(torch.int64)], nv)
    for kind in ("lin", "neo"):
        a = _form(oracle, V, kind, 1.0 / max(n))
        bcs = _bcs(V, "mixed")
        S = _assembled(a, bcs)
        op = fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method="planned")
        assert op.num_chunks >= 3 and op.redundancy > 1.0
        _check_mult(op, S, dev, f"permuted {name} {kind}")
    _check_block_diag(op, S, f"permuted {name}")


def test_fan_mesh_falls_back_to_generic(oracle, dev):
    """300 triangles around vertex 0: more cells at one node than a chunk's 256-cell tile holds."""
    from femasm import _lib, fem

    m = fan(300, dev)
    V = fem.functionspace(m, ("Lagrange", 1, (2,)))
    a = _form(oracle, V, "lin", 1.0)
    ring = torch.nonzero(m.x[:, 0] > 0.5, as_tuple=False).reshape(-1)
    bcs = [fem.dirichletbc(0.0, ring, V, components=[1])]
    with pytest.raises(_lib.FemasmError, match=r"300 cells.*256"):
        fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method="planned")
    S = _assembled(a, bcs)
    op = fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method="auto")
    assert op.num_chunks == 0 and op.plan_bytes == 0
    _check_mult(op, S, dev, "fan auto")
    _check_block_diag(op, S, "fan")


@pytest.mark.parametrize("ct,p,n,kinds", [(4, 2, (3, 3), ("lin", "neo")), (8, 1, (2, 2, 2), ("lin", "neo")),
                                          (8, 3, (2, 1, 1), ("lin",))])
def test_generic_kernel_non_affine_cells(oracle, dev, ct, p, n, kinds):
    from femasm import fem

    m = _mesh(ct, n, dev, perturb=0.3)
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    bcs = _bcs(V, "mixed")
    for kind in kinds:
        a = _form(oracle, V, kind, 1.0 / (p * max(n)))
        S = _assembled(a, bcs)
        op = fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG)  # auto: no plan for tensor cells
        assert op.num_chunks == 0
        with pytest.raises(ValueError):
            fem.JacobianOperator(a, bcs=bcs, method="planned")
        _check_mult(op, S, dev, f"cell {ct} Q{p} {kind} generic")
        _check_block_diag(op, S, f"cell {ct} Q{p} {kind}")


def test_reproducible_no_allocation_no_alias(oracle, dev):
    from femasm import fem

    V, a, bcs, S = _planned_case(oracle, dev, "p2tet", "neo")
    x = _rand(V.num_dofs, 9, dev)
    for method in ("planned", "generic"):
        op = fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method=method)
        y1 = op.mult(x)
        y2 = torch.full_like(x, float("nan"))
        op.mult(x, y2)  # (also warms the caches: bc marker, element tables)
        assert torch.equal(y1, y2)
        before = torch.cuda.memory_allocated(dev)
        op.mult(x, y2)
        assert torch.cuda.memory_allocated(dev) == before
        assert torch.equal(y1, y2)
        with pytest.raises(ValueError, match="alias"):
            op.mult(x, x)
        with pytest.raises(ValueError, match="alias"):
            op.mult(x, x.view(-1))
    # the operator reads u live: after a change of the state it equals the matrix assembled there
    a.u.mul_(0.5)
    _check_mult(op, _assembled(a, bcs), dev, "p2tet neo at a new state")
    a.u.mul_(2.0)


def _newton_problem(oracle, dev, kind, ct, p, n, matrix_free):
    from femasm import fem, nls

    m = _mesh(ct, n, dev)
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    E = _E(oracle, m)
    u = fem.Function(V)
    f = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
    f[1::m.gdim] = -1e3
    if kind == 1:
        xn = V.tabulate_dof_coordinates()
        d = (0.6 * torch.exp(-20 * ((xn[:, 0] - 0.5) ** 2 + (xn[:, 1] - 0.5) ** 2))).contiguous()
        form = fem.AsymDamage(V, E=E, nu=0.3, u=u, d=d, f=f)
    else:
        form = fem.NeoHookean(V, E=E, nu=0.3, u=u, f=f)
    left = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.zeros_like(x[0])))
    right = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.ones_like(x[0])))
    disp = 0.05 if kind == 2 else 1e-3
    bcs = [fem.dirichletbc(0.0, left, V), fem.dirichletbc([disp] + [0.0] * (m.gdim - 1), right, V)]
    problem = nls.NonlinearProblem(form, u, bcs, matrix_free=matrix_free)
    solver = nls.NewtonSolver(None, problem)
    solver.rtol, solver.atol, solver.max_it = 1e-7, 5e-8, 10  # the reference's settings
    it, conv = solver.solve(u)
    return problem, V, it, conv, _np(u.x)


@pytest.mark.parametrize("kind,ct,p,n", [(2, -4, 2, (3, 2, 2)), (1, 3, 1, (10, 8))])
def test_newton_matrix_free(oracle, dev, kind, ct, p, n):
    """Two cases of tests/test_gpu_newton.py with no matrix: same Newton iteration, both Krylov solves
    at rtol 1e-12, solutions to that test's 1e-9."""
    from femasm import fem
    from femasm.la import MatrixCSR

    pa, _, it_a, conv_a, ua = _newton_problem(oracle, dev, kind, ct, p, n, False)
    pm, V, it_m, conv_m, um = _newton_problem(oracle, dev, kind, ct, p, n, True)
    assert conv_a and conv_m
    assert abs(it_m - it_a) <= 1, (it_m, it_a)
    assert np.abs(um - ua).max() <= 1e-9 * np.abs(ua).max()
    assert isinstance(pa.matrix(), MatrixCSR)
    op = pm.matrix()
    assert isinstance(op, fem.JacobianOperator)
    assert op.num_chunks >= 1
    assert 0 < op.plan_bytes <= 16 * V.mesh.num_cells * V.nn + 64 * op.num_chunks
