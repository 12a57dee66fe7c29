"""The aligned per-quarter LDS add order (csrc/plan_order.h, run by k_order_slots for every default plan)
only permutes each lane's blocks over the steps: every matrix assembled through the default plan equals
the CPU oracle's at the per-row bar of tests/rowparity.py (RTOL = 1e-12 per scalar row, identical
patterns), matrices pre-filled with NaN so that every block must be written, and assembled with
FA_CHECK_ERRORS (check=True) so that a slot word that decodes outside its chunk (the gather's pattern-error
bit) raises. Deterministic mode is bit-identical from run to run on the new order."""
import numpy as np
import pytest
import torch

import irregular_meshes as im
from rowparity import RTOL, assert_rows_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t):
    return t.detach().cpu().numpy()


def _box(ct, n, dev):
    from femasm import mesh

    return mesh.create_unit_square(*n, cell_type=ct, device=dev) if len(n) == 2 else \
        mesh.create_unit_cube(*n, cell_type=ct, device=dev)


def _ref_bcs(V):
    """the reference's bcs: the lowest-x plane clamped, the highest-x plane prescribed"""
    from femasm import fem

    xn = V.tabulate_dof_coordinates()
    lo, hi = xn[:, 0].min(), xn[:, 0].max()
    left = torch.nonzero(torch.isclose(xn[:, 0], lo), as_tuple=False).reshape(-1)
    right = torch.nonzero(torch.isclose(xn[:, 0], hi), as_tuple=False).reshape(-1)
    assert left.numel() > 0 and right.numel() > 0
    return [fem.dirichletbc(0.0, left, V), fem.dirichletbc([0.01] + [0.0] * (V.mesh.gdim - 1), right, V)]


def _assemble_checked(a, bcs, **kw):
    """NaN-filled matrix, assembled with FA_CHECK_ERRORS"""
    from femasm import fem

    A = fem.create_matrix(a)
    for _, _, d in A.parts:
        d.fill_(float("nan"))
    return fem.assemble_matrix(a, bcs=bcs, A=A, check=True, **kw)


def _check_linear(oracle, V, a, bcs, A, what):
    from femasm import fem

    m = V.mesh
    marker, _ = fem._combine_bcs(V, bcs)
    ip, ix = oracle.sparsity(_np(V.dofmap), V.num_nodes)
    lam, mu = oracle.lame(_np(a.E), a.nu)
    ref = oracle.assemble_elasticity(int(m.cell_type), V.degree, _np(V.dofmap), _np(m.cells), _np(m.x), lam, mu, ip, ix,
                                     bc=_np(marker), diag=1.0, qdeg=a.qdeg)
    np.testing.assert_array_equal(_np(A.indptr), ip)
    np.testing.assert_array_equal(_np(A.indices), ix)
    got = _np(A.data)
    assert np.isfinite(got).all(), f"{what}: blocks not written"
    rel = assert_rows_close(got, ref, ip, RTOL, what)
    print(f"{what}: worst row error {rel:.3e}")


# P2 tets, P2 triangles (default plan: block-owner gather; owner=False: the table gather the order is
# for), P1 tets, Q2 quads
LINEAR = [(-4, 2, (4, 3, 3), None), (3, 2, (5, 4), None), (3, 2, (5, 4), dict(owner=False)), (-4, 1, (4, 4, 4), None),
          (4, 2, (6, 5), None)]


@pytest.mark.parametrize("ct,p,n,plan", LINEAR)
def test_default_plan_equals_oracle(oracle, dev, ct, p, n, plan):
    from femasm import fem

    m = _box(ct, n, dev)
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    E = torch.tensor(oracle.e_range()[np.arange(m.num_cells) % 200], device=dev)
    a = fem.LinearElasticity(V, E=E, nu=0.3)
    bcs = _ref_bcs(V)
    A = _assemble_checked(a, bcs, **({"plan": plan} if plan else {}))
    _check_linear(oracle, V, a, bcs, A, f"cell {ct} P{p} {n} {plan or ''}")
    if ct != 3 or plan:  # the table gathers' plans are ordered (positional: the entries moved too)
        gp = fem.gather_plan(V, A, 0, a.kind, **(plan or {}))
        assert gp.slot_order > 0 and gp.eadj


def test_neohookean_default_plan_equals_oracle(oracle, dev):
    from femasm import fem

    ct, p, n = -4, 2, (3, 2, 2)
    m = _box(ct, n, dev)
    V = fem.functionspace(m, ("Lagrange", p, (3,)))
    u = (0.05 * torch.sin(torch.pi * V.tabulate_dof_coordinates())).reshape(-1).contiguous()
    E = torch.tensor(oracle.e_range()[np.arange(m.num_cells) % 200], device=dev)
    a = fem.NeoHookean(V, E=E, nu=0.3, u=u)
    bcs = _ref_bcs(V)
    A = _assemble_checked(a, bcs)
    marker, _ = fem._combine_bcs(V, bcs)
    ip, ix = oracle.sparsity(_np(V.dofmap), V.num_nodes)
    lam, mu = oracle.lame(_np(a.E), 0.3)
    ref = oracle.assemble_neohookean(ct, p, _np(V.dofmap), _np(m.cells), _np(m.x), lam, mu, _np(a.u), ip, ix,
                                     bc=_np(marker))
    got = _np(A.data)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    rel = assert_rows_close(got, ref, ip, RTOL, "neo-Hookean P2 tets")
    print(f"neo-Hookean P2 tets {n}: worst row error {rel:.3e}")
    assert fem.gather_plan(V, A, 0, a.kind).slot_order > 0


def test_irregular_valence_mesh_equals_oracle(oracle, dev):
    """Delaunay tetrahedra (tests/irregular_meshes.py), P2: rows of many valences, so partial quarters
    and short chunks."""
    from femasm import fem

    m = im.CASES["delaunay"][0](dev)
    V = fem.functionspace(m, ("Lagrange", 2, (3,)))
    E = torch.tensor(oracle.e_range()[np.arange(m.num_cells) % 200], device=dev)
    a = fem.LinearElasticity(V, E=E, nu=0.3)
    bcs = _ref_bcs(V)
    A = _assemble_checked(a, bcs)
    _check_linear(oracle, V, a, bcs, A, "Delaunay P2 tets")
    gp = fem.gather_plan(V, A, 0, a.kind)
    assert gp.slot_order > 0 and gp.eadj


def test_deterministic_mode_is_bit_identical(oracle, dev):
    from femasm import fem

    m = _box(-4, (4, 3, 3), dev)
    V = fem.functionspace(m, ("Lagrange", 2, (3,)))
    E = torch.tensor(oracle.e_range()[np.arange(m.num_cells) % 200], device=dev)
    a = fem.LinearElasticity(V, E=E, nu=0.3)
    bcs = _ref_bcs(V)
    A1 = _assemble_checked(a, bcs, deterministic=True)
    A2 = _assemble_checked(a, bcs, deterministic=True)
    assert torch.equal(A1.data.view(torch.int64), A2.data.view(torch.int64))
    _check_linear(oracle, V, a, bcs, A1, "deterministic P2 tets")
