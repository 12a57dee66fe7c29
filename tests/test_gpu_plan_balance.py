"""The table gather's lanes without an item add nothing (k_gather_lin: one lane-divergent region around the
unrolled block loop instead of zero adds), and the plan's placement stays the greedy fill's, on meshes
where a plan or the last item wave of a chunk can go wrong.

Per mesh: the eperm the device wrote (read back through eadj) equals the fill of the stand-alone host
driver on the same chunks (tools/plan_order/plan_balance_host.cpp, mode "fill"; its exchange descent was
measured and left out of the plan, DESIGN.md 3.2b "Quarter balance"); the assembled matrix meets the CPU
oracle at the per-row bar of tests/rowparity.py (RTOL = 1e-12 per scalar row), NaN-filled first and
assembled with FA_CHECK_ERRORS, with bcs and without, in default and deterministic mode (linear
elasticity; the neo-Hookean gather has no deterministic mode); two deterministic assemblies are
bit-identical.

Idle lanes: row windows whose only chunk holds 1, 63, 65 and 129 items (affine Q1 quadrilaterals, one
item per entry: a nearly empty wave, one lane short of a wave, one over, two waves and a lane) and 2, 64,
66, 130 items (P2 tetrahedra, two items per entry)."""
import numpy as np
import pytest
import torch

import irregular_meshes as im
import plan_chunks as pc
from rowparity import RTOL, assert_rows_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return pc.compile_driver(pc.BALANCE_SRC, str(tmp_path_factory.mktemp("plan_balance") / "plan_balance_host"))


def _np(t):
    return t.detach().cpu().numpy()


def _box(ct, n, dev):
    from femasm import mesh

    return mesh.create_unit_square(*n, cell_type=ct, device=dev) if len(n) == 2 else \
        mesh.create_unit_cube(*n, cell_type=ct, device=dev)


def _ref_bcs(V):
    """the bench's two bcs: the lowest-x plane clamped, the highest-x plane prescribed"""
    from femasm import fem

    xn = V.tabulate_dof_coordinates()
    lo, hi = xn[:, 0].min(), xn[:, 0].max()
    left = torch.nonzero(torch.isclose(xn[:, 0], lo), as_tuple=False).reshape(-1)
    right = torch.nonzero(torch.isclose(xn[:, 0], hi), as_tuple=False).reshape(-1)
    assert left.numel() > 0 and right.numel() > 0
    return [fem.dirichletbc(0.0, left, V), fem.dirichletbc([0.01] + [0.0] * (V.mesh.gdim - 1), right, V)]


def _filled(a, **kw):
    from femasm import fem

    A = fem.create_matrix(a, **kw)
    for _, _, d in A.parts:
        d.fill_(float("nan"))
    return A


def _reference(oracle, V, a, bcs):
    """the oracle's matrix and pattern, once per (form, bcs)"""
    from femasm import fem

    m = V.mesh
    marker = _np(fem._combine_bcs(V, bcs)[0]) if bcs else None
    ip, ix = oracle.sparsity(_np(V.dofmap), V.num_nodes)
    lam, mu = oracle.lame(_np(a.E), a.nu)
    if isinstance(a, fem.NeoHookean):
        ref = oracle.assemble_neohookean(int(m.cell_type), V.degree, _np(V.dofmap), _np(m.cells), _np(m.x), lam, mu,
                                         _np(a.u), ip, ix, bc=marker)
    else:
        ref = oracle.assemble_elasticity(int(m.cell_type), V.degree, _np(V.dofmap), _np(m.cells), _np(m.x), lam, mu, ip, ix,
                                         bc=marker, diag=1.0, qdeg=a.qdeg)
    assert np.isfinite(ref).all()
    return ref, ip, ix


def _check_plans(V, driver, what):
    """every cached positional plan of V: the device's eperm against the host driver's"""
    n = bad = 0
    for which in range(len(V._plans)):
        rec = list(V._plans.values())[which]
        if len(rec) < 5 or rec[4] is None:
            continue  # (a contribution plan)
        ns, chunks, eperms = pc.plan_chunks(V, which)
        small = max(len(c) for c in chunks) * ns <= 256
        mq = 16 if small else 512 * ns // 16
        visits = [pc.visit_order(len(c)) for c in chunks]
        b0, b1, mv, perms = pc.run_balance(driver, V.nn, ns, mq, [c[v] for c, v in zip(chunks, visits)], mode="fill")
        bad += sum(int(not (v[p] == e).all()) for v, p, e in zip(visits, perms, eperms))
        n += len(chunks)
        print(f"{what} plan {which}: {len(chunks)} chunks, bound {b0.sum()}")
    assert n > 0, "no positional plan"
    assert bad == 0, f"{what}: the device's eperm differs from the host driver's on {bad} of {n} chunks"


def _run_case(oracle, dev, driver, V, a, what, deterministic=True, plan=None, create=None):
    from femasm import fem

    kw = {"plan": plan} if plan else {}
    for bcs in (_ref_bcs(V), None):
        ref, ip, ix = _reference(oracle, V, a, bcs)
        modes = [dict(), dict(deterministic=True)] if deterministic else [dict()]
        for mode in modes:
            A = fem.assemble_matrix(a, bcs=bcs, A=_filled(a, **(create or {})), check=True, **mode, **kw)
            np.testing.assert_array_equal(_np(A.indices), ix)
            got = _np(A.data)
            assert np.isfinite(got).all(), f"{what}: blocks not written"
            rel = assert_rows_close(got, ref, ip, RTOL, what)
            print(f"{what} bcs={'yes' if bcs else 'no'} {mode}: worst row error {rel:.3e}")
            if mode:
                B = fem.assemble_matrix(a, bcs=bcs, A=_filled(a, **(create or {})), check=True, **mode, **kw)
                assert torch.equal(A.data.view(torch.int64), B.data.view(torch.int64)), f"{what}: deterministic runs differ"
    _check_plans(V, driver, what)


def _linear(oracle, dev, m, p):
    from femasm import fem

    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    E = torch.tensor(oracle.e_range()[np.arange(m.num_cells) % 200], device=dev)
    return V, fem.LinearElasticity(V, E=E, nu=0.3)


# P2 tets on the (4,3,3) box and the 6^3 cube, P2 triangles through the table gather, affine Q2
# quadrilaterals (whole entries per lane), P1 tets (fused records)
LINEAR = [(-4, 2, (4, 3, 3), None), (-4, 2, (6, 6, 6), None), (3, 2, (5, 4), dict(owner=False)), (4, 2, (5, 4), None),
          (-4, 1, (4, 4, 4), None)]


@pytest.mark.parametrize("ct,p,n,plan", LINEAR)
def test_plan_equals_oracle_and_host_fill(oracle, dev, driver, ct, p, n, plan):
    V, a = _linear(oracle, dev, _box(ct, n, dev), p)
    _run_case(oracle, dev, driver, V, a, f"cell {ct} P{p} {n}", plan=plan)


def test_row_parts(oracle, dev, driver):
    """P2 tets (4,3,3) in several row parts: every part has its own plan and ends in a short chunk"""
    V, a = _linear(oracle, dev, _box(-4, (4, 3, 3), dev), 2)
    create = dict(max_part_bytes=200_000)
    assert len(_filled(a, **create).parts) >= 3
    _run_case(oracle, dev, driver, V, a, "P2 tets (4,3,3), row parts", create=create)


def test_irregular_valence(oracle, dev, driver):
    V, a = _linear(oracle, dev, im.CASES["delaunay"][0](dev), 2)
    _run_case(oracle, dev, driver, V, a, "Delaunay P2 tets")


def test_neohookean(oracle, dev, driver):
    from femasm import fem

    m = _box(-4, (4, 3, 3), dev)
    V = fem.functionspace(m, ("Lagrange", 2, (3,)))
    u = (0.05 * torch.sin(torch.pi * V.tabulate_dof_coordinates())).reshape(-1).contiguous()
    E = torch.tensor(oracle.e_range()[np.arange(m.num_cells) % 200], device=dev)
    a = fem.NeoHookean(V, E=E, nu=0.3, u=u)
    _run_case(oracle, dev, driver, V, a, "neo-Hookean P2 tets (4,3,3)", deterministic=False)


def _window_of(ptr, items, ns):
    """rows [r0, r1) whose adjacency entries number items / ns, or None"""
    want = items // ns
    at = {int(v): i for i, v in enumerate(ptr)}
    for r0 in range(len(ptr) - 1):
        r1 = at.get(int(ptr[r0]) + want)
        if r1 is not None and r1 > r0:
            return r0, r1
    return None


@pytest.mark.parametrize("ct,p,n,ns,items", [(4, 1, (7, 6), 1, (1, 63, 65, 129)), (-4, 2, (3, 3, 3), 2, (2, 64, 66, 130))])
def test_short_last_waves(oracle, dev, ct, p, n, ns, items):
    """a row window that is one chunk of the given item count, against the oracle's rows of the window"""
    from femasm import fem
    from femasm.la import MatrixCSR

    V, a = _linear(oracle, dev, _box(ct, n, dev), p)
    bcs = _ref_bcs(V)
    ref, ip, ix = _reference(oracle, V, a, bcs)
    ptr = _np(V.adjacency()[0])
    full = fem.create_matrix(a)
    for k in items:
        win = _window_of(ptr, k, ns)
        assert win is not None, f"no row window of {k} items"
        r0, r1 = win
        for mode in (dict(), dict(deterministic=True)):
            A = MatrixCSR(full.indptr, full.indices, V.bs, window=win)
            A.parts[0][2].fill_(float("nan"))
            fem.assemble_matrix(a, bcs=bcs, A=A, check=True, **mode)
            gp = fem.gather_plan(V, A, 0, a.kind, **mode)
            assert gp.nchunks == 1 and gp.max_adj * ns == k and gp.slot_order == ns and gp.eadj
            got = _np(A.parts[0][2])
            assert np.isfinite(got).all(), f"{k} items: blocks not written"
            lo, hi = ip[r0], ip[r1]
            rel = assert_rows_close(got, ref[lo:hi], ip[r0:r1 + 1] - lo, RTOL, f"{k} items")
            print(f"cell {ct} P{p}: chunk of {k} items (rows {r0} .. {r1}) {mode}: worst row error {rel:.3e}")
