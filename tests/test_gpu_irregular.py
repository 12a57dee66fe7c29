"""Assembly on irregular-valence meshes (tests/irregular_meshes.py): Delaunay tetrahedra, the reference's
Gmsh square and its refinement, fans and cones whose one high-valence row sits over a planner target or
cap. tests/test_irregular_meshes_host.py states, on the host, which side of each limit a case is on; the
tests here take the plan the assembly runs with from fem.gather_plan and assert the route from its fields.

Bar: rowparity.assert_rows_close at RTOL = 1e-12 per scalar row against the CPU oracle, identical
patterns; vectors max |b - ref| <= 1e-12 max |ref| (tests/test_gpu_vector.py). Matrices are pre-filled
with NaN before every assembly: every block must be written.

Neo-Hookean states: u = 0.05 sin(pi x) plus white noise of amplitude 0.05 x the mesh's shortest edge (the
rule of tests/test_gpu_matrix_free.py for a mesh with no single spacing); the oracle's tangent there is
asserted finite.

What the library does not do, stated as tests of the refusal: degree-3 simplices do not exist
(NotImplementedError); deterministic mode runs the table gather only, so a mesh with a row over the entry
target is refused with FA_E_UNSUPPORTED ("deterministic") and the refusal returns its scratch.
"""
import numpy as np
import pytest
import torch

import irregular_meshes as im
from rowparity import RTOL, assert_rows_close
from test_gpu_deterministic import _pool_used_bytes
from test_gpu_matrix_free import DIAG, _check_block_diag, _check_mult

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _space(name, p, dev):
    """A fresh mesh and space per test (plans, prepared state and their counters live on the space)."""
    from femasm import fem

    m = im.CASES[name][0](dev)
    return m, fem.functionspace(m, ("Lagrange", p, (m.gdim,)))


def _E_host(oracle, nc, k):
    """E = e_range()[cell % 200]; k = 1: the table read from another offset (the in-place change)."""
    return oracle.e_range()[(np.arange(nc) + 37 * k) % 200]


def _bcs(V, which):
    """ref: the reference's bcs, the lowest-x plane clamped and the highest-x plane prescribed;
    comp: the single-component pair of test_component_dirichlet (lowest x: u_x, lowest y: u_y)."""
    from femasm import fem

    xn = V.tabulate_dof_coordinates()
    gd = V.mesh.gdim

    def plane(axis, v):
        return torch.nonzero(torch.isclose(xn[:, axis], torch.full_like(xn[:, axis], v)), as_tuple=False).reshape(-1)

    xlo, xhi, ylo = float(xn[:, 0].min()), float(xn[:, 0].max()), float(xn[:, 1].min())
    if which == "ref":
        left, right = plane(0, xlo), plane(0, xhi)
        assert left.numel() > 0 and right.numel() > 0
        return [fem.dirichletbc(0.0, left, V), fem.dirichletbc([0.01] + [0.0] * (gd - 1), right, V)]
    x0, y0 = plane(0, xlo), plane(1, ylo)
    assert x0.numel() > 0 and y0.numel() > 0
    return [fem.dirichletbc(0.0, x0, V, components=[0]), fem.dirichletbc(0.0, y0, V, components=[1])]


_ref_cache = {}


def _pattern(oracle, V, name, p):
    key = ("pat", name, p)
    if key not in _ref_cache:
        _ref_cache[key] = oracle.sparsity(_np(V.dofmap), V.num_nodes)
    return _ref_cache[key]


def _ref_lin(oracle, V, name, p, bc, k, marker):
    """Oracle values of linear elasticity on (case, degree) with bcs `bc` at coefficient version k
    (computed once per module and left unchanged)."""
    key = ("lin", name, p, bc, k)
    if key not in _ref_cache:
        m = V.mesh
        ip, ix = _pattern(oracle, V, name, p)
        lam, mu = oracle.lame(_E_host(oracle, m.num_cells, k), 0.3)
        _ref_cache[key] = oracle.assemble_elasticity(int(m.cell_type), p, _np(V.dofmap), _np(m.cells), _np(m.x), lam, mu,
                                                     ip, ix, bc=_np(marker), diag=1.0)
    return _ref_cache[key]


def _check_matrix(A, ref, pattern, what):
    ip, ix = pattern
    np.testing.assert_array_equal(_np(A.indptr), ip)
    np.testing.assert_array_equal(_np(A.indices), ix)
    got = _np(A.data)
    assert np.isfinite(got).all(), f"{what}: blocks not written or not finite"
    rel = assert_rows_close(got, ref, ip, RTOL, what)
    print(f"{what}: worst row error {rel:.3e}")
    return rel


def _fill_nan(A):
    for _, _, d in A.parts:
        d.fill_(float("nan"))


# route id -> assemble_matrix keywords
ROUTES = {
    "gather": dict(),
    "scatter": dict(method="scatter"),
    "deterministic": dict(deterministic=True),
    "owner": dict(plan=dict(owner=True)),
    "lds": dict(plan=dict(owner=False)),
    "generic": dict(plan=dict(owner=False, order="none")),
}
# the cases every row of which is within the entry targets (host tests: route "table")
REGULAR = [("square", 1), ("square", 2), ("square_r1", 2), ("delaunay", 1), ("delaunay", 2), ("cone98", 1)]
# one row over the entry target, inside the caps: off the table gather
OVER = [("cone98", 2), ("cone1212", 1), ("fan150", 2), ("fan300", 1), ("fan300", 2)]


def _plan_of(V, A, a, kw):
    from femasm import fem

    if kw.get("method") == "scatter":
        return None
    return fem.gather_plan(V, A, 0, a.kind, deterministic=kw.get("deterministic", False), **kw.get("plan", {}))


def _assemble_twice(oracle, dev, name, p, route, max_part_bytes=None):
    """Linear elasticity through `route`, with both bc sets, twice on one matrix with E changed in place
    in between: both assemblies against the oracle at their E. Returns (V, plan of part 0)."""
    from femasm import fem

    m, V = _space(name, p, dev)
    E = torch.tensor(_E_host(oracle, m.num_cells, 0), device=dev)
    a = fem.LinearElasticity(V, E=E, nu=0.3)
    kw = ROUTES[route]
    A = fem.create_matrix(a, max_part_bytes=max_part_bytes, check=True)
    pattern = _pattern(oracle, V, name, p)
    for bc in ("ref", "comp"):
        bcs = _bcs(V, bc)
        marker, _ = fem._combine_bcs(V, bcs)
        assert 0 < int(marker.sum()) < V.num_dofs
        for k in (0, 1):
            E.copy_(torch.tensor(_E_host(oracle, m.num_cells, k), device=dev))  # in place: the form's own tensor
            _fill_nan(A)
            fem.assemble_matrix(a, bcs=bcs, A=A, **kw)
            _check_matrix(A, _ref_lin(oracle, V, name, p, bc, k, marker), pattern, f"{name} P{p} {route} bc={bc} E{k}")
    return V, A, a, _plan_of(V, A, a, kw)


def test_pattern_matches_oracle(oracle, dev):
    from femasm import fem

    for name, (_, degrees) in im.CASES.items():
        if name == "fan700":
            continue  # over kSparsityCap: test_sparsity_cap_is_refused
        for p in degrees:
            m, V = _space(name, p, dev)
            A = fem.create_matrix(fem.LinearElasticity(V, E=1.0, nu=0.3), check=True)
            ip, ix = _pattern(oracle, V, name, p)
            np.testing.assert_array_equal(_np(A.indptr), ip)
            np.testing.assert_array_equal(_np(A.indices), ix)


def test_degree_three_simplices_do_not_exist(dev):
    """The library has P1 and P2 simplices; degree 3 on square.msh is refused before any kernel runs."""
    from femasm import fem

    m = im.square_msh(dev)
    with pytest.raises(NotImplementedError):
        fem.functionspace(m, ("Lagrange", 3, (2,)))


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name,p", REGULAR)
def test_linear_elasticity(oracle, dev, name, p, route):
    """Every route of the linear-elasticity assembly on the meshes within the entry targets, and the plan
    each ran with. Observed on an MI355X: every FP64 route is at or below 6e-14 of its row's scale; the
    deterministic (fixed-point) route depends on cell shape, 5e-14 on square.msh, 1e-13 .. 3e-13 on the
    Delaunay tetrahedra and 7.7e-13 on cone98 P1 (slender cells: its per-block scale comes from a bound
    on the block, which such cells are far below) -- inside the 1e-12 bar, with the least margin here."""
    from femasm import _lib

    V, A, a, plan = _assemble_twice(oracle, dev, name, p, route)
    ct = int(V.mesh.cell_type)
    if plan is None:
        return
    assert plan.nchunks >= 1
    if route == "owner" or (route == "gather" and ct == _lib.FA_TRIANGLE):  # the block-owner plan
        assert plan.contrib and plan.max_adj <= im.OWN_CCAP and plan.max_blocks <= im.own_maxb(ct)
        return
    assert not plan.contrib and plan.max_adj <= im.entry_target(ct, p) and plan.max_blocks <= im.block_cap(ct, p)
    if route == "generic":  # plain slot map, no positional entries: k_gather's item loop
        assert not plan.eadj
        return
    assert plan.eadj  # positional: the table gather
    # prepared cell state (P2 table items): the static records are built once for both E and kept
    # across the two bc sets' first builds (one per marker)
    if p == 2:
        assert V._prepared_builds == 2, V._prepared_builds


@pytest.mark.parametrize("route", ["gather", "scatter", "deterministic"])
@pytest.mark.parametrize("name,p", [("square_r1", 2), ("delaunay", 2)])
def test_row_parts_start_mid_mesh(oracle, dev, name, p, route):
    """max_part_bytes = 4096: the values in many row parts, each its own window and plan."""
    V, A, a, plan = _assemble_twice(oracle, dev, name, p, route, max_part_bytes=4096)
    assert len(A.parts) > 3


def test_prepared_state_survives_a_coefficient_change(oracle, dev):
    """delaunay P2 through the default gather: one build of the static records serves both values of E."""
    from femasm import fem

    name, p = "delaunay", 2
    m, V = _space(name, p, dev)
    E = torch.tensor(_E_host(oracle, m.num_cells, 0), device=dev)
    a = fem.LinearElasticity(V, E=E, nu=0.3)
    bcs = _bcs(V, "ref")
    marker, _ = fem._combine_bcs(V, bcs)
    A = fem.create_matrix(a)
    for k in (0, 1, 0):
        E.copy_(torch.tensor(_E_host(oracle, m.num_cells, k), device=dev))
        _fill_nan(A)
        fem.assemble_matrix(a, bcs=bcs, A=A)
        _check_matrix(A, _ref_lin(oracle, V, name, p, "ref", k, marker), _pattern(oracle, V, name, p), f"prepared E{k}")
        assert V._prepared_builds == 1


# ------------------------------------------------------------------------------------- over the target
@pytest.mark.parametrize("name,p", OVER)
def test_over_entry_target_plan(oracle, dev, name, p):
    """The plans these meshes get, from the plans' own fields: the high-valence row is a chunk of its own
    with more entries than the table gather has lanes for, nothing was refused, and the block-owner
    plan is declined wherever the row is over its caps."""
    from femasm import _lib, fem

    m, V = _space(name, p, dev)
    ct = int(m.cell_type)
    a = fem.LinearElasticity(V, E=1.0, nu=0.3)
    A = fem.create_matrix(a)
    ip, _ = _pattern(oracle, V, name, p)
    st = im.row_stats(_np(V.dofmap), V.num_nodes, ip)
    lds = fem.gather_plan(V, A, 0, a.kind, owner=False)
    assert not lds.contrib and lds.eadj  # a positional plan of the LDS-atomic gather
    assert lds.max_adj == st["entries"] > im.entry_target(ct, p)  # ... that the table gather cannot run
    assert lds.max_adj * im.NSPLIT[(ct, p)] > im.LIN_THREADS
    assert lds.max_adj <= im.GATHER_MAX_ADJ and st["blocks"] <= lds.max_blocks <= im.block_cap(ct, p)
    assert lds.nchunks >= 2
    default = fem.gather_plan(V, A, 0, a.kind)
    forced = fem.gather_plan(V, A, 0, a.kind, owner=True)
    owner_fits = st["entries"] <= im.OWN_CCAP and st["blocks"] <= im.own_maxb(ct)
    assert owner_fits == (name == "fan150")
    assert bool(forced.contrib) == owner_fits
    assert bool(default.contrib) == (owner_fits and ct == _lib.FA_TRIANGLE)
    neo = fem.gather_plan(V, A, 0, _lib.FA_NEO_HOOKEAN)
    assert neo.eadj and not neo.contrib and neo.max_adj == st["entries"] > im.entry_target(ct, p, "neo")
    assert neo.max_adj <= im.GATHER_MAX_ADJ and neo.max_blocks <= im.block_cap(ct, p, "neo")


@pytest.mark.parametrize("route", ["gather", "scatter", "owner", "lds", "generic"])
@pytest.mark.parametrize("name,p", OVER)
def test_over_entry_target_linear_elasticity(oracle, dev, name, p, route):
    V, A, a, plan = _assemble_twice(oracle, dev, name, p, route)
    if plan is None:
        return
    ct = int(V.mesh.cell_type)
    if plan.contrib:  # only fan150: inside a block-owner chunk
        assert name == "fan150" and route in ("gather", "owner")
        return
    # off the table gather and the owner route: more items in the largest chunk than k_gather_lin has lanes
    assert plan.max_adj * im.NSPLIT[(ct, p)] > im.LIN_THREADS and plan.max_adj <= im.GATHER_MAX_ADJ
    assert plan.nchunks >= 2 and plan.max_blocks <= im.block_cap(ct, p)


@pytest.mark.parametrize("name,p", OVER)
def test_over_entry_target_deterministic_is_refused(oracle, dev, name, p):
    """Deterministic mode is the table gather's (fixed-point sums in k_gather_lin): a mesh off that route
    is refused, loudly, and ten refusals leave the stream-ordered pool as it was."""
    from femasm import _lib, fem

    m, V = _space(name, p, dev)
    a = fem.LinearElasticity(V, E=torch.tensor(_E_host(oracle, m.num_cells, 0), device=dev), nu=0.3)
    bcs = _bcs(V, "ref")
    A = fem.create_matrix(a)

    def refused():
        with pytest.raises(_lib.FemasmError, match="deterministic"):
            fem.assemble_matrix(a, bcs=bcs, A=A, deterministic=True)

    for _ in range(2):
        refused()
    torch.cuda.synchronize()
    before = (_pool_used_bytes(dev), torch.cuda.memory_allocated(dev))
    for _ in range(10):
        refused()
    torch.cuda.synchronize()
    assert (_pool_used_bytes(dev), torch.cuda.memory_allocated(dev)) == before


# ------------------------------------------------------------------------------------- neo-Hookean
def _neo_state(V, k):
    m = V.mesh
    h = im.shortest_edge(_np(m.x), _np(m.cells))
    xn = V.tabulate_dof_coordinates()
    g = torch.Generator().manual_seed(11)
    noise = (0.05 * h * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).to(m.device)
    u = (0.05 * torch.sin(torch.pi * xn).reshape(-1) + noise).contiguous()
    return u * (0.5 if k else 1.0)  # k = 1: the state after an in-place change


def _ref_neo(oracle, V, name, p, k, marker):
    key = ("neo", name, p, k)
    if key not in _ref_cache:
        m = V.mesh
        ip, ix = _pattern(oracle, V, name, p)
        lam, mu = oracle.lame(_E_host(oracle, m.num_cells, 0), 0.3)
        ref = oracle.assemble_neohookean(int(m.cell_type), p, _np(V.dofmap), _np(m.cells), _np(m.x), lam, mu,
                                         _np(_neo_state(V, k)), ip, ix, bc=_np(marker), diag=1.0)
        assert np.isfinite(ref).all(), "the oracle's tangent is not finite at this state"
        _ref_cache[key] = ref
    return _ref_cache[key]


NEO = [("square_r1", 2), ("delaunay", 1), ("delaunay", 2)]
NEO_OVER = [("cone98", 2), ("cone1212", 1), ("fan300", 1), ("fan300", 2)]


@pytest.mark.parametrize("method", ["gather", "scatter"])
@pytest.mark.parametrize("name,p", NEO + NEO_OVER)
def test_neohookean(oracle, dev, name, p, method):
    """The tangent at two states (the second reached by changing u in place). Over the entry target the
    gather runs k_gather_neo's multi-pass variant (a chunk of more than 256 items)."""
    from femasm import _lib, fem

    m, V = _space(name, p, dev)
    ct = int(m.cell_type)
    E = torch.tensor(_E_host(oracle, m.num_cells, 0), device=dev)
    a = fem.NeoHookean(V, E=E, nu=0.3, u=_neo_state(V, 0))
    bcs = _bcs(V, "ref")
    marker, _ = fem._combine_bcs(V, bcs)
    A = fem.create_matrix(a)
    if method == "gather":
        plan = fem.gather_plan(V, A, 0, _lib.FA_NEO_HOOKEAN)
        over = plan.max_adj * im.NSPLIT[(ct, p)] > im.NEO_THREADS
        assert over == ((name, p) in NEO_OVER)
        assert plan.eadj and plan.max_adj <= im.GATHER_MAX_ADJ and plan.max_blocks <= im.block_cap(ct, p, "neo")
    for k in (0, 1):
        if k:
            a.u.mul_(0.5)
        _fill_nan(A)
        fem.assemble_matrix(a, bcs=bcs, A=A, method=method)
        _check_matrix(A, _ref_neo(oracle, V, name, p, k, marker), _pattern(oracle, V, name, p),
                      f"{name} P{p} neo {method} state {k}")


# ------------------------------------------------------------------------------------- damage law
@pytest.mark.parametrize("method", ["gather", "scatter"])
@pytest.mark.parametrize("tangent", ["hand", "ad"])
def test_asym_damage(oracle, dev, tangent, method):
    from femasm import fem

    name, p = "square_r1", 1
    m, V = _space(name, p, dev)
    g = torch.Generator().manual_seed(5)
    u = (1e-3 * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).to(dev)
    d = torch.rand(V.num_nodes, generator=g, dtype=torch.float64)
    d[d < 0.4] = 0.0  # damaged and undamaged cells
    d = d.to(dev)
    Eh = _E_host(oracle, m.num_cells, 0)
    a = fem.AsymDamage(V, E=torch.tensor(Eh, device=dev), nu=0.3, u=u, d=d, tangent=tangent)
    bcs = _bcs(V, "ref")
    marker, _ = fem._combine_bcs(V, bcs)
    A = fem.create_matrix(a)
    _fill_nan(A)
    fem.assemble_matrix(a, bcs=bcs, A=A, method=method)
    key = ("dam", name)
    if key not in _ref_cache:
        ip, ix = _pattern(oracle, V, name, p)
        lam, mu = oracle.lame(Eh, 0.3)
        _ref_cache[key] = oracle.assemble_damage(_np(V.dofmap), _np(m.cells), _np(m.x), lam, mu, _np(u), _np(d), ip, ix,
                                                 bc=_np(marker), diag=1.0)
    _check_matrix(A, _ref_cache[key], _pattern(oracle, V, name, p), f"{name} damage {tangent} {method}")


# ------------------------------------------------------------------------------------- vectors
@pytest.mark.parametrize("kind", ["lin", "neo"])
@pytest.mark.parametrize("name,p", [("square", 2), ("delaunay", 2)])
def test_residual_lifting_set_bc(oracle, dev, name, p, kind):
    """assemble_vector, then the reference's setF sequence apply_lifting(alpha = -1) + set_bc, each step
    against the oracle at the bar of tests/test_gpu_vector.py."""
    from femasm import fem

    m, V = _space(name, p, dev)
    ct = int(m.cell_type)
    g = torch.Generator().manual_seed(1)
    if kind == "lin":
        u = (1e-3 * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).to(dev)
    else:
        u = _neo_state(V, 0)
    f = (1e4 * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).to(dev)
    Eh = _E_host(oracle, m.num_cells, 0)
    E = torch.tensor(Eh, device=dev)
    J = fem.LinearElasticity(V, E=E, nu=0.3, u=u, f=f) if kind == "lin" else fem.NeoHookean(V, E=E, nu=0.3, u=u, f=f)
    okind = 0 if kind == "lin" else 2
    bcs = _bcs(V, "ref")
    marker, gv = fem._combine_bcs(V, bcs)
    lam, mu = oracle.lame(Eh, 0.3)
    args = (ct, p, _np(V.dofmap), _np(m.cells), _np(m.x), lam, mu)

    def close(b, ref, what):
        err = np.abs(_np(b) - ref).max() / np.abs(ref).max()
        print(f"{name} P{p} {kind} {what}: {err:.3e}")
        assert np.isfinite(ref).all() and err <= RTOL, f"{what}: {err:.3e}"

    b = fem.assemble_vector(J)
    ref = oracle.assemble_residual(*args, u=_np(u), f=_np(f), kind=okind)
    close(b, ref, "residual")
    fem.apply_lifting(b, [J], [bcs], x0=[u], alpha=-1.0)
    ref = oracle.apply_lifting(*args, ref, _np(marker), _np(gv), x0=_np(u), alpha=-1.0,
                               u=_np(u) if okind else None, kind=okind)
    close(b, ref, "lifting")
    fem.set_bc(b, bcs, x0=u, alpha=-1.0)
    mk = _np(marker).astype(bool)
    ref[mk] = -1.0 * (_np(gv)[mk] - _np(u)[mk])
    close(b, ref, "set_bc")


# ------------------------------------------------------------------------------------- matrix-free
@pytest.mark.parametrize("kind", ["lin", "neo"])
@pytest.mark.parametrize("p", [1, 2])
def test_jacobian_operator(oracle, dev, p, kind):
    """fem.JacobianOperator, planned and generic, on the Delaunay mesh against the assembled matrix
    (itself held to the oracle above)."""
    from femasm import fem

    name = "delaunay"
    m, V = _space(name, p, dev)
    E = torch.tensor(_E_host(oracle, m.num_cells, 0), device=dev)
    a = fem.LinearElasticity(V, E=E, nu=0.3) if kind == "lin" else fem.NeoHookean(V, E=E, nu=0.3, u=_neo_state(V, 0))
    bcs = _bcs(V, "comp")
    S = fem.assemble_matrix(a, bcs=bcs, diagonal=DIAG).to_scipy().tocsr()
    for method in ("planned", "generic"):
        op = fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method=method)
        assert (op.num_chunks >= 1) == (method == "planned")
        _check_mult(op, S, dev, f"{name} P{p} {kind} {method}")
        _check_block_diag(op, S, f"{name} P{p} {kind} {method}")


# ------------------------------------------------------------------------------------- refusals
def test_row_over_the_hard_caps_is_refused(oracle, dev):
    """fan(600) P1: row 0 has 600 entries / 601 blocks, over the gather's hard caps (512 / 512), and 1800
    sparsity candidates, so the pattern builds. The gather names the row, its counts and FA_SCATTER; the
    scatter assembles it; ten refusals leave the device memory as it was."""
    from femasm import _lib, fem

    name, p = "fan600", 1
    m, V = _space(name, p, dev)
    a = fem.LinearElasticity(V, E=torch.tensor(_E_host(oracle, m.num_cells, 0), device=dev), nu=0.3)
    bcs = _bcs(V, "comp")
    marker, _ = fem._combine_bcs(V, bcs)
    A = fem.create_matrix(a, check=True)

    def refused(**kw):
        with pytest.raises(_lib.FemasmError, match=r"row 0 has 601 blocks / 600 cells.*512.*FA_SCATTER"):
            fem.assemble_matrix(a, bcs=bcs, A=A, **kw)

    for kw in (dict(), dict(plan=dict(owner=False)), dict(plan=dict(owner=True)), dict(deterministic=True)):
        refused(**kw)
    torch.cuda.synchronize()
    before = (_pool_used_bytes(dev), torch.cuda.memory_allocated(dev))
    for _ in range(10):
        refused()
    torch.cuda.synchronize()
    after = (_pool_used_bytes(dev), torch.cuda.memory_allocated(dev))
    print(f"(pool, torch) bytes in use: {before} before, {after} after ten refused calls")
    assert after == before
    u = _neo_state(V, 0)
    with pytest.raises(_lib.FemasmError, match=r"row 0 has 601 blocks / 600 cells.*FA_SCATTER"):
        fem.assemble_matrix(fem.NeoHookean(V, E=a.E, nu=0.3, u=u), bcs=bcs, A=A)
    _fill_nan(A)
    fem.assemble_matrix(a, bcs=bcs, A=A, method="scatter")
    _check_matrix(A, _ref_lin(oracle, V, name, p, "comp", 0, marker), _pattern(oracle, V, name, p), "fan600 scatter")


def test_sparsity_cap_is_refused(dev):
    """fan(700) P1: 2100 (cell, node) candidates in row 0, over kSparsityCap = 2048."""
    from femasm import _lib, fem

    m, V = _space("fan700", 1, dev)
    with pytest.raises(_lib.FemasmError, match=rf"more than {im.SPARSITY_CAP} \(cell, node\) candidates"):
        fem.create_matrix(fem.LinearElasticity(V, E=1.0, nu=0.3))
