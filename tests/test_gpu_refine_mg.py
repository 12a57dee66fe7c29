"""Uniform refinement and the multigrid over refined meshes on the GPU (mesh.refine over
fa_refine_cells / fa_edge_midpoints, mg.EdgeTransfer over fa_prolong_edges / fa_restrict_edges,
mg.GeometricMultigrid on meshes without a lattice): device refinement against the host definition, the
edge transfer kernels against ``mg.edge_transfer_matrix`` (itself checked in test_refine_host.py), the
V-cycle as a symmetric positive definite operator, MG-preconditioned CG against block-Jacobi CG, and the
Newton driver with the preconditioner set.

Measured on the MI355X (also in DESIGN.md section 3.9):
  V-cycle asymmetry |<Mr1,r2> - <r1,Mr2>| / (|Mr1| |r2|): square.msh r=2 P2 (4 levels) 2.1e-18, refined
  (2,2,2) box P1 (2 levels) 5.1e-18 (bar 1e-8).
  Linear elasticity on square.msh r=3, P1, rtol 1e-12: block-Jacobi 504 its, MG 17, solutions 9.5e-12 apart.
  At rtol 1e-10 and r = 2, 3, 4: block-Jacobi 230, 458, 916; MG 12, 14, 16 (not flat: two more per level).
  Newton: AsymDamage P1 triangles 4 / 4 steps, Krylov iterations 1045 block-Jacobi, 58 MG; NeoHookean P2
  tetrahedra 4 / 4 steps, 696 and 87.
"""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sps
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = os.path.join(ROOT, "tests", "golden", "square.msh")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _dev(a, dev, dtype=torch.float64):
    return torch.tensor(a, dtype=dtype, device=dev)


def _single(ct):
    from femasm import mesh

    if ct == 3:
        x = torch.tensor([[0.1, 0.0], [1.3, 0.2], [0.4, 0.9]], dtype=torch.float64)
        return mesh.Mesh(mesh.CellType.triangle, x, torch.tensor([[0, 1, 2]], dtype=torch.int32),
                         torch.tensor([7], dtype=torch.int32))
    x = torch.tensor([[0.0, 0.1, 0.0], [1.2, 0.0, 0.1], [0.3, 0.9, 0.0], [0.2, 0.3, 1.1]], dtype=torch.float64)
    return mesh.Mesh(mesh.CellType.tetrahedron, x, torch.tensor([[0, 1, 2, 3]], dtype=torch.int32),
                     torch.tensor([5], dtype=torch.int32))


def _box(n, lengths=(1.0, 1.0, 1.0), tags=False):
    """A tetrahedral box without its lattice record: an unstructured mesh as far as the package knows."""
    from femasm import mesh

    b = mesh.create_box(lengths, n, mesh.CellType.tetrahedron)
    t = (torch.arange(b.num_cells, dtype=torch.int32) % 5) if tags else None
    return mesh.Mesh(b.cell_type, b.x, b.cells, t, None)


def _square():
    from femasm import mesh

    return mesh.read_gmsh(SQUARE, gdim=2)


def _fan(ntri=70):
    """ntri triangles around vertex 0: a node of valence ntri, more than one wavefront of edges."""
    from femasm import mesh

    t = torch.arange(ntri, dtype=torch.float64) * (2 * np.pi / ntri)
    x = torch.cat([torch.zeros(1, 2, dtype=torch.float64), torch.stack([torch.cos(t), torch.sin(t)], 1)])
    i = torch.arange(ntri)
    cells = torch.stack([torch.zeros_like(i), 1 + i, 1 + (i + 1) % ntri], 1).to(torch.int32)
    return mesh.Mesh(mesh.CellType.triangle, x, cells)


def _refined(m, r):
    from femasm import mesh

    for _ in range(r):
        m = mesh.refine(m)
    return m


# ------------------------------------------------------------------------------------ 1. refinement parity
@pytest.mark.parametrize("name,r", [("triangle", 1), ("tetrahedron", 1), ("square", 3), ("box", 1)])
def test_device_refine_equals_host_refine(dev, name, r):
    from femasm import mesh

    m = {"triangle": lambda: _single(3), "tetrahedron": lambda: _single(-4), "square": _square,
         "box": lambda: _box((5, 4, 3), (1.0, 0.9, 0.7), tags=True)}[name]()
    h, d = m, m.to(dev)
    for _ in range(r):
        h, d = mesh.refine(h), mesh.refine(d)
        assert d.device.type == "cuda" and d.structured is None and d.parent is not None
        assert d.cells.dtype == torch.int32 and torch.equal(d.cells.cpu(), h.cells)  # exactly
        assert torch.equal(d.cell_tags.cpu(), h.cell_tags)
        # bit for bit: compare the float64 patterns
        assert torch.equal(d.x.cpu().view(torch.int64), h.x.view(torch.int64))
    up = h.to(dev)
    assert up.parent is not None and up.parent.device.type == "cuda" and torch.equal(up.cells, d.cells)
    if name == "triangle":  # quadrilaterals are refused on the device as on the host
        with pytest.raises(ValueError):
            mesh.refine(mesh.create_rectangle((1, 1), (2, 2), mesh.CellType.quadrilateral, device=dev))


def test_untagged_mesh_refines_on_the_device(dev):
    from femasm import mesh

    m = _box((1, 2, 1))
    h, d = mesh.refine(m), mesh.refine(m.to(dev))
    assert d.cell_tags is None and h.cell_tags is None
    assert torch.equal(d.cells.cpu(), h.cells) and torch.equal(d.x.cpu().view(torch.int64), h.x.view(torch.int64))


# ------------------------------------------------------------------------------------ 2. edge transfers
TRANSFER_MESHES = {"triangle": lambda: _single(3), "square": _square, "box121": lambda: _box((1, 2, 1)),
                   "box543": lambda: _box((5, 4, 3)), "fan70": _fan}


@pytest.mark.parametrize("name", list(TRANSFER_MESHES))
def test_edge_transfer_kernels_match_the_stencil_matrix(dev, name):
    from femasm import mesh, mg

    m = TRANSFER_MESHES[name]()
    ev = mesh.entities(m, 1)[0]
    if name == "fan70":
        assert int(torch.bincount(ev.reshape(-1)).max()) == 70
    rng = np.random.default_rng(7)
    P1 = mg.edge_transfer_matrix(mg.EdgeTransfer(ev, m.num_vertices, 1))
    for bs in (1, 2, 3):
        t = mg.EdgeTransfer(ev.to(dev), m.num_vertices, bs)
        P = sps.kron(P1, sps.identity(bs), format="csr")
        nf, ncd = P.shape
        assert (nf, ncd) == (t.num_fine_dofs, t.num_coarse_dofs)
        absP = abs(P)
        for masked in (False, True):
            mc = (rng.random(ncd) < 0.2).astype(np.int8) if masked else np.zeros(ncd, np.int8)
            mf = (rng.random(nf) < 0.2).astype(np.int8) if masked else np.zeros(nf, np.int8)
            bc_c = _dev(mc, dev, torch.int8) if masked else None
            bc_f = _dev(mf, dev, torch.int8) if masked else None
            xc, rf = rng.standard_normal(ncd), rng.standard_normal(nf)
            xc_m, rf_m = xc * (mc == 0), rf * (mf == 0)
            for add in (False, True):
                y0 = rng.standard_normal(nf) if add else np.full(nf, np.nan)
                y = _dev(y0, dev)
                mg.prolong(t, _dev(xc, dev), y, bc_c=bc_c, bc_f=bc_f, add=add)
                ref = (P @ xc_m) * (mf == 0)
                bound = 1e-14 * (absP @ np.abs(xc_m)) * (mf == 0)
                if add:
                    ref, bound = ref + y0, bound + 1e-14 * np.abs(y0) * (mf == 0)
                err = np.abs(_np(y) - ref)
                assert np.isfinite(err).all() and (err <= bound).all(), (bs, masked, add, err.max())
            out = torch.full((ncd,), float("nan"), dtype=torch.float64, device=dev)
            mg.restrict(t, _dev(rf, dev), out, bc_f=bc_f, bc_c=bc_c)
            ref = (P.T @ rf_m) * (mc == 0)
            bound = 1e-14 * (absP.T @ np.abs(rf_m)) * (mc == 0)
            err = np.abs(_np(out) - ref)
            assert np.isfinite(err).all() and (err <= bound).all(), (bs, masked, err.max())
            again = torch.full((ncd,), float("nan"), dtype=torch.float64, device=dev)
            mg.restrict(t, _dev(rf, dev), again, bc_f=bc_f, bc_c=bc_c)
            assert torch.equal(out, again)  # bit-identical


def test_edge_transfer_argument_errors(dev):
    from femasm import _lib, mesh, mg

    L = _lib.load()
    sh = _lib.stream_handle(dev)
    m = _single(3)
    t = mg.EdgeTransfer(mesh.entities(m, 1)[0].to(dev), 3, 1)
    # outputs poisoned: an error must return before anything is launched
    x = torch.full((64,), float("nan"), dtype=torch.float64, device=dev)
    fa = t._fa()
    assert L.fa_prolong_edges(ctypes.byref(fa), None, None, None, 0, x.data_ptr(), sh) == _lib.FA_E_ARG
    assert b"null" in L.fa_last_error()
    assert L.fa_restrict_edges(None, x.data_ptr(), None, None, x.data_ptr(), sh) == _lib.FA_E_ARG
    assert L.fa_prolong_edges(None, x.data_ptr(), None, None, 0, x.data_ptr(), sh) == _lib.FA_E_ARG

    def desc(**kw):
        d = _lib.fa_edge_transfer()
        d.ncoarse, d.nedges, d.bs = fa.ncoarse, fa.nedges, fa.bs
        d.edge_verts, d.vptr, d.vedges = fa.edge_verts, fa.vptr, fa.vedges
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for bad in (dict(edge_verts=None), dict(vptr=None), dict(vedges=None), dict(ncoarse=-1), dict(nedges=-1)):
        d = desc(**bad)
        assert L.fa_restrict_edges(ctypes.byref(d), x.data_ptr(), None, None, x.data_ptr(), sh) == _lib.FA_E_ARG, bad
        assert L.fa_prolong_edges(ctypes.byref(d), x.data_ptr(), None, None, 0, x.data_ptr(), sh) == _lib.FA_E_ARG, bad
    for bs in (0, 4):
        d = desc(bs=bs)
        assert L.fa_prolong_edges(ctypes.byref(d), x.data_ptr(), None, None, 0, x.data_ptr(), sh) == _lib.FA_E_UNSUPPORTED
        assert L.fa_restrict_edges(ctypes.byref(d), x.data_ptr(), None, None, x.data_ptr(), sh) == _lib.FA_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all())
    with pytest.raises(ValueError):
        mg.prolong(t, x[:3], x[:7])  # 6 fine dofs expected
    with pytest.raises(ValueError):
        mg.restrict(t, x[:6].cpu(), x[:3].cpu())  # the tables are on the device
    # refinement entry points
    i32 = torch.zeros(64, dtype=torch.int32, device=dev)
    assert L.fa_refine_cells(4, 1, 4, i32.data_ptr(), i32.data_ptr(), x.data_ptr(), None, i32.data_ptr(), None, sh) \
        == _lib.FA_E_UNSUPPORTED
    assert L.fa_refine_cells(-4, 1, 4, i32.data_ptr(), i32.data_ptr(), None, None, i32.data_ptr(), None, sh) == _lib.FA_E_ARG
    assert L.fa_refine_cells(3, 2 ** 30, 4, i32.data_ptr(), i32.data_ptr(), None, None, i32.data_ptr(), None, sh) \
        == _lib.FA_E_CAPACITY
    assert L.fa_edge_midpoints(-1, 2, i32.data_ptr(), x.data_ptr(), x.data_ptr(), sh) == _lib.FA_E_ARG
    assert L.fa_edge_midpoints(1, 4, i32.data_ptr(), x.data_ptr(), x.data_ptr(), sh) == _lib.FA_E_ARG
    torch.cuda.synchronize()
    assert bool((i32 == 0).all())


# ------------------------------------------------------------------------------------ 3. V-cycle
def _bcs(V, comps_right=None, disp=1e-3):
    from femasm import fem

    g = V.mesh.gdim
    left = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.zeros_like(x[0])))
    right = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.ones_like(x[0])))
    return [fem.dirichletbc(0.0, left, V), fem.dirichletbc([disp] + [0.0] * (g - 1), right, V, components=comps_right)]


def _cell_E(oracle, m):
    """E per physical tag where the mesh has tags (as the reference assigns it), else per cell."""
    key = m.cell_tags.cpu().numpy() if m.cell_tags is not None else np.arange(m.num_cells)
    return torch.tensor(oracle.e_range()[key % 200], device=m.device)


@pytest.mark.parametrize("name,r,p,coarse_dofs,degrees", [("square", 2, 2, 200, [2, 1, 1, 1]),
                                                           ("box", 1, 1, 100, [1, 1])])
def test_vcycle_is_symmetric_positive_definite(oracle, dev, name, r, p, coarse_dofs, degrees):
    """Mixed bcs: x = 0 clamped, x = 1 constrained in its first component only."""
    from femasm import fem, mg

    diagonal = 2.0
    m = _refined((_square() if name == "square" else _box((2, 2, 2))).to(dev), r)
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    a = fem.LinearElasticity(V, E=_cell_E(oracle, m), nu=0.3)
    bcs = _bcs(V, comps_right=[0])
    M = mg.GeometricMultigrid(a, bcs, diagonal=diagonal, coarse_dofs=coarse_dofs)
    assert [lv[0] for lv in M.levels] == degrees and all(lv[1] is None for lv in M.levels)
    assert M.levels[0][2:] == (V.num_dofs, "matrix-free") and M.levels[-1][3] == "direct"
    assert M.levels[-1][2] <= coarse_dofs < M.levels[-2][2]
    assert all(lv[3] == "assembled" for lv in M.levels[1:-1])
    M.update()
    g = torch.Generator().manual_seed(3)
    r1, r2 = (torch.randn(V.num_dofs, generator=g, dtype=torch.float64).to(dev) for _ in range(2))
    z1, z2 = M.apply(r1).clone(), M.apply(r2, torch.empty_like(r2))
    asym = abs(float(torch.dot(z1, r2) - torch.dot(r1, z2))) / float(z1.norm() * r2.norm())
    print(f"{name} r={r} P{p}: V-cycle asymmetry {asym:.3e} ({M.levels})")
    assert asym <= 1e-8
    assert float(torch.dot(z1, r1)) > 0 and float(torch.dot(z2, r2)) > 0
    marker, _ = fem._combine_bcs(V, bcs, with_g=False)
    on = marker != 0
    assert int(on.sum()) > 0
    assert torch.equal(z1[on], r1[on] / diagonal)
    torch.cuda.synchronize()
    n0 = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    M.apply(r1, z2)
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == n0
    assert torch.equal(z2, z1)


# ------------------------------------------------------------------------------------ 4. PCG
def solve_pair(oracle, dev, r, rtol):
    """Linear elasticity on square.msh refined r times, P1, E per tag, x = 0 clamped, x = 1 prescribed,
    body force along y: [(iterations, solution)] of block-Jacobi PCG and of multigrid PCG."""
    from femasm import fem, mg, nls

    m = _refined(_square().to(dev), r)
    V = fem.functionspace(m, ("Lagrange", 1, (2,)))
    u = fem.Function(V)
    f = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
    f[1::2] = -1e3
    a = fem.LinearElasticity(V, E=_cell_E(oracle, m), nu=0.3, u=u, f=f)
    bcs = _bcs(V)
    problem = nls.NonlinearProblem(a, u, bcs, matrix_free=True)
    b = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
    problem.F(u.x, b)
    A = problem.matrix()
    out = []
    for use_mg in (False, True):
        ks = nls.KrylovSolver(rtol=rtol, max_it=20000)
        if use_mg:
            ks.set_preconditioner(mg.GeometricMultigrid(a, bcs, fine_operator=A, coarse_dofs=200))
        ks.set_operator(A)
        x = torch.zeros_like(b)
        out.append((ks.solve(x, b), x))
    return out, V.num_dofs


def test_mg_pcg_matches_jacobi_pcg_with_fewer_iterations(oracle, dev):
    """Both solvers stop at rtol 1e-12 on their preconditioned residual; the error left is at most rtol
    times the condition number of the preconditioned operator. For block-Jacobi on P1 with one clamped
    side that is about 32 / (pi h)^2 for the Laplacian (lambda_min ~ (pi h)^2 / 16, lambda_max ~ 2), times
    the spread of E (2.7 between the two tags) and a factor of about 3 for elasticity at nu = 0.3: with
    h = 1 / 56 (7 cells per side, refined three times) about 1e5, so the two solutions agree to 1e-7."""
    (its_j, x_j), (its_mg, x_mg) = solve_pair(oracle, dev, 3, 1e-12)[0]
    rel = float((x_mg - x_j).norm() / x_j.norm())
    print(f"square.msh r=3 P1: block-Jacobi {its_j} its, MG {its_mg} its, solutions differ by {rel:.3e}")
    assert rel <= 1e-7
    assert its_mg < its_j


# ------------------------------------------------------------------------------------ 5. Newton
@pytest.mark.parametrize("kind", ["damage-p1-triangles", "neo-p2-tetrahedra"])
def test_newton_with_multigrid_matches_newton(oracle, dev, kind):
    """AsymDamage on P1 triangles (square.msh refined twice, E per tag, damage 0.5 on the nodes of the
    cells of tag 2) and NeoHookean on P2 tetrahedra (a refined box): matrix-free Newton with the
    refined-mesh multigrid against plain Newton, loads of test_gpu_newton.py."""
    from femasm import fem, mg, nls

    results = []
    for use_mg in (False, True):
        if kind == "damage-p1-triangles":
            m = _refined(_square().to(dev), 2)
            V = fem.functionspace(m, ("Lagrange", 1, (2,)))
            coarse_dofs, disp = 200, 1e-3
        else:
            m = _refined(_box((2, 2, 2)).to(dev), 1)
            V = fem.functionspace(m, ("Lagrange", 2, (3,)))
            coarse_dofs, disp = 300, 0.05
        E = _cell_E(oracle, m)
        u = fem.Function(V)
        f = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
        f[1::m.gdim] = -1e3
        if kind == "damage-p1-triangles":
            d = torch.zeros(V.num_nodes, dtype=torch.float64, device=dev)
            d[m.cells[m.cell_tags == 2].to(torch.int64).reshape(-1)] = 0.5
            assert 0 < int((d > 0).sum()) < V.num_nodes
            form = fem.AsymDamage(V, E=E, nu=0.3, u=u, d=d, f=f)
        else:
            form = fem.NeoHookean(V, E=E, nu=0.3, u=u, f=f)
        bcs = _bcs(V, disp=disp)
        problem = nls.NonlinearProblem(form, u, bcs, matrix_free=use_mg)
        solver = nls.NewtonSolver(None, problem)
        solver.rtol, solver.atol, solver.max_it = 1e-7, 5e-8, 10
        M = None
        if use_mg:
            M = mg.GeometricMultigrid(form, bcs, fine_operator=problem.matrix(), coarse_dofs=coarse_dofs)
            assert len(M.levels) == 3 and M.levels[-1][3] == "direct" and M.levels[0][3] == "matrix-free"
            solver.krylov_solver.set_preconditioner(M)
        it, conv = solver.solve(u)
        assert conv
        results.append((it, u.x.clone(), solver.krylov_iterations, M))
    (it0, u0, k0, _), (it1, u1, k1, M) = results
    print(f"{kind}: Newton {it0} / {it1} steps, Krylov iterations block-Jacobi {k0}, MG {k1} ({M.levels})")
    assert float((u1 - u0).norm() / u0.norm()) <= 1e-8
    assert abs(it1 - it0) <= 1
    assert M.updates == it1  # one update per Newton step
    assert k1 < k0
