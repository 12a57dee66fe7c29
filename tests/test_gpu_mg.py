"""Geometric multigrid on the GPU (femasm.mg over femasm_mg.hip): the transfer kernels against the
stencil matrix ``mg.transfer_matrix`` (itself checked against brute-force point location in
test_mg_host.py), the fused smoother step against its torch formula, the V-cycle as a symmetric
positive definite operator, MG-preconditioned CG against block-Jacobi CG (same solution, fewer
iterations, slower growth with the mesh), and the Newton driver with the preconditioner set.

Measured on the MI355X (also in DESIGN.md section 3.8):
  V-cycle asymmetry |<Mr1,r2> - <r1,Mr2>| / (|Mr1| |r2|): P2 tetrahedra 8^3 0 (the inner products agree to
  the last bit), Q2 quadrilaterals 16^2 7.8e-18 (bar 1e-8).
  Linear elasticity, P2 tetrahedra, rtol 1e-10: 8^3 block-Jacobi 278 its, MG 16; 16^3 block-Jacobi 544, MG 17;
  the solutions differ by 1.0e-9 and 1.5e-9.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sps
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _dev(a, dev, dtype=torch.float64):
    return torch.tensor(a, dtype=dtype, device=dev)


def _corner_dofs(points, bs):
    """All dofs of the lattice's corner nodes (index 0 fastest)."""
    nodes = []
    for corner in np.ndindex(*(2,) * len(points)):
        idx = 0
        for d in range(len(points) - 1, -1, -1):
            idx = idx * points[d] + corner[d] * (points[d] - 1)
        nodes.append(idx)
    return np.array([n * bs + c for n in sorted(set(nodes)) for c in range(bs)])


def _mask(rng, n, points, bs):
    m = (rng.random(n) < 0.2).astype(np.int8)
    m[_corner_dofs(points, bs)] = 1
    return m


# coarse lattices with an axis of length 1, and one that needs several workgroups with unequal strides
@pytest.mark.parametrize("nc", [(2, 1, 2), (1, 2), (12, 10, 6)])
@pytest.mark.parametrize("simplex", [True, False])
def test_transfer_kernels_match_the_stencil_matrix(dev, nc, simplex):
    from femasm import mg

    rng = np.random.default_rng(7)
    P1 = mg.transfer_matrix(mg.Transfer(len(nc), simplex, 1, nc))
    for bs in (1, 2, 3):
        t = mg.Transfer(len(nc), simplex, bs, nc)
        P = sps.kron(P1, sps.identity(bs), format="csr")
        nf, ncd = P.shape
        assert (nf, ncd) == (t.num_fine_dofs, t.num_coarse_dofs)
        absP = abs(P)
        for masked in (False, True):
            mc = _mask(rng, ncd, t.coarse_points, bs) if masked else np.zeros(ncd, np.int8)
            mf = _mask(rng, nf, t.fine_points, bs) if masked else np.zeros(nf, np.int8)
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


def test_transfer_and_smoother_argument_errors(dev):
    from femasm import _lib, mg

    L = _lib.load()
    sh = _lib.stream_handle(dev)
    x = torch.zeros(64, dtype=torch.float64, device=dev)
    t = mg.Transfer(2, True, 1, (1, 1))._fa()
    assert L.fa_prolong(ctypes.byref(t), None, None, None, 0, x.data_ptr(), sh) == _lib.FA_E_ARG
    assert b"null" in L.fa_last_error()
    assert L.fa_restrict(None, x.data_ptr(), None, None, x.data_ptr(), sh) == _lib.FA_E_ARG
    for bad in (dict(tdim=4), dict(simplex=2), dict(nc0=0)):
        t = mg.Transfer(2, True, 1, (1, 1))._fa()
        t.tdim = bad.get("tdim", t.tdim)
        t.simplex = bad.get("simplex", t.simplex)
        t.nc[0] = bad.get("nc0", t.nc[0])
        assert L.fa_restrict(ctypes.byref(t), x.data_ptr(), None, None, x.data_ptr(), sh) == _lib.FA_E_ARG, bad
    t = mg.Transfer(2, True, 1, (1, 1))._fa()
    t.bs = 4
    assert L.fa_prolong(ctypes.byref(t), x.data_ptr(), None, None, 0, x.data_ptr(), sh) == _lib.FA_E_UNSUPPORTED
    assert L.fa_cheb_step(4, 1, None, x.data_ptr(), None, 0.0, 1.0, x.data_ptr(), x.data_ptr(), sh) == _lib.FA_E_ARG
    assert L.fa_cheb_step(4, 5, x.data_ptr(), x.data_ptr(), None, 0.0, 1.0, x.data_ptr(), x.data_ptr(), sh) \
        == _lib.FA_E_UNSUPPORTED
    with pytest.raises(ValueError):
        mg.prolong(mg.Transfer(2, True, 1, (1, 1)), x[:4], x[:10])  # 9 fine dofs expected


@pytest.mark.parametrize("bs", [1, 2, 3])
def test_cheb_step_matches_torch(dev, bs):
    from femasm import mg

    g = torch.Generator().manual_seed(11 + bs)
    nn = 1037  # several workgroups, not a multiple of the block
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dev)
    Dinv, b, Ax, d0, x0 = rnd(nn, bs, bs), rnd(nn * bs), rnd(nn * bs), rnd(nn * bs), rnd(nn * bs)
    absmv = lambda v: torch.bmm(Dinv.abs(), v.view(-1, bs, 1)).reshape(-1)
    for c_d, c_r, use_Ax in ((0.37, -1.3, True), (0.0, 0.8, True), (0.21, 0.6, False)):
        res = b - Ax if use_Ax else b
        d_ref = c_d * d0 + c_r * torch.bmm(Dinv, res.view(-1, bs, 1)).reshape(-1)
        x_ref = x0 + d_ref
        # c_d == 0 must not read d: poison it
        d = torch.full_like(d0, float("nan")) if c_d == 0.0 else d0.clone()
        x = x0.clone()
        mg.cheb_step(Dinv, b, Ax if use_Ax else None, c_d, c_r, d, x)
        mag = abs(c_d) * d0.abs() + abs(c_r) * absmv(b.abs() + (Ax.abs() if use_Ax else 0))
        assert bool((torch.abs(d - d_ref) <= 1e-14 * mag).all()), float(torch.abs(d - d_ref).max())
        assert bool((torch.abs(x - x_ref) <= 1e-14 * (mag + x0.abs())).all())


def _elasticity(oracle, dev, ct, p, n, comps_right=None, u=False, body_force=None):
    from femasm import fem, mesh

    m = (mesh.create_unit_square(*n, cell_type=ct, device=dev) if len(n) == 2
         else mesh.create_unit_cube(*n, cell_type=ct, device=dev))
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    E = torch.tensor(oracle.e_range()[np.arange(m.num_cells) % 200], device=dev)
    uf = fem.Function(V) if u else None
    f = None
    if body_force is not None:  # along y, as the reference's f
        f = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
        f[1::m.gdim] = body_force
    a = fem.LinearElasticity(V, E=E, nu=0.3, u=uf, f=f)
    left = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.zeros_like(x[0])))
    right = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.ones_like(x[0])))
    bcs = [fem.dirichletbc(0.0, left, V),
           fem.dirichletbc([1e-3] + [0.0] * (m.gdim - 1), right, V, components=comps_right)]
    return V, a, bcs, uf


@pytest.mark.parametrize("ct,n,coarse_dofs,nlevels", [(-4, (8, 8, 8), 200, 4), (4, (16, 16), 100, 4)])
def test_vcycle_is_symmetric_positive_definite(oracle, dev, ct, n, coarse_dofs, nlevels):
    """Mixed bcs: x = 0 clamped, x = 1 constrained in its first component only. A missing mask or
    unequal pre / post polynomials break the symmetry at the 1e-2 level."""
    from femasm import fem, mg

    diagonal = 2.0
    V, a, bcs, _ = _elasticity(oracle, dev, ct, 2, n, comps_right=[0])
    M = mg.GeometricMultigrid(a, bcs, diagonal=diagonal, coarse_dofs=coarse_dofs)
    assert len(M.levels) == nlevels and M.levels[0][:3] == (2, n, V.num_dofs)
    assert M.levels[1][:2] == (1, n) and M.levels[-1][3] == "direct" and M.levels[0][3] == "matrix-free"
    assert 1.0 < M.operator_complexity < 1.5
    M.update()
    g = torch.Generator().manual_seed(3)
    r1, r2 = (torch.randn(V.num_dofs, generator=g, dtype=torch.float64).to(dev) for _ in range(2))
    z1, z2 = M.apply(r1).clone(), M.apply(r2, torch.empty_like(r2))
    asym = abs(float(torch.dot(z1, r2) - torch.dot(r1, z2))) / float(z1.norm() * r2.norm())
    print(f"V-cycle asymmetry {asym:.3e} ({M.levels})")
    assert asym <= 1e-8
    assert float(torch.dot(z1, r1)) > 0 and float(torch.dot(z2, r2)) > 0
    marker, _ = fem._combine_bcs(V, bcs, with_g=False)
    on = marker != 0
    assert int(on.sum()) > 0
    assert torch.equal(z1[on], r1[on] / diagonal)
    # the preconditioner is a fixed linear operator: the same input gives the same bits; with z given
    # the call allocates no device memory
    torch.cuda.synchronize()
    n0 = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    M.apply(r1, z2)
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == n0
    assert torch.equal(z2, z1)


def test_one_level_and_polynomial_coarsest_level(oracle, dev):
    """The two ends of the hierarchy rule: a space of at most coarse_dofs dofs is one level, inverted
    densely (the preconditioner is then the inverse); a coarsest level above coarse_dofs (max_levels
    reached) gets a fixed Chebyshev polynomial and the cycle stays symmetric positive definite."""
    from femasm import fem, mg, nls

    V, a, bcs, _ = _elasticity(oracle, dev, 3, 2, (4, 4))
    M = mg.GeometricMultigrid(a, bcs)
    assert M.levels == [(2, (4, 4), V.num_dofs, "direct")] and M.operator_complexity == 1.0
    g = torch.Generator().manual_seed(5)
    r = torch.randn(V.num_dofs, generator=g, dtype=torch.float64).to(dev)
    z = M.apply(r)
    A = fem.JacobianOperator(a, bcs=bcs)
    assert float((A.mult(z) - r).norm()) <= 1e-10 * float(r.norm())

    V, a, bcs, _ = _elasticity(oracle, dev, -4, 2, (4, 4, 4), comps_right=[0])
    M = mg.GeometricMultigrid(a, bcs, coarse_dofs=0, max_levels=2)
    assert [lv[3] for lv in M.levels] == ["matrix-free", "chebyshev"] and M.levels[1][:2] == (1, (4, 4, 4))
    r1, r2 = (torch.randn(V.num_dofs, generator=g, dtype=torch.float64).to(dev) for _ in range(2))
    z1, z2 = M.apply(r1).clone(), M.apply(r2).clone()
    asym = abs(float(torch.dot(z1, r2) - torch.dot(r1, z2))) / float(z1.norm() * r2.norm())
    assert asym <= 1e-8 and float(torch.dot(z1, r1)) > 0 and float(torch.dot(z2, r2)) > 0
    A = fem.JacobianOperator(a, bcs=bcs)
    # both solves at rtol 1e-12 on the preconditioned residual: the error left is at most that times
    # the condition number of the preconditioned operator, a few hundred for block-Jacobi on this mesh
    # (its iteration count k ~ sqrt(kappa) ln(2 / rtol) / 2), so the two agree well within 1e-8
    xs = []
    for pre in (None, M):
        ks = nls.KrylovSolver(rtol=1e-12)
        ks.set_preconditioner(pre)
        ks.set_operator(A)
        x = torch.zeros_like(r1)
        xs.append((ks.solve(x, r1), x))
    assert xs[1][0] < xs[0][0]
    assert float((xs[1][1] - xs[0][1]).norm()) <= 1e-8 * float(xs[0][1].norm())


def _solve_pair(oracle, dev, n):
    from femasm import mg, nls

    V, a, bcs, u = _elasticity(oracle, dev, -4, 2, n, u=True, body_force=-1e3)
    problem = nls.NonlinearProblem(a, u, bcs, matrix_free=True)
    b = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
    problem.F(u.x, b)
    A = problem.matrix()
    out = []
    for use_mg in (False, True):
        ks = nls.KrylovSolver(rtol=1e-10)
        if use_mg:
            ks.set_preconditioner(mg.GeometricMultigrid(a, bcs, fine_operator=A))
        ks.set_operator(A)
        x = torch.zeros_like(b)
        out.append((ks.solve(x, b), x))
    return out


def test_mg_pcg_matches_jacobi_pcg_with_fewer_iterations(oracle, dev):
    """Linear elasticity, E_range[cell % 200], nu 0.3, x = 0 clamped and x = 1 prescribed, P2
    tetrahedra 8^3 and 16^3, both solvers at rtol 1e-10."""
    its = {}
    for side in (8, 16):
        (its_j, x_j), (its_mg, x_mg) = _solve_pair(oracle, dev, (side,) * 3)
        rel = float((x_mg - x_j).norm() / x_j.norm())
        print(f"side {side}: block-Jacobi {its_j} its, MG {its_mg} its, solutions differ by {rel:.3e}")
        assert rel <= 1e-8
        assert its_mg < its_j
        its[side] = (its_j, its_mg)
    # halfway between flat growth and block-Jacobi's growth
    assert its[16][1] / its[8][1] <= (1 + its[16][0] / its[8][0]) / 2, its


@pytest.mark.parametrize("kind,ct,p,n,coarse_dofs,matrix_free", [(2, -4, 2, (4, 4, 4), 300, True),
                                                                 (1, 3, 1, (16, 16), 100, False)])
def test_newton_with_multigrid_matches_newton(oracle, dev, kind, ct, p, n, coarse_dofs, matrix_free):
    """NeoHookean on P2 tetrahedra (matrix-free fine level) and AsymDamage on P1 triangles (the
    assembled Jacobian as the fine level), loads of test_gpu_newton.py."""
    from femasm import fem, mesh, mg, nls

    results = []
    for use_mg in (False, True):
        m = (mesh.create_unit_square(*n, cell_type=ct, device=dev) if len(n) == 2
             else mesh.create_unit_cube(*n, cell_type=ct, device=dev))
        V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
        E = torch.tensor(oracle.e_range()[np.arange(m.num_cells) % 200], device=dev)
        u = fem.Function(V)
        f = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
        f[1::m.gdim] = -1e3
        if kind == 1:
            xn = V.tabulate_dof_coordinates()
            d = (0.6 * torch.exp(-20 * ((xn[:, 0] - 0.5) ** 2 + (xn[:, 1] - 0.5) ** 2))).contiguous()
            form = fem.AsymDamage(V, E=E, nu=0.3, u=u, d=d, f=f)
        else:
            form = fem.NeoHookean(V, E=E, nu=0.3, u=u, f=f)
        disp = 0.05 if kind == 2 else 1e-3
        left = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.zeros_like(x[0])))
        right = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.ones_like(x[0])))
        bcs = [fem.dirichletbc(0.0, left, V), fem.dirichletbc([disp] + [0.0] * (m.gdim - 1), right, V)]
        problem = nls.NonlinearProblem(form, u, bcs, matrix_free=matrix_free and use_mg)
        solver = nls.NewtonSolver(None, problem)
        solver.rtol, solver.atol, solver.max_it = 1e-7, 5e-8, 10
        M = None
        if use_mg:
            M = mg.GeometricMultigrid(form, bcs, fine_operator=problem.matrix(), coarse_dofs=coarse_dofs)
            assert len(M.levels) == 3 and M.levels[-1][3] == "direct"
            solver.krylov_solver.set_preconditioner(M)
        it, conv = solver.solve(u)
        assert conv
        results.append((it, u.x.clone(), solver.krylov_iterations, M))
    (it0, u0, k0, _), (it1, u1, k1, M) = results
    print(f"Newton {it0} / {it1} steps, Krylov iterations block-Jacobi {k0}, MG {k1}")
    assert float((u1 - u0).norm() / u0.norm()) <= 1e-8
    assert abs(it1 - it0) <= 1
    assert M.updates == it1  # one update per Newton step
    assert k1 < k0
