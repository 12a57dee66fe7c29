"""GPU checks of the exterior-facet loads: k_facet_load (fa_facet_load_apply) against the independent
reference of tests/facet_reference.py and against the library's torch definition, the wiring into
``assemble_vector``, equilibrium at known homogeneous solutions and a load-controlled Newton solve.

Bar: max|b - ref| <= 1e-12 max|ref| (tests/test_gpu_vector.py RTOL). Tensor cells pass
quadrature_degree = 2p + 2, the reference's own p + 2 point Gauss rule: the area element of a warped
hexahedron face is no polynomial, so the two sides compare the same quadrature sum there (see
tests/test_facet_host.py). Newton solve reached (DESIGN.md, section "Exterior-facet loads"): both variants
take 3 iterations and end 2.0e-10 max|u| from the homogeneous field, against the 1e-6 asserted."""
import numpy as np
import pytest
import torch

import facet_reference as FR
from test_gpu_vector import CASES

pytestmark = pytest.mark.gpu
RTOL = 1e-12


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _close(b, ref, what=""):
    b = _np(b) if isinstance(b, torch.Tensor) else b
    err, scale = np.abs(b - ref).max(), np.abs(ref).max()
    print(f"{what}: max|b - ref| = {err:.3e}, max|ref| = {scale:.3e}, ratio {err / scale:.3e}")
    assert err <= RTOL * scale


def _mesh(ct, n, dev):
    from femasm import mesh

    return mesh.create_unit_square(*n, cell_type=ct, device=dev) if len(n) == 2 else \
        mesh.create_unit_cube(*n, cell_type=ct, device=dev)


def _on_plane(m, axis, value):
    from femasm import mesh

    return mesh.locate_entities_boundary(m, m.tdim - 1,
                                         lambda x: torch.isclose(x[axis], torch.full_like(x[axis], value)))


# ------------------------------------------------------------------------------------ 6. the kernel
@pytest.mark.parametrize("ct,p,n", CASES + [(4, 3, (2, 2)), (8, 3, (1, 1, 2))])
def test_kernel_matches_reference(dev, ct, p, n):
    from femasm import fem, mesh

    m = _mesh(ct, n, dev)
    face = _on_plane(m, 0, 1.0)  # (located before the vertices move)
    g = torch.Generator().manual_seed(7)
    h = 1.0 / max(n)
    m.x += (0.1 * h * (torch.rand(m.x.shape, generator=g, dtype=torch.float64) - 0.5)).to(dev)  # interior and boundary
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    qd = None if fem.is_simplex(ct) else 2 * p + 2
    for f in (mesh.exterior_facets(m), face.to(torch.int64)):
        nf = int(f.numel())
        assert nf > 0
        tn = (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5).to(dev)
        pf = torch.rand(nf, generator=g, dtype=torch.float64).to(dev)
        perm = torch.randperm(nf, generator=g).to(dev)
        for kw, ref_kw in ((dict(traction=tn), dict(t_nodal=_np(tn))),
                           (dict(pressure=pf), dict(p_facet=_np(pf))),
                           (dict(traction=tn, pressure=pf), dict(t_nodal=_np(tn), p_facet=_np(pf)))):
            ld = fem.SurfaceLoad(V, f, quadrature_degree=qd, **kw)
            b = fem.assemble_surface_load(ld)
            ref = FR.reference_load(V, _np(f), **ref_kw)
            _close(b, ref, f"{ct} P{p} {nf} facets {sorted(kw)}")
            assert torch.equal(fem.assemble_surface_load(ld), b)  # run to run
            kwp = {k: (v[perm] if k == "pressure" else v) for k, v in kw.items()}
            assert torch.equal(fem.assemble_surface_load(fem.SurfaceLoad(V, f[perm], quadrature_degree=qd, **kwp)), b)
            host = fem._surface_load_host(ld, 1.0, torch.zeros_like(b))
            _close(host, _np(b), "torch definition")
            _close(host, ref, "torch definition against the reference")


def test_constant_values_alpha_and_default_rule(dev):
    """Constant traction and pressure, alpha and accumulation into a given b, at the default quadrature
    degree (exact on unperturbed cells)."""
    from femasm import fem, mesh

    for ct, p, n in ((3, 2, (3, 2)), (8, 1, (2, 2, 1))):
        m = _mesh(ct, n, dev)
        V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
        f = mesh.exterior_facets(m)
        t = [0.3, -0.2, 0.1][:m.gdim]
        ld = fem.SurfaceLoad(V, f, traction=t, pressure=1.5)
        ref = FR.reference_load(V, _np(f), t_const=np.array(t), p_const=1.5)
        b0 = torch.ones(V.num_dofs, dtype=torch.float64, device=dev)
        out = fem.assemble_surface_load(ld, b0, alpha=-2.0)
        assert out is b0
        _close(b0, 1.0 - 2.0 * ref, f"{ct} P{p} constant values")


# ------------------------------------------------------------------------------------ 7. assemble_vector
@pytest.mark.parametrize("law", ["linear", "neo"])
def test_assemble_vector_subtracts_loads(dev, law):
    from femasm import fem

    m = _mesh(-4, (2, 2, 2), dev)
    V = fem.functionspace(m, ("Lagrange", 2, (3,)))
    g = torch.Generator().manual_seed(3)
    u = (1e-2 * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).to(dev)
    f1, f2 = _on_plane(m, 0, 1.0), _on_plane(m, 2, 0.0)
    loads = [fem.SurfaceLoad(V, f1, traction=[2.0, 0.5, 0.0]),
             fem.SurfaceLoad(V, f2, pressure=torch.rand(int(f2.numel()), generator=g, dtype=torch.float64).to(dev))]
    Form = fem.LinearElasticity if law == "linear" else fem.NeoHookean
    kw = dict(E=3.0, nu=0.3, u=u)
    b_with = fem.assemble_vector(Form(V, loads=loads, **kw))
    b_cell = fem.assemble_vector(Form(V, **kw))
    want = b_cell.clone()
    for ld in loads:
        want -= fem.assemble_surface_load(ld)
    assert float((b_cell - b_with).abs().max()) > 0.1
    _close(b_with, _np(want), law)


# ------------------------------------------------------------------------------------ 8. equilibrium
def _rollers(V, m, dev):
    from femasm import fem

    return [fem.dirichletbc(0.0, fem.locate_dofs_geometrical(V, lambda x, k=k: torch.isclose(x[k], torch.zeros_like(x[k]))),
                            V, components=[k]) for k in range(m.gdim)]


def _free_residual(form, V, bcs):
    from femasm import fem

    b = fem.assemble_vector(form)
    marker, _ = fem._combine_bcs(V, bcs)
    return _np(b)[~_np(marker).astype(bool)]


def _neo_stretches(t, lam, mu):
    """(l1, l2) of F = diag(l1, l2, l2) with P11 = t, P22 = 0 for P = mu (F - F^-T) + lam ln J F^-T."""
    s = np.array([1.0, 1.0])
    for _ in range(50):
        def P(s):
            lnJ = np.log(s[0] * s[1] ** 2)
            return np.array([mu * (s[0] - 1 / s[0]) + lam * lnJ / s[0] - t, mu * (s[1] - 1 / s[1]) + lam * lnJ / s[1]])
        r = P(s)
        Jm = np.stack([(P(s + 1e-7 * e) - P(s - 1e-7 * e)) / 2e-7 for e in np.eye(2)], 1)
        ds = np.linalg.solve(Jm, r)
        s = s - ds
        if np.abs(ds).max() < 1e-15:
            break
    assert np.abs(P(s)).max() < 1e-14 * max(mu, lam)
    return s


@pytest.mark.parametrize("ct,p,n", [(3, 1, (3, 2)), (3, 2, (2, 2)), (-4, 1, (2, 2, 2)), (-4, 2, (2, 1, 2))])
def test_linear_equilibrium_under_traction(dev, ct, p, n):
    from femasm import fem

    m = _mesh(ct, n, dev)
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    E, nu, t = 5.0, 0.3, 0.4
    eps = [t / E, -nu * t / E, -nu * t / E] if m.gdim == 3 else [t * (1 - nu ** 2) / E, -nu * (1 + nu) * t / E]
    u = fem.Function(V)
    u.interpolate(lambda x: torch.stack([eps[k] * x[k] for k in range(m.gdim)]))
    bcs = _rollers(V, m, dev)
    ld = fem.SurfaceLoad(V, _on_plane(m, 0, 1.0), traction=[t] + [0.0] * (m.gdim - 1))
    internal = np.abs(_np(fem.assemble_vector(fem.LinearElasticity(V, E=E, nu=nu, u=u)))).max()
    res = _free_residual(fem.LinearElasticity(V, E=E, nu=nu, u=u, loads=[ld]), V, bcs)
    print(f"free residual {np.abs(res).max():.3e}, internal force {internal:.3e}")
    assert np.abs(res).max() <= 1e-11 * internal


NEO = dict(E=1.0, nu=0.3)


def _neo_problem(dev, p, n):
    from femasm import fem

    m = _mesh(-4, n, dev)
    V = fem.functionspace(m, ("Lagrange", p, (3,)))
    E, nu = NEO["E"], NEO["nu"]
    t = 0.05 * E
    mu, lam = E / (2 * (1 + nu)), E * nu / ((1 + nu) * (1 - 2 * nu))
    l1, l2 = _neo_stretches(t, lam, mu)
    exact = fem.Function(V)
    exact.interpolate(lambda x: torch.stack([(l1 - 1) * x[0], (l2 - 1) * x[1], (l2 - 1) * x[2]]))
    ld = fem.SurfaceLoad(V, _on_plane(m, 0, 1.0), traction=[t, 0.0, 0.0])
    return m, V, ld, exact


@pytest.mark.parametrize("p,n", [(1, (2, 2, 2)), (2, (2, 1, 2))])
def test_neo_hookean_equilibrium_under_traction(dev, p, n):
    from femasm import fem

    m, V, ld, exact = _neo_problem(dev, p, n)
    bcs = _rollers(V, m, dev)
    internal = np.abs(_np(fem.assemble_vector(fem.NeoHookean(V, u=exact, **NEO)))).max()
    res = _free_residual(fem.NeoHookean(V, u=exact, loads=[ld], **NEO), V, bcs)
    print(f"free residual {np.abs(res).max():.3e}, internal force {internal:.3e}")
    assert np.abs(res).max() <= 1e-11 * internal


# ------------------------------------------------------------------------------------ 9. end to end
@pytest.mark.parametrize("matrix_free", [False, True])
def test_newton_solve_under_traction(dev, matrix_free):
    from femasm import fem, nls

    m, V, ld, exact = _neo_problem(dev, 1, (2, 2, 2))
    u = fem.Function(V)
    F = fem.NeoHookean(V, u=u, loads=[ld], **NEO)
    problem = nls.NonlinearProblem(F, u, bcs=_rollers(V, m, dev), matrix_free=matrix_free)
    solver = nls.NewtonSolver(None, problem)
    its, converged = solver.solve(u)
    err = float((u.x - exact.x).abs().max()) / float(exact.x.abs().max())
    print(f"matrix_free={matrix_free}: {its} Newton iterations, max|u - exact| / max|exact| = {err:.3e}")
    assert converged and its > 0
    assert err <= 1e-6
