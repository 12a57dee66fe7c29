"""CPU checks of the scalar functionals (fem.assemble_scalar on a mesh on the CPU: the torch definitions
the device kernels are held to), of fa_quadrature and of the Newton energy line search.

Bars. Quadrature: 1e-14 relative to the closed form. Values of functionals: 1e-13 * value. Linear strain
energy against 1/2 u^T K u with the oracle's K: 1e-12 * 1/2 |u|^T |K| |u|. Gradient of the host total energy
(torch.autograd) against the oracle's residual b: max_i |g_i - b_i| <= 1e-11 max_i |b_i| (each row carries
rounding of a few eps times at most a few dozen contributions of size <= max|b|; a global bar because
autograd yields no per-row magnitudes)."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SQUARE = os.path.join(ROOT, "tests", "golden", "square.msh")

TRI, QUAD, TET, HEX = 3, 4, -4, 8


@pytest.fixture(scope="module")
def L():
    from femasm import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libfemasm.so not built (run __graft_entry__.build())")
    return _lib.load()


def _mesh(ct, n):
    from femasm import mesh

    return mesh.create_unit_square(*n, cell_type=ct) if len(n) == 2 else mesh.create_unit_cube(*n, cell_type=ct)


def _rand(n, seed, amp=1.0):
    return amp * (torch.rand(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) - 0.5)


# ------------------------------------------------------------------------------------ 1. fa_quadrature
def test_version_and_symbols(L):
    import ctypes

    from femasm import _lib

    assert L.fa_version() >= 107
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("fa_quadrature", "fa_functional_work_bytes", "fa_assemble_scalar"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES


def _monomials(td, m):
    return [e for e in np.ndindex(*([m + 1] * td)) if sum(e) <= m]


@pytest.mark.parametrize("ct", [TRI, QUAD, TET, HEX])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6])
def test_quadrature_integrates_monomials(L, ct, m):
    from femasm import fem

    pts, wts = fem.quadrature(ct, m)
    td = pts.shape[1]
    simplex = ct in (TRI, TET)
    vol = 1.0 / math.factorial(td) if simplex else 1.0
    assert abs(math.fsum(wts) - vol) <= 1e-14 * vol
    worst = 0.0
    for e in _monomials(td, m):
        got = math.fsum(wts * np.prod(pts ** np.array(e), axis=1))
        if simplex:
            exact = math.prod(math.factorial(a) for a in e) / math.factorial(sum(e) + td)
        else:
            exact = 1.0 / math.prod(a + 1 for a in e)
        worst = max(worst, abs(got - exact) / exact)
        assert abs(got - exact) <= 1e-14 * exact, (e, got, exact)
    print(f"cell {ct} degree {m}: {len(wts)} points, worst relative error {worst:.2e}")


def test_quadrature_sizes_and_refusals(L):
    import ctypes

    from femasm import _lib

    nq = ctypes.c_int32(0)
    assert L.fa_quadrature(TET, 2, ctypes.byref(nq), None, None) == 0 and nq.value == 4
    pts = np.empty(12)
    nq.value = 3  # short
    assert L.fa_quadrature(TET, 2, ctypes.byref(nq), pts.ctypes.data, None) == _lib.FA_E_ARG
    assert L.fa_quadrature(TET, 2, None, None, None) == _lib.FA_E_ARG
    assert L.fa_quadrature(7, 2, ctypes.byref(nq), None, None) == _lib.FA_E_UNSUPPORTED
    nb = ctypes.c_int64(0)
    assert L.fa_functional_work_bytes(None, ctypes.byref(nb)) == _lib.FA_E_ARG
    assert L.fa_assemble_scalar(None, None, 0, None, None, -1, None, None, 0, None, None) == _lib.FA_E_ARG


# ------------------------------------------------------------------------------------ 2. host functionals
def test_measure_of_a_box(L):
    from femasm import fem, mesh

    m = mesh.create_box((2.0, 3.0, 0.5), (3, 2, 2))
    V = fem.functionspace(m, ("Lagrange", 1, (3,)))
    v = float(fem.assemble_scalar(fem.Measure(V)))
    assert abs(v - 3.0) <= 1e-13 * 3.0
    cells = fem.assemble_scalar(fem.Measure(V), cellwise=True)
    assert cells.shape == (m.num_cells,) and abs(float(cells.sum()) - 3.0) <= 1e-13 * 3.0


@pytest.mark.parametrize("p", [1, 2])
def test_norms_of_the_identity_field(L, p):
    from femasm import fem

    m = _mesh(TRI, (3, 2))
    V = fem.functionspace(m, ("Lagrange", p, (2,)))
    w = fem.Function(V)
    w.interpolate(lambda x: torch.stack([x[0], x[1]]))
    l2 = float(fem.assemble_scalar(fem.L2Norm2(w)))
    h1 = float(fem.assemble_scalar(fem.H1Semi2(w)))
    assert abs(l2 - 2.0 / 3.0) <= 1e-13 * (2.0 / 3.0)
    assert abs(h1 - 2.0) <= 1e-13 * 2.0
    xq = fem.quadrature_points(V, 2 * p)
    assert xq.shape == (m.num_cells, len(fem.quadrature(TRI, 2 * p)[1]), 2)
    zero = float(fem.assemble_scalar(fem.L2Norm2(w, g=xq.contiguous())))
    assert 0.0 <= zero <= 1e-28
    G = torch.eye(2, dtype=torch.float64).expand(m.num_cells, xq.shape[1], 2, 2).contiguous()
    assert 0.0 <= float(fem.assemble_scalar(fem.H1Semi2(w, G=G))) <= 1e-28
    # a tensor with its space, and an explicit rule
    assert abs(float(fem.assemble_scalar(fem.L2Norm2(w.x, V=V, qdeg=4))) - 2.0 / 3.0) <= 1e-13


# ------------------------------------------------------------------------------------ 3. 1/2 u^T K u
@pytest.mark.parametrize("case", ["square-P1", "tet-P2"])
def test_linear_strain_energy_is_half_uKu(L, oracle, case):
    from femasm import fem, mesh

    if case == "square-P1":
        m, p = mesh.read_gmsh(SQUARE, gdim=2), 1
    else:
        m, p = _mesh(TET, (2, 2, 2)), 2
    gd = m.gdim
    V = fem.functionspace(m, ("Lagrange", p, (gd,)))
    E = oracle.e_range()[np.arange(m.num_cells) % 200]
    lam, mu = oracle.lame(E, 0.3)
    cells = V.dofmap.numpy()
    ip, ix = oracle.sparsity(cells, V.num_nodes)
    K = oracle.bsr_to_dense(ip, ix, oracle.assemble_elasticity(int(m.cell_type), p, cells, m.cells.numpy(), m.x.numpy(),
                                                                lam, mu, ip, ix), V.num_nodes)
    u = _rand(V.num_dofs, 5, 1e-2)
    got = float(fem.assemble_scalar(fem.StrainEnergy(fem.LinearElasticity(V, E=torch.tensor(E), nu=0.3, u=u))))
    un = u.numpy()
    want, scale = 0.5 * un @ K @ un, 0.5 * np.abs(un) @ np.abs(K) @ np.abs(un)
    print(f"{case}: energy {got:.6e}, 1/2 uKu {want:.6e}, |diff| / scale {abs(got - want) / scale:.2e}")
    assert abs(got - want) <= 1e-12 * scale


# ------------------------------------------------------------------------------------ 4. grad Pi = residual
def _gradient_case(oracle, ct, p, n, law):
    """(autograd gradient of the host TotalEnergy, the oracle's residual) at the law's test state."""
    from femasm import fem

    m = _mesh(ct, n)
    gd = m.gdim
    V = fem.functionspace(m, ("Lagrange", p, (gd,)))
    E = oracle.e_range()[np.arange(m.num_cells) % 200]
    lam, mu = oracle.lame(E, 0.3)
    xn = V.tabulate_dof_coordinates()
    h = 1.0 / (max(n) * p)
    f = _rand(V.num_dofs, 2, 1e-2 * float(E.mean()))
    d = None
    if law == "lin":
        u = _rand(V.num_dofs, 1, 1e-3)
        form = fem.LinearElasticity(V, E=torch.tensor(E), nu=0.3, u=u, f=f)
    elif law == "neo":
        u = (0.05 * torch.sin(torch.pi * xn).reshape(-1) + _rand(V.num_dofs, 11, 0.05 * h)).contiguous()
        form = fem.NeoHookean(V, E=torch.tensor(E), nu=0.3, u=u, f=f)
    else:
        sgn = 1.0 if law == "dam+" else -1.0
        A = torch.tensor([[2e-2, 1e-2], [0.0, -5e-3]], dtype=torch.float64)
        u = sgn * (xn @ A.T + 5e-4 * torch.stack([torch.sin(3 * xn[:, 0] + 2 * xn[:, 1]),
                                                  torch.cos(2 * xn[:, 0] - 3 * xn[:, 1])], 1)).reshape(-1).contiguous()
        r = torch.rand(V.num_nodes, generator=torch.Generator().manual_seed(8), dtype=torch.float64)
        d = torch.where(r < 1.0 / 3.0, 0.9 * (1.0 - 3.0 * r), torch.zeros_like(r))  # (0, 0.9] on a third of the nodes
        assert 0.2 < float((d > 0).double().mean()) < 0.5 and float(d.max()) <= 0.9
        form = fem.AsymDamage(V, E=torch.tensor(E), nu=0.3, u=u, d=d, f=f)
        # both strain invariants of every cell away from the potential's branch tests (hand = AD branch)
        X = m.x[m.cells.to(torch.int64)]
        U = u.view(-1, 2)[V.dofmap.to(torch.int64)]
        J = torch.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]], 2)
        G = torch.stack([U[:, 1] - U[:, 0], U[:, 2] - U[:, 0]], 2) @ torch.linalg.inv(J)
        e12 = 0.5 * (G[:, 0, 1] + G[:, 1, 0])
        I1, I2 = G[:, 0, 0] + G[:, 1, 1], e12 * e12 - G[:, 0, 0] * G[:, 1, 1]
        assert float(I1.abs().min()) > 1e-6 and float(I2.abs().min()) > 1e-6
    Pi = fem.TotalEnergy(form)
    form.u = u.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(fem.assemble_scalar(Pi), form.u)
    kind = {"lin": 0, "neo": 2}.get(law, 1)
    b = oracle.assemble_residual(int(m.cell_type), p, V.dofmap.numpy(), m.cells.numpy(), m.x.numpy(), lam, mu,
                                 u=u.numpy(), f=f.numpy(), d=None if d is None else d.numpy(), kind=kind)
    return g.numpy(), b


GRAD_CASES = [(ct, p, n, "lin") for ct, n in ((TRI, (3, 2)), (QUAD, (3, 2)), (TET, (2, 2, 2)), (HEX, (2, 2, 1)))
              for p in (1, 2)]
GRAD_CASES += [(ct, p, n, "neo") for ct, n in ((TRI, (3, 2)), (TET, (2, 2, 2))) for p in (1, 2)]
GRAD_CASES += [(TRI, 1, (4, 3), "dam+"), (TRI, 1, (4, 3), "dam-")]


@pytest.mark.parametrize("ct,p,n,law", GRAD_CASES)
def test_gradient_of_total_energy_is_the_residual(L, oracle, ct, p, n, law):
    g, b = _gradient_case(oracle, ct, p, n, law)
    err, scale = np.abs(g - b).max(), np.abs(b).max()
    print(f"cell {ct} P{p} {law}: max|g - b| = {err:.3e}, max|b| = {scale:.3e}, ratio {err / scale:.2e}")
    assert np.isfinite(b).all() and scale > 0
    assert err <= 1e-11 * scale


def test_total_energy_includes_surface_loads(L):
    """b_ext holds every SurfaceLoad: grad Pi = grad(strain energy) - the load vector."""
    from femasm import fem, mesh

    m = _mesh(TET, (2, 2, 2))
    V = fem.functionspace(m, ("Lagrange", 1, (3,)))
    face = mesh.locate_entities_boundary(m, 2, lambda x: torch.isclose(x[0], torch.ones_like(x[0])))
    ld = fem.SurfaceLoad(V, face, traction=[0.3, 0.1, 0.0], pressure=0.7)
    u = _rand(V.num_dofs, 4, 1e-2)
    form = fem.NeoHookean(V, E=2.0, nu=0.3, u=u, loads=[ld])
    Pi = fem.TotalEnergy(form)
    bl = fem.assemble_surface_load(ld)
    assert torch.equal(Pi.b_ext, bl)
    form.u = u.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(fem.assemble_scalar(Pi), form.u)
    (gs,) = torch.autograd.grad(fem.assemble_scalar(Pi.strain), form.u)
    assert float((g - (gs - bl)).abs().max()) <= 1e-15 * float(gs.abs().max())
    with pytest.raises(ValueError):
        fem.assemble_scalar(Pi, cellwise=True)


# ------------------------------------------------------------------------------------ 5. line search on a stub
class _Scalar:
    """F(x) = atan x with the potential Pi = x atan x - 1/2 ln(1 + x^2): only F, J, matrix and energy."""

    def __init__(self, nan_above=None):
        self.A = SimpleNamespace(bs=1, v=1.0)
        self.A.block_diagonal = lambda: torch.full((1, 1, 1), self.A.v, dtype=torch.float64)
        self.A.mult = lambda x, y: y.copy_(self.A.v * x)
        self.iterates = []
        self.nan_above = nan_above

    def F(self, x, b):
        self.iterates.append(float(x[0]))
        b.copy_(torch.atan(x))

    def J(self, x, A):
        A.v = 1.0 / (1.0 + float(x[0]) ** 2)

    def matrix(self):
        return self.A

    def energy(self, x):
        v = float(x[0])
        if self.nan_above is not None and abs(v) > self.nan_above:
            return math.nan
        return v * math.atan(v) - 0.5 * math.log1p(v * v)


def _solve_stub(line_search, max_it, nan_above=None):
    from femasm import nls

    P = _Scalar(nan_above)
    u = SimpleNamespace(x=torch.tensor([3.0], dtype=torch.float64))
    s = nls.NewtonSolver(None, P)
    s.line_search, s.max_it, s.rtol, s.error_on_nonconvergence = line_search, max_it, 0.0, False
    it, conv = s.solve(u)
    return P, s, u, it, conv


def test_plain_newton_diverges_on_atan():
    P, s, _, it, conv = _solve_stub(None, 4)
    assert not conv and it == 4 and s.steps == [] and s.energies == []
    xs = np.abs(P.iterates)
    assert len(xs) == 5 and (xs[1:] > xs[:-1]).all()  # |x| grows at every step


def test_energy_line_search_converges_on_atan():
    P, s, u, it, conv = _solve_stub("energy", 50)
    print(f"{it} iterations, steps {s.steps}, energies {s.energies}")
    assert conv and abs(float(u.x[0])) < 1e-8
    assert len(s.steps) == it and len(s.energies) == it + 1
    assert all(b <= a for a, b in zip(s.energies, s.energies[1:]))
    assert min(s.steps) < 1.0


def test_line_search_rejects_a_nan_energy():
    """From x0 = 3 the full step lands at -9.5: a potential that is NaN beyond |x| = 5 must reject it (and
    any other such trial point), not accept it because a comparison with NaN is false."""
    P, s, u, it, conv = _solve_stub("energy", 50, nan_above=5.0)
    assert conv and abs(float(u.x[0])) < 1e-8
    assert s.steps[0] < 1.0 and all(math.isfinite(e) for e in s.energies)
    assert max(abs(x) for x in P.iterates) <= 5.0


def test_line_search_gives_up_and_names_the_option():
    from femasm import nls

    P = _Scalar()
    u = SimpleNamespace(x=torch.tensor([3.0], dtype=torch.float64))
    s = nls.NewtonSolver(None, P)
    s.line_search = "energy"
    P.energy = lambda x, P=P: 1.0 if float(x[0]) == 3.0 else math.nan
    with pytest.raises(RuntimeError, match="line search"):
        s.solve(u)
    assert float(u.x[0]) == 3.0  # the state is restored
    s.line_search = "wolfe"
    with pytest.raises(ValueError):
        s.solve(u)
