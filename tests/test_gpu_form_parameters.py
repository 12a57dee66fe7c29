"""Every kernel route at Poisson ratios other than 0.3 and at quadrature rules other than the default
(tests/form_parameters.py), against the CPU oracle called with the same nu and qdeg.

nu chooses the kernel (csrc/femasm.hip lin_uniform_nu(): the uniform-nu kernels for -0.99 < nu < 0.49,
the general lam/mu kernels outside) and enters the arithmetic (rlm = 2 nu / (1 - 2 nu), trc = 1 / (1 + rlm),
the fixed-point bound of deterministic=True). The rule chooses it too: dispatch_gather() and
launch_hex_mfma() match the default point counts, any other rule runs the generic scatter.

Bars, the suite's own: matrices per scalar row 1e-12 with identical patterns (rowparity); vectors
max|b - ref| <= 1e-12 max|ref| (test_gpu_vector); the operator action and its block diagonal per row
against the assembled matrix (test_gpu_matrix_free._check_mult / _check_block_diag); functionals per cell
1e-12 of the cell's magnitude (test_gpu_scalar). Every test prints its worst ratio on a line that starts
with "form-parameters"; profiles/form_parameters/gpu_errors.txt keeps those of one run.

Sections: A matrices over nu, B deterministic=True over nu, C nu changing under the cached prepared
state, D residual / lifting / set_bc over nu (with Q3, which no residual test ran before), E Jacobian action
over nu, F the quadrature sweep."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import form_parameters as FP
from rowparity import RTOL, row_errors
from test_gpu_matrix_free import DIAG, _check_block_diag, _check_mult

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _say(what, ratio):
    print(f"form-parameters {what}: {ratio:.3e}")


def _mesh(ct, n, dev, perturb=0.0):
    from femasm import mesh

    m = mesh.create_unit_square(*n, cell_type=ct, device=dev) if len(n) == 2 else \
        mesh.create_unit_cube(*n, cell_type=ct, device=dev)
    if perturb:  # as test_gpu_parity._mesh
        g = torch.Generator().manual_seed(3)
        x = m.x.cpu()
        interior = ((x > 1e-9) & (x < 1 - 1e-9)).all(1)
        x[interior] += perturb / max(n) * (torch.rand(x[interior].shape, generator=g, dtype=torch.float64) - 0.5)
        m.x = x.to(dev)
    return m


class Case:
    """One mesh and space with the reference bcs (x = 0 clamped, x = 1 prescribed), E per cell from the
    reference's table, random u and f as in test_gpu_vector, and the oracle's view of all of it."""

    def __init__(self, oracle, dev, ct, p, n, perturb=0.0):
        from femasm import fem

        self.oracle, self.ct, self.p, self.n = oracle, ct, p, n
        m = self.m = _mesh(ct, n, dev, perturb)
        V = self.V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
        self.E = torch.tensor(oracle.e_range()[np.arange(m.num_cells) % 200], dtype=torch.float64, device=dev)
        left = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.zeros_like(x[0])))
        right = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.ones_like(x[0])))
        self.bcs = [fem.dirichletbc(0.0, left, V), fem.dirichletbc([0.01] + [0.0] * (m.gdim - 1), right, V)]
        marker, gv = fem._combine_bcs(V, self.bcs)
        self.marker, self.gv = _np(marker), _np(gv)
        self.cells, self.geom, self.x, self.En = _np(V.dofmap), _np(m.cells), _np(m.x), _np(self.E)
        self.indptr, self.indices = oracle.sparsity(self.cells, V.num_nodes)
        g = torch.Generator().manual_seed(1)
        self.u = (1e-3 * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).to(dev)
        self.f = (1e4 * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).to(dev)
        d = torch.rand(V.num_nodes, generator=g, dtype=torch.float64)
        d[d < 0.4] = 0.0  # damaged and undamaged cells
        self.d = d.to(dev)
        xn = V.tabulate_dof_coordinates()
        self.u_neo = (0.05 * torch.sin(torch.pi * xn)).reshape(-1).contiguous()  # test_gpu_neohookean's state
        self._ref = {}

    def args(self, nu):
        lam, mu = self.oracle.lame(self.En, nu)
        return (self.ct, self.p, self.cells, self.geom, self.x, lam, mu)

    def matrix(self, nu, qdeg=-1, bc=True, law="lin", diag=1.0):
        """Oracle BSR values, computed once per parameter set."""
        key = (nu, qdeg, bc, law, diag)
        if key not in self._ref:
            O, mk = self.oracle, self.marker if bc else None
            if law == "lin":
                v = O.assemble_elasticity(*self.args(nu), self.indptr, self.indices, bc=mk, diag=diag, qdeg=qdeg)
            elif law == "neo":
                v = O.assemble_neohookean(*self.args(nu), _np(self.u_neo), self.indptr, self.indices, bc=mk, diag=diag,
                                          qdeg=qdeg)
            else:
                lam, mu = O.lame(self.En, nu)
                v = O.assemble_damage(self.cells, self.geom, self.x, lam, mu, _np(self.u), _np(self.d), self.indptr,
                                      self.indices, bc=mk, diag=diag)
            self._ref[key] = v
        return self._ref[key]

    def scipy(self, nu, qdeg=-1, law="lin"):
        v = self.matrix(nu, qdeg, True, law, DIAG)
        return sp.bsr_matrix((v, self.indices, self.indptr)).tocsr()

    def setF(self, nu, qdeg=-1, kind=0, u=None, d=None):
        """The oracle's residual, and the reference's setF sequence on it (test_lifting_and_set_bc)."""
        O, a = self.oracle, self.args(nu)
        u = _np(self.u if u is None else u)
        b0 = O.assemble_residual(*a, u=u, f=_np(self.f), d=_np(d), kind=kind, qdeg=qdeg)
        b = O.apply_lifting(*a, b0, self.marker, self.gv, x0=u, alpha=-1.0, u=u if kind else None, d=_np(d), kind=kind,
                            qdeg=qdeg)
        mk = self.marker.astype(bool)
        b[mk] = -1.0 * (self.gv[mk] - u[mk])
        return b0, b


_cases = {}


def _case(oracle, dev, elem, perturb=0.0, table=None):
    table = FP.ELEMENTS if table is None else table
    ct, p, n = table[elem] if isinstance(elem, str) else elem
    key = (ct, p, n, perturb)
    if key not in _cases:
        _cases[key] = Case(oracle, dev, ct, p, n, perturb)
    return _cases[key]


def _rows(C, A, ref, what):
    """Identical pattern and the per-row bar; prints and returns the worst row's ratio."""
    np.testing.assert_array_equal(_np(A.indptr), C.indptr)
    np.testing.assert_array_equal(_np(A.indices), C.indices)
    got = _np(A.data)
    assert np.isfinite(got).all(), what
    rel, r = row_errors(got, ref, C.indptr)
    _say(what, rel)
    assert rel <= RTOL, f"{what}: per-row parity {rel:.3e} > {RTOL:g} (block row {r})"
    return rel


def _vec(b, ref, what):
    got = _np(b)
    assert np.isfinite(got).all(), what
    rel = float(np.abs(got - ref).max() / np.abs(ref).max())
    _say(what, rel)
    assert rel <= RTOL, f"{what}: {rel:.3e} > {RTOL:g}"


def _lin(C, nu, qdeg=None, **kw):
    from femasm import fem

    return fem.LinearElasticity(C.V, E=C.E, nu=nu, quadrature_degree=qdeg, **kw)


def _tag(elem, perturb):
    return f"{elem}{' non-affine' if perturb else ''}"


def _setF_device(J, C, u):
    """b = F(u); apply_lifting(b, [J], [bcs], [u], -1); set_bc(b, bcs, u, -1): (b before, b after)."""
    from femasm import fem

    b = fem.assemble_vector(J)
    b0 = b.clone()
    fem.apply_lifting(b, [J], [C.bcs], x0=[u], alpha=-1.0)
    fem.set_bc(b, C.bcs, x0=u, alpha=-1.0)
    return b0, b


# ------------------------------------------------------------------------------------ A. matrices over nu
@pytest.mark.parametrize("nu", FP.NU)
@pytest.mark.parametrize("elem,perturb", FP.MESHES)
def test_matrix_gather(oracle, dev, elem, perturb, nu):
    from femasm import fem

    C = _case(oracle, dev, elem, perturb)
    A = fem.assemble_matrix(_lin(C, nu), bcs=C.bcs, method="gather")
    _rows(C, A, C.matrix(nu), f"A gather bcs {_tag(elem, perturb)} nu={nu}")


@pytest.mark.parametrize("nu", FP.NU_SHORT)
@pytest.mark.parametrize("elem,perturb", FP.MESHES)
def test_matrix_scatter_and_no_bcs(oracle, dev, elem, perturb, nu):
    from femasm import fem

    C = _case(oracle, dev, elem, perturb)
    a = _lin(C, nu)
    A = fem.assemble_matrix(a, bcs=C.bcs, method="scatter")
    _rows(C, A, C.matrix(nu), f"A scatter bcs {_tag(elem, perturb)} nu={nu}")
    for method in ("gather", "scatter"):
        A = fem.assemble_matrix(a, method=method)
        _rows(C, A, C.matrix(nu, bc=False), f"A {method} no-bcs {_tag(elem, perturb)} nu={nu}")


@pytest.mark.parametrize("nu", [0.4999, -0.5])
@pytest.mark.parametrize("elem,perturb", FP.MESHES)
def test_matrix_from_lame_arrays(oracle, dev, elem, perturb, nu):
    """The same forms given as lam / mu per cell (nu -0.5: negative lam): the general kernels."""
    from femasm import fem

    C = _case(oracle, dev, elem, perturb)
    lam, mu = oracle.lame(C.En, nu)
    a = fem.LinearElasticity(C.V, lam=torch.tensor(lam, device=dev), mu=torch.tensor(mu, device=dev))
    for method in ("gather", "scatter"):
        A = fem.assemble_matrix(a, bcs=C.bcs, method=method)
        _rows(C, A, C.matrix(nu), f"A {method} lam/mu {_tag(elem, perturb)} nu={nu}")


@pytest.mark.parametrize("nu", FP.NU_SHORT)
@pytest.mark.parametrize("elem", list(FP.NEO))
def test_neohookean_matrix(oracle, dev, elem, nu):
    from femasm import fem

    C = _case(oracle, dev, elem, table=FP.NEO)
    a = fem.NeoHookean(C.V, E=C.E, nu=nu, u=C.u_neo)
    for method in ("gather", "scatter"):
        A = fem.assemble_matrix(a, bcs=C.bcs, method=method)
        _rows(C, A, C.matrix(nu, law="neo"), f"A {method} neo {elem} nu={nu}")


@pytest.mark.parametrize("nu", FP.NU_SHORT)
@pytest.mark.parametrize("tangent", ["hand", "ad"])
def test_damage_matrix(oracle, dev, tangent, nu):
    """Both device tangents against the oracle's hand tangent (the same derivative: test_gpu_damage_ad)."""
    from femasm import fem

    C = _case(oracle, dev, FP.DAMAGE)
    a = fem.AsymDamage(C.V, E=C.E, nu=nu, u=C.u, d=C.d, tangent=tangent)
    for method in ("gather", "scatter"):
        A = fem.assemble_matrix(a, bcs=C.bcs, method=method)
        _rows(C, A, C.matrix(nu, law="dam"), f"A {method} damage-{tangent} nu={nu}")


# ------------------------------------------------------------------------------------ B. deterministic=True over nu
@pytest.mark.parametrize("nu", FP.NU)
@pytest.mark.parametrize("elem", FP.DETERMINISTIC)
def test_deterministic(oracle, dev, elem, nu):
    """Inside the uniform-nu interval two assemblies are bit-identical and meet the per-row bar (the
    fixed-point bound lin_fix_bound grows with |rlm| and |trc|). At and beyond the thresholds the general
    kernel runs, which has no fixed-point mode: the call raises, it never returns other values."""
    from femasm import _lib, fem

    C = _case(oracle, dev, elem)
    a = _lin(C, nu)
    if not FP.uniform_nu(nu):
        with pytest.raises(_lib.FemasmError, match="deterministic"):
            fem.assemble_matrix(a, bcs=C.bcs, deterministic=True)
        return
    A = fem.assemble_matrix(a, bcs=C.bcs, deterministic=True)
    first = A.data.clone()
    A.data.fill_(float("nan"))
    fem.assemble_matrix(a, bcs=C.bcs, A=A, deterministic=True)
    assert torch.equal(A.data, first)
    _rows(C, A, C.matrix(nu), f"B deterministic {elem} nu={nu}")


# ------------------------------------------------------------------------------------ C. nu under cached state
def _fresh(oracle, dev, elem):
    ct, p, n = FP.ELEMENTS[elem]
    return Case(oracle, dev, ct, p, n)  # (its own V: the prepared-state counters start at zero)


@pytest.mark.parametrize("elem", ["tet-P2", "tri-P1"])
def test_nu_changes_between_assemblies(oracle, dev, elem):
    """One V and one A; forms of nu 0.3, 0.45, 0.4999, 0.3 sharing E, then one form whose nu is reassigned.
    The prepared records (s Ji, sign, bc bits) do not depend on nu, so P2 tetrahedra build them once."""
    from femasm import fem

    C = _fresh(oracle, dev, elem)
    V = C.V
    A = fem.create_matrix(_lin(C, 0.3))
    for step, nu in enumerate([0.3, 0.45, 0.4999, 0.3]):
        A.data.fill_(float("nan"))
        fem.assemble_matrix(_lin(C, nu), bcs=C.bcs, A=A)
        _rows(C, A, C.matrix(nu), f"C forms {elem} step {step} nu={nu}")
        print(f"form-parameters C forms {elem} step {step}: prepared builds {V._prepared_builds}")
    a = _lin(C, 0.3)
    for step, nu in enumerate([0.3, -0.5, 0.4899]):
        a.nu = nu
        A.data.fill_(float("nan"))
        fem.assemble_matrix(a, bcs=C.bcs, A=A)
        _rows(C, A, C.matrix(nu), f"C reassigned {elem} step {step} nu={nu}")
        print(f"form-parameters C reassigned {elem} step {step}: prepared builds {V._prepared_builds}")
    assert V._prepared_builds == (1 if elem == "tet-P2" else 0)


def test_prepared_state_survives_a_form_it_refuses(oracle, dev):
    """A first assembly at nu = 0.4999 (the general kernel: no prepared state) must not keep the space
    from preparing for the next form inside the interval."""
    from femasm import fem

    C = _fresh(oracle, dev, "tet-P2")
    for nu, builds in [(0.4999, 0), (0.3, 1), (0.4999, 1), (0.45, 1)]:
        A = fem.assemble_matrix(_lin(C, nu), bcs=C.bcs)
        _rows(C, A, C.matrix(nu), f"C refused-first tet-P2 nu={nu}")
        print(f"form-parameters C refused-first nu={nu}: prepared builds {C.V._prepared_builds}")
        assert C.V._prepared_builds == builds


@pytest.mark.parametrize("method", ["auto", "generic"])
@pytest.mark.parametrize("elem", ["tet-P2", "tri-P1"])
def test_nu_changes_under_an_operator(oracle, dev, elem, method):
    from femasm import fem

    C = _fresh(oracle, dev, elem)
    for step, nu in enumerate([0.3, 0.45, 0.4999, 0.3]):
        op = fem.JacobianOperator(_lin(C, nu), bcs=C.bcs, diagonal=DIAG, method=method)
        _check_mult(op, C.scipy(nu), dev, f"form-parameters C operator forms {method} {elem} step {step} nu={nu}")
    a = _lin(C, 0.3)
    op = fem.JacobianOperator(a, bcs=C.bcs, diagonal=DIAG, method=method)
    for step, nu in enumerate([0.3, -0.5, 0.4899]):
        a.nu = nu
        _check_mult(op, C.scipy(nu), dev, f"form-parameters C operator reassigned {method} {elem} step {step} nu={nu}")
        _check_block_diag(op, C.scipy(nu), f"form-parameters C operator reassigned {method} {elem} step {step} nu={nu}")


# ------------------------------------------------------------------------------------ D. residual, lifting, set_bc
@pytest.mark.parametrize("elem,nu", [(e, nu) for e in FP.VECTOR_CASES for nu in FP.NU_SHORT] + [(e, 0.3) for e in FP.Q3])
def test_residual_and_setF(oracle, dev, elem, nu):
    C = _case(oracle, dev, elem, table=FP.VECTOR_CASES)
    b0, b = _setF_device(_lin(C, nu, u=C.u, f=C.f), C, C.u)
    r0, r = C.setF(nu)
    _vec(b0, r0, f"D residual {elem} nu={nu}")
    _vec(b, r, f"D setF {elem} nu={nu}")


@pytest.mark.parametrize("nu", FP.NU_SHORT)
@pytest.mark.parametrize("elem", list(FP.NEO))
def test_residual_and_setF_neohookean(oracle, dev, elem, nu):
    from femasm import fem

    C = _case(oracle, dev, elem, table=FP.NEO)
    b0, b = _setF_device(fem.NeoHookean(C.V, E=C.E, nu=nu, u=C.u, f=C.f), C, C.u)
    r0, r = C.setF(nu, kind=2)
    _vec(b0, r0, f"D residual neo {elem} nu={nu}")
    _vec(b, r, f"D setF neo {elem} nu={nu}")


@pytest.mark.parametrize("nu", FP.NU_SHORT)
@pytest.mark.parametrize("tangent", ["hand", "ad"])
def test_residual_and_setF_damage(oracle, dev, tangent, nu):
    from femasm import fem

    C = _case(oracle, dev, FP.DAMAGE)
    b0, b = _setF_device(fem.AsymDamage(C.V, E=C.E, nu=nu, u=C.u, d=C.d, f=C.f, tangent=tangent), C, C.u)
    r0, r = C.setF(nu, kind=1, d=C.d)
    _vec(b0, r0, f"D residual damage-{tangent} nu={nu}")
    _vec(b, r, f"D setF damage-{tangent} nu={nu}")


# ------------------------------------------------------------------------------------ E. Jacobian action over nu
@pytest.mark.parametrize("nu", FP.NU_SHORT)
@pytest.mark.parametrize("law", ["lin", "neo"])
@pytest.mark.parametrize("elem", FP.OPERATOR)
def test_operator(oracle, dev, elem, law, nu):
    """op.mult and op.block_diagonal against the assembled matrix of the same form (which section A holds
    to the oracle), planned kernels on simplices and the generic kernel on quad Q2 / hex Q1."""
    from femasm import fem

    C = _case(oracle, dev, elem)
    a = _lin(C, nu) if law == "lin" else fem.NeoHookean(C.V, E=C.E, nu=nu, u=C.u_neo)
    S = fem.assemble_matrix(a, bcs=C.bcs, diagonal=DIAG).to_scipy().tocsr()
    op = fem.JacobianOperator(a, bcs=C.bcs, diagonal=DIAG)
    assert (op.num_chunks >= 1) == fem.JacobianOperator.has_plan(C.V)
    what = f"form-parameters E {elem} {law} nu={nu}"
    _check_mult(op, S, dev, what)
    _check_block_diag(op, S, what)


# ------------------------------------------------------------------------------------ F. quadrature sweep
QDEG_NON_AFFINE = [(e, q) for e in FP.NON_AFFINE for q in FP.QDEG[e]]


@pytest.mark.parametrize("method", ["gather", "scatter"])
@pytest.mark.parametrize("elem,qdeg,perturb", [(e, q, 0.0) for e, q in FP.QDEG_CASES] +
                         [(e, q, FP.PERTURB) for e, q in QDEG_NON_AFFINE])
def test_rule_matrix(oracle, dev, elem, qdeg, perturb, method):
    from femasm import fem

    C = _case(oracle, dev, elem, perturb)
    A = fem.assemble_matrix(_lin(C, 0.3, qdeg), bcs=C.bcs, method=method)
    _rows(C, A, C.matrix(0.3, qdeg), f"F A {method} {_tag(elem, perturb)} qdeg={qdeg}")


@pytest.mark.parametrize("elem,qdeg", FP.QDEG_CASES)
def test_rule_tabulate(oracle, dev, elem, qdeg):
    from femasm import fem

    C = _case(oracle, dev, elem)
    Ae = _np(fem.tabulate_cells(_lin(C, 0.3, qdeg)))
    ref = oracle.cell_matrices_elasticity(*C.args(0.3), qdeg=qdeg)
    rel = float(np.abs(Ae - ref).max() / np.abs(ref).max())  # test_tabulate_matches_oracle's bar
    _say(f"F tabulate {elem} qdeg={qdeg}", rel)
    assert rel <= RTOL


@pytest.mark.parametrize("elem,qdeg", FP.QDEG_CASES)
def test_rule_residual_and_setF(oracle, dev, elem, qdeg):
    """Only the sigma term follows the form's rule; the load term stays on degree 2 p."""
    C = _case(oracle, dev, elem, table=FP.VECTOR_CASES)
    b0, b = _setF_device(_lin(C, 0.3, qdeg, u=C.u, f=C.f), C, C.u)
    r0, r = C.setF(0.3, qdeg)
    _vec(b0, r0, f"F residual {elem} qdeg={qdeg}")
    _vec(b, r, f"F setF {elem} qdeg={qdeg}")


@pytest.mark.parametrize("elem,qdeg", FP.QDEG_CASES)
def test_rule_operator(oracle, dev, elem, qdeg):
    from femasm import fem

    C = _case(oracle, dev, elem)
    a = _lin(C, 0.3, qdeg)
    S = C.scipy(0.3, qdeg)
    for method in ("auto", "generic"):
        op = fem.JacobianOperator(a, bcs=C.bcs, diagonal=DIAG, method=method)
        what = f"form-parameters F operator {method} {elem} qdeg={qdeg}"
        _check_mult(op, S, dev, what)
        _check_block_diag(op, S, what)


@pytest.mark.parametrize("elem,qdeg", FP.NEO_QDEG)
def test_rule_neohookean(oracle, dev, elem, qdeg):
    from femasm import fem

    C = _case(oracle, dev, elem, table=FP.NEO)
    a = fem.NeoHookean(C.V, E=C.E, nu=0.3, u=C.u_neo, quadrature_degree=qdeg)
    for method in ("gather", "scatter"):
        A = fem.assemble_matrix(a, bcs=C.bcs, method=method)
        _rows(C, A, C.matrix(0.3, qdeg, law="neo"), f"F A {method} neo {elem} qdeg={qdeg}")
    b0, b = _setF_device(fem.NeoHookean(C.V, E=C.E, nu=0.3, u=C.u, f=C.f, quadrature_degree=qdeg), C, C.u)
    r0, r = C.setF(0.3, qdeg, kind=2)
    _vec(b0, r0, f"F residual neo {elem} qdeg={qdeg}")
    _vec(b, r, f"F setF neo {elem} qdeg={qdeg}")


@pytest.mark.parametrize("elem,qdeg", FP.QDEG_CASES)
def test_rule_strain_energy(oracle, dev, elem, qdeg):
    """assemble_scalar(StrainEnergy(form)) per cell and in total against the same call on a CPU copy of the
    mesh (the torch definition), at test_gpu_scalar's bars: per cell 1e-12 of the cell's magnitude; the total
    within 1e-12 of the summed magnitudes, and of the device's own cell values summed exactly."""
    from femasm import fem

    C = _case(oracle, dev, elem)
    Vh = fem.FunctionSpace.from_dofmap(C.m.to("cpu"), C.p, C.m.gdim, C.V.dofmap.cpu(), C.V.num_nodes)
    M = fem.StrainEnergy(_lin(C, 0.3, qdeg, u=C.u))
    Mh = fem.StrainEnergy(fem.LinearElasticity(Vh, E=C.E.cpu(), nu=0.3, quadrature_degree=qdeg, u=C.u.cpu()))
    got = _np(fem.assemble_scalar(M, cellwise=True))
    want, mag = (_np(t) for t in fem.assemble_scalar_host(Mh))
    np.testing.assert_array_equal(_np(fem.assemble_scalar(Mh, cellwise=True)), want)
    assert np.isfinite(got).all() and (mag > 0).all()
    rel = float((np.abs(got - want) / mag).max())
    _say(f"F energy cellwise {elem} qdeg={qdeg}", rel)
    assert rel <= RTOL
    total, total_h = float(fem.assemble_scalar(M)), float(fem.assemble_scalar(Mh))
    rel = abs(total - total_h) / math.fsum(mag)
    _say(f"F energy total {elem} qdeg={qdeg}", rel)
    assert rel <= RTOL
    assert abs(total - math.fsum(got)) <= RTOL * math.fsum(np.abs(got))


@pytest.mark.parametrize("elem,qdeg", [("tri-P1", 2), ("tet-P2", 4), ("quad-Q1", 4), ("hex-Q1", 4)])
def test_rule_refuses_deterministic(oracle, dev, elem, qdeg):
    """Another rule falls back to the element scatter (FP64 atomics): deterministic=True must say so."""
    from femasm import _lib, fem

    C = _case(oracle, dev, elem)
    with pytest.raises(_lib.FemasmError, match="deterministic"):
        fem.assemble_matrix(_lin(C, 0.3, qdeg), bcs=C.bcs, deterministic=True)


@pytest.mark.parametrize("elem", ["tet-P2", "quad-Q1"])
def test_rules_alternate_on_one_space(oracle, dev, elem):
    """A default-rule form and a qdeg = 4 form in turn, twice, on one V: the prepared-state key holds the
    rule, so each assembly matches its own oracle."""
    from femasm import fem

    C = _fresh(oracle, dev, elem)
    A = fem.create_matrix(_lin(C, 0.3))
    for step, qdeg in enumerate([None, 4, None, 4]):
        A.data.fill_(float("nan"))
        fem.assemble_matrix(_lin(C, 0.3, qdeg), bcs=C.bcs, A=A)
        _rows(C, A, C.matrix(0.3, -1 if qdeg is None else qdeg), f"F alternate {elem} step {step} qdeg={qdeg}")
        print(f"form-parameters F alternate {elem} step {step}: prepared builds {C.V._prepared_builds}")


def test_rule_and_nu_combined(oracle, dev):
    from femasm import fem

    C = _case(oracle, dev, "tet-P2")
    a = _lin(C, 0.4999, 4, u=C.u, f=C.f)
    for method in ("gather", "scatter"):
        A = fem.assemble_matrix(a, bcs=C.bcs, method=method)
        _rows(C, A, C.matrix(0.4999, 4), f"F A {method} tet-P2 nu=0.4999 qdeg=4")
    b0, b = _setF_device(a, C, C.u)
    r0, r = C.setF(0.4999, 4)
    _vec(b0, r0, "F residual tet-P2 nu=0.4999 qdeg=4")
    _vec(b, r, "F setF tet-P2 nu=0.4999 qdeg=4")
    op = fem.JacobianOperator(a, bcs=C.bcs, diagonal=DIAG)
    _check_mult(op, C.scipy(0.4999, 4), dev, "form-parameters F operator tet-P2 nu=0.4999 qdeg=4")
