"""Every kernel route under Dirichlet sets other than two planes (tests/dirichlet_sets.py), against the CPU
oracle called with the builders' own marker and prescribed values (tests/test_dirichlet_sets_host.py pins
both on the CPU).

The marker goes through its own code in every route: cell_bcmask and the record's sign word, k_rec_bcbits
from the node side, k_pack_nodes of the fused P1 records, the BIGM branch of the gather (Q2 / Q3 hexahedra),
the block-owner gather's row / column bits, k_hex_mfma, the element scatter, k_lifting, k_set_bc, the two
Jacobian-action kernels, and the Dirichlet diagonal lists per row window.

Bars, the suite's own: matrices per scalar row 1e-12 with identical patterns (rowparity), constrained rows
and columns exactly zero with `diagonal` on the diagonal (test_gpu_prepared.check_bc_structure), every
matrix filled with NaN before its assembly; vectors max|b - ref| <= 1e-12 max|ref|; the operator action and
its block diagonal per row against the matrix assembled with the same set. Every test prints one line that
starts with "dirichlet-sets" and carries its worst ratio; profiles/dirichlet_sets/gpu_errors.txt keeps
those of one run.

`empty` against bcs=None of the same route: bit for bit on the deterministic route alone. Every other route
sums in floating point with atomics in a timing-dependent order (gather, lds, generic: ds_add_f64 from four
waves; owner: its segment ends; scatter: FP64 global atomics), so two runs of one of them differ in the last
bits whatever the marker; those are held to the per-row bar against each other.

Sections: A matrices of linear elasticity, B general-coefficient kernels and other laws, C the prepared
state under changing sets, D row windows, E residual / lifting / set_bc, F the Jacobian action."""
import numpy as np
import pytest
import torch

import dirichlet_sets as DS
import form_parameters as FP
from rowparity import RTOL, row_errors
from test_gpu_form_parameters import Case, _lin, _np, _tag
from test_gpu_invariance import routes_of
from test_gpu_irregular import ROUTES, _fill_nan
from test_gpu_matrix_free import DIAG, _check_block_diag, _check_mult
from test_gpu_prepared import IDS as PREPARED_IDS
from test_gpu_prepared import MESHES as PREPARED_MESHES
from test_gpu_prepared import Problem, check_bc_structure

pytestmark = pytest.mark.gpu

SEED = 0
ATOMIC_ROUTES = ["gather", "scatter", "owner", "lds", "generic"]  # floating-point atomics: see the docstring


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


class Worst:
    """The worst ratio of a test, printed once on the way out (also when an assertion ends the test)."""

    def __init__(self, what):
        self.what, self.ratio, self.at = what, 0.0, "-"

    def add(self, ratio, at):
        if ratio >= self.ratio:
            self.ratio, self.at = float(ratio), at

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        print(f"dirichlet-sets {self.what}: {self.ratio:.3e} (worst: {self.at})")
        return False


class SetCase(Case):
    """A form-parameters case with the Dirichlet sets on its space, one matrix, and the oracle's results
    per (set, parameters), each computed once and left unchanged."""

    def __init__(self, oracle, dev, ct, p, n, perturb=0.0):
        super().__init__(oracle, dev, ct, p, n, perturb)
        self._sets, self._mref, self._vref, self._none = {}, {}, {}, {}
        self.A = None

    def set(self, name):
        if name not in self._sets:
            self._sets[name] = DS.build(name, self.V, SEED)
        return self._sets[name]

    def matrix_of(self, a):
        from femasm import fem

        if self.A is None:
            self.A = fem.create_matrix(a, check=True)
            np.testing.assert_array_equal(_np(self.A.indptr), self.indptr)
            np.testing.assert_array_equal(_np(self.A.indices), self.indices)
        return self.A

    def ref(self, name, nu=0.3, law="lin", diag=1.0):
        key = (name, nu, law, diag)
        if key not in self._mref:
            O, mk = self.oracle, None if name is None else self.set(name)[1]
            if law == "lin":
                v = O.assemble_elasticity(*self.args(nu), self.indptr, self.indices, bc=mk, diag=diag)
            elif law == "neo":
                v = O.assemble_neohookean(*self.args(nu), _np(self.u_neo), self.indptr, self.indices, bc=mk, diag=diag)
            else:
                lam, mu = O.lame(self.En, nu)
                v = O.assemble_damage(self.cells, self.geom, self.x, lam, mu, _np(self.u), _np(self.d), self.indptr,
                                      self.indices, bc=mk, diag=diag)
            self._mref[key] = v
        return self._mref[key]

    def residual(self, kind):
        """The oracle's residual of a kind (0 linear, 1 damage, 2 neo-Hookean) at u, f (and d), once."""
        if kind not in self._vref:
            u, d = _np(self.u), _np(self.d) if kind == 1 else None
            self._vref[kind] = self.oracle.assemble_residual(*self.args(0.3), u=u, f=_np(self.f), d=d, kind=kind)
        return self._vref[kind]

    def setF(self, name, kind, with_x0, alpha):
        """The oracle's lifting of its residual and the set-bc overwrite, with the builder's g per dof."""
        _, marker, g = self.set(name)
        u, d = _np(self.u), _np(self.d) if kind == 1 else None
        b = self.oracle.apply_lifting(*self.args(0.3), self.residual(kind), marker, g, x0=u if with_x0 else None,
                                      alpha=alpha, u=u if kind else None, d=d, kind=kind)
        mk = marker.astype(bool)
        b[mk] = alpha * (g[mk] - (u[mk] if with_x0 else 0.0))
        return b


_cases = {}


def _case(oracle, dev, elem, perturb=0.0, table=None):
    ct, p, n = DS.mesh_of(elem, table) if isinstance(elem, str) else elem
    key = (ct, p, n, perturb)
    if key not in _cases:
        _cases[key] = SetCase(oracle, dev, ct, p, n, perturb)
    return _cases[key]


def _check(C, A, ref, marker, diag, what, w):
    """Finite, the per-row bar, and the exact structure of the constrained rows and columns."""
    got = _np(A.data)
    assert np.isfinite(got).all(), f"{what}: blocks not written or not finite"
    rel, r = row_errors(got, ref, C.indptr)
    w.add(rel, what)
    assert rel <= RTOL, f"{what}: per-row parity {rel:.3e} > {RTOL:g} (block row {r})"
    check_bc_structure(got, C.indptr, C.indices, marker, diag, ref.shape[1])
    return got


def _assemble(C, a, name, kw, diag=1.0):
    from femasm import fem

    A = C.matrix_of(a)
    _fill_nan(A)
    fem.assemble_matrix(a, bcs=None if name is None else C.set(name)[0], diagonal=diag, A=A, **kw)
    return A


def _identity(C, diag):
    bs = C.m.gdim
    rows = np.repeat(np.arange(len(C.indptr) - 1), np.diff(C.indptr))
    out = np.zeros((len(C.indices), bs, bs))
    out[rows == C.indices] = diag * np.eye(bs)
    return out


def _routes(elem, perturb):
    r = routes_of(elem)
    if perturb:  # the deterministic mode serves affine cells
        r.pop("deterministic", None)
    return r


# ------------------------------------------------------------------------------------ A. matrices, linear elasticity
@pytest.mark.parametrize("name", DS.SETS)
@pytest.mark.parametrize("elem,perturb", FP.MESHES)
def test_matrix_routes(oracle, dev, elem, perturb, name):
    """Every route of the element under the set, diagonal 1; on gather and scatter also diagonals 0 and
    2.5 for `scatter` and `all`. `all` is exactly diagonal * I on the pattern; `empty` is the same route's
    bcs=None matrix (bit for bit where the route has no floating-point atomics)."""
    C = _case(oracle, dev, elem, perturb)
    a = _lin(C, 0.3)
    marker = C.set(name)[1]
    routes = _routes(elem, perturb)
    assert set(routes) == set(ROUTES) if C.ct in (FP.TRI, FP.TET) else {"gather", "scatter"} <= set(routes)
    with Worst(f"A {_tag(elem, perturb)} {name}") as w:
        for route, kw in routes.items():
            diags = [1.0] + ([0.0, 2.5] if route in ("gather", "scatter") and name in ("scatter", "all") else [])
            for diag in diags:
                what = f"{route} diag={diag}"
                got = _check(C, _assemble(C, a, name, kw, diag), C.ref(name, diag=diag), marker, diag, what, w)
                if name == "all":
                    assert np.array_equal(got, _identity(C, diag)), f"{what}: not diagonal * I"
            if name == "empty":
                if route not in C._none:
                    C._none[route] = _np(_assemble(C, a, None, kw).data).copy()
                    _check(C, C.A, C.ref(None), None, 1.0, f"{route} no-bcs", w)
                free = C._none[route]
                if route in ATOMIC_ROUTES:
                    rel, r = row_errors(got, free, C.indptr)
                    w.add(rel, f"{route} empty vs none")
                    assert rel <= RTOL, f"{route}: empty vs bcs=None {rel:.3e} (block row {r})"
                else:
                    assert np.array_equal(got, free), f"{route}: empty differs from bcs=None"


# ------------------------------------------------------------------------------------ B. general kernels, other laws
@pytest.mark.parametrize("name", ["scatter", "last-component"])
@pytest.mark.parametrize("elem,perturb", FP.MESHES)
def test_matrix_general_coefficients(oracle, dev, elem, perturb, name):
    """nu = 0.4999 (outside the uniform-nu interval) and lam / mu per cell: the general lam/mu kernels."""
    from femasm import fem

    C = _case(oracle, dev, elem, perturb)
    marker = C.set(name)[1]
    lam, mu = oracle.lame(C.En, 0.3)
    forms = {"nu=0.4999": (_lin(C, 0.4999), 0.4999),
             "lam/mu": (fem.LinearElasticity(C.V, lam=torch.tensor(lam, device=dev), mu=torch.tensor(mu, device=dev)), 0.3)}
    with Worst(f"B general {_tag(elem, perturb)} {name}") as w:
        for tag, (a, nu) in forms.items():
            for route in ("gather", "scatter"):
                _check(C, _assemble(C, a, name, ROUTES[route]), C.ref(name, nu=nu), marker, 1.0, f"{tag} {route}", w)


LAW_SETS = ["scatter", "scatter-complement", "interior", "all"]


@pytest.mark.parametrize("name", LAW_SETS)
@pytest.mark.parametrize("elem", list(FP.NEO))
def test_matrix_neohookean(oracle, dev, elem, name):
    from femasm import fem

    C = _case(oracle, dev, elem, table=FP.NEO)
    a = fem.NeoHookean(C.V, E=C.E, nu=0.3, u=C.u_neo)
    with Worst(f"B neo {elem} {name}") as w:
        for route in ("gather", "scatter"):
            got = _check(C, _assemble(C, a, name, ROUTES[route]), C.ref(name, law="neo"), C.set(name)[1], 1.0, route, w)
            if name == "all":
                assert np.array_equal(got, _identity(C, 1.0))


@pytest.mark.parametrize("name", LAW_SETS)
@pytest.mark.parametrize("tangent", ["hand", "ad"])
def test_matrix_damage(oracle, dev, tangent, name):
    from femasm import fem

    C = _case(oracle, dev, FP.DAMAGE)
    a = fem.AsymDamage(C.V, E=C.E, nu=0.3, u=C.u, d=C.d, tangent=tangent)
    with Worst(f"B damage-{tangent} {name}") as w:
        for route in ("gather", "scatter"):
            got = _check(C, _assemble(C, a, name, ROUTES[route]), C.ref(name, law="dam"), C.set(name)[1], 1.0, route, w)
            if name == "all":
                assert np.array_equal(got, _identity(C, 1.0))


# ------------------------------------------------------------------------------------ C. prepared state, changing sets
class SetProblem:
    """test_gpu_prepared.Problem with the sets on its space and the oracle called with their own markers."""

    def __init__(self, dev, oracle, ct, n):
        self.P = P = Problem(dev, oracle, ct, n)
        self.oracle, self.V, self.a = oracle, P.V, P.a
        self.indptr, self.indices = P.indptr, P.indices
        self.m = P.m
        self.lam, self.mu = oracle.lame(_np(P.E), 0.3)

    def ref(self, marker, diag=1.0):
        P = self.P
        return self.oracle.assemble_elasticity(int(P.m.cell_type), P.degree, P.cells, _np(P.m.cells), _np(P.m.x), self.lam,
                                               self.mu, P.indptr, P.indices, bc=marker, diag=diag)

    def window(self):
        """The prepared window of the state built or found last."""
        st = list(self.V._prepared.values())[-1]
        return st, list(st.windows.values())[-1][0]


@pytest.mark.parametrize("ct,n,plan", PREPARED_MESHES, ids=PREPARED_IDS)
def test_prepared_state_follows_the_set(dev, oracle, ct, n, plan):
    """One space, one matrix; scatter, single, empty, None, all, scatter-complement, scatter again, then a
    `scatter` bc whose dofs are edited in place. k_rec_bcbits only ORs: records reused across markers would
    keep the bits of `scatter` under `single`, its subset. The space keeps three prepared states and every
    marker here is a new one (`scatter` is evicted before it returns, and the edit makes a new marker), so
    every step builds: _prepared_builds is the step's number."""
    from femasm import fem

    S = SetProblem(dev, oracle, ct, n)
    V = S.V
    sets = {k: DS.build(k, V, SEED) for k in ("scatter", "single", "empty", "all", "scatter-complement")}
    A = fem.create_matrix(S.a)
    free = None
    with Worst(f"C {ct}") as w:
        steps = ["scatter", "single", "empty", None, "all", "scatter-complement", "scatter"]
        for step, name in enumerate(steps):
            bcs, marker = (None, None) if name is None else sets[name][:2]
            _fill_nan(A)
            fem.assemble_matrix(S.a, bcs=bcs, A=A, plan=plan)
            got = _check(S, A, S.ref(marker), marker, 1.0, f"step {step} {name}", w)
            print(f"  C {ct} step {step} {name}: prepared builds {V._prepared_builds}")
            assert V._prepared_builds == step + 1
            st, pp = S.window()
            assert st.marker is (None if name is None else fem._combine_bcs(V, bcs, with_g=False)[0])
            nmark = 0 if marker is None else int(marker.sum())
            assert pp.ndiag == nmark and bool(pp.diag_off) == (nmark > 0)  # `empty`, None: no diagonal list
            if name == "empty":
                free = got.copy()
            if name is None:
                rel, r = row_errors(free, got, S.indptr)  # (ds_add_f64 order: the per-row bar, not bits)
                w.add(rel, "empty vs none")
                assert rel <= RTOL
                assert not pp.has_bc
        bcs, marker, _ = sets["scatter"]
        marker = marker.copy()
        drop, add = DS.swap_one_dof(V, bcs[0], marker)
        marker[drop], marker[add] = 0, 1
        _fill_nan(A)
        fem.assemble_matrix(S.a, bcs=bcs, A=A, plan=plan)
        _check(S, A, S.ref(marker), marker, 1.0, "dofs edited in place", w)
        print(f"  C {ct} edited: prepared builds {V._prepared_builds}")
        assert V._prepared_builds == len(steps) + 1


# ------------------------------------------------------------------------------------ D. row windows
def _fresh(oracle, dev, elem):
    return SetCase(oracle, dev, *DS.mesh_of(elem))


@pytest.mark.parametrize("name", ["scatter", "all"])
def test_row_parts(oracle, dev, name):
    """tet-P2 in three or more row parts: every window's diagonal list (a dense one under `all`), its
    capacity from the count kernel and its offsets relative to indptr[row_begin]."""
    from femasm import fem

    C = _fresh(oracle, dev, "tet-P2")
    a = _lin(C, 0.3)
    bcs, marker, _ = C.set(name)
    A = fem.create_matrix(a, max_part_bytes=(len(C.indices) // 3) * 8 * 9)
    assert len(A.parts) >= 3
    ref = C.ref(name)
    with Worst(f"D parts tet-P2 {name}") as w:
        for k in range(2):
            _fill_nan(A)
            fem.assemble_matrix(a, bcs=bcs, A=A)
            got = _check(C, A, ref, marker, 1.0, f"assembly {k}", w)
            for r0, r1, _d in A.parts:
                b0, b1 = C.indptr[r0], C.indptr[r1]
                rel, r = row_errors(got[b0:b1], ref[b0:b1], C.indptr[r0:r1 + 1] - b0)
                w.add(rel, f"part [{r0}, {r1})")
                assert rel <= RTOL, f"part [{r0}, {r1}): {rel:.3e}"
        assert C.V._prepared_builds == 1
        st = next(iter(C.V._prepared.values()))
        assert len(st.windows) == len(A.parts)
        mk = marker.reshape(-1, C.m.gdim)
        for (r0, r1, _d), (pp, off, _ip) in zip(A.parts, st.windows.values()):
            assert pp.ndiag == int(mk[r0:r1].sum())  # one list per part, one entry per constrained dof
            if pp.ndiag == 0:  # (a last part of one row, none of whose dofs `scatter` holds: no list)
                assert off is None and not pp.diag_off
                continue
            o = np.sort(_np(off))
            assert o[0] >= 0 and o[-1] < (C.indptr[r1] - C.indptr[r0]) * mk.shape[1] ** 2 and np.unique(o).size == o.size


@pytest.mark.parametrize("name", ["scatter", "all"])
def test_split_gather(oracle, dev, name):
    """SplitGather over two uneven node ranges of tet-P2, the second range first."""
    from femasm import fem

    C = _fresh(oracle, dev, "tet-P2")
    a = _lin(C, 0.3)
    bcs, marker, _ = C.set(name)
    N = C.V.num_nodes
    A = fem.create_matrix(a)
    sg = fem.SplitGather(a, bcs, A, [(0, N // 3), (N // 3, N)])
    with Worst(f"D split tet-P2 {name}") as w:
        for k in range(2):
            _fill_nan(A)
            sg.prepare()
            sg.rows(1)
            sg.rows(0)
            assert sg._prep is not None, "the split gather did not run on the prepared state"
            _check(C, A, C.ref(name), marker, 1.0, f"step {k}", w)
        st = next(iter(C.V._prepared.values()))
        mk = marker.reshape(-1, C.m.gdim)
        assert sorted(pp.ndiag for pp, _o, _i in st.windows.values()) == sorted(
            [int(mk[:N // 3].sum()), int(mk[N // 3:].sum())])


# ------------------------------------------------------------------------------------ E. residual, lifting, set_bc
VEC_SETS = ["scatter", "scatter-complement", "last-component", "overlap", "all", "empty"]


def _setF_case(C, J, kind, name, w):
    """The reference's setF sequence (test_gpu_form_parameters._setF_device) for x0 = u and None and
    alpha = -1 and +1, on clones of one assembled residual."""
    from femasm import fem

    bcs, marker, g = C.set(name)
    mk = marker.astype(bool)
    b0 = fem.assemble_vector(J)
    r0 = C.residual(kind)
    rel = float(np.abs(_np(b0) - r0).max() / np.abs(r0).max())
    w.add(rel, "residual")
    assert rel <= RTOL, f"residual: {rel:.3e}"
    u = _np(C.u)
    for with_x0 in (True, False):
        for alpha in (-1.0, 1.0):
            b = b0.clone()
            fem.apply_lifting(b, [J], [bcs], x0=[C.u] if with_x0 else None, alpha=alpha)
            fem.set_bc(b, bcs, x0=C.u if with_x0 else None, alpha=alpha)
            got, ref = _np(b), C.setF(name, kind, with_x0, alpha)
            what = f"x0={'u' if with_x0 else None} alpha={alpha:+g}"
            assert np.isfinite(got).all(), what
            rel = float(np.abs(got - ref).max() / np.abs(ref).max())
            w.add(rel, what)
            assert rel <= RTOL, f"{what}: {rel:.3e} > {RTOL:g}"
            # the constrained entries are alpha (g - x0) of the bc that comes last, exactly
            want = alpha * (g[mk] - (u[mk] if with_x0 else 0.0))
            assert np.array_equal(got[mk], want), f"{what}: constrained entries"


@pytest.mark.parametrize("name", VEC_SETS)
@pytest.mark.parametrize("elem", list(FP.VECTOR_CASES))
def test_setF(oracle, dev, elem, name):
    C = _case(oracle, dev, elem, table=FP.VECTOR_CASES)
    with Worst(f"E lin {elem} {name}") as w:
        _setF_case(C, _lin(C, 0.3, u=C.u, f=C.f), 0, name, w)


@pytest.mark.parametrize("name", VEC_SETS)
@pytest.mark.parametrize("elem", list(FP.NEO))
def test_setF_neohookean(oracle, dev, elem, name):
    from femasm import fem

    C = _case(oracle, dev, elem, table=FP.NEO)
    with Worst(f"E neo {elem} {name}") as w:
        _setF_case(C, fem.NeoHookean(C.V, E=C.E, nu=0.3, u=C.u, f=C.f), 2, name, w)


@pytest.mark.parametrize("name", VEC_SETS)
@pytest.mark.parametrize("tangent", ["hand", "ad"])
def test_setF_damage(oracle, dev, tangent, name):
    from femasm import fem

    C = _case(oracle, dev, FP.DAMAGE)
    with Worst(f"E damage-{tangent} {name}") as w:
        _setF_case(C, fem.AsymDamage(C.V, E=C.E, nu=0.3, u=C.u, d=C.d, f=C.f, tangent=tangent), 1, name, w)


# ------------------------------------------------------------------------------------ F. Jacobian action
OP_SETS = ["scatter", "scatter-complement", "last-component", "single", "all", "empty"]


@pytest.mark.parametrize("name", OP_SETS)
@pytest.mark.parametrize("elem", FP.OPERATOR)
def test_operator(oracle, dev, elem, name):
    """op.mult and op.block_diagonal, planned ("auto" on simplices) and generic, against the matrix assembled
    with the same set and diagonal (which section A holds to the oracle). `all`: mult(x) is diagonal * x."""
    from femasm import fem

    C = _case(oracle, dev, elem)
    a = _lin(C, 0.3)
    bcs, marker, _ = C.set(name)
    with Worst(f"F {elem} {name}") as w:
        for diag in (1.0, DIAG):
            S = _assemble(C, a, name, ROUTES["gather"], diag).to_scipy().tocsr()
            for method in ("auto", "generic"):
                op = fem.JacobianOperator(a, bcs=bcs, diagonal=diag, method=method)
                if method == "auto":
                    assert (op.num_chunks >= 1) == fem.JacobianOperator.has_plan(C.V)
                what = f"  F {elem} {name} {method} diag={diag}"
                x, y = _check_mult(op, S, dev, what)
                _check_block_diag(op, S, what)
                xh, yh = _np(x), _np(y)
                scale = abs(S) @ np.abs(xh)
                nz = scale > 0
                w.add(float((np.abs(yh - S @ xh)[nz] / scale[nz]).max(initial=0.0)), f"{method} diag={diag}")
                if name == "all":
                    assert np.array_equal(yh, diag * xh), f"{what}: mult(x) is not diagonal * x"
