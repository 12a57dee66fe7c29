"""GPU: every kernel route on rotated, mirrored, scaled, sheared, stretched and shifted meshes
(tests/transformed_meshes.py; the host model of the inputs and of the bars is tests/test_invariance_host.py).

The rest of the suite assembles on the unit square or cube: the affine tensor route (MAT_AFFT) sees a
diagonal J there, no tensor cell has det J < 0, every length is order one and every coordinate in [0, 1].
Here the vertices go through x' = s x G^T + T before the space is built, and two kinds of check run:

  parity      against the CPU oracle on the transformed mesh, at the suite's bars (rowparity.RTOL = 1e-12
              per scalar row; vectors 1e-12 of max |ref|), Dirichlet rows / columns exactly;
  covariance  no oracle: under x' = s Q x, u' = s Q u (Q orthogonal) blocks map as s^(d-2) Q K Q^T, forces as
              s^(d-1) Q r, gradient / strain / stress as Q (.) Q^T, energy density not at all. The GPU result on
              the transformed mesh is compared with the map of the GPU result on the untransformed mesh on the
              same route. Each side may sit 1e-12 from the truth, hence 2e-12, plus the oracle's own
              covariance error for the case (the floor of the comparison, computed here, some 1e-15; for the
              damage law 1e-13: cancellation in its spectral decomposition, which the kernel orders
              differently, hence 4x that floor for its residual).

Dirichlet set: all components on the face x0 = 0 of the UNtransformed mesh, by node index; the diagonal is
s^(d-2) (a power of two), so that constrained blocks are covariant too. E = e_range()[cell % 200], nu = 0.3.

Shifted meshes (T = 1e3, 1e4 on every axis) are held to 1e-12 + 4 c(T): c(T) is the oracle's own error under
the translation (oracle against oracle, never the GPU's figure), 4 = twice the worst ratio of the affine-route
model to c(T) on the host (three-edge J against the oracle's eight-term sum). Near-threshold meshes (one
vertex moved by delta h) are held to the plain bar whichever route the plan takes.

Observed on an MI355X (profiles/invariance/errors.txt): FP64 routes at or below 7.5e-14 on parity and
2.4e-15 .. 2.1e-13 on covariance; the deterministic route up to 1.8e-13 (tet-P1 stretch); damage residual
2.2e-13; shifted meshes at most a quarter of their bar; near-threshold cases 1.7e-13 where the plan stays
affine. With k_check_affine's tolerance at 1e-12 hex-Q3 at dev / h = 8.7e-13 was assembled 2.6e-12 off
(profiles/invariance/near_threshold_tol_1e-12.txt), which is why the tolerance is 1e-13.

Every case prints one line `INV <case> | <route> | affine=<plan flag> | <error> / <bar>`
(profiles/invariance/errors.txt).
"""
import numpy as np
import pytest
import torch

import facet_reference as FR
import test_invariance_host as H
import transformed_meshes as tm
from rowparity import RTOL, row_errors
from test_gpu_expression import _points, _reduce
from test_gpu_irregular import ROUTES, _fill_nan
from test_gpu_matrix_free import _check_mult
from test_gpu_prepared import check_bc_structure

pytestmark = pytest.mark.gpu

TENSOR_DET = ["quad-Q1", "quad-Q2", "hex-Q1"]  # affine tensor families with a deterministic mode
G_BC = [0.01, 0.002, -0.003]                   # prescribed on the Dirichlet set (lifting, set_bc)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t):
    return t.detach().cpu().numpy()


def _say(case, route, flag, err, bar):
    print(f"INV {case} | {route} | affine={flag} | {err:.3e} / {bar:.3e}")


def routes_of(family):
    if family in tm.SIMPLEX:
        return dict(ROUTES)
    r = {"gather": dict(), "scatter": dict(method="scatter")}
    if family in TENSOR_DET:
        r["deterministic"] = dict(deterministic=True)
    return r


def _t(a, dev):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)


class Setup:
    """A family on one transformed copy on the GPU: mesh, space, E and the Dirichlet set of the host
    problem P (same cells, same dofmap, same node indices)."""

    def __init__(self, oracle, dev, family, tr, mesh=None):
        from femasm import fem

        self.P = P = H.problem(oracle, family)
        self.family, self.tr, self.dev = family, tr, dev
        m = mesh if mesh is not None else (P.m0 if tr is None else tm.apply(P.m0, tr))
        self.m = m.to(dev)
        self.V = V = fem.functionspace(self.m, ("Lagrange", P.p, (P.gd,)))
        assert np.array_equal(_np(V.dofmap), P.dofmap) and V.num_nodes == P.num_nodes
        self.E = _t(P.E, dev)
        self.s, self.Q = P.sQ(tr)
        self.left = torch.tensor(P.left, dtype=torch.int64, device=dev)

    def bcs(self, g=0.0):
        """The Dirichlet set with the value g (a vector: moved with the mesh, g' = s Q g)."""
        from femasm import fem

        if not np.isscalar(g):
            g = list(self.s * (self.Q @ np.asarray(g[:self.P.gd])))
        return [fem.dirichletbc(g, self.left, self.V)]

    def vec(self, v, power):
        return _t(self.P.moved(v, self.tr, power), self.dev)

    def form(self, kind, tangent="hand", with_f=False, state=None):
        from femasm import fem

        P, V = self.P, self.V
        f = self.vec(P.body_force(), -1) if with_f else None
        if kind == "lin":
            u = None if state is None else self.vec(P.state(state), 1)
            return fem.LinearElasticity(V, E=self.E, nu=0.3, u=u, f=f)
        if kind == "neo":
            return fem.NeoHookean(V, E=self.E, nu=0.3, u=self.vec(P.state("neo"), 1), f=f)
        return fem.AsymDamage(V, E=self.E, nu=0.3, u=self.vec(P.state("dam"), 1), d=_t(P.damage(), self.dev), f=f,
                              tangent=tangent)

    def flag(self, A, a, kw):
        """FA_PLAN_AFFINE of the plan the route assembles with (None: the scatter has no plan)."""
        from femasm import _lib, fem

        if kw.get("method") == "scatter":
            return None
        plan = fem.gather_plan(self.V, A, 0, a.kind, deterministic=kw.get("deterministic", False), **kw.get("plan", {}))
        return bool(plan.cell_flags & _lib.FA_PLAN_AFFINE)

    def assemble(self, a, kw, repeat=False):
        """Values [nb, d, d] of the form through the route kw with the Dirichlet set and diagonal s^(d-2),
        into a matrix pre-filled with NaN (twice on the same matrix when `repeat`: the kept cell state)."""
        from femasm import fem

        P = self.P
        A = fem.create_matrix(a, check=True)
        np.testing.assert_array_equal(_np(A.indptr), P.ip)
        np.testing.assert_array_equal(_np(A.indices), P.ix)
        for _ in range(2 if repeat else 1):
            _fill_nan(A)
            fem.assemble_matrix(a, bcs=self.bcs(), diagonal=P.diag(self.tr), A=A, **kw)
        got = _np(A.data)
        assert np.isfinite(got).all(), "blocks not written or not finite"
        check_bc_structure(got, P.ip, P.ix, P.marker, P.diag(self.tr), P.gd)
        return got, self.flag(A, a, kw)


_base = {}  # (family, kind, route) -> GPU values on the untransformed mesh, computed once and left unchanged


def _base_matrix(oracle, dev, family, kind, route, kw, tangent="hand"):
    key = (family, kind, route, tangent)
    if key not in _base:
        S = Setup(oracle, dev, family, None)
        _base[key] = S.assemble(S.form(kind, tangent), kw)[0]
    return _base[key]


def _matrix_case(oracle, dev, family, tr, kind, routes, tangent="hand"):
    """Parity with the oracle on the transformed mesh and, for the orthogonal transforms, covariance
    against the same route's matrix on the untransformed mesh."""
    S = Setup(oracle, dev, family, tr)
    P = S.P
    ref = P.matrix(kind, tr)
    case = f"{family} {tr} {kind}" + ("" if tangent == "hand" else "-ad")
    for route, kw in routes.items():
        got, flag = S.assemble(S.form(kind, tangent), kw, repeat=(route == "gather"))
        err = row_errors(got, ref, P.ip)[0]
        _say(case + " parity", route, flag, err, RTOL)
        assert err <= RTOL, f"{case} {route}: per-row parity {err:.3e}"
        if flag is not None and family not in tm.SIMPLEX and kind == "lin":
            assert flag == tm.is_affine(family), f"{case} {route}: plan flag {flag}"
        if tr in tm.ORTHOGONAL:
            want = tm.map_blocks(_base_matrix(oracle, dev, family, kind, route, kw, tangent), S.s, S.Q)
            bar = 2e-12 + H.matrix_covariance(P, kind, tr)
            err = row_errors(got, want, P.ip)[0]
            _say(case + " covariance", route, flag, err, bar)
            assert err <= bar, f"{case} {route}: covariance {err:.3e} > {bar:.3e}"


# ------------------------------------------------------------------------------------------- matrices
@pytest.mark.parametrize("tr", tm.PARITY)
@pytest.mark.parametrize("family", list(tm.FAMILIES))
def test_linear_elasticity(oracle, dev, family, tr):
    """Every route of the family: simplices all of test_gpu_irregular.ROUTES; affine tensor cells the
    default gather (MAT_AFFT, its prepared records on the second assembly), the deterministic mode where
    there is one, and the scatter; warped tensor cells the default gather and the scatter. The plan of an
    affine tensor family is affine under every transform here, that of a warped one is not."""
    _matrix_case(oracle, dev, family, tr, "lin", routes_of(family))


@pytest.mark.parametrize("tr", tm.PARITY)
@pytest.mark.parametrize("family", ["tet-P1", "tet-P2", "tri-P2", "quad-Q2", "hex-Q1"])
def test_neohookean_tangent(oracle, dev, family, tr):
    _matrix_case(oracle, dev, family, tr, "neo", {"gather": dict(), "scatter": dict(method="scatter")})


@pytest.mark.parametrize("tangent", ["hand", "ad"])
@pytest.mark.parametrize("tr", tm.PARITY)
def test_damage_tangent(oracle, dev, tr, tangent):
    """At the sheared state (the reference's law is not frame-indifferent at zero shear:
    tests/test_invariance_host.py)."""
    _matrix_case(oracle, dev, "tri-P1", tr, "dam", {"gather": dict(), "scatter": dict(method="scatter")}, tangent)


# ------------------------------------------------------------------------------------------- shifted meshes
@pytest.mark.parametrize("tr", tm.SHIFTS)
@pytest.mark.parametrize("family", list(tm.FAMILIES))
def test_shifted_mesh(oracle, dev, family, tr):
    S = Setup(oracle, dev, family, tr)
    P = S.P
    ref = P.matrix("lin", tr)
    c = H.translation_error(P, tr)
    bar = RTOL + 4.0 * c
    for route, kw in (("gather", dict()), ("scatter", dict(method="scatter"))):
        got, flag = S.assemble(S.form("lin"), kw)
        err = row_errors(got, ref, P.ip)[0]
        _say(f"{family} {tr} c(T)={c:.2e} parity", route, flag, err, bar)
        assert err <= bar, f"{family} {tr} {route}: {err:.3e} > {bar:.3e}"


# ------------------------------------------------------------------------------------------- near threshold
@pytest.mark.parametrize("delta", tm.DELTAS)
@pytest.mark.parametrize("family", tm.NEAR_THRESHOLD)
def test_near_threshold_mesh(oracle, dev, family, delta):
    """One vertex moved by delta h: whichever route the plan takes, the matrix is the trilinear oracle's
    to the plain bar. (With the affinity threshold at 1e-12 of the cell size the affine route served
    dev / h up to 1e-12 and cost up to 3 dev / h, tests/test_invariance_host.py; it is 1e-13 now.)"""
    P = H.problem(oracle, family)
    m = tm.nudge_vertex(P.m0, delta)
    S = Setup(oracle, dev, family, None, mesh=m)
    x = m.x.numpy()
    ref = P.matrix("lin", None, x=x)
    got, flag = S.assemble(S.form("lin"), dict())
    err = row_errors(got, ref, P.ip)[0]
    dev_h = tm.affine_deviation(x, P.geom).max()
    _say(f"{family} delta={delta:g} dev/h={dev_h:.2e} parity", "gather", flag, err, RTOL)
    assert err <= RTOL, f"{family} delta {delta:g}: {err:.3e} (plan affine: {flag})"


# ------------------------------------------------------------------------------------------- vectors
@pytest.mark.parametrize("tr", tm.PARITY)
@pytest.mark.parametrize("family", list(tm.FAMILIES))
def test_residual_lifting_set_bc(oracle, dev, family, tr):
    """assemble_vector, apply_lifting(alpha = -1) and set_bc, each against the oracle on the transformed
    mesh and, for the orthogonal transforms, against the map of the same step on the untransformed mesh
    (constrained rows after set_bc hold -(g - u): they move like a displacement, s Q)."""
    from femasm import fem

    P = H.problem(oracle, family)
    okind = {"lin": 0, "dam": 1, "neo": 2}
    for kind in tm.forms_of(family):
        steps = {}
        for frame in ((None, tr) if tr in tm.ORTHOGONAL else (tr,)):
            key = (family, kind, "vec")
            if frame is None and key in _base:
                steps[None] = _base[key]
                continue
            S = Setup(oracle, dev, family, frame)
            J = S.form(kind, with_f=True, state=kind)
            bcs = S.bcs(G_BC)
            marker, gv = fem._combine_bcs(S.V, bcs)
            np.testing.assert_array_equal(_np(marker), P.marker)
            u = P.moved(P.state(kind), frame, 1)
            d = P.damage() if kind == "dam" else None
            args = (P.ct, P.p, P.dofmap, P.geom, P.x(frame), P.lam, P.mu)
            out = []

            def close(b, ref, what):
                err = tm.vector_error(_np(b), ref)
                if frame is not None:
                    _say(f"{family} {tr} {kind} {what} parity", "vector", None, err, RTOL)
                assert np.isfinite(ref).all() and err <= RTOL, f"{family} {frame} {kind} {what}: {err:.3e}"
                out.append(_np(b).copy())

            b = fem.assemble_vector(J)
            ref = P.residual(kind, frame)
            close(b, ref, "residual")
            fem.apply_lifting(b, [J], [bcs], x0=[J.u], alpha=-1.0)
            ref = oracle.apply_lifting(*args, ref, P.marker, _np(gv), x0=u, alpha=-1.0, u=u if okind[kind] else None, d=d,
                                       kind=okind[kind])
            close(b, ref, "lifting")
            fem.set_bc(b, bcs, x0=J.u, alpha=-1.0)
            mk = P.marker.astype(bool)
            ref[mk] = -1.0 * (_np(gv)[mk] - u[mk])
            close(b, ref, "set_bc")
            steps[frame] = out
            if frame is None:
                _base[key] = out
        if tr not in tm.ORTHOGONAL:
            continue
        s, Q = P.sQ(tr)
        floor = H.residual_covariance(P, kind, tr)
        bar = 2e-12 + (4.0 * floor if kind == "dam" else 0.0)
        mk = P.marker.astype(bool)
        for k, what in enumerate(("residual", "lifting", "set_bc")):
            want = tm.map_vector(steps[None][k], s, Q)
            if what == "set_bc":
                want[mk] = tm.map_vector(steps[None][k], s, Q, power=1)[mk]
            free = np.ones_like(mk) if what != "set_bc" else ~mk
            err = np.abs(steps[tr][k] - want)[free].max() / np.abs(want[free]).max()
            _say(f"{family} {tr} {kind} {what} covariance", "vector", None, err, bar)
            assert err <= bar, f"{family} {tr} {kind} {what}: covariance {err:.3e} > {bar:.3e}"
            if what == "set_bc":  # the constrained rows, at their own scale
                err = tm.vector_error(steps[tr][k][mk], want[mk])
                assert err <= bar, f"{family} {tr} {kind} set_bc rows: {err:.3e}"


# ------------------------------------------------------------------------------------------- matrix-free
OPERATOR = [("tri-P1", "planned"), ("tri-P2", "planned"), ("tet-P1", "planned"), ("tet-P2", "planned"),
            ("tri-P2", "generic"), ("tet-P2", "generic"), ("quad-Q2", "generic"), ("hex-Q1", "generic"),
            ("hex-Q2", "generic"), ("quad-Q2-warp", "generic"), ("hex-Q1-warp", "generic"), ("hex-Q2-warp", "generic")]


@pytest.mark.parametrize("tr", tm.ORTHOGONAL)
@pytest.mark.parametrize("family,method", OPERATOR)
def test_jacobian_operator(oracle, dev, family, method, tr):
    """op'.mult(Q x) = s^(d-2) Q op.mult(x), and op' against the assembled matrix of the transformed mesh
    row by row (tests/test_gpu_matrix_free.py's bar). Covariance bar per node: each side is within 1e-12 of
    its rows' scale (|S| |x|); Q mixes the d components of a node, so (1 + d) 1e-12 of the node's scale."""
    from femasm import fem

    P = H.problem(oracle, family)
    d = P.gd
    for kind in ("lin", "neo"):
        y = {}
        for frame in (None, tr):
            S = Setup(oracle, dev, family, frame)
            a = S.form(kind)
            diag = 2.5 * P.diag(frame)
            bcs = S.bcs()
            op = fem.JacobianOperator(a, bcs=bcs, diagonal=diag, method=method)
            assert (op.num_chunks >= 1) == (method == "planned")
            M = fem.assemble_matrix(a, bcs=bcs, diagonal=diag).to_scipy().tocsr()
            x0, _ = _check_mult(op, M, dev, f"{family} {frame} {kind} {method}")
            x = S.vec(_np(x0), 0) if frame is not None else x0  # x' = Q x
            y[frame] = (_np(op.mult(x)), abs(M) @ np.abs(_np(x)))
        s, Q = P.sQ(tr)
        want = tm.map_vector(y[None][0], s, Q, power=d - 2)
        scale = np.repeat(y[tr][1].reshape(-1, d).max(1), d)
        err = (np.abs(y[tr][0] - want) / scale).max()
        bar = (1 + d) * 1e-12
        _say(f"{family} {tr} {kind} operator covariance", method, None, err, bar)
        assert err <= bar, f"{family} {tr} {kind} {method}: {err:.3e}"


# ------------------------------------------------------------------------------------------- expressions
def _full(r, gd):
    """Reduced [..., gd (gd + 1) / 2] -> symmetric [..., gd, gd] (the inverse of test_gpu_expression._reduce)."""
    out = np.zeros(r.shape[:-1] + (gd, gd))
    k = 0
    for i in range(gd):
        for j in range(i, gd):
            out[..., i, j] = out[..., j, i] = r[..., k]
            k += 1
    assert np.array_equal(_reduce(out), r)
    return out


@pytest.mark.parametrize("tr", tm.ORTHOGONAL)
@pytest.mark.parametrize("family", ["tet-P2", "hex-Q2", "hex-Q2-warp", "quad-Q2"])
def test_evaluate(oracle, dev, family, tr):
    """grad, strain, stress (and, for the linear law, energy) at the midpoint and at several points: tensors
    of the transformed problem are Q (.) Q^T of the untransformed problem's, the energy density is the same,
    to 1e-12 of each quantity's largest value (the neo-Hookean stress is the first Piola stress, full)."""
    from femasm import fem

    P = H.problem(oracle, family)
    gd = P.gd
    s, Q = P.sQ(tr)
    for kind in ("lin", "neo"):
        names = ("grad", "strain", "stress") + (("energy",) if kind == "lin" else ())
        for X in (None, _points(oracle, P.ct)):
            res = {}
            for frame in (None, tr):
                S = Setup(oracle, dev, family, frame)
                a = S.form(kind, state="lin")
                res[frame] = {k: _np(v) for k, v in fem.evaluate(a, names, X=X).items()}
            nc = P.m0.num_cells
            for q in names:
                got, base = res[tr][q], res[None][q]
                if q == "energy":
                    want = base
                elif q == "grad" or (q == "stress" and kind == "neo"):
                    want = tm.map_tensor(base.reshape(nc, -1, gd, gd), Q).reshape(nc, -1)
                else:
                    want = _reduce(tm.map_tensor(_full(base.reshape(nc, -1, gd * (gd + 1) // 2), gd), Q)).reshape(nc, -1)
                assert np.isfinite(got).all() and np.abs(want).max() > 0
                err = tm.vector_error(got, want)
                _say(f"{family} {tr} {kind} {q} {'midpoint' if X is None else 'points'} covariance", "evaluate", None, err, RTOL)
                assert err <= RTOL, f"{family} {tr} {kind} {q}: {err:.3e}"


# ------------------------------------------------------------------------------------------- surface loads
@pytest.mark.parametrize("tr", tm.ORTHOGONAL)
@pytest.mark.parametrize("family", ["tri-P1", "tri-P2", "tet-P1", "tet-P2", "quad-Q1", "quad-Q2", "quad-Q3", "hex-Q1",
                                    "hex-Q2"])
def test_surface_load(oracle, dev, family, tr):
    """Pressure p and traction Q t on the face x0 = 1 (facet ids taken before the transform): b' = s^(d-1) Q b,
    parity with tests/facet_reference.py on the transformed mesh (under `mirror` the outward normal must
    stay outward), and any facet order gives the same bits."""
    from femasm import fem, mesh

    P = H.problem(oracle, family)
    m0 = P.m0
    face = mesh.locate_entities_boundary(m0, m0.tdim - 1, lambda x: torch.isclose(x[0], torch.ones_like(x[0])))
    face = face.to(torch.int64)
    nf = int(face.numel())
    assert nf > 0
    rng = np.random.default_rng(7)
    tn, pf = rng.random(P.xn.size) - 0.5, rng.random(nf)
    perm = torch.randperm(nf, generator=torch.Generator().manual_seed(7))
    qd = None if family in tm.SIMPLEX else 2 * P.p + 2
    s, Q = P.sQ(tr)
    for kw in (("traction",), ("pressure",), ("traction", "pressure")):
        b = {}
        for frame in (None, tr):
            S = Setup(oracle, dev, family, frame)
            t = P.moved(tn, frame, 0)
            vals = dict(traction=_t(t, dev), pressure=_t(pf, dev))
            f = face.to(dev)
            ld = fem.SurfaceLoad(S.V, f, quadrature_degree=qd, **{k: vals[k] for k in kw})
            bb = fem.assemble_surface_load(ld)
            ref = FR.reference_load(S.V, _np(f), t_nodal=t if "traction" in kw else None,
                                    p_facet=pf if "pressure" in kw else None)
            err = tm.vector_error(_np(bb), ref)
            if frame is not None:
                _say(f"{family} {tr} load {'+'.join(kw)} parity", "facet", None, err, RTOL)
            assert err <= RTOL, f"{family} {frame} {kw}: {err:.3e}"
            pv = {k: (vals[k][perm.to(dev)] if k == "pressure" else vals[k]) for k in kw}
            ldp = fem.SurfaceLoad(S.V, f[perm.to(dev)], quadrature_degree=qd, **pv)
            assert torch.equal(fem.assemble_surface_load(ldp), bb), "facet order changed the bits"
            b[frame] = _np(bb)
        err = tm.vector_error(b[tr], tm.map_vector(b[None], s, Q))
        _say(f"{family} {tr} load {'+'.join(kw)} covariance", "facet", None, err, 2e-12)
        assert err <= 2e-12, f"{family} {tr} {kw}: covariance {err:.3e}"
