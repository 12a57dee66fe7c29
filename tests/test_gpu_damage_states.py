"""Every device route of the asymmetric damage law at the law's branch states (tests/damage_states.py:
zero and null strains, double eigenvalues, uniaxial and zero-shear states, I1 = 0, d = 1, d barely above 0),
with neighbouring lanes of a wave in different branches (the "interleaved" soup), with branch-uniform waves
(the "sorted" soup: the same cells, bit-identical results), on rotated scalene triangles (the "generic"
mesh) and on the reference driver's first two states of a structured mesh.

References: the oracle (the reference's hand tangent and hand stress) for tangent="hand"; the long-double
gradient and frozen-indicator Hessian of the reference potential for tangent="ad". The hand hook is that
Hessian at every state (tests/test_damage_states_host.py), so both tangents are held to the oracle's
matrices; the hand stress is not the gradient on damage_states.HAND_STRESS_NOT_GRADIENT, so each residual
is held to its own reference and their difference to the oracle's.

Bars: 1e-12 times the cell's scale (damage_states), matrices per row through rowparity. Every output must be
finite; a non-finite value is reported with its state's name."""
import numpy as np
import pytest
import torch

import damage_states as ds
from rowparity import RTOL, assert_rows_close

pytestmark = pytest.mark.gpu
LD = np.longdouble
DIAG = 2.5
TANGENTS = ("hand", "ad")
TABLE = {}  # route -> {state class: worst error / scale}, printed by the last test


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t):
    return t.detach().cpu().numpy()


def _form(case, dev, tangent):
    from femasm import fem, mesh

    m = mesh.Mesh(mesh.CellType.triangle, torch.tensor(case.x, device=dev), torch.tensor(case.cells, device=dev),
                  None, None)
    V = fem.functionspace(m, ("Lagrange", 1, (2,)))
    assert np.array_equal(_np(V.dofmap), case.cells)
    a = fem.AsymDamage(V, E=torch.tensor(case.E, device=dev), nu=ds.NU, u=torch.tensor(case.u, device=dev),
                       d=torch.tensor(case.d, device=dev), tangent=tangent)
    return fem, V, a


def _cell_routes(case, dev, tangent):
    """The per-cell routes of one form: element matrices, residual, midpoint expressions, cellwise energy."""
    fem, V, a = _form(case, dev, tangent)
    ev = fem.evaluate(a, ["strain", "stress", "energy"])
    return {"Ke": _np(fem.tabulate_cells(a)), "b": _np(fem.assemble_vector(a)).reshape(case.nc, 6),
            "strain": _np(ev["strain"]), "stress": _np(ev["stress"]), "eps:sigma": _np(ev["energy"]).reshape(-1),
            "energy": _np(fem.assemble_scalar(fem.StrainEnergy(a), cellwise=True)),
            "total": float(fem.assemble_scalar(fem.StrainEnergy(a)))}


class _Refs:
    def __init__(self, oracle, case):
        self.case = case
        self.ref = r = ds.references(case)
        self.hook, self.osig = ds.oracle_cells(oracle, case)  # hand tangent and hand stress, per cell
        self.Ke_hand = ds.element_matrices(self.hook, r)
        self.ob = oracle.assemble_residual(3, 1, case.cells, case.cells, case.x, case.lam, case.mu, u=case.u, d=case.d,
                                           kind=1).reshape(case.nc, 6)
        self.indptr, self.indices = oracle.sparsity(case.cells, 3 * case.nc)
        self.named = (r.branch != "linear") & np.array(
            [ds.STATE_NAMES[s] in ds.HAND_STRESS_NOT_GRADIENT for s in case.state])
        # The hand stress takes r = sqrt(I1^2 + 4 I2) (asym_stress): at a double eigenvalue whose strain carries
        # roundoff the sum cancels to +-ulp(I1^2) = 2^-52 I1^2 and r, hence both principal strains, move by
        # 2^-26 |I1| = 1.5e-8 |I1| from one rounding (an FMA contraction, say) to the next. The oracle is then
        # good to that and no better: such cells' hand stresses are held to 3e-8 of the scale. The soup's
        # strains are exact (r = 0 exactly) and keep the 1e-12 bar; so do the AD stress, both tangents and the
        # energy everywhere (they depend on r^2 or on r * dr, which do not amplify).
        self.hand_slack = np.where((case.order == "generic") & (r.branch == "double"), 3e-8 / ds.BAR, 1.0)

    def stress(self, tangent):  # (s11, s22, s12) per cell
        return self.osig.astype(LD) if tangent == "hand" else self.ref.sig

    def residual(self, tangent):
        return self.ob.astype(LD) if tangent == "hand" else self.ref.re


def _record(route, err, scale, case):
    TABLE[route] = ds.by_class(err, scale, case)


def _check_cell_routes(R, out, tangent, tag):
    case, r = R.case, R.ref
    for k, v in out.items():
        if k != "total":
            ds.assert_finite(v, case, f"{tag} {k}")
    w = r.w
    slack = R.hand_slack if tangent == "hand" else 1.0
    _record(f"{tag} tabulate_cells", ds.assert_close(out["Ke"], R.Ke_hand, r.s_tangent * w, case, f"{tag} tabulate_cells"),
            r.s_tangent * w, case)
    if tangent == "ad":  # the AD tangent is also the long-double Hessian itself
        ds.assert_close(out["Ke"], r.Ke, r.s_tangent * w, case, f"{tag} tabulate_cells vs long-double Hessian")
    _record(f"{tag} assemble_vector", ds.assert_close(out["b"], R.residual(tangent), r.s_stress * w * slack, case, f"{tag} assemble_vector"),
            r.s_stress * w * slack, case)
    emax = np.abs(r.eps).max(1)
    ds.assert_close(out["strain"], r.eps[:, [0, 2, 1]], emax, case, f"{tag} evaluate strain")
    sig = R.stress(tangent)
    _record(f"{tag} evaluate stress", ds.assert_close(out["stress"], sig[:, [0, 2, 1]], r.s_stress * slack, case, f"{tag} evaluate stress"),
            r.s_stress * slack, case)
    en = r.eps[:, 0] * sig[:, 0] + r.eps[:, 1] * sig[:, 1] + 2 * r.eps[:, 2] * sig[:, 2]
    _record(f"{tag} evaluate energy", ds.assert_close(out["eps:sigma"], en, r.s_energy * slack, case, f"{tag} evaluate energy"),
            r.s_energy * slack, case)
    _record(f"{tag} assemble_scalar cellwise", ds.assert_close(out["energy"], r.energy, r.s_energy * w, case, f"{tag} cellwise energy"),
            r.s_energy * w, case)
    total, bar = float(r.energy.sum()), float(ds.BAR * (r.s_energy * w).sum())
    assert np.isfinite(out["total"]) and abs(out["total"] - total) <= bar, (tag, out["total"], total)
    TABLE[f"{tag} assemble_scalar total"] = {"whole mesh": abs(out["total"] - total) / float((r.s_energy * w).sum())}


@pytest.fixture(scope="module")
def soup(oracle):
    return _Refs(oracle, ds.soup("interleaved"))


@pytest.fixture(scope="module")
def soup_out(soup, dev):
    return {t: _cell_routes(soup.case, dev, t) for t in TANGENTS}


@pytest.mark.parametrize("tangent", TANGENTS)
def test_cell_routes_interleaved(soup, soup_out, tangent):
    _check_cell_routes(soup, soup_out[tangent], tangent, tangent)


def test_hand_and_ad_differ_only_where_the_oracle_does(soup, soup_out):
    """Residual and midpoint stress: hand - AD is the oracle's own (hand stress - gradient), which is beyond
    the bar exactly on the named states."""
    case, r = soup.case, soup.ref
    for key, oref, gref, scale in (("b", soup.ob, r.re, r.s_stress * r.w),
                                   ("stress", soup.osig[:, [0, 2, 1]], r.sig[:, [0, 2, 1]], r.s_stress)):
        dd = soup_out["hand"][key].astype(LD) - soup_out["ad"][key]
        want = oref.astype(LD) - gref
        ds.assert_close(dd, want, scale, case, f"hand - ad ({key})", bar=2 * ds.BAR)
        beyond = np.abs(dd).max(1) > 2 * ds.BAR * scale
        assert not (beyond & ~soup.named).any()
        for name in ds.HAND_STRESS_NOT_GRADIENT:
            sel = (case.state == ds.STATE_NAMES.index(name)) & (np.abs(r.d - LD(0.4)) < 1e-15)
            assert beyond[sel].all(), name


def _bcs(fem, V, case):
    nodes = torch.arange(1, 3 * case.nc, 3, device=V.mesh.device)  # vertex 1 of every cell
    return [fem.dirichletbc([0.01, -0.02], nodes, V)]


@pytest.mark.parametrize("tangent", TANGENTS)
def test_matrix_routes_interleaved(oracle, soup, dev, tangent):
    """assemble_matrix (gather, scatter) against the oracle per row; JacobianOperator (planned and generic
    kernels) against the assembled matrix times x per row; block_diagonal; apply_lifting against the oracle."""
    case, r = soup.case, soup.ref
    fem, V, a = _form(case, dev, tangent)
    bcs = _bcs(fem, V, case)
    marker, gv = fem._combine_bcs(V, bcs)
    ref_free = oracle.assemble_damage(case.cells, case.cells, case.x, case.lam, case.mu, case.u, case.d, soup.indptr,
                                      soup.indices)
    ref_bc = oracle.assemble_damage(case.cells, case.cells, case.x, case.lam, case.mu, case.u, case.d, soup.indptr,
                                    soup.indices, bc=_np(marker), diag=DIAG)
    for method in ("gather", "scatter"):
        for bc_, ref in ((None, ref_free), (bcs, ref_bc)):
            A = fem.assemble_matrix(a, bcs=bc_, diagonal=DIAG, method=method)
            np.testing.assert_array_equal(_np(A.indices), soup.indices)
            ds.assert_finite(_np(A.data), case, f"{tangent} assemble_matrix {method}")
            rel = assert_rows_close(_np(A.data), ref, soup.indptr, RTOL, f"{tangent} {method} bc={bc_ is not None}")
            TABLE[f"{tangent} assemble_matrix {method}{' bc' if bc_ else ''}"] = {"worst row": rel}
    S = fem.assemble_matrix(a, bcs=bcs, diagonal=DIAG).to_scipy().tocsr()
    n = S.shape[0]
    x = (2.0 * (torch.rand(n, generator=torch.Generator().manual_seed(1), dtype=torch.float64) - 0.5)).to(dev)
    xh = _np(x)
    want, scale = S @ xh, abs(S) @ np.abs(xh)
    for method in ("planned", "generic"):
        op = fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method=method)
        assert (op.num_chunks == 0) == (method == "generic")
        y = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        op.mult(x, y)
        yh = _np(y)
        ds.assert_finite(yh, case, f"{tangent} JacobianOperator {method}")
        err = np.abs(yh - want)
        assert (err <= RTOL * scale).all(), (tangent, method, float((err / np.where(scale > 0, scale, 1)).max()))
        TABLE[f"{tangent} JacobianOperator {method}"] = {"worst row": float((err / np.where(scale > 0, scale, 1)).max())}
        D = _np(op.block_diagonal())
        ds.assert_finite(D, case, f"{tangent} block_diagonal {method}")
        rowmax = np.asarray(abs(S).max(axis=1).todense()).reshape(-1, 2)
        nodes = np.arange(n // 2)
        for i in range(2):
            for k in range(2):
                e = np.abs(D[:, i, k] - np.asarray(S[nodes * 2 + i, nodes * 2 + k]).reshape(-1))
                assert (e <= RTOL * rowmax[:, i]).all(), (tangent, method, i, k)
    b = torch.zeros(n, dtype=torch.float64, device=dev)
    fem.apply_lifting(b, [a], [bcs], x0=[a.u], alpha=-1.0)
    lref = oracle.apply_lifting(3, 1, case.cells, case.cells, case.x, case.lam, case.mu, np.zeros(n), _np(marker), _np(gv),
                                x0=case.u, alpha=-1.0, u=case.u, d=case.d, kind=1)
    gap = np.abs(np.array([0.01, -0.02]) - case.u.reshape(-1, 2)[1::3]).max(1)  # |g - x0| on the cell's bc node
    s = r.s_tangent * r.w * gap
    _record(f"{tangent} apply_lifting", ds.assert_close(_np(b).reshape(case.nc, 6), lref.reshape(case.nc, 6), s, case,
                                                       f"{tangent} apply_lifting"), s, case)


@pytest.mark.parametrize("tangent", TANGENTS)
def test_sorted_order_is_bit_identical(soup, soup_out, dev, tangent):
    """Branch-uniform waves give, cell by cell, the bits of the mixed waves (every node has one cell: no sum
    order enters)."""
    other = ds.soup("sorted")
    out = _cell_routes(other, dev, tangent)
    pos = np.argsort(other.ident)[soup.case.ident]  # where the sorted soup holds the interleaved soup's cells
    for k in ("Ke", "b", "strain", "stress", "eps:sigma", "energy"):
        ds.assert_finite(out[k], other, f"sorted {tangent} {k}")
        assert np.array_equal(out[k][pos], soup_out[tangent][k]), f"{tangent} {k}: the order of the cells changed bits"


@pytest.mark.parametrize("tangent", TANGENTS)
def test_generic_mesh(oracle, dev, tangent):
    """The states whose branch survives roundoff, on rotated scalene triangles."""
    case = ds.generic()
    R = _Refs(oracle, case)
    _check_cell_routes(R, _cell_routes(case, dev, tangent), tangent, f"generic {tangent}")
    fem, V, a = _form(case, dev, tangent)
    ref = oracle.assemble_damage(case.cells, case.cells, case.x, case.lam, case.mu, case.u, case.d, R.indptr, R.indices)
    for method in ("gather", "scatter"):
        A = fem.assemble_matrix(a, method=method)
        ds.assert_finite(_np(A.data), case, f"generic {tangent} {method}")
        assert_rows_close(_np(A.data), ref, R.indptr, RTOL, f"generic {tangent} {method}")


@pytest.mark.parametrize("state", ["u=0", "uniaxial"])
@pytest.mark.parametrize("tangent", TANGENTS)
def test_structured_mesh_first_newton_states(oracle, dev, tangent, state):
    """The reference driver's start: u = 0 with a Gaussian d (every damaged cell in the null branch), then
    the exact uniaxial field u = (2^-10 x, 0) (every cell at the kink ev2 = 0 with zero shear)."""
    from femasm import fem, mesh

    m = mesh.create_unit_square(8, 8, cell_type=mesh.CellType.triangle, device=dev)
    V = fem.functionspace(m, ("Lagrange", 1, (2,)))
    x = _np(V.tabulate_dof_coordinates())
    dfun, u0, u1 = ds.structured_states()
    d, u = dfun(x), (u0 if state == "u=0" else u1)(x)
    E = oracle.e_range()[np.arange(m.num_cells) % 200]
    lam, mu = oracle.lame(E, ds.NU)
    a = fem.AsymDamage(V, E=torch.tensor(E, device=dev), nu=ds.NU, u=torch.tensor(u, device=dev),
                       d=torch.tensor(d, device=dev), tangent=tangent)
    left = fem.locate_dofs_geometrical(V, lambda p: torch.isclose(p[0], torch.zeros_like(p[0])))
    right = fem.locate_dofs_geometrical(V, lambda p: torch.isclose(p[0], torch.ones_like(p[0])))
    bcs = [fem.dirichletbc(0.0, left, V), fem.dirichletbc([2.0 ** -10, 0.0], right, V)]
    marker, _ = fem._combine_bcs(V, bcs)
    cells, geom, xv = _np(V.dofmap), _np(m.cells), _np(m.x)
    indptr, indices = oracle.sparsity(cells, V.num_nodes)
    ref = oracle.assemble_damage(cells, geom, xv, lam, mu, u, d, indptr, indices, bc=_np(marker), diag=DIAG)
    A = fem.assemble_matrix(a, bcs=bcs, diagonal=DIAG)
    assert np.isfinite(_np(A.data)).all(), f"{tangent} {state}: non-finite tangent"
    assert_rows_close(_np(A.data), ref, indptr, RTOL, f"structured {tangent} {state}")
    b = _np(fem.assemble_vector(a))
    bref = oracle.assemble_residual(3, 1, cells, geom, xv, lam, mu, u=u, d=d, kind=1)
    assert np.isfinite(b).all(), f"{tangent} {state}: non-finite residual"
    # per row: the sum over the node's cells of their stress scales (u = 0: exactly zero)
    sc = np.zeros(V.num_nodes)
    np.add.at(sc, cells.reshape(-1), np.repeat((lam + 2 * mu) * (0.0 if state == "u=0" else ds.S) / 128.0, 3))
    assert (np.abs(b - bref).reshape(-1, 2).max(1) <= ds.BAR * sc).all(), float(np.abs(b - bref).max())
    S = A.to_scipy().tocsr()
    xr = (torch.rand(S.shape[0], generator=torch.Generator().manual_seed(2), dtype=torch.float64) - 0.5).to(dev)
    for method in ("planned", "generic"):
        y = _np(fem.JacobianOperator(a, bcs=bcs, diagonal=DIAG, method=method).mult(xr))
        assert np.isfinite(y).all()
        assert (np.abs(y - S @ _np(xr)) <= RTOL * (abs(S) @ np.abs(_np(xr)))).all(), (tangent, state, method)


def test_print_error_table():
    """Not a check: the measured worst errors over the bar's scale, per route and state class."""
    for route in sorted(TABLE):
        print(f"ERRTABLE {route:45s} " + "  ".join(f"{k}={v:.2e}" for k, v in TABLE[route].items()))
