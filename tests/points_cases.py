"""Query points for the point-location tests, and the acceptance rule restated in numpy (test infrastructure;
never imported by the product package).

  interior_queries   seeded reference points of every cell with every barycentric (simplices) or every X_d and
                     1 - X_d (tensor cells) >= 0.05, mapped with the host geometry basis
  entity_queries     every vertex, edge midpoint and (3-D) face centre of the mesh (the centre of a bilinear
                     face is the mean of its four vertices); the expected cell is the smallest id among the
                     cells that hold the entity, from connectivity (mesh.entities), not from floating point
  outside_queries    points outside the reference domain [0, 1]^d by 1e-3 h on every side, pushed through the
                     transform with apply_x
  margin             min_i lambda_i or min_d min(X_d, 1 - X_d) of points in GIVEN cells (numpy rule)
  brute_force        the rule applied to every (point, cell) pair, smallest accepted cell: no grid
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import transformed_meshes as TM  # noqa: E402

TOL = 1e-10
NEWTON_CAP, NEWTON_STOP = 12, 1e-12  # as include/femasm.h states them
_MESHES = {}


def family_mesh(family: str, tr: str | None):
    """The (cached) host mesh of a family under a named transform."""
    key = (family, tr)
    if key not in _MESHES:
        m = TM.base_mesh(family)
        _MESHES[key] = m if tr is None else TM.apply(m, tr)
    return _MESHES[key]


def is_simplex(m) -> bool:
    return int(m.cell_type) in (TM.TRI, TM.TET)


def map_points(m, cells: np.ndarray, X: np.ndarray) -> np.ndarray:
    """x(X) in the given cells with the host P1 / Q1 geometry basis."""
    from femasm import fem

    psi = fem._geometry_basis(m.cell_type, X)  # [n, nv]
    xv = m.x.numpy()[m.cells.numpy().astype(np.int64)[cells]]  # [n, nv, gd]
    return np.einsum("nv,nvd->nd", psi, xv)


def interior_queries(m, per_cell: int = 3, seed: int = 5):
    """(x [n, gd], cell [n], X [n, gd]): per_cell seeded points of every cell, margins >= 0.05."""
    rng = np.random.default_rng(seed)
    nc, gd = m.num_cells, m.gdim
    cells = np.repeat(np.arange(nc), per_cell)
    n = cells.size
    if is_simplex(m):
        lam = rng.dirichlet(np.ones(gd + 1), n)
        lam = 0.05 + (1.0 - 0.05 * (gd + 1)) * lam
        X = lam[:, 1:]
    else:
        X = 0.05 + 0.9 * rng.random((n, gd))
    return map_points(m, cells, X), cells, X


def entity_queries(m):
    """(x [n, gd], expected cell [n]) of every vertex, edge midpoint and (3-D) face centre."""
    from femasm import mesh as fmesh

    x = m.x.numpy()
    nc = m.num_cells
    pts, exp = [], []
    for dim in range(m.tdim):
        if dim == 0:
            ev = np.arange(m.num_vertices)[:, None]
            ce = m.cells.numpy().astype(np.int64)
        else:
            ev_t, ce_t = fmesh.entities(m, dim)
            ev, ce = ev_t.numpy(), ce_t.numpy()
        first = np.full(ev.shape[0], nc, dtype=np.int64)
        np.minimum.at(first, ce.reshape(-1), np.repeat(np.arange(nc), ce.shape[1]))
        used = first < nc  # (a vertex no cell uses is no entity of the mesh)
        pts.append(x[ev[used]].mean(1))
        exp.append(first[used])
    return np.concatenate(pts), np.concatenate(exp)


def outside_queries(family: str, tr: str | None, per_side: int = 4, seed: int = 9):
    """Points 1e-3 h outside every side of the reference domain, in the transformed frame."""
    n = TM.FAMILIES[family][2]
    gd = len(n)
    h = 1.0 / max(n)
    rng = np.random.default_rng(seed)
    out = []
    for d in range(gd):
        for side in (-1e-3 * h, 1.0 + 1e-3 * h):
            p = rng.random((per_side, gd))
            p[:, d] = side
            out.append(p)
    p = np.concatenate(out)
    return p if tr is None else TM.apply_x(p, tr)


# ------------------------------------------------------------------------------------------- the rule, numpy
def _q1(X):
    gd = X.shape[1]
    nv = 1 << gd
    psi = np.ones((X.shape[0], nv))
    dpsi = np.ones((X.shape[0], nv, gd))
    for v in range(nv):
        for d in range(gd):
            up = (v >> d) & 1
            f = X[:, d] if up else 1.0 - X[:, d]
            psi[:, v] *= f
            for k in range(gd):
                dpsi[:, v, k] *= (1.0 if up else -1.0) if k == d else f
    return psi, dpsi


def pull_back(m, x: np.ndarray, cells: np.ndarray):
    """(X [n, gd], converged [n]) of the points in the given cells: the rule's solve (LU instead of cofactors)."""
    xv = m.x.numpy()[m.cells.numpy().astype(np.int64)[cells]]
    e = xv[:, 1:] - xv[:, :1]
    dx = x - xv[:, 0]
    n, gd = x.shape
    if is_simplex(m):
        X = np.linalg.solve(np.swapaxes(e, 1, 2), dx[:, :, None])[:, :, 0]
        return X, np.ones(n, dtype=bool)
    X = np.full((n, gd), 0.5)
    live = np.ones(n, dtype=bool)
    conv = np.zeros(n, dtype=bool)
    sign = None
    for it in range(NEWTON_CAP):
        psi, dpsi = _q1(X)
        r = np.einsum("nv,nvi->ni", psi[:, 1:], e) - dx
        J = np.einsum("nvi,nvk->nik", e, dpsi[:, 1:])
        det = np.linalg.det(J)
        sign = det if it == 0 else sign
        with np.errstate(all="ignore"):
            dX = -np.linalg.solve(J, r[:, :, None])[:, :, 0]
        Xn = X + dX
        go = live & ~conv
        ok = (det * sign > 0) & ((Xn >= -1) & (Xn <= 2)).all(1)
        upd = go & ok
        X = np.where(upd[:, None], Xn, X)
        conv |= upd & (np.abs(dX).max(1) <= NEWTON_STOP)
        live &= ok | ~go
    return X, live & conv


def margin(m, x: np.ndarray, cells: np.ndarray) -> np.ndarray:
    """Signed distance to the acceptance boundary in reference coordinates (negative: outside)."""
    X, ok = pull_back(m, x, cells)
    if is_simplex(m):
        mg = np.minimum(X.min(1), 1.0 - X.sum(1))
    else:
        mg = np.minimum(X, 1.0 - X).min(1)
    return np.where(ok, mg, -np.inf)


def brute_force(m, x: np.ndarray, tol: float = TOL) -> np.ndarray:
    """The smallest cell id whose margin is >= -tol, over ALL cells (no grid); -1 when there is none."""
    n, nc = x.shape[0], m.num_cells
    out = np.full(n, -1, dtype=np.int64)
    finite = np.isfinite(x).all(1)
    idx = np.nonzero(finite)[0]
    if idx.size == 0 or nc == 0:
        return out
    P, C = np.meshgrid(idx, np.arange(nc), indexing="ij")
    with np.errstate(all="ignore"):
        mg = margin(m, x[P.reshape(-1)], C.reshape(-1)).reshape(idx.size, nc)
    acc = mg >= -tol
    out[idx] = np.where(acc.any(1), acc.argmax(1), -1)
    return out


def round_trip_bar(m, x: np.ndarray, cells: np.ndarray) -> np.ndarray:
    """1e-12 * (|x|_inf + the cell's largest vertex coordinate): the bar of |x(X) - x|_inf per point."""
    xv = m.x.numpy()[m.cells.numpy().astype(np.int64)[cells]]
    return 1e-12 * (np.abs(x).max(1) + np.abs(xv).max((1, 2)))


def hole_mesh(n: int = 6):
    """The unit square's n x n x 2 triangles with the middle block of cells removed, and points in the hole."""
    from femasm import mesh

    m = mesh.create_unit_square(n, n)
    xc = m.x[m.cells.to(torch.int64)].mean(1)
    keep = ~(((xc - 0.5).abs() < 1.0 / 6.0).all(1))
    holed = mesh.Mesh(m.cell_type, m.x, m.cells[keep].contiguous())
    rng = np.random.default_rng(4)
    pts = 0.5 + (rng.random((20, 2)) - 0.5) * (2.0 / 6.0 - 0.02)
    return holed, pts


# ------------------------------------------------------------------------------------------- shared checks
TAIL_COUNTS = (1, 63, 65, 257)


def locate(m_host, x: np.ndarray, device, **kw):
    """(cells, X) as numpy, located on `device` (None: the host path)."""
    from femasm import geometry

    m = m_host if device is None else on_device(m_host, device)
    c, X = geometry.locate_points(m, torch.tensor(x, dtype=torch.float64).reshape(-1, m_host.gdim), **kw)
    return c.cpu().numpy(), X.cpu().numpy()


_ON_DEVICE = {}


def on_device(m_host, device):
    key = (id(m_host), str(device))
    if key not in _ON_DEVICE:
        _ON_DEVICE[key] = (m_host, m_host.to(device))  # (the host mesh is kept: its id stays taken)
    return _ON_DEVICE[key][1]


def check_interior(m, device, per_cell: int = 3):
    """Test 1 on one mesh: exact cells, the round trip within its bar, at the tail counts and the full set."""
    x, cells, _ = interior_queries(m, per_cell)
    mg = margin(m, x, cells)
    assert mg.min() > 1e-6, f"an interior query sits {mg.min():.2e} from its cell's boundary"
    for n in TAIL_COUNTS + (x.shape[0],):
        n = min(n, x.shape[0])
        c, X = locate(m, x[:n], device)
        assert c.dtype == np.int32 and np.array_equal(c, cells[:n]), f"{int((c != cells[:n]).sum())} of {n} cells differ"
        err = np.abs(map_points(m, cells[:n], X) - x[:n]).max(1)
        bar = round_trip_bar(m, x[:n], cells[:n])
        print(f"n {n}: round trip max err/bar {float((err / bar).max()):.3e}")
        assert (err <= bar).all(), float((err / bar).max())
    return x, cells


def check_entities(m, device):
    """Test 2 on one mesh: every vertex, edge midpoint and face centre goes to the smallest cell holding it."""
    x, exp = entity_queries(m)
    mg = margin(m, x, exp)
    assert np.abs(mg).max() < 1e-13, f"an entity query is {np.abs(mg).max():.2e} off its expected cell's boundary"
    c, X = locate(m, x, device)
    assert np.array_equal(c, exp), f"{int((c != exp).sum())} of {x.shape[0]} entity points in another cell"
    assert np.isfinite(X).all()
    return x, exp


def check_rejected(m, x: np.ndarray, device):
    c, X = locate(m, x, device)
    assert (c == -1).all(), f"{int((c != -1).sum())} of {x.shape[0]} outside points were placed in a cell"
    assert np.isnan(X).all()


# ------------------------------------------------------------------------------------------- fields
def space_of(m, family, bs):
    from femasm import fem

    return fem.functionspace(m, ("Lagrange", TM.FAMILIES[family][1], (bs,)))


def check_affine_field(family, tr, device, quadratic=False):
    """Test 6: u = A x + b (or a quadratic) interpolated into the space and evaluated at interior points."""
    from femasm import fem

    m_host = family_mesh(family, tr)
    m = m_host if device is None else on_device(m_host, device)
    gd = m.gdim
    rng = np.random.default_rng(12)
    for bs in (1, gd):
        V = space_of(m, family, bs)
        A, b = rng.standard_normal((bs, gd)), rng.standard_normal(bs)
        Q = rng.standard_normal((bs, gd, gd)) if quadratic else np.zeros((bs, gd, gd))
        At, bt, Qt = (torch.tensor(v, device=m.device) for v in (A, b, Q))
        u = fem.Function(V)
        # nodal interpolation at the TRANSFORMED mesh's nodes (tabulate_dof_coordinates would give a structured
        # mesh's generator lattice)
        xn = V._mapped_node_coordinates().T
        u.x = (At @ xn + bt[:, None] + torch.einsum("rij,in,jn->rn", Qt, xn, xn)).T.contiguous().reshape(-1)
        x, cells, _ = interior_queries(m_host, 2, seed=6)
        val, g = fem.eval_points(u, torch.tensor(x), grad=True)
        val, g = val.cpu().numpy(), g.cpu().numpy()
        ax = np.abs(x)
        exact = x @ A.T + b + np.einsum("rij,ni,nj->nr", Q, x, x)
        bar = 1e-12 * (ax @ np.abs(A).T + np.abs(b) + np.einsum("rij,ni,nj->nr", np.abs(Q), ax, ax))
        r = np.abs(val - exact) / bar
        print(f"{family} {tr} bs {bs}: value err/bar {r.max():.3e}")
        assert (r <= 1.0).all(), r.max()
        # gradient: A + (Q + Q^T) x, on the magnitude bar of the sum that forms it
        gexact = A[None] + np.einsum("rij,nj->nri", Q, x) + np.einsum("rji,nj->nri", Q, x)
        _, _, _, gbar = host_reference(V, u.x.cpu(), cells, torch.tensor(pull_back(m_host, x, cells)[0]))
        rg = np.abs(g - gexact) / (1e-12 * gbar)
        print(f"{family} {tr} bs {bs}: gradient err/bar {rg.max():.3e}")
        assert (rg <= 1.0).all(), rg.max()


def host_reference(V, w, cells, X):
    """(val, grad, value magnitude, gradient magnitude) from fem._space_basis / _space_basis_gradients and the
    host Jacobian at X, in numpy; the magnitudes are the same sums with every product in absolute value."""
    from femasm import fem

    m = V.mesh
    ct, p, bs = m.cell_type, V.degree, V.bs
    Xn = np.asarray(X)
    phi = fem._space_basis(ct, p, Xn)
    dphi = fem._space_basis_gradients(ct, p, Xn)
    gg = fem._geometry_gradients(ct, Xn)
    xv = m.x.cpu().numpy()[m.cells.cpu().numpy().astype(np.int64)[cells]]
    J = np.einsum("nvi,nvk->nik", xv - xv[:, :1], gg)
    Ji = np.linalg.inv(J)
    wc = np.asarray(w).reshape(-1, bs)[V.dofmap.cpu().numpy().astype(np.int64)[cells]]
    val = np.einsum("na,nar->nr", phi, wc)
    grad = np.einsum("nar,nak,nkj->nrj", wc, dphi, Ji)
    gmag = np.einsum("nar,nak,nkj->nrj", np.abs(wc), np.abs(dphi), np.abs(Ji))
    vmag = np.einsum("na,nar->nr", np.abs(phi), np.abs(wc))
    return val, grad, vmag, gmag


def _plain(m):
    """The mesh without its lattice record: its P2 space then has the documented numbering (vertices, edges)."""
    from femasm import mesh

    return mesh.Mesh(m.cell_type, m.x, m.cells)


def check_across_meshes(device):
    from femasm import fem, mesh

    for ct, n in ((mesh.CellType.triangle, (3, 2)), (mesh.CellType.tetrahedron, (2, 2, 1))):
        m = _plain(mesh.create_unit_square(*n) if len(n) == 2 else mesh.create_unit_cube(*n))
        m = m if device is None else m.to(device)
        gd = m.gdim
        fine = mesh.refine(m)
        V2 = fem.functionspace(m, ("Lagrange", 2, (gd,)))
        u = fem.Function(V2)
        # random signs, magnitudes in [0.5, 1] (at a node the bar is 1e-12 |w_node|: see test_eval_against_host_basis)
        gen = torch.Generator().manual_seed(3)
        w = 0.5 + 0.5 * torch.rand(V2.num_dofs, generator=gen, dtype=torch.float64)
        u.x = (w * torch.where(torch.rand(V2.num_dofs, generator=gen) < 0.5, -1.0, 1.0)).to(m.device)
        # P2 on m -> P1 on refine(m): node for node
        V1 = fem.functionspace(fine, ("Lagrange", 1, (gd,)))
        assert V1.num_nodes == V2.num_nodes
        u1 = fem.Function(V1)
        u1.interpolate(u)
        xn = V1.tabulate_dof_coordinates()
        from femasm import geometry

        c, X = geometry.locate_points(m, xn)
        assert (c >= 0).all()
        vmag = host_reference(V2, u.x.cpu(), c.cpu().numpy().astype(np.int64), X.cpu())[2]
        err = np.abs((u1.x - u.x).cpu().numpy().reshape(-1, gd))
        assert (err <= 1e-12 * vmag).all(), (err / vmag).max()
        # P2 on m -> P2 on refine(m), and the L2 distance of the two through the quadrature points
        Vr = fem.functionspace(fine, ("Lagrange", 2, (gd,)))
        ur = fem.Function(Vr)
        ur.interpolate(u)
        xq = fem.quadrature_points(Vr, 4)
        g = fem.eval_points(u, xq.reshape(-1, gd)).reshape(xq.shape).contiguous()
        assert torch.isfinite(g).all()
        d2 = float(fem.assemble_scalar(fem.L2Norm2(ur, g=g)))
        n2 = float(fem.assemble_scalar(fem.L2Norm2(ur)))
        print(f"{ct.name}: |u_ref - u|^2 / |u|^2 = {d2 / n2:.3e}")
        assert 0.0 <= d2 <= 1e-24 * n2


def check_missing_and_dg0(device):
    from femasm import fem, mesh

    src = mesh.create_unit_square(4, 4)
    tgt = mesh.create_unit_square(5, 5)
    tgt.x = tgt.x * 1.2
    if device is not None:
        src, tgt = src.to(device), tgt.to(device)
    Vs, Vt = fem.functionspace(src, ("Lagrange", 2, (1,))), fem.functionspace(tgt, ("Lagrange", 1, (1,)))
    u = fem.Function(Vs)
    u.interpolate(lambda x: (1.0 + x[0] + 2.0 * x[1] * x[1])[None])
    xt = Vt.tabulate_dof_coordinates()
    out = ((xt > 1.0 + 1e-9).any(1))
    assert 0 < int(out.sum()) < xt.shape[0]
    exact = 1.0 + xt[:, 0] + 2.0 * xt[:, 1] ** 2
    t = fem.Function(Vt)
    with pytest.raises(ValueError, match=f"{int(out.sum())} of {xt.shape[0]}"):
        t.interpolate(u)
    t.x = torch.full_like(t.x, 7.0)
    t.interpolate(u, missing="keep")
    assert (t.x[out] == 7.0).all() and torch.allclose(t.x[~out], exact[~out], rtol=1e-13)
    t.interpolate(u, missing="nan")
    assert torch.isnan(t.x[out]).all() and torch.allclose(t.x[~out], exact[~out], rtol=1e-13)
    with pytest.raises(ValueError):
        t.interpolate(u, missing="zero")
    # DG0 source: the cell's value; DG0 target: the source at the cell midpoints
    D = fem.functionspace(src, ("DG", 0))
    d = fem.Function(D)
    d.x = torch.arange(src.num_cells, dtype=torch.float64, device=src.device)
    xq, cells, _ = interior_queries(src if device is None else src.to("cpu"), 1)
    got = fem.eval_points(d, torch.tensor(xq, device=src.device))
    assert torch.equal(got[:, 0].cpu(), torch.tensor(cells, dtype=torch.float64))
    with pytest.raises(ValueError):
        fem.eval_points(d, torch.tensor(xq, device=src.device), grad=True)
    Dt = fem.functionspace(tgt, ("DG", 0))
    dt = fem.Function(Dt)
    dt.interpolate(u, missing="nan")
    mid = tgt.x[tgt.cells.to(torch.int64)].mean(1)
    inside = (mid <= 1.0).all(1)
    assert torch.allclose(dt.x[inside], 1.0 + mid[inside, 0] + 2.0 * mid[inside, 1] ** 2, rtol=1e-13)
    assert torch.isnan(dt.x[~inside]).all() and int((~inside).sum()) > 0
