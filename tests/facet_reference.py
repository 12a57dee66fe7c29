"""Independent reference for the exterior-facet load  b[a, i] = sum_F int_F (t_i - p n_i) phi_a dS.

Nothing here comes from the library's element tables or from its torch definition: the Lagrange basis is
the inverse of the Vandermonde matrix on ``fem.reference_nodes``, the rules are
``numpy.polynomial.legendre.leggauss`` with p + 2 points per direction (Duffy-collapsed on triangle faces),
and normals and surface elements are explicit edge and face cross products of the physical vertices,
oriented away from the cell's centroid (a bilinear hexahedron face: the cross product of its two tangents
at every point). Dense loops over facets, for the small meshes of the tests only."""
import itertools

import numpy as np

from femasm import fem, mesh
from femasm.mesh import CellType


def _exponents(ct, p):
    td = mesh.GDIM[CellType(ct)]
    full = itertools.product(range(p + 1), repeat=td)
    return np.array([e for e in full if not fem.is_simplex(ct) or sum(e) <= p])


def _monomials(ex, X):
    # in 2 X - 1: centred on the cell, which keeps the Vandermonde matrix well conditioned (Q3 hexahedron:
    # condition number ~1e3, against ~1e7 for monomials in X)
    return np.prod((2.0 * X[:, None, :] - 1.0) ** ex[None, :, :], axis=2)  # [n, nmono]


class Basis:
    """Degree-p Lagrange basis on fem.reference_nodes(ct, p): phi(X) = monomials(X) @ inv(Vandermonde)."""

    def __init__(self, ct, p):
        self.ex = _exponents(ct, p)
        nodes = fem.reference_nodes(ct, p)
        assert nodes.shape[0] == self.ex.shape[0]
        self.C = np.linalg.inv(_monomials(self.ex, nodes))

    def __call__(self, X):
        return _monomials(self.ex, X) @ self.C  # [n, nn]


def _gauss(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def facet_rule(ct, n):
    """Parameters [nq, tdim - 1] and weights of the reference facet: [0, 1], the unit square, or the unit
    triangle (Duffy: (u (1 - v), v) with weight (1 - v))."""
    x, w = _gauss(n)
    ct = CellType(ct)
    if mesh.GDIM[ct] == 2:
        return x[:, None], w
    uv = np.array([[a, b] for a in x for b in x])
    ww = np.array([a * b for a in w for b in w])
    if ct == CellType.hexahedron:
        return uv, ww
    return np.stack([uv[:, 0] * (1.0 - uv[:, 1]), uv[:, 1]], 1), ww * (1.0 - uv[:, 1])


def reference_load(V, facets, t_const=None, t_facet=None, t_nodal=None, p_const=None, p_facet=None, p_nodal=None,
                   npts=None):
    """The load vector [num_dofs] (numpy) of the facets (ids of mesh.entities(m, tdim - 1)); per-facet values
    are in the order of ``facets``."""
    m = V.mesh
    ct, p, gd = CellType(m.cell_type), V.degree, m.gdim
    x = m.x.cpu().numpy()
    cells = m.cells.cpu().numpy().astype(np.int64)
    dm = V.dofmap.cpu().numpy().astype(np.int64)
    fverts = mesh.entities(m, m.tdim - 1)[0].cpu().numpy()
    RV = np.array(mesh.REF_VERTS[ct], dtype=np.float64)
    subs = mesh.sub_entities(ct, m.tdim - 1)
    where = {}
    for c in range(cells.shape[0]):
        for lf, S in enumerate(subs):
            where.setdefault(tuple(sorted(cells[c, list(S)])), []).append((c, lf))
    basis = Basis(ct, p)
    prm, w = facet_rule(ct, npts or p + 2)
    tn = None if t_nodal is None else np.asarray(t_nodal).reshape(-1, gd)
    b = np.zeros((V.num_nodes, gd))
    for k, f in enumerate(np.asarray(facets).astype(np.int64)):
        (c, lf), = where[tuple(fverts[f])]
        S = list(subs[lf])
        P = x[cells[c, S]]  # the facet's physical vertices, in the local facet's order
        cen = x[cells[c]].mean(0)
        R = RV[S]
        if gd == 2:
            X = R[0] + prm[:, [0]] * (R[1] - R[0])
            xq = P[0] + prm[:, [0]] * (P[1] - P[0])
            e = P[1] - P[0]
            nds = np.tile(np.array([e[1], -e[0]]), (len(w), 1))
        elif ct == CellType.tetrahedron:
            X = R[0] + prm[:, [0]] * (R[1] - R[0]) + prm[:, [1]] * (R[2] - R[0])
            xq = P[0] + prm[:, [0]] * (P[1] - P[0]) + prm[:, [1]] * (P[2] - P[0])
            nds = np.tile(np.cross(P[1] - P[0], P[2] - P[0]), (len(w), 1))
        else:
            s, t = prm[:, [0]], prm[:, [1]]
            X = R[0] + s * (R[1] - R[0]) + t * (R[2] - R[0])
            xq = (1 - s) * (1 - t) * P[0] + s * (1 - t) * P[1] + (1 - s) * t * P[2] + s * t * P[3]
            nds = np.cross((1 - t) * (P[1] - P[0]) + t * (P[3] - P[2]), (1 - s) * (P[2] - P[0]) + s * (P[3] - P[1]))
        out = np.sign(np.einsum("qi,qi->q", nds, xq - cen))
        assert np.all(out != 0.0)
        nds = nds * out[:, None]
        dS = np.linalg.norm(nds, axis=1)
        phi = basis(X)  # [nq, nn]
        tq = np.zeros((len(w), gd))
        if t_const is not None:
            tq = tq + np.asarray(t_const)[None, :]
        if t_facet is not None:
            tq = tq + np.asarray(t_facet)[k][None, :]
        if tn is not None:
            tq = tq + phi @ tn[dm[c]]
        pq = np.zeros(len(w))
        if p_const is not None:
            pq = pq + float(p_const)
        if p_facet is not None:
            pq = pq + float(np.asarray(p_facet)[k])
        if p_nodal is not None:
            pq = pq + phi @ np.asarray(p_nodal)[dm[c]]
        g = tq * dS[:, None] - pq[:, None] * nds  # [nq, gd]
        np.add.at(b, dm[c], np.einsum("q,qa,qi->ai", w, phi, g))
    return b.reshape(-1)


def facet_measure(m, facets):
    """Length (2-D) or area (triangles; 3-D) of each facet from its vertex coordinates."""
    x = m.x.cpu().numpy()
    fv = mesh.entities(m, m.tdim - 1)[0].cpu().numpy()[np.asarray(facets).astype(np.int64)]
    if fv.shape[1] == 2:
        return np.linalg.norm(x[fv[:, 1]] - x[fv[:, 0]], axis=1)
    assert fv.shape[1] == 3
    return 0.5 * np.linalg.norm(np.cross(x[fv[:, 1]] - x[fv[:, 0]], x[fv[:, 2]] - x[fv[:, 0]]), axis=1)
