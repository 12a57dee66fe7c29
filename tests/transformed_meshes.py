"""Rotated, mirrored, scaled, sheared, stretched and shifted copies of the small structured meshes, and
the covariance maps of isotropic elasticity (test infrastructure; never imported by the product package).

Every other mesh of the suite sits in the unit square or cube with its cells along the axes (or is an
order-one Gmsh / Delaunay fixture). Here the vertices of a family's mesh go through

    x' = s x G^T + T        (x rows; G a matrix, s a scalar, T one number added on every axis)

before the function space is built, so the cells keep their connectivity, their numbering and their
lattice dofmap while the Jacobian becomes full (rot, shear), changes sign (mirror), changes size (scale,
stretch) or is formed from large coordinates (shift).

Covariance. With G = Q orthogonal and u'(x') = s Q u(x), isotropic elasticity (linear, neo-Hookean, and
the damage law away from its zero-shear branch) obeys, with d the dimension,

    blocks    K'_ab = s^(d-2) Q K_ab Q^T          vectors   r'_a = s^(d-1) Q r_a
    tensors   grad u, strain, stress -> Q (.) Q^T  energy density unchanged

(grad u' = Q grad u Q^T because u' and x' carry the same s). No oracle enters these maps.

affinise / affine_deviation are the CPU model of the affine tensor route: the first replaces every cell
by the parallelepiped of its three edges at vertex 0 (what MAT_AFFT assembles), the second restates
k_check_affine's dev / h.
"""
from __future__ import annotations

import numpy as np
import torch

TRI, QUAD, TET, HEX = 3, 4, -4, 8
_GDIM = {TRI: 2, QUAD: 2, TET: 3, HEX: 3}

# name -> (cell type, degree, cells per axis, perturbation of the interior vertices in units of h)
FAMILIES = {
    "tri-P1": (TRI, 1, (4, 3), 0.0), "tri-P2": (TRI, 2, (3, 2), 0.0),
    "tet-P1": (TET, 1, (2, 3, 2), 0.0), "tet-P2": (TET, 2, (2, 2, 2), 0.0),
    "quad-Q1": (QUAD, 1, (4, 3), 0.0), "quad-Q2": (QUAD, 2, (3, 3), 0.0), "quad-Q3": (QUAD, 3, (2, 2), 0.0),
    "hex-Q1": (HEX, 1, (3, 2, 2), 0.0), "hex-Q2": (HEX, 2, (2, 2, 2), 0.0), "hex-Q3": (HEX, 3, (2, 1, 2), 0.0),
    "quad-Q2-warp": (QUAD, 2, (3, 3), 0.3), "hex-Q1-warp": (HEX, 1, (3, 2, 2), 0.3),
    "hex-Q2-warp": (HEX, 2, (2, 2, 2), 0.3), "hex-Q3-warp": (HEX, 3, (2, 2, 2), 0.3),
}
SIMPLEX = [k for k, v in FAMILIES.items() if v[0] in (TRI, TET)]
AFFINE_TENSOR = [k for k, v in FAMILIES.items() if v[0] in (QUAD, HEX) and v[3] == 0.0]
WARPED = [k for k, v in FAMILIES.items() if v[3] != 0.0]


def gdim(family: str) -> int:
    return _GDIM[FAMILIES[family][0]]


def is_affine(family: str) -> bool:
    return FAMILIES[family][3] == 0.0


def base_mesh(family: str, device=None):
    """The untransformed mesh of a family (interior vertices of the warped variants moved by
    perturb * h * (rand - 0.5), seeded as in tests/test_gpu_parity._mesh)."""
    from femasm import mesh

    ct, _, n, perturb = FAMILIES[family]
    m = mesh.create_unit_square(*n, cell_type=ct) if len(n) == 2 else mesh.create_unit_cube(*n, cell_type=ct)
    if perturb:
        g = torch.Generator().manual_seed(3)
        x = m.x.clone()
        interior = ((x > 1e-9) & (x < 1 - 1e-9)).all(1)
        h = 1.0 / max(n)
        x[interior] += perturb * h * (torch.rand(x[interior].shape, generator=g, dtype=torch.float64) - 0.5)
        m.x = x
    return m.to(device) if device is not None else m


# ------------------------------------------------------------------------------------------- transforms
def rotation(gd: int) -> np.ndarray:
    """The fixed generic rotation: angle 0.7 in 2-D, Rz(0.7) Ry(-0.4) Rx(1.1) in 3-D (no entry is zero)."""
    def c_s(t):
        return np.cos(t), np.sin(t)

    c, s = c_s(0.7)
    if gd == 2:
        return np.array([[c, -s], [s, c]])
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    c, s = c_s(-0.4)
    Ry = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    c, s = c_s(1.1)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    return Rz @ Ry @ Rx


def mirror(gd: int) -> np.ndarray:
    return np.diag([-1.0] + [1.0] * (gd - 1))


def shear(gd: int) -> np.ndarray:
    G = np.eye(gd)
    G[0, 1] = 0.3
    if gd == 3:
        G[0, 2], G[1, 2] = 0.2, 0.1
    return G


def stretch(gd: int) -> np.ndarray:
    return np.diag([1.0, 1.0 / 16.0, 16.0][:gd])


# name -> (s, G(gd), T, orthogonal)
TRANSFORMS = {
    "rot": (1.0, rotation, 0.0, True),
    "mirror": (1.0, mirror, 0.0, True),
    "rotmirror": (1.0, lambda gd: rotation(gd) @ mirror(gd), 0.0, True),
    "scale-down": (2.0 ** -10, rotation, 0.0, True),
    "scale-up": (2.0 ** 10, rotation, 0.0, True),
    "shear": (1.0, shear, 0.0, False),
    "stretch": (1.0, stretch, 0.0, False),
    "shift1e3": (1.0, rotation, 1e3, True),
    "shift1e4": (1.0, rotation, 1e4, True),
}
ORTHOGONAL = ["rot", "mirror", "rotmirror", "scale-down", "scale-up"]  # the covariance checks' transforms
PARITY = ORTHOGONAL + ["shear", "stretch"]                              # the oracle-parity transforms
SHIFTS = ["shift1e3", "shift1e4"]


def transform(name: str, gd: int):
    """(s, G [gd, gd], T) of a named transform."""
    s, G, T, _ = TRANSFORMS[name]
    return s, G(gd), T


def apply_x(x: np.ndarray, name: str) -> np.ndarray:
    s, G, T = transform(name, x.shape[1])
    return s * (x @ G.T) + T


def apply(m, name: str):
    """A new mesh: the cells, tags and lattice of m with x' = s x G^T + T."""
    from femasm import mesh

    x = torch.tensor(apply_x(m.x.cpu().numpy(), name), dtype=torch.float64, device=m.device).contiguous()
    return mesh.Mesh(m.cell_type, x, m.cells, m.cell_tags, m.structured)


# ------------------------------------------------------------------------------------------- covariance
def map_blocks(K: np.ndarray, s: float, Q: np.ndarray) -> np.ndarray:
    """BSR blocks [nb, d, d] -> s^(d-2) Q K Q^T."""
    d = Q.shape[0]
    return s ** (d - 2) * np.einsum("ij,bjk,lk->bil", Q, K, Q)


def map_vector(v: np.ndarray, s: float, Q: np.ndarray, power: int | None = None) -> np.ndarray:
    """Nodal vector [nnodes * d] -> s^power Q v per node (power: d - 1 for forces, the default; 1 for
    displacements; 0 for a plain rotation)."""
    d = Q.shape[0]
    power = d - 1 if power is None else power
    return (s ** power * (v.reshape(-1, d) @ Q.T)).reshape(-1)


def map_tensor(t: np.ndarray, Q: np.ndarray) -> np.ndarray:
    """[..., d, d] -> Q t Q^T."""
    return np.einsum("ij,...jk,lk->...il", Q, t, Q)


# ------------------------------------------------------------------------------------------- affine route
def affinise(x: np.ndarray, geom: np.ndarray):
    """Every tensor cell replaced by the parallelepiped of its edges from vertex 0 to vertices 1, 2 (and
    4): x_v = x_0 + sum_k bit_k(v) (x_{2^k} - x_0), on a disjoint geometry (one vertex set per cell).
    Returns (x [nc * nv, gd], geom [nc, nv])."""
    nc, nv = geom.shape
    gd = x.shape[1]
    X = x[geom.astype(np.int64)]  # [nc, nv, gd]
    out = np.empty_like(X)
    for v in range(nv):
        p = X[:, 0].copy()
        for k in range(gd):
            if (v >> k) & 1:
                p = p + (X[:, 1 << k] - X[:, 0])
        out[:, v] = p
    return out.reshape(nc * nv, gd), np.arange(nc * nv, dtype=np.int32).reshape(nc, nv)


def affine_deviation(x: np.ndarray, geom: np.ndarray) -> np.ndarray:
    """k_check_affine in numpy, per cell: dev / h with dev = max_{v,i} |x_v - predicted|_i, the prediction
    accumulated edge by edge in the kernel's order, and h = max_{v,i} |x_v - x_0|_i. The plan calls a mesh
    affine when no cell is over the kernel's threshold."""
    nv = geom.shape[1]
    gd = x.shape[1]
    X = x[geom.astype(np.int64)]
    dev = np.zeros(geom.shape[0])
    h = np.zeros(geom.shape[0])
    for v in range(1, nv):
        pred = X[:, 0].copy()
        for k in range(gd):
            if (v >> k) & 1:
                pred = pred + (X[:, 1 << k] - X[:, 0])
        dev = np.maximum(dev, np.abs(X[:, v] - pred).max(1))
        h = np.maximum(h, np.abs(X[:, v] - X[:, 0]).max(1))
    return dev / h


def nudge_vertex(m, delta: float):
    """The near-threshold meshes: the vertex shared by the most cells (the first of them: an interior
    vertex wherever the mesh has one; hex-Q3's 2 x 1 x 2 cells have none, there it is the centre of the
    face y = 0) of an affine tensor mesh moved by delta * h along (1, -1[, 1]) / sqrt(d), h = the lattice
    spacing 1 / max(n)."""
    from femasm import mesh

    x = m.x.cpu().clone()
    valence = np.bincount(m.cells.cpu().numpy().reshape(-1), minlength=x.shape[0])
    h = 1.0 / max(m.structured["n"])
    d = torch.tensor([1.0, -1.0, 1.0][:x.shape[1]], dtype=torch.float64) / np.sqrt(x.shape[1])
    x[int(valence.argmax())] += delta * h * d
    return mesh.Mesh(m.cell_type, x.to(m.device).contiguous(), m.cells, m.cell_tags, m.structured)


DELTAS = [1e-14, 1e-13, 5e-13, 1.5e-12, 5e-12]  # (1.5e-12: dev / h just under 1e-12 on hex-Q3)
NEAR_THRESHOLD = ["hex-Q1", "hex-Q2", "hex-Q3", "quad-Q2"]


# ------------------------------------------------------------------------------------------- problems
class Problem:
    """One family on the host: the untransformed mesh and space, the pattern, E = e_range()[cell % 200]
    with nu = 0.3, the Dirichlet set (all components on the face x0 = 0 of the UNtransformed mesh, by
    node index, so that it is the same set of dofs on every transformed copy) and the states, given at
    the untransformed node coordinates; `oracle` is the oracle module. Everything numpy."""

    def __init__(self, oracle, family: str):
        from femasm import fem

        self.oracle, self.family = oracle, family
        self.ct, self.p, self.n, _ = FAMILIES[family]
        self.gd = _GDIM[self.ct]
        self.m0 = m = base_mesh(family)
        self.V0 = V = fem.functionspace(m, ("Lagrange", self.p, (self.gd,)))
        self.dofmap = V.dofmap.numpy()
        self.geom = m.cells.numpy()
        self.x0 = m.x.numpy()
        self.num_nodes = V.num_nodes
        self.ip, self.ix = oracle.sparsity(self.dofmap, V.num_nodes)
        self.E = oracle.e_range()[np.arange(m.num_cells) % 200]
        self.lam, self.mu = oracle.lame(self.E, 0.3)
        self.xn = V.tabulate_dof_coordinates().numpy()
        self.left = np.nonzero(np.isclose(self.xn[:, 0], 0.0))[0]
        assert 0 < self.left.size < V.num_nodes
        self.marker = np.zeros((V.num_nodes, self.gd), dtype=np.int8)
        self.marker[self.left] = 1
        self.marker = self.marker.reshape(-1)

    # ---- coordinates and states
    def x(self, tr: str | None) -> np.ndarray:
        return self.x0 if tr is None else apply_x(self.x0, tr)

    def sQ(self, tr: str | None):
        if tr is None:
            return 1.0, np.eye(self.gd)
        s, G, _ = transform(tr, self.gd)
        return s, G

    def state(self, kind: str) -> np.ndarray:
        """u at the untransformed nodes. lin: seeded noise of amplitude 1e-3; neo: 0.05 sin(pi x);
        dam: the sheared state 1e-3 (sin(3x + 2y + .3), cos(2x - 3y + .1))."""
        xn = self.xn
        if kind == "lin":
            return 1e-3 * (np.random.default_rng(1).random(xn.size) - 0.5)
        if kind == "neo":
            return (0.05 * np.sin(np.pi * xn)).reshape(-1)
        assert kind == "dam" and self.gd == 2
        return 1e-3 * np.stack([np.sin(3 * xn[:, 0] + 2 * xn[:, 1] + 0.3),
                                np.cos(2 * xn[:, 0] - 3 * xn[:, 1] + 0.1)], 1).reshape(-1)

    def damage(self) -> np.ndarray:
        """Nodal damage: seeded, a third of the nodes undamaged."""
        d = np.random.default_rng(8).random(self.num_nodes)
        d[d < 0.35] = 0.0
        return d

    def body_force(self) -> np.ndarray:
        return 1e4 * (np.random.default_rng(2).random(self.xn.size) - 0.5)

    def moved(self, v: np.ndarray, tr: str | None, power: int) -> np.ndarray:
        s, Q = self.sQ(tr)
        return map_vector(v, s, Q, power)

    def diag(self, tr: str | None) -> float:
        """The Dirichlet diagonal that keeps constrained blocks covariant: s^(d-2) (a power of two)."""
        return self.sQ(tr)[0] ** (self.gd - 2)

    # ---- the oracle on a transformed copy (or on explicit coordinates / geometry)
    def matrix(self, kind: str, tr: str | None = None, bc: bool = True, diag: float | None = None, x=None, geom=None):
        """Oracle tangent of kind lin | neo | dam at the state moved with the mesh (u' = s Q u)."""
        o = self.oracle
        x = self.x(tr) if x is None else x
        geom = self.geom if geom is None else geom
        mk = self.marker if bc else None
        diag = self.diag(tr) if diag is None else diag
        if kind == "lin":
            out = o.assemble_elasticity(self.ct, self.p, self.dofmap, geom, x, self.lam, self.mu, self.ip, self.ix,
                                        bc=mk, diag=diag)
        elif kind == "neo":
            out = o.assemble_neohookean(self.ct, self.p, self.dofmap, geom, x, self.lam, self.mu,
                                        self.moved(self.state("neo"), tr, 1), self.ip, self.ix, bc=mk, diag=diag)
        else:
            out = o.assemble_damage(self.dofmap, geom, x, self.lam, self.mu, self.moved(self.state("dam"), tr, 1),
                                    self.damage(), self.ip, self.ix, bc=mk, diag=diag)
        assert np.isfinite(out).all()
        return out

    def residual(self, kind: str, tr: str | None = None):
        """Oracle residual at u' = s Q u with the body force f' = Q f / s (so that r' = s^(d-1) Q r)."""
        u = self.moved(self.state(kind), tr, 1)
        f = self.moved(self.body_force(), tr, -1)
        out = self.oracle.assemble_residual(self.ct, self.p, self.dofmap, self.geom, self.x(tr), self.lam, self.mu, u=u, f=f,
                                            d=self.damage() if kind == "dam" else None,
                                            kind={"lin": 0, "dam": 1, "neo": 2}[kind])
        assert np.isfinite(out).all()
        return out

    def shear_strain(self, tr: str | None = None) -> np.ndarray:
        """eps_xy per cell of the damage state on P1 triangles (constant per cell)."""
        assert self.ct == TRI and self.p == 1
        X = self.x(tr)[self.geom.astype(np.int64)]
        U = self.moved(self.state("dam"), tr, 1).reshape(-1, 2)[self.dofmap.astype(np.int64)]
        J = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]], 2)      # [c, i, k]
        dU = np.stack([U[:, 1] - U[:, 0], U[:, 2] - U[:, 0]], 2)     # [c, i, k]
        G = dU @ np.linalg.inv(J)
        return 0.5 * (G[:, 0, 1] + G[:, 1, 0])


def forms_of(family: str):
    """The laws a family is assembled with: the damage law is the reference's 2-D P1-triangle model."""
    return ("lin", "neo", "dam") if family == "tri-P1" else ("lin", "neo")


def vector_error(got: np.ndarray, ref: np.ndarray) -> float:
    return float(np.abs(got - ref).max() / np.abs(ref).max())
