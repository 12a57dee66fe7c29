"""Geometric multigrid preconditioner for the Newton-Krylov solve on the structured meshes.

The reference preconditions its Krylov solve with BoomerAMG (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:720-813,
MFEM/mechanic2d/asym_elasto_damage_model.cc:1502-1528); ``nls.KrylovSolver`` alone has block-Jacobi, whose
iteration count grows like 1/h. ``GeometricMultigrid`` needs no assembled fine matrix: level 0 is the
matrix-free ``fem.JacobianOperator`` (or any operator with ``mult`` / ``block_diagonal``), the coarser
levels are rediscretised and assembled (a degree-1 level is at most 1/8 of the fine dofs).

One stencil serves every transfer. With the lattice node numbering of the structured meshes the degree-2
nodes of an ``n`` mesh and the degree-1 nodes of a ``2n`` mesh are the same lattice, and the right-diagonal
triangle / Kuhn tetrahedron mesh of ``2n`` refines that of ``n``; so linear interpolation between a coarse
lattice of ``nc + 1`` points per axis and the fine lattice of ``2 nc + 1`` points is both the P2 -> P1
transfer on one mesh (p-coarsening) and the P1(h) -> P1(2h) transfer (h-coarsening). A fine point ``I``
with odd mask ``o = I & 1`` takes, on simplices, half of each of the coarse points ``(I - o) / 2`` and
``(I + o) / 2`` (``o`` is always an edge direction of the mesh), and on tensor cells the mean of the
``2^|o|`` coarse points ``(I +- o) / 2``. ``fa_prolong`` / ``fa_restrict`` apply it (gathers, no atomics)
and ``fa_cheb_step`` is the fused Chebyshev / block-Jacobi smoother update (femasm_mg.hip).

Meshes without a lattice are served through ``mesh.refine``: it numbers the midpoint of edge ``e`` as
vertex ``nv + e``, the numbering of the degree-2 nodes (``fem._generic_dofmap``), so the P1 nodes of
``refine(m)`` are the P2 nodes of ``m`` and one edge stencil (an edge node takes half of each end vertex:
``EdgeTransfer``, ``fa_prolong_edges`` / ``fa_restrict_edges`` in femasm_refine.hip) is again both the
p- and the h-transfer. The hierarchy is the chain of ``mesh.parent`` (``plan_refined_hierarchy``);
everything from ``update()`` down is shared with the lattice path.

A mesh with neither a lattice nor parents is served by ``SmoothedAggregation``: below the degree-1 level its
levels are algebraic (``femasm.amg``: MIS(2) aggregates, rigid-body modes, a smoothed prolongator and Galerkin
products over ``fa_bcsr_product`` / ``fa_bcsr_mult`` in femasm_amg.hip). Smoother, eigenvalue estimate, coarse
solve and V-cycle are the same code (``_VCycle``).
"""
from __future__ import annotations

import ctypes
import itertools
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, amg, fem
from . import mesh as fmesh
from .mesh import CellType

# Chebyshev interval as fractions of the estimated largest eigenvalue of D^-1 A (PETSc's defaults for
# PCMG's Chebyshev smoother) and the steps of the eigenvalue estimate
CHEB_LOWER, CHEB_UPPER = 0.1, 1.1
EIG_STEPS = 10
COARSE_CHEB_DEGREE = 8  # the fixed polynomial standing in for a solve on a coarsest level too large to factor

# local cube vertices (v = i + 2 j + 4 k) of the sub-simplices of a lattice square / cube, in the cell
# order of mesh.create_rectangle(diagonal="right") and mesh.create_box
_SUB_SIMPLICES = {CellType.triangle: ((0, 1, 3), (0, 2, 3)), CellType.tetrahedron: fmesh.KUHN_TETS}


@dataclass(frozen=True)
class Transfer:
    """Coarse lattice of ``nc[d] + 1`` points per axis <-> fine lattice of ``2 nc[d] + 1`` points
    (fa_transfer); dof = node * bs + comp."""
    tdim: int
    simplex: bool
    bs: int
    nc: tuple

    @property
    def coarse_points(self) -> tuple:
        return tuple(int(k) + 1 for k in self.nc)

    @property
    def fine_points(self) -> tuple:
        return tuple(2 * int(k) + 1 for k in self.nc)

    @property
    def num_coarse_dofs(self) -> int:
        return int(np.prod(self.coarse_points)) * self.bs

    @property
    def num_fine_dofs(self) -> int:
        return int(np.prod(self.fine_points)) * self.bs

    def _fa(self) -> _lib.fa_transfer:
        t = _lib.fa_transfer()
        t.tdim, t.simplex, t.bs = self.tdim, int(self.simplex), self.bs
        for d in range(3):
            t.nc[d] = int(self.nc[d]) if d < self.tdim else 0
        return t


class EdgeTransfer:
    """``ncoarse`` coarse nodes <-> ``ncoarse + nedges`` fine nodes, fine node ``ncoarse + e`` sitting on
    edge ``e`` of ``edge_verts`` [nedges, 2] (fa_edge_transfer); dof = node * bs + comp. With the edges of
    ``mesh.entities(m, 1)`` this is the P2 -> P1 transfer on ``m`` and the P1 transfer between
    ``mesh.refine(m)`` and ``m``. The edge-to-vertex CSR of the restriction (each coarse node's edges in
    ascending order) is built here, once, on the device of ``edge_verts``."""

    def __init__(self, edge_verts: torch.Tensor, ncoarse: int, bs: int):
        ev = torch.as_tensor(edge_verts)
        if ev.dim() != 2 or ev.shape[1] != 2 or ev.is_floating_point():
            raise ValueError("edge_verts must be an integer tensor [nedges, 2]")
        if not 1 <= int(bs) <= 3:
            raise ValueError(f"block size {bs} (1 to 3)")
        self.ncoarse, self.nedges, self.bs = int(ncoarse), int(ev.shape[0]), int(bs)
        if self.ncoarse < 0 or self.ncoarse + self.nedges > 2 ** 31 - 1:
            raise ValueError("the node count must be non-negative and fit int32")
        if self.nedges and (int(ev.min()) < 0 or int(ev.max()) >= self.ncoarse):
            raise ValueError(f"edge_verts must name coarse nodes 0 .. {self.ncoarse - 1}")
        self.edge_verts = ev.to(torch.int32).contiguous()
        flat = ev.reshape(-1).to(torch.int64)  # entry i belongs to edge i // 2
        order = torch.sort(flat, stable=True).indices  # stable: a node's edges stay in ascending order
        self.vedges = torch.div(order, 2, rounding_mode="floor").to(torch.int32).contiguous()
        self.vptr = torch.zeros(self.ncoarse + 1, dtype=torch.int64, device=ev.device)
        self.vptr[1:] = torch.cumsum(torch.bincount(flat, minlength=self.ncoarse), 0)
        fa = _lib.fa_edge_transfer()
        fa.ncoarse, fa.nedges, fa.bs = self.ncoarse, self.nedges, self.bs
        fa.edge_verts, fa.vptr, fa.vedges = self.edge_verts.data_ptr(), self.vptr.data_ptr(), self.vedges.data_ptr()
        self._desc = fa

    @property
    def num_coarse_dofs(self) -> int:
        return self.ncoarse * self.bs

    @property
    def num_fine_dofs(self) -> int:
        return (self.ncoarse + self.nedges) * self.bs

    def _fa(self) -> _lib.fa_edge_transfer:
        return self._desc


def edge_transfer_matrix(t: EdgeTransfer):
    """The prolongation P [fine dofs, coarse dofs] of an edge transfer as a scipy CSR matrix (host; tests
    and debugging): the identity on the first ``ncoarse`` nodes, 1/2 and 1/2 on an edge node."""
    import scipy.sparse as sp

    ev = t.edge_verts.cpu().numpy().astype(np.int64)
    nc, ne = t.ncoarse, t.nedges
    rows = np.concatenate([np.arange(nc), nc + np.arange(ne), nc + np.arange(ne)])
    cols = np.concatenate([np.arange(nc), ev[:, 0], ev[:, 1]])
    vals = np.concatenate([np.ones(nc), np.full(2 * ne, 0.5)])
    P = sp.coo_matrix((vals, (rows, cols)), shape=(nc + ne, nc)).tocsr()
    P.sum_duplicates()
    return sp.kron(P, sp.identity(t.bs), format="csr") if t.bs > 1 else P


def _lattice_index(points, dims):
    """Node index of lattice points [..., tdim] (index 0 fastest)."""
    idx = points[..., len(dims) - 1]
    for d in range(len(dims) - 2, -1, -1):
        idx = idx * dims[d] + points[..., d]
    return idx


def transfer_matrix(t: Transfer):
    """The prolongation P [fine dofs, coarse dofs] of ``t`` as a scipy CSR matrix (host; tests and
    debugging): ``P[i_f, i_c]`` = the coarse P1 / Q1 basis function ``i_c`` at fine node ``i_f``."""
    import scipy.sparse as sp

    pf, pc = t.fine_points, t.coarse_points
    grids = np.meshgrid(*[np.arange(k) for k in reversed(pf)], indexing="ij")
    I = np.stack([g.reshape(-1) for g in reversed(grids)], 1)  # [nf, tdim], index 0 fastest
    o = I & 1
    a = (I - o) // 2
    nf = I.shape[0]
    rows, cols, vals = [], [], []
    # each odd axis splits the weight over its two coarse neighbours; an even axis sends both halves to
    # the same point (duplicates are summed). Simplices move along the whole vector o at once.
    combos = [(0,) * t.tdim, (1,) * t.tdim] if t.simplex else list(itertools.product((0, 1), repeat=t.tdim))
    for s in combos:
        rows.append(np.arange(nf))
        cols.append(_lattice_index(a + np.array(s) * o, pc))
        vals.append(np.full(nf, 1.0 / len(combos)))
    P = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                      shape=(nf, int(np.prod(pc)))).tocsr()
    P.sum_duplicates()
    return sp.kron(P, sp.identity(t.bs), format="csr") if t.bs > 1 else P


def injection_nodes(t: Transfer, device=None) -> torch.Tensor:
    """Fine node index of every coarse node (coarse point I coincides with fine point 2 I), int64."""
    pc, pf = t.coarse_points, t.fine_points
    axes = [torch.arange(k, device=device, dtype=torch.int64) for k in reversed(pc)]
    grids = torch.meshgrid(*axes, indexing="ij")
    I = torch.stack([g.reshape(-1) for g in reversed(grids)], 1)
    return _lattice_index(2 * I, pf)


def coarsen_marker(marker: torch.Tensor | None, t: Transfer) -> torch.Tensor | None:
    """Constraint marker of the coarse level: a coarse node is constrained in the components in which
    its coinciding fine node is."""
    if marker is None:
        return None
    return marker.view(-1, t.bs)[injection_nodes(t, marker.device)].reshape(-1).contiguous()


def parent_cells(cell_type, nc, device=None) -> torch.Tensor:
    """Parent (coarse) cell of every cell of the structured ``2 nc`` mesh in the ``nc`` mesh, int64
    [fine cells], with the cell numbering of mesh.create_rectangle(diagonal="right") / create_box. The
    fine cell's centroid in coarse lattice units gives the coarse square / cube (floor) and, on
    simplices, the sub-simplex (the order of its local coordinates)."""
    ct = CellType(cell_type)
    nc = tuple(int(k) for k in nc)
    tdim = len(nc)
    subs = _SUB_SIMPLICES.get(ct)
    m = len(subs) if subs else 1
    nf = tuple(2 * k for k in nc)
    axes = [torch.arange(k, device=device, dtype=torch.int64) for k in reversed(nf)]
    grids = torch.meshgrid(*axes, indexing="ij")
    sq = torch.stack([g.reshape(-1) for g in reversed(grids)], 1)  # fine squares, index 0 fastest
    csq = _lattice_index(torch.div(sq, 2, rounding_mode="floor"), nc)  # coarse square of each fine one
    if subs is None:
        return csq
    bits = lambda v: [(v >> d) & 1 for d in range(tdim)]
    # centroid of each fine sub-simplex in fine lattice units, relative to its square
    cref = torch.tensor([[sum(bits(v)[d] for v in s) / len(s) for d in range(tdim)] for s in subs],
                        dtype=torch.float64, device=device)
    xi = (sq[:, None, :].to(torch.float64) + cref[None, :, :]) / 2.0
    xi = xi - torch.floor(xi)  # local coordinates in the coarse square [nsq, m, tdim]
    # sub-simplex s is the region xi[a1] >= xi[a2] (>= xi[a3]), a_k = the axis its k-th edge of the path
    # from vertex 0 to the far corner runs along; key = the axes in descending order of xi
    table = torch.zeros(tdim ** tdim, dtype=torch.int64, device=device)
    for s, verts in enumerate(subs):
        path = sorted(verts, key=lambda v: bin(v).count("1"))
        order = [(path[k + 1] ^ path[k]).bit_length() - 1 for k in range(tdim)]
        table[sum(a * tdim ** (tdim - 1 - k) for k, a in enumerate(order))] = s
    order = torch.argsort(xi, dim=-1, descending=True, stable=True)
    key = sum(order[..., k] * tdim ** (tdim - 1 - k) for k in range(tdim))
    return (csq[:, None] * m + table[key]).reshape(-1)


def plan_hierarchy(V: fem.FunctionSpace, coarse_dofs: int = 6000, max_levels: int | None = None) -> list:
    """Level table [(degree, n), ...] of a space on a structured mesh: the space itself, degree 1 on the
    same mesh if it has degree 2, then every ``n`` halved while all are even and >= 2, until a level has
    at most ``coarse_dofs`` dofs or ``max_levels`` levels exist. ValueError for the spaces geometric
    multigrid cannot serve."""
    m = V.mesh
    st = m.structured
    if st is None:
        raise ValueError("GeometricMultigrid needs a structured mesh (mesh.create_rectangle / create_box): "
                         "unstructured meshes have no lattice to coarsen")
    n = tuple(int(k) for k in st["n"])
    if st.get("z_range") is not None and tuple(st["z_range"]) != (0, n[-1]):
        raise ValueError(f"GeometricMultigrid needs the whole box, not the z_range={tuple(st['z_range'])} slab")
    if m.cell_type == CellType.triangle and st.get("diagonal", "right") != "right":
        raise ValueError("GeometricMultigrid needs diagonal='right' triangles: the 'left' mesh of 2n does not "
                         "refine that of n along the lattice stencil")
    if V.family in ("DG", "Discontinuous Lagrange") or V.degree not in (1, 2):
        raise ValueError(f"GeometricMultigrid serves Lagrange degree 1 and 2, not {V.family} degree {V.degree} "
                         "(the degree-3 GLL nodes are not nested in a finer lattice)")
    if max_levels is not None and max_levels < 1:
        raise ValueError("max_levels must be at least 1")
    ndofs = lambda p, k: int(np.prod([p * j + 1 for j in k])) * V.bs
    levels = [(V.degree, n)]
    while (max_levels is None or len(levels) < max_levels) and ndofs(*levels[-1]) > coarse_dofs:
        p, k = levels[-1]
        if p == 2:
            levels.append((1, k))
        elif all(j % 2 == 0 and j >= 2 for j in k):
            levels.append((1, tuple(j // 2 for j in k)))
        else:
            break
    if len(levels) == 1 and (max_levels is None or max_levels > 1) and ndofs(*levels[0]) > coarse_dofs:
        raise ValueError(f"a degree-1 space on n={n} has no coarser level (every n must be even and >= 2) and "
                         f"its {ndofs(1, n)} dofs exceed coarse_dofs={coarse_dofs}")
    return levels


def plan_refined_hierarchy(V: fem.FunctionSpace, coarse_dofs: int = 6000, max_levels: int | None = None) -> list:
    """Level table [(degree, mesh), ...] of a space on an unstructured simplex mesh: the space itself,
    degree 1 on the same mesh if it has degree 2, then degree 1 on every ``mesh.parent`` (the chain
    ``mesh.refine`` leaves behind), until a level has at most ``coarse_dofs`` dofs, ``max_levels`` levels
    exist or the chain ends. ValueError for the spaces geometric multigrid cannot serve."""
    m = V.mesh
    if m.structured is not None:
        raise ValueError("plan_refined_hierarchy serves meshes without a lattice; a structured mesh goes "
                         "through plan_hierarchy")
    if not fem.is_simplex(m.cell_type):
        raise ValueError(f"GeometricMultigrid on an unstructured mesh needs triangles or tetrahedra, not "
                         f"{CellType(m.cell_type).name} cells (mesh.refine serves simplices)")
    if V.family in ("DG", "Discontinuous Lagrange") or V.degree not in (1, 2):
        raise ValueError(f"GeometricMultigrid serves Lagrange degree 1 and 2, not {V.family} degree {V.degree}")
    if max_levels is not None and max_levels < 1:
        raise ValueError("max_levels must be at least 1")
    ndofs = lambda p, k: (k.num_vertices + (int(fmesh.entities(k, 1)[0].shape[0]) if p == 2 else 0)) * V.bs
    levels = [(V.degree, m)]
    while (max_levels is None or len(levels) < max_levels) and ndofs(*levels[-1]) > coarse_dofs:
        p, k = levels[-1]
        if p == 2:
            levels.append((1, k))
        elif k.parent is not None:
            levels.append((1, k.parent))
        else:
            break
    if len(levels) == 1 and (max_levels is None or max_levels > 1) and ndofs(*levels[0]) > coarse_dofs:
        raise ValueError(f"GeometricMultigrid needs a structured mesh (mesh.create_rectangle / create_box) or a "
                         f"mesh made by mesh.refine: this degree-1 space has no parent mesh to coarsen to and its "
                         f"{ndofs(1, m)} dofs exceed coarse_dofs={coarse_dofs}")
    return levels


class _Level:
    pass


def _transfer_call(name, t, *args):
    fa = t._fa()
    if isinstance(t, EdgeTransfer):
        name += "_edges"
    _lib.check(getattr(_lib.load(), name)(ctypes.byref(fa), *args), name)


def prolong(t, xc: torch.Tensor, xf: torch.Tensor, bc_c=None, bc_f=None, add: bool = False) -> torch.Tensor:
    """xf (+)= M_f P M_c xc (fa_prolong for a Transfer, fa_prolong_edges for an EdgeTransfer); markers
    int8 per dof or None."""
    _check_transfer_args(t, xc, xf, bc_c, bc_f)
    _transfer_call("fa_prolong", t, xc.data_ptr(), _lib.ptr(bc_c), _lib.ptr(bc_f), int(bool(add)), xf.data_ptr(),
                   _lib.stream_handle(xf.device))
    return xf


def restrict(t, rf: torch.Tensor, rc: torch.Tensor, bc_f=None, bc_c=None) -> torch.Tensor:
    """rc = M_c P^T M_f rf (fa_restrict / fa_restrict_edges); bit-reproducible."""
    _check_transfer_args(t, rc, rf, bc_c, bc_f)
    _transfer_call("fa_restrict", t, rf.data_ptr(), _lib.ptr(bc_f), _lib.ptr(bc_c), rc.data_ptr(),
                   _lib.stream_handle(rc.device))
    return rc


def _check_transfer_args(t, c, f, bc_c, bc_f):
    if isinstance(t, EdgeTransfer) and isinstance(f, torch.Tensor) and t.edge_verts.device != f.device:
        raise ValueError(f"the transfer's edge table is on {t.edge_verts.device}, the fine vector on {f.device}")
    for name, v, n, dt in (("coarse vector", c, t.num_coarse_dofs, torch.float64),
                           ("fine vector", f, t.num_fine_dofs, torch.float64),
                           ("coarse marker", bc_c, t.num_coarse_dofs, torch.int8),
                           ("fine marker", bc_f, t.num_fine_dofs, torch.int8)):
        if v is None and "marker" in name:
            continue
        if not isinstance(v, torch.Tensor) or v.dtype != dt or v.numel() != n or not v.is_contiguous():
            raise ValueError(f"the {name} must be a contiguous {dt} tensor of {n} entries")
        if v.device != f.device:
            raise ValueError(f"the {name} is on {v.device}, the fine vector on {f.device}")


def cheb_step(Dinv: torch.Tensor, b: torch.Tensor, Ax: torch.Tensor | None, c_d: float, c_r: float,
              d: torch.Tensor, x: torch.Tensor):
    """d <- c_d d + c_r Dinv (b - Ax), x <- x + d in one pass (fa_cheb_step). Dinv [nnodes, bs, bs];
    Ax None: A x = 0."""
    nn, bs = int(Dinv.shape[0]), int(Dinv.shape[1])
    for v in (b, Ax, d, x):
        if v is not None and (v.dtype != torch.float64 or v.numel() != nn * bs or not v.is_contiguous()
                              or v.device != Dinv.device):
            raise ValueError(f"fa_cheb_step vectors must be contiguous float64 of {nn * bs} entries on {Dinv.device}")
    if Dinv.dtype != torch.float64 or not Dinv.is_contiguous() or Dinv.shape[2] != bs:
        raise ValueError("Dinv must be a contiguous float64 [nnodes, bs, bs] tensor")
    if bs == 6:  # the 6-dof nodes of the algebraic levels in 3-D
        _lib.check(_lib.load().fa_cheb_step6(nn, Dinv.data_ptr(), b.data_ptr(), _lib.ptr(Ax), float(c_d), float(c_r),
                                             d.data_ptr(), x.data_ptr(), _lib.stream_handle(x.device)), "fa_cheb_step6")
        return
    _lib.check(_lib.load().fa_cheb_step(nn, bs, Dinv.data_ptr(), b.data_ptr(), _lib.ptr(Ax), float(c_d), float(c_r),
                                        d.data_ptr(), x.data_ptr(), _lib.stream_handle(x.device)), "fa_cheb_step")


def chebyshev_coefficients(lo: float, hi: float, degree: int) -> list:
    """(c_d, c_r) of each step of the Chebyshev iteration on [lo, hi] (Saad, Iterative Methods, alg. 12.1)."""
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    out = [(0.0, 1.0 / theta)]
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma - rho)
        out.append((rho_new * rho, 2.0 * rho_new / delta))
        rho = rho_new
    return out


class _VCycle:
    """What the multigrid preconditioners share: the level records, the rediscretised degree-1 level below
    a degree-2 space, the block-Jacobi / Chebyshev smoother with its eigenvalue estimate, the dense inverse
    of the coarsest level and the V-cycle. A level ``L`` has ``bs`` dofs per node, ``ndofs`` dofs, an
    operator ``A`` (``mult`` / ``block_diagonal``), a constraint ``marker`` or None, the scratch vectors
    ``r, z, d, t`` and, unless it is the last, the ``transfer`` to the next level."""

    def _init_common(self, a, bcs, diagonal, smoother_degree, coarse_dofs):
        if not isinstance(a, fem.LinearElasticity):
            raise TypeError("expected a femasm form descriptor (LinearElasticity, AsymDamage, ...)")
        if smoother_degree < 1:
            raise ValueError("smoother_degree must be at least 1")
        self.a, self.V = a, a.V
        self.bcs = list(bcs or [])
        self.diagonal = float(diagonal)
        self.smoother_degree = int(smoother_degree)
        self.coarse_dofs = int(coarse_dofs)
        self.updates = 0
        self._levels = []
        self._gen = torch.Generator(device=a.V.mesh.device)
        self._nnz0 = None

    def _fine_level(self, fine_operator):
        """Level 0: the form's own space with ``fine_operator`` or the matrix-free Jacobian."""
        L = _Level()
        V = self.V
        L.degree, L.n = V.degree, None
        L.V, L.a = V, self.a
        L.marker, _ = fem._combine_bcs(V, self.bcs, with_g=False)
        L.A = fine_operator if fine_operator is not None else \
            fem.JacobianOperator(self.a, bcs=self.bcs, diagonal=self.diagonal)
        L.kind = "matrix-free" if isinstance(L.A, fem.JacobianOperator) else "operator"
        return self._add_level(L, V.bs, V.num_dofs)

    def _geometric_level(self, F, n, refined: bool):
        """The assembled degree-1 level below level F: on the lattice ``n`` (``n == F.n``: F's own mesh,
        below a degree-2 level) or, refined, on the mesh ``n`` (F's own below degree 2, else its parent)."""
        L = _Level()
        m, dev, bs = self.V.mesh, self.V.mesh.device, self.V.bs
        st = m.structured
        L.degree, L.n = 1, (None if refined else n)
        if refined:
            # n is the level's mesh: the same one below a degree-2 level, else the parent. Either
            # way the fine nodes are the coarse mesh's vertices, then one per edge of it
            cm = n
            F.transfer = EdgeTransfer(fmesh.entities(cm, 1)[0], cm.num_vertices, bs)
            if F.transfer.num_fine_dofs != F.V.num_dofs:
                raise ValueError("the mesh's parent does not have the numbering of mesh.refine")
            F.inject = slice(0, cm.num_vertices)
            F.parents = None if cm is F.V.mesh else \
                torch.arange(F.V.mesh.num_cells, device=dev, dtype=torch.int64) >> m.tdim
            L.marker = None if F.marker is None else F.marker[:F.transfer.num_coarse_dofs].contiguous()
        else:
            if n == F.n:
                cm = F.V.mesh
            elif m.tdim == 2:
                cm = fmesh.create_rectangle(st["lengths"], n, m.cell_type, st.get("diagonal", "right"), dev)
            else:
                cm = fmesh.create_box(st["lengths"], n, m.cell_type, dev)
            F.transfer = Transfer(m.tdim, fem.is_simplex(m.cell_type), bs, n)
            F.inject = injection_nodes(F.transfer, dev)
            F.parents = None if n == F.n else parent_cells(m.cell_type, n, dev)
            L.marker = coarsen_marker(F.marker, F.transfer)
        L.V = fem.functionspace(cm, ("Lagrange", 1, (bs,)))
        self._coarse_form(F, L)
        L.A = fem.create_matrix(L.a)
        L.kind = "assembled"
        return self._add_level(L, bs, L.V.num_dofs)

    def _add_level(self, L, bs: int, ndofs: int):
        L.bs, L.ndofs = int(bs), int(ndofs)
        L.transfer = None
        dev = self.V.mesh.device
        L.r, L.z, L.d, L.t = (torch.zeros(L.ndofs, dtype=torch.float64, device=dev) for _ in range(4))
        L.Dinv = L.coef = L.Ainv = None
        self._levels.append(L)
        return L

    def _close_hierarchy(self):
        """The last level is inverted densely if it is small enough, else it gets the fixed polynomial."""
        last = self._levels[-1]
        last.direct = last.ndofs <= self.coarse_dofs
        if len(self._levels) > 1 or last.direct:
            last.kind = "direct" if last.direct else "chebyshev"
        mk = self._levels[0].marker
        self._free = None if mk is None else (mk == 0).to(torch.float64)
        # z = r / diagonal on the constrained dofs, + 0 (r / inf) on the free ones
        self._cdiv = None if mk is None else torch.where(mk != 0, self.diagonal, float("inf")).to(torch.float64)

    # ------------------------------------------------------------------------------ hierarchy
    def _coarse_form(self, F, L):
        """Rediscretise F.a on L.V with storage of its own for the coefficients and the state
        (update() refills it in place)."""
        a, t = F.a, F.transfer
        dev = L.V.mesh.device
        nc = L.V.mesh.num_cells
        same = F.parents is None
        L.cell = {}
        for k in ("E", "lam", "mu"):
            v = getattr(a, k)
            if v is not None:
                L.cell[k] = v if same else torch.empty(nc, dtype=torch.float64, device=dev)
        L.u = None if a.u is None else torch.zeros(t.num_coarse_dofs, dtype=torch.float64, device=dev)
        L.dmg = None if a.d is None else torch.zeros(t.num_coarse_dofs // t.bs, dtype=torch.float64, device=dev)
        kw = dict(nu=a.nu, u=L.u, **L.cell)
        if isinstance(a, fem.AsymDamage):
            L.a = fem.AsymDamage(L.V, d=L.dmg, tangent=a.tangent, **kw)
        elif isinstance(a, fem.NeoHookean):
            L.a = fem.NeoHookean(L.V, **kw)
        else:
            L.a = fem.LinearElasticity(L.V, **kw)
        if L.marker is not None and bool(L.marker.any()):
            dofs = torch.nonzero(L.marker, as_tuple=False).reshape(-1)
            L.bcs = [fem.DirichletBC(L.V, dofs, torch.zeros(L.V.num_dofs, dtype=torch.float64, device=dev))]
        else:
            L.bcs = None

    def _refill(self, F, L):
        """Coefficients (mean over the children) and state (injection) of level L from level F."""
        if F.parents is not None:
            children = float(2 ** self.V.mesh.tdim)
            for k, vc in L.cell.items():
                vc.zero_().index_add_(0, F.parents, getattr(F.a, k)).div_(children)
        bs = F.transfer.bs
        if L.u is not None:
            L.u.copy_(F.a.u.view(-1, bs)[F.inject].reshape(-1))
        if L.dmg is not None:
            L.dmg.copy_(F.a.d[F.inject])

    @property
    def levels(self) -> list:
        return [(L.degree, L.n, L.ndofs, L.kind) for L in self._levels]

    @property
    def operator_complexity(self) -> float:
        """Matrix entries of all levels (the level-0 matrix counted as if assembled) over those of the
        level-0 matrix. Builds level 0's sparsity pattern on first use when that level is matrix-free."""
        if self._nnz0 is None:
            A0 = self._levels[0].A
            self._nnz0 = A0.nnz if hasattr(A0, "nnz") else \
                int(fem.sparsity_pattern(self.V)[1].numel()) * self.V.bs ** 2
        return (self._nnz0 + sum(L.A.nnz for L in self._levels[1:])) / self._nnz0

    # ------------------------------------------------------------------------------ setup
    def _estimate_lmax(self, L) -> float:
        """Largest eigenvalue of D^-1 A from EIG_STEPS steps of block-Jacobi CG on a seeded right-hand
        side (the Lanczos tridiagonal of the CG coefficients); deterministic."""
        bs = L.bs
        r, z, p, Ap = L.r, L.z, L.d, L.t
        self._gen.manual_seed(1234)
        r.uniform_(-1.0, 1.0, generator=self._gen)
        if L.marker is not None:
            r.mul_(L.marker == 0)
        prec = lambda v, out: torch.bmm(L.Dinv, v.view(-1, bs, 1), out=out.view(-1, bs, 1))
        prec(r, z)
        p.copy_(z)
        rz = torch.dot(r, z)
        alphas, betas = [], []
        for _ in range(EIG_STEPS):
            L.A.mult(p, Ap)
            alpha = rz / torch.dot(p, Ap)
            r.sub_(alpha * Ap)
            prec(r, z)
            rz_new = torch.dot(r, z)
            beta = rz_new / rz
            p.mul_(beta).add_(z)
            rz = rz_new
            alphas.append(alpha)
            betas.append(beta)
        al, be = torch.stack(alphas).cpu().numpy(), torch.stack(betas).cpu().numpy()
        k = 0  # steps before a breakdown (an exact solve on a tiny level)
        while k < EIG_STEPS and np.isfinite(al[k]) and al[k] > 0 and (k == 0 or (np.isfinite(be[k - 1]) and be[k - 1] > 0)):
            k += 1
        if k == 0:
            raise RuntimeError("eigenvalue estimate broke down: is the operator symmetric positive definite?")
        T = np.zeros((k, k))
        for j in range(k):
            T[j, j] = 1.0 / al[j] + (be[j - 1] / al[j - 1] if j else 0.0)
            if j + 1 < k:
                T[j, j + 1] = T[j + 1, j] = np.sqrt(be[j]) / al[j]
        for v in (r, z, p, Ap):
            v.zero_()
        return float(np.linalg.eigvalsh(T)[-1])

    def _setup_level(self, L, last: bool):
        """The level's block-Jacobi inverse, eigenvalue estimate and polynomial, or, on a last level small
        enough, its dense inverse."""
        if last and L.direct:
            L.Ainv = self._dense_inverse(L)
            return
        D = L.A.block_diagonal()
        bad = D.abs().sum((1, 2)) == 0  # rows without a diagonal block keep identity (as KrylovSolver)
        D[bad] = torch.eye(L.bs, dtype=D.dtype, device=D.device)
        L.Dinv = torch.linalg.inv(D).contiguous()
        L.lmax = self._estimate_lmax(L)
        degree = COARSE_CHEB_DEGREE if last else self.smoother_degree
        L.coef = chebyshev_coefficients(CHEB_LOWER * L.lmax, CHEB_UPPER * L.lmax, degree)

    def _dense_inverse(self, L) -> torch.Tensor:
        A = L.A
        if not hasattr(A, "indptr"):  # a single matrix-free level: probe it with the identity
            n = L.ndofs
            eye = torch.eye(n, dtype=torch.float64, device=L.r.device)
            M = torch.stack([A.mult(eye[j].contiguous()) for j in range(n)], 1)
        else:
            nb, bs = A.num_block_rows, A.bs
            rows = torch.repeat_interleave(torch.arange(nb, device=A.indices.device), A.indptr[1:] - A.indptr[:-1])
            M = torch.zeros((nb, bs, nb, bs), dtype=torch.float64, device=A.indices.device)
            M[rows, :, A.indices.to(torch.int64), :] = A.data
            M = M.reshape(nb * bs, nb * bs)
        Minv = torch.linalg.inv(M)
        return (0.5 * (Minv + Minv.T)).contiguous()

    # ------------------------------------------------------------------------------ cycle
    def _smooth(self, L, zero_guess: bool):
        """z <- z + p(D^-1 A) D^-1 (r - A z), the level's Chebyshev polynomial (z = 0 on entry when
        zero_guess: the first residual is r itself)."""
        for k, (cd, cr) in enumerate(L.coef):
            if k == 0 and zero_guess:
                L.z.zero_()
                Ax = None
            else:
                Ax = L.A.mult(L.z, L.t)
            cheb_step(L.Dinv, L.r, Ax, cd, cr, L.d, L.z)

    def _restrict(self, L, C):
        """C.r = the restriction of the residual in L.t."""
        restrict(L.transfer, L.t, C.r, bc_f=L.marker, bc_c=C.marker)

    def _prolong(self, L, C):
        """L.z += the prolongation of the coarse correction C.z."""
        prolong(L.transfer, C.z, L.z, bc_c=C.marker, bc_f=L.marker, add=True)

    def _cycle(self, li: int):
        L = self._levels[li]
        if li == len(self._levels) - 1:
            if L.direct:
                L.z.addmv_(L.Ainv, L.r, beta=0.0)  # (torch.mv(out=...) allocates a temporary)
            else:
                self._smooth(L, True)
            return
        C = self._levels[li + 1]
        self._smooth(L, True)
        L.A.mult(L.z, L.t)
        torch.sub(L.r, L.t, out=L.t)
        self._restrict(L, C)
        self._cycle(li + 1)
        self._prolong(L, C)
        self._smooth(L, False)

    def apply(self, r: torch.Tensor, z: torch.Tensor | None = None) -> torch.Tensor:
        """z = M r: one V-cycle on the free dofs, z = r / diagonal on the constrained ones (they are
        decoupled from the rest, so M stays symmetric positive definite). With z given the call
        allocates nothing."""
        if self.updates == 0:
            self.update()
        L0 = self._levels[0]
        if z is None:
            z = torch.empty_like(r)
        if self._free is None:
            L0.r.copy_(r)
        else:
            torch.mul(r, self._free, out=L0.r)
        self._cycle(0)
        if self._free is None:
            z.copy_(L0.z)
        else:
            torch.addcdiv(L0.z, r, self._cdiv, out=z)
        return z


class GeometricMultigrid(_VCycle):
    """One V-cycle of geometric multigrid as a fixed, symmetric positive definite preconditioner
    (``apply(r, z)`` / ``update()``: the interface of ``nls.KrylovSolver.set_preconditioner``).

    a: the Jacobian form on a structured mesh (LinearElasticity / AsymDamage / NeoHookean); bcs, diagonal
    as ``fem.assemble_matrix``. Level 0 is the form's own space with ``fine_operator`` (anything with
    ``mult(x, y)`` and ``block_diagonal()``) or ``fem.JacobianOperator(a, bcs, diagonal)``; a degree-2
    space is followed by degree 1 on the same mesh; further levels halve every ``n`` (``plan_hierarchy``).
    Coarse forms are rediscretised with the same form class: per-cell coefficients are the mean over the
    child cells, the nodal state is injected, a coarse node is constrained where its coinciding fine node
    is; coarse operators are assembled (``fem.assemble_matrix``). The smoother is Chebyshev of degree
    ``smoother_degree`` over block-Jacobi on [0.1, 1.1] x the estimated largest eigenvalue of D^-1 A,
    the same polynomial before and after the coarse correction. A coarsest level of at most
    ``coarse_dofs`` dofs is inverted densely at ``update()``, a larger one gets a fixed Chebyshev
    polynomial of degree 8.

    On a mesh without a lattice (``mesh.structured is None``: triangles and tetrahedra) the levels follow
    ``plan_refined_hierarchy``: degree 2 to degree 1 on the same mesh, then degree 1 on every
    ``mesh.parent`` that ``mesh.refine`` left behind. The transfer is an ``EdgeTransfer``, injection takes
    the first ``ncoarse`` nodes, the coarse marker is the leading slice of the fine one, the parent of cell
    ``j`` is ``j >> tdim``; ``levels`` reports ``n = None``.

    ``update()`` must follow every change of the state (``KrylovSolver.set_operator`` calls it); the
    first ``apply`` runs it if nobody has. ``levels``: [(degree, n, num_dofs, kind)];
    ``operator_complexity``: stored matrix entries of all levels over those of the level-0 matrix."""

    def __init__(self, a, bcs=None, diagonal: float = 1.0, fine_operator=None, smoother_degree: int = 2,
                 coarse_dofs: int = 6000, max_levels: int | None = None):
        self._init_common(a, bcs, diagonal, smoother_degree, coarse_dofs)
        V = a.V
        refined = V.mesh.structured is None
        table = (plan_refined_hierarchy if refined else plan_hierarchy)(V, coarse_dofs, max_levels)
        if V.bs != V.mesh.gdim:
            raise ValueError("the form's space must be a vector Lagrange space (bs = gdim)")
        for li, (p, n) in enumerate(table):
            if li == 0:
                L = self._fine_level(fine_operator)
                L.n = None if refined else n
            else:
                self._geometric_level(self._levels[-1], n, refined)
        self._close_hierarchy()

    def update(self):
        """Re-inject the state, re-assemble the coarse matrices and refresh each level's block-Jacobi
        inverse, eigenvalue estimate and the coarsest level's dense inverse."""
        Ls = self._levels
        for F, L in zip(Ls[:-1], Ls[1:]):
            self._refill(F, L)
            fem.assemble_matrix(L.a, bcs=L.bcs, diagonal=self.diagonal, A=L.A)
        for L in Ls:
            self._setup_level(L, L is Ls[-1])
        self.updates += 1


class SmoothedAggregation(_VCycle):
    """One V-cycle of smoothed-aggregation algebraic multigrid as a fixed, symmetric positive definite
    preconditioner: ``GeometricMultigrid``'s contract (``apply(r, z)`` / ``update()``, ``levels``,
    ``operator_complexity``, usable in ``nls.KrylovSolver.set_preconditioner``) on meshes that have neither a
    lattice nor a chain of ``mesh.parent``. The coarse levels come from the matrix and the node coordinates
    alone, with the rigid-body modes as the near-null space (``femasm.amg``).

    a: the Jacobian form on a vector Lagrange space with ``bs == gdim`` in 2-D or 3-D: degree 1 with any cell
    type on any mesh, or degree 2 where ``GeometricMultigrid`` has a P2 -> P1 step (simplices anywhere,
    lattice meshes); everything else (scalar spaces, DG, degree 3, ``z_range`` slabs) raises ValueError.
    Level 0 is the form's space with ``fine_operator`` or a matrix-free ``fem.JacobianOperator``; a degree-2
    level is followed by the rediscretised, assembled degree-1 level on the same mesh, exactly as in
    ``GeometricMultigrid``; below the degree-1 level every level is algebraic: 3 (2-D) or 6 (3-D) dofs per
    aggregate, ``A_c = P^T A P`` with ``P = M_f (T - omega D^-1 A T)``.

    The algebraic set-up reads the degree-1 level's matrix entries: the level's own assembled matrix below
    degree 2; at degree 1 a ``la.MatrixCSR`` given as ``fine_operator`` (what ``problem.matrix()`` is in
    assembled mode); at degree 1 otherwise a matrix this class assembles at every ``update()`` and keeps
    resident, while the given or matrix-free operator still does the level-0 smoothing.

    ``update(rebuild=False)`` redoes the numeric Galerkin products, the block-Jacobi inverses, the eigenvalue
    estimates and the dense inverse of the coarsest level. Aggregates, sparsity patterns, product lists and
    the prolongators' values are built once, at the first ``update()``, from the matrix of that moment;
    ``update(rebuild=True)`` smooths the prolongators again with the current matrices. ``updates`` and
    ``rebuilds`` count the two kinds of call (the first ``update()`` is both). Levels stop at ``coarse_dofs``
    dofs (dense inverse) or at ``max_levels`` (fixed Chebyshev polynomial), as in ``GeometricMultigrid``.

    ``levels``: [(degree, None, num_dofs, kind)], degree 0 and kind "galerkin" on the algebraic levels; it and
    ``operator_complexity`` run the first ``update()`` if nobody has, since the hierarchy is not known before."""

    def __init__(self, a, bcs=None, diagonal: float = 1.0, fine_operator=None, smoother_degree: int = 2,
                 coarse_dofs: int = 6000, max_levels: int | None = None):
        from .la import MatrixCSR

        self._init_common(a, bcs, diagonal, smoother_degree, coarse_dofs)
        V = a.V
        m = V.mesh
        st = m.structured
        if V.family in ("DG", "Discontinuous Lagrange") or V.degree not in (1, 2):
            raise ValueError(f"SmoothedAggregation serves Lagrange degree 1 and 2, not {V.family} degree {V.degree}")
        if V.bs != m.gdim or m.gdim not in (2, 3):
            raise ValueError("the form's space must be a vector Lagrange space (bs = gdim) in 2-D or 3-D: the "
                             "rigid-body modes are the near-null space")
        if st is not None and st.get("z_range") is not None and tuple(st["z_range"]) != (0, int(st["n"][-1])):
            raise ValueError(f"SmoothedAggregation needs the whole box, not the z_range={tuple(st['z_range'])} slab")
        if V.degree == 2:
            if st is None and not fem.is_simplex(m.cell_type):
                raise ValueError(f"SmoothedAggregation at degree 2 on an unstructured mesh needs triangles or "
                                 f"tetrahedra, not {CellType(m.cell_type).name} cells (the P2 -> P1 edge transfer)")
            if st is not None and m.cell_type == CellType.triangle and st.get("diagonal", "right") != "right":
                raise ValueError("SmoothedAggregation at degree 2 needs diagonal='right' triangles (the lattice "
                                 "P2 -> P1 transfer)")
        if max_levels is not None and max_levels < 1:
            raise ValueError("max_levels must be at least 1")
        self.max_levels = max_levels
        self.rebuilds = 0
        more = lambda: (max_levels is None or len(self._levels) < max_levels) and \
            self._levels[-1].ndofs > self.coarse_dofs
        L = self._fine_level(fine_operator)
        if V.degree == 2 and more():
            if st is not None:
                L.n = tuple(int(k) for k in st["n"])  # (the lattice transfer on the same n)
            L = self._geometric_level(L, L.n if st is not None else m, st is None)
            self._levels[0].n = L.n = None
        # the degree-1 level, whose matrix entries the algebraic set-up reads
        self._p1 = L if L.degree == 1 else None
        self._A1 = None
        if self._p1 is not None:
            self._p1.x = self._p1.V.tabulate_dof_coordinates()
            # (a matrix of this class's own, where the level's operator is none, is created by the first update())
            self._p1.entries = self._p1.A if isinstance(self._p1.A, MatrixCSR) else None
        self._more = more
        self._built = False  # the algebraic levels are added, and the hierarchy closed, by the first update()

    @property
    def levels(self) -> list:
        if not self._built:
            self.update()
        return super().levels

    @property
    def operator_complexity(self) -> float:
        if not self._built:
            self.update()
        return _VCycle.operator_complexity.fget(self)

    @property
    def transfers(self) -> list:
        """The ``amg.Aggregation`` of every algebraic transfer, finest first."""
        return [L.transfer for L in self._levels if isinstance(L.transfer, amg.Aggregation)]

    def _restrict(self, L, C):
        if isinstance(L.transfer, amg.Aggregation):
            L.transfer.Pt.mult(L.t, C.r)
        else:
            super()._restrict(L, C)

    def _prolong(self, L, C):
        if isinstance(L.transfer, amg.Aggregation):
            L.transfer.P.mult(C.z, L.z, add=True)
        else:
            super()._prolong(L, C)

    def _coarsen(self, L):
        """Aggregate level L and append the level below it; False when there is nothing to gain."""
        tr = amg.Aggregation(L.entries, L.x, L.marker)
        nr = tr.nr
        if tr.nagg == 0 or tr.nagg * nr >= L.ndofs:
            return False
        C = _Level()
        C.degree, C.n, C.kind = 0, None, "galerkin"
        C.A = C.entries = tr.Ac
        C.x, C.marker = tr.xc, tr.marker_c
        L.transfer = tr
        self._add_level(C, nr, tr.nagg * nr)
        return True

    def update(self, rebuild: bool = False):
        """Redo everything that depends on the matrix entries; with ``rebuild`` (and at the first call) also
        the prolongators' values. See the class."""
        Ls = self._levels
        first = not self._built
        p1 = self._p1
        if p1 is None:  # a degree-2 space small enough to invert, or max_levels = 1
            if first:
                self._close_hierarchy()
            self._setup_level(Ls[0], True)
        else:
            i1 = Ls.index(p1)
            if i1 == 1:
                self._refill(Ls[0], p1)
                fem.assemble_matrix(p1.a, bcs=p1.bcs, diagonal=self.diagonal, A=p1.A)
                self._setup_level(Ls[0], False)
            elif p1.entries is None or self._A1 is not None:
                if self._A1 is None:
                    p1.entries = self._A1 = fem.create_matrix(self.a)
                fem.assemble_matrix(self.a, bcs=self.bcs, diagonal=self.diagonal, A=self._A1)
            li = i1
            while True:
                L = Ls[li]
                if first and li == len(Ls) - 1 and self._more():
                    self._coarsen(L)
                last = li == len(Ls) - 1
                if last and first:
                    self._close_hierarchy()
                self._setup_level(L, last)
                if last:
                    break
                if first or rebuild:
                    L.transfer.smooth(L.entries, L.Dinv, L.lmax)
                L.transfer.galerkin(L.entries)
                li += 1
        self._built = True
        self.updates += 1
        if first or rebuild:
            self.rebuilds += 1
