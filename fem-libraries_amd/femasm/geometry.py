"""dolfinx.geometry-shaped point location: which cell of a mesh holds a physical point, and where in it.

``bb_tree(mesh)`` builds the search plan, a uniform grid over the cells' padded bounding boxes (torch on the
mesh's device: plumbing, built once per mesh and coordinates and cached on the mesh). ``locate_points`` then
finds, for every query point, the smallest id among the cells that accept it and the point's reference
coordinates there: on a GPU mesh the HIP kernel k_locate_points (fa_locate_points, one lane per point), on a
CPU mesh the same definition in vectorised torch, over the same grid and with the same acceptance rule.

Acceptance rule (include/femasm.h states it for the kernel; ``_accept`` below is its torch form). Vertex 0 is
subtracted first: e_v = x_v - x_v0, dx = x - x_v0.

  simplices      X = adj(J) dx / det J with J = [e_1 .. e_tdim] (cofactor form: either sign of det J, mirrored
                 meshes are supported); accept when every barycentric lambda_i >= -tol.
  quads, hexes   Newton on the Q1 map from the cell centre, at most NEWTON_CAP steps, converged when a step has
                 |dX|_inf <= NEWTON_STOP; a step whose det J has not the sign of det J at the centre, or that
                 leaves [-1, 2]^tdim, rejects the cell (not the point), as does running out of steps; accept when
                 converged and -tol <= X_d <= 1 + tol.

``tol`` is in reference coordinates. Points on a shared vertex, edge or face belong to the smallest cell id
that accepts them, whatever the grid: every bin lists its cells in ascending order and a point's bin lists every
cell that can accept it.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .mesh import CellType, Mesh, NVERTS

NEWTON_CAP = 12       # kLocateNewtonCap of femasm_points.hip
NEWTON_STOP = 1e-12   # kLocateNewtonStop
PADDING = 1e-6        # default padding of a cell's bounding box, as a fraction of the box's diagonal
PAIR_CAP = 32         # (bin, cell) pairs per cell above which the bin counts are halved
_PAIR_CHUNK = 1 << 21  # (point, candidate) pairs the host path tests at a time


@dataclass
class CellGrid:
    """The uniform grid of ``bb_tree`` (fa_cell_grid): bin of x along d = clamp(floor((x[d] - lo[d]) * inv_h[d]),
    0, dims[d] - 1), bin index (k * dims[1] + j) * dims[0] + i; ``bin_cells[bin_ptr[b]:bin_ptr[b + 1]]`` are the
    cells whose padded bounding box meets bin b, in ascending order. ``padding`` is the fraction of each
    cell's box diagonal its box was grown by on every side."""
    gdim: int
    dims: tuple
    lo: tuple
    inv_h: tuple
    bin_ptr: torch.Tensor    # int64 [nbins + 1]
    bin_cells: torch.Tensor  # int32 [npairs]
    padding: float
    num_cells: int

    @property
    def num_bins(self) -> int:
        return int(np.prod(self.dims))

    @property
    def num_pairs(self) -> int:
        return int(self.bin_cells.numel())

    def cells_per_bin(self) -> tuple:
        """(mean, maximum) number of cells listed per bin."""
        n = self.bin_ptr[1:] - self.bin_ptr[:-1]
        return float(n.to(torch.float64).mean()), int(n.max())

    def _fa_cell_grid(self) -> _lib.fa_cell_grid:
        g = _lib.fa_cell_grid()
        for d in range(3):
            g.dims[d] = self.dims[d]
            g.lo[d] = self.lo[d]
            g.inv_h[d] = self.inv_h[d]
        g.bin_ptr = self.bin_ptr.data_ptr()
        g.bin_cells = self.bin_cells.data_ptr()
        return g


def _default_dims(ext, nc: int) -> list:
    """Bins per axis proportional to the axis' extent, about nc bins in total."""
    gd = len(ext)
    s = (nc / float(np.prod(ext))) ** (1.0 / gd)
    return [max(1, int(round(e * s))) for e in ext]


def _build(mesh: Mesh, padding: float, dims) -> CellGrid:
    gd, dev, nc = mesh.gdim, mesh.device, mesh.num_cells
    if nc == 0:
        return CellGrid(gd, (1, 1, 1), (0.0,) * 3, (1.0,) * 3, torch.zeros(2, dtype=torch.int64, device=dev),
                        torch.zeros(0, dtype=torch.int32, device=dev), padding, 0)
    xv = mesh.x[mesh.cells.to(torch.int64)]  # [nc, nv, gd]
    blo, bhi = xv.min(1).values, xv.max(1).values
    # (the vertices' box bounds bilinear / trilinear cells too: the Q1 basis is a non-negative partition of unity)
    pad = padding * (bhi - blo).norm(dim=1, keepdim=True)
    blo, bhi = blo - pad, bhi + pad
    lo_t, hi_t = blo.min(0).values, bhi.max(0).values
    lo, ext = lo_t.tolist(), (hi_t - lo_t).tolist()
    if not all(np.isfinite(e) and e > 0.0 for e in ext):
        raise ValueError("bb_tree: the mesh's bounding box is empty or not finite")
    fixed = dims is not None
    dims = [int(d) for d in dims] if fixed else _default_dims(ext, nc)
    if len(dims) != gd or min(dims) < 1:
        raise ValueError(f"bb_tree: dims must be {gd} positive bin counts")
    while True:
        if int(np.prod(dims)) >= 2 ** 31:
            raise ValueError("bb_tree: 2^31 bins or more")
        inv_h = [dims[d] / ext[d] for d in range(gd)]
        dm1 = torch.tensor([d - 1 for d in dims], dtype=torch.int64, device=dev)
        lo_d = torch.tensor(lo, dtype=torch.float64, device=dev)
        ih_d = torch.tensor(inv_h, dtype=torch.float64, device=dev)
        i0 = torch.minimum(torch.floor((blo - lo_d) * ih_d).to(torch.int64).clamp_(min=0), dm1)
        i1 = torch.minimum(torch.floor((bhi - lo_d) * ih_d).to(torch.int64).clamp_(min=0), dm1)
        w = i1 - i0 + 1  # [nc, gd] bins met per axis
        counts = w.prod(1)
        total = int(counts.sum())
        if fixed or total <= PAIR_CAP * nc or max(dims) == 1:
            break
        dims = [(d + 1) // 2 for d in dims]
    # (bin, cell) pairs in cell order, then a stable sort by bin: ascending cell ids within every bin
    cid = torch.repeat_interleave(torch.arange(nc, device=dev), counts)
    off = torch.arange(total, device=dev) - torch.repeat_interleave(torch.cumsum(counts, 0) - counts, counts)
    wp, i0p = w[cid], i0[cid]
    b = torch.zeros(total, dtype=torch.int64, device=dev)
    stride = 1
    rem = off
    for d in range(gd):
        b += (i0p[:, d] + rem % wp[:, d]) * stride
        rem = torch.div(rem, wp[:, d], rounding_mode="floor")
        stride *= dims[d]
    order = torch.sort(b, stable=True).indices
    nbins = int(np.prod(dims))
    ptr = torch.zeros(nbins + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(torch.bincount(b, minlength=nbins), 0)
    d3 = tuple(dims) + (1,) * (3 - gd)
    return CellGrid(gd, d3, tuple(lo) + (0.0,) * (3 - gd), tuple(inv_h) + (1.0,) * (3 - gd), ptr,
                    cid[order].to(torch.int32).contiguous(), padding, nc)


def bb_tree(mesh: Mesh, padding: float | None = None, dims=None) -> CellGrid:
    """The search grid of ``mesh`` (dolfinx.geometry.bb_tree; a uniform grid, not a tree).

    Every cell's bounding box (of its vertices) is grown by ``padding`` times its diagonal on every side
    (default PADDING = 1e-6; ``locate_points`` needs padding >= 4 tol, so that a point accepted within tol,
    which lies at most tdim * tol box extents outside the box, is always listed). The grid spans the padded
    boxes; each axis gets a bin count proportional to its extent, about ``num_cells`` bins in total, and a
    cell is listed in every bin its padded box meets. When that takes more than PAIR_CAP = 32 (bin, cell) pairs
    per cell (stretched cells: a cubic bin of the cell's volume is much shorter than the cell's box), the bin
    counts are halved until it does not. ``dims`` fixes the bins per axis instead (no halving).
    Built with torch on the mesh's device and cached on the mesh, keyed on the coordinates' version: moving
    ``mesh.x`` in place, or replacing it, rebuilds."""
    from .fem import _coords_version

    padding = PADDING if padding is None else float(padding)
    if not padding > 0.0:
        raise ValueError("bb_tree: padding must be positive")
    key = (padding, None if dims is None else tuple(int(d) for d in dims))
    ver = _coords_version(mesh) + (mesh.cells.data_ptr(), mesh.cells._version)
    cache = mesh.__dict__.setdefault("_bb_trees", {})
    hit = cache.get(key)
    if hit is not None and hit[0] == ver:
        return hit[1]
    tree = _build(mesh, padding, dims)
    if len(cache) >= 4:
        cache.pop(next(iter(cache)))
    cache[key] = (ver, tree)
    return tree


# ------------------------------------------------------------------------------------------- acceptance rule
def _det_adj(A: torch.Tensor):
    """(det [m], adjugate [m, gd, gd]) of A [m, gd, gd] in the kernel's cofactor form."""
    if A.shape[-1] == 2:
        det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 1, 0]
        C = torch.stack([torch.stack([A[:, 1, 1], -A[:, 0, 1]], 1), torch.stack([-A[:, 1, 0], A[:, 0, 0]], 1)], 1)
        return det, C
    a = A
    c00 = a[:, 1, 1] * a[:, 2, 2] - a[:, 1, 2] * a[:, 2, 1]
    c01 = a[:, 0, 2] * a[:, 2, 1] - a[:, 0, 1] * a[:, 2, 2]
    c02 = a[:, 0, 1] * a[:, 1, 2] - a[:, 0, 2] * a[:, 1, 1]
    c10 = a[:, 1, 2] * a[:, 2, 0] - a[:, 1, 0] * a[:, 2, 2]
    c11 = a[:, 0, 0] * a[:, 2, 2] - a[:, 0, 2] * a[:, 2, 0]
    c12 = a[:, 0, 2] * a[:, 1, 0] - a[:, 0, 0] * a[:, 1, 2]
    c20 = a[:, 1, 0] * a[:, 2, 1] - a[:, 1, 1] * a[:, 2, 0]
    c21 = a[:, 0, 1] * a[:, 2, 0] - a[:, 0, 0] * a[:, 2, 1]
    c22 = a[:, 0, 0] * a[:, 1, 1] - a[:, 0, 1] * a[:, 1, 0]
    det = a[:, 0, 0] * c00 + a[:, 0, 1] * c10 + a[:, 0, 2] * c20
    C = torch.stack([torch.stack([c00, c01, c02], 1), torch.stack([c10, c11, c12], 1),
                     torch.stack([c20, c21, c22], 1)], 1)
    return det, C


def _q1(X: torch.Tensor):
    """Q1 basis [m, nv] and reference gradients [m, nv, gd] at X [m, gd] (vertex v = i + 2 j + 4 k)."""
    gd = X.shape[1]
    psi, dpsi = [], []
    for v in range(1 << gd):
        f = [X[:, d] if (v >> d) & 1 else 1.0 - X[:, d] for d in range(gd)]
        p = f[0]
        for d in range(1, gd):
            p = p * f[d]
        psi.append(p)
        row = []
        for k in range(gd):
            g = torch.full_like(X[:, 0], 1.0 if (v >> k) & 1 else -1.0)
            for d in range(gd):
                if d != k:
                    g = g * f[d]
            row.append(g)
        dpsi.append(torch.stack(row, 1))
    return torch.stack(psi, 1), torch.stack(dpsi, 1)


def _accept(ct, xv: torch.Tensor, xp: torch.Tensor, tol: float):
    """The acceptance rule on (cell, point) pairs: xv [m, nv, gd] the cells' vertices, xp [m, gd] the points.
    Returns (accepted [m] bool, X [m, gd]); X is meaningful where accepted (and, for simplices, everywhere)."""
    gd = xp.shape[1]
    e = xv[:, 1:] - xv[:, :1]
    dx = xp - xv[:, 0]
    if CellType(ct) in (CellType.triangle, CellType.tetrahedron):
        det, C = _det_adj(e.transpose(1, 2))  # J[i][k] = e_k[i]
        X = torch.einsum("mki,mi->mk", C, dx) / det[:, None]
        l0 = 1.0 - X.sum(1)
        return (X >= -tol).all(1) & (l0 >= -tol), X
    m = xp.shape[0]
    X = torch.full((m, gd), 0.5, dtype=torch.float64, device=xp.device)
    live = torch.ones(m, dtype=torch.bool, device=xp.device)
    conv = torch.zeros_like(live)
    sign = None
    for it in range(NEWTON_CAP):
        go = live & ~conv
        if not bool(go.any()):
            break
        psi, dpsi = _q1(X)
        r = torch.einsum("mv,mvi->mi", psi[:, 1:], e) - dx
        J = torch.einsum("mvi,mvk->mik", e, dpsi[:, 1:])
        det, C = _det_adj(J)
        if it == 0:
            sign = det
        dX = -torch.einsum("mki,mi->mk", C, r) / det[:, None]
        Xn = X + dX
        ok = (det * sign > 0.0) & ((Xn >= -1.0) & (Xn <= 2.0)).all(1)
        step = dX.abs().max(1).values
        upd = go & ok
        X = torch.where(upd[:, None], Xn, X)
        conv = conv | (upd & (step <= NEWTON_STOP))
        live = live & (ok | ~go)
    return live & conv & ((X >= -tol) & (X <= 1.0 + tol)).all(1), X


def pull_back(mesh: Mesh, x: torch.Tensor, cells: torch.Tensor) -> torch.Tensor:
    """Reference coordinates X [n, gdim] of the points x in the GIVEN cells (the acceptance rule's solve with
    no test: points outside their cell get the extrapolated X, NaN where Newton fails). Torch, any device."""
    c = cells.to(torch.int64)
    safe = c.clamp(min=0)
    _, X = _accept(mesh.cell_type, mesh.x[mesh.cells.to(torch.int64)[safe]], x, float("inf"))
    return torch.where((c >= 0)[:, None], X, torch.full_like(X, float("nan")))


def _bins(tree: CellGrid, x: torch.Tensor):
    """(inside [n] bool, bin [n] int64) of the points, as the kernel computes them."""
    gd = tree.gdim
    dev = x.device
    lo = torch.tensor(tree.lo[:gd], dtype=torch.float64, device=dev)
    ih = torch.tensor(tree.inv_h[:gd], dtype=torch.float64, device=dev)
    dims = torch.tensor(tree.dims[:gd], dtype=torch.int64, device=dev)
    t = (x - lo) * ih
    inside = ((t >= 0.0) & (t <= dims.to(torch.float64))).all(1)
    b = torch.minimum(torch.where(inside[:, None], t, torch.zeros_like(t)).to(torch.int64), dims - 1)
    bin_ = torch.zeros(x.shape[0], dtype=torch.int64, device=dev)
    for d in range(gd - 1, -1, -1):
        bin_ = bin_ * tree.dims[d] + b[:, d]
    return inside, bin_


def _locate_host(mesh: Mesh, tree: CellGrid, x: torch.Tensor, tol: float):
    """k_locate_points in vectorised torch: every (point, candidate) pair of the point's bin is tested and the
    smallest accepted cell id kept (the kernel stops at the first accepted cell of an ascending list)."""
    n, gd = x.shape
    dev = x.device
    cells = torch.full((n,), -1, dtype=torch.int32, device=dev)
    X = torch.full((n, gd), float("nan"), dtype=torch.float64, device=dev)
    if n == 0 or mesh.num_cells == 0:
        return cells, X
    inside, bin_ = _bins(tree, x)
    pts = torch.nonzero(inside).reshape(-1)
    start = tree.bin_ptr[bin_[pts]]
    cnt = tree.bin_ptr[bin_[pts] + 1] - start
    cum = torch.cumsum(cnt, 0)
    geom = mesh.cells.to(torch.int64)
    big = torch.iinfo(torch.int64).max
    p0 = 0
    while p0 < pts.numel():
        base = int(cum[p0 - 1]) if p0 else 0
        p1 = int(torch.searchsorted(cum, torch.tensor(base + _PAIR_CHUNK, device=dev), right=True))
        p1 = max(p1, p0 + 1)
        c = cnt[p0:p1]
        tot = int(c.sum())
        if tot:
            loc = torch.repeat_interleave(torch.arange(p1 - p0, device=dev), c)
            off = torch.arange(tot, device=dev) - torch.repeat_interleave(torch.cumsum(c, 0) - c, c)
            cand = tree.bin_cells[start[p0:p1][loc] + off].to(torch.int64)
            pid = pts[p0:p1][loc]
            ok, Xc = _accept(mesh.cell_type, mesh.x[geom[cand]], x[pid], tol)
            best = torch.full((p1 - p0,), big, dtype=torch.int64, device=dev)
            best.scatter_reduce_(0, loc[ok], cand[ok], reduce="amin")
            win = ok & (cand == best[loc])
            cells[pid[win]] = cand[win].to(torch.int32)
            X[pid[win]] = Xc[win]
        p0 = p1
    return cells, X


def _fa_geometry_mesh(mesh: Mesh) -> _lib.fa_mesh:
    """The mesh as its own P1 / Q1 space (fa_locate_points reads the geometry only)."""
    s = _lib.fa_mesh()
    s.cell_type = int(mesh.cell_type)
    s.degree = 1
    s.gdim = mesh.gdim
    s.nn = s.nv = NVERTS[mesh.cell_type]
    s.ncells = mesh.num_cells
    s.nnodes = mesh.num_vertices
    s.cells = s.geom = mesh.cells.data_ptr()
    s.x = mesh.x.data_ptr()
    return s


def locate_points(mesh: Mesh, x, tol: float = 1e-10, tree: CellGrid | None = None):
    """(cells int32 [n], X float64 [n, gdim]): for every point x[i] the smallest id among the cells of ``mesh``
    that accept it (module docstring) and its reference coordinates there; -1 and NaN where no cell does (a
    point outside the mesh, in a hole, or with a NaN / infinite coordinate). dolfinx:
    compute_collisions_points + compute_colliding_cells, one cell per point.
    A GPU mesh runs k_locate_points (asynchronous, one lane per point); a CPU mesh the same rule in torch."""
    gd = mesh.gdim
    x = torch.as_tensor(x, dtype=torch.float64, device=mesh.device).reshape(-1, gd).contiguous()
    tol = float(tol)
    if not tol >= 0.0:
        raise ValueError("locate_points: tol must be >= 0")
    tree = bb_tree(mesh) if tree is None else tree
    if tree.gdim != gd or tree.num_cells != mesh.num_cells or tree.bin_ptr.device != mesh.device:
        raise ValueError("locate_points: the tree belongs to another mesh")
    if tree.padding < 4.0 * tol:
        raise ValueError(f"locate_points: tol {tol:g} needs a tree with padding >= {4 * tol:g} (bb_tree(mesh, padding))")
    n = x.shape[0]
    if mesh.device.type != "cuda":
        return _locate_host(mesh, tree, x, tol)
    cells = torch.empty(n, dtype=torch.int32, device=mesh.device)
    X = torch.empty((n, gd), dtype=torch.float64, device=mesh.device)
    if n == 0 or mesh.num_cells == 0:
        return cells.fill_(-1), X.fill_(float("nan"))
    fm = _fa_geometry_mesh(mesh)
    g = tree._fa_cell_grid()
    _lib.check(_lib.load().fa_locate_points(ctypes.byref(fm), ctypes.byref(g), n, x.data_ptr(), tol, cells.data_ptr(),
                                            X.data_ptr(), _lib.stream_handle(mesh.device)), "fa_locate_points")
    return cells, X
