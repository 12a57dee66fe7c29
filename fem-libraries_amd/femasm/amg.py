"""Set-up of the smoothed-aggregation hierarchy of ``mg.SmoothedAggregation``: everything between one level's
block matrix and the next level's.

A level has ``n`` nodes with coordinates ``x`` [n, gdim], ``b`` dofs per node (``gdim`` on the degree-1
level; ``nr`` = 3 in 2-D, 6 in 3-D below it: the rigid-body modes of an aggregate), a square block-CSR matrix
``A`` and a constraint marker per dof. ``Aggregation`` builds, once and with torch ops on the matrix's device,

1. the graph: the block pattern of ``A`` among the *free* nodes (at least one unconstrained dof); a fully
   constrained node belongs to no aggregate and no distance-2 path runs through it;
2. the aggregates, by a deterministic parallel MIS(2) over ``csr_row_max`` (``aggregate``);
3. the tentative prolongator ``T`` of the rigid-body modes about each aggregate's centroid and the coarse
   nodes' coordinates, the centroids (``tentative``);
4. the aggregates that cannot span their rotations (too few members, or collinear ones in 3-D): their
   rotation columns are zero and those coarse dofs are constrained, with a unit diagonal;
5. the patterns and inverted product lists of ``A T`` (the pattern of ``P``), ``Y = A P`` and
   ``A_c = P^T Y``, and the permutation that stores ``P^T`` (``ProductPlan``).

``smooth`` then sets ``P = M_f (T - omega D^-1 A T)``, ``omega = 4 / (3 lambda_max)``, and ``galerkin`` redoes
``A_c = P^T (A P)`` from the current entries of ``A``: the only work per Newton step. Both run the numeric
product ``fa_bcsr_product`` on the device and the same sums (``index_add`` in list order) on the CPU.
"""
from __future__ import annotations

import torch

from . import _lib
from .la import BlockCSR

PRIORITY_MULTIPLIER = 2654435761  # Knuth's multiplicative hash: the order in which nodes become roots


def csr_row_max(indptr: torch.Tensor, indices: torch.Tensor, vals: torch.Tensor, free: torch.Tensor | None = None,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """out[i] = free[i] ? max over row i of vals[indices] : 0 on int64 values (fa_csr_row_max; an empty row
    gives 0). free: int8 per row or None."""
    n = int(indptr.numel()) - 1
    if vals.dtype != torch.int64 or not vals.is_contiguous():
        raise ValueError("csr_row_max values must be a contiguous int64 tensor")
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=vals.device)
    if vals.device.type == "cuda":
        _lib.check(_lib.load().fa_csr_row_max(n, indptr.data_ptr(), indices.data_ptr(), _lib.ptr(free), vals.data_ptr(),
                                              int(vals.numel()), out.data_ptr(), _lib.stream_handle(vals.device)),
                   "fa_csr_row_max")
        return out
    rows = torch.repeat_interleave(torch.arange(n), indptr[1:] - indptr[:-1])
    out.zero_()
    out.scatter_reduce_(0, rows, vals[indices.to(torch.int64)], "amax", include_self=False)
    if free is not None:
        out[free == 0] = 0
    return out


def node_priorities(n: int, device=None) -> torch.Tensor:
    """(((i * 2654435761) mod 2^32) << 31) + i + 1: distinct, positive, below 2^63 for i < 2^31."""
    i = torch.arange(n, dtype=torch.int64, device=device)
    return (((i * PRIORITY_MULTIPLIER) % (1 << 32)) << 31) + i + 1


def aggregate(indptr: torch.Tensor, indices: torch.Tensor, free: torch.Tensor) -> tuple:
    """Aggregates of the graph (indptr, indices) among the free nodes: (agg int64 [n], -1 on the nodes that are
    not free; the number of aggregates). Each round an undecided node becomes a root if its priority is the
    largest among the undecided nodes within distance 2, and every undecided node within distance 2 of a new
    root is removed. Roots are numbered in ascending node order; a free node takes the largest root number
    among itself and its neighbours, one still without an aggregate the largest aggregate number among its
    neighbours."""
    n = int(indptr.numel()) - 1
    if n >= 2 ** 31:
        raise ValueError("node indices must fit int32")
    fb = free != 0
    f8 = fb.to(torch.int8).contiguous()
    zero = torch.zeros(n, dtype=torch.int64, device=indices.device)
    prio = torch.where(fb, node_priorities(n, indices.device), zero)
    near = lambda v: torch.maximum(csr_row_max(indptr, indices, v, f8), v)  # the node itself and its neighbours
    undecided = fb.clone()
    root = torch.zeros_like(fb)
    while bool(undecided.any()):
        m2 = near(near(torch.where(undecided, prio, zero)))
        new = undecided & (prio == m2)
        taken = near(near(new.to(torch.int64)))
        root |= new
        undecided &= taken == 0
    number = torch.where(root, torch.cumsum(root.to(torch.int64), 0), zero)  # 1-based
    own = near(number)
    agg = torch.where(own > 0, own, csr_row_max(indptr, indices, own.contiguous(), f8))
    return torch.where(fb, agg, zero) - 1, int(root.sum())


def _padded_members(agg: torch.Tensor, nagg: int):
    """(member nodes sorted by aggregate, their aggregate, their position in it, members per aggregate): the
    layout over which per-aggregate sums run in a fixed order (a dense [nagg, max members] table)."""
    idx = torch.nonzero(agg >= 0).reshape(-1)
    a = agg[idx]
    cnt = torch.bincount(a, minlength=nagg)
    order = torch.sort(a, stable=True).indices
    a_s = a[order]
    pos = torch.arange(a.numel(), device=agg.device) - (torch.cumsum(cnt, 0) - cnt)[a_s]
    return idx[order], a_s, pos, cnt


def tentative(x: torch.Tensor, agg: torch.Tensor, nagg: int, b: int) -> tuple:
    """(T, xc, dead): the tentative prolongator as a BlockCSR of [b, nr] blocks, one per free node in the
    column of its aggregate; the aggregates' centroids [nagg, gdim] (unweighted means); the aggregates that
    keep translations only (bool [nagg]).

    With dx = x_i - c_I: in 2-D the block is [[1, 0, -dx_y], [0, 1, dx_x]] and, for b = 3, a third row
    [0, 0, 1]; in 3-D [I | R(dx)] with R(dx) w = w x dx, and for b = 6 the rows [0 | I] below it."""
    n, gdim = int(x.shape[0]), int(x.shape[1])
    nr = 3 if gdim == 2 else 6
    if gdim not in (2, 3) or b not in (gdim, nr):
        raise ValueError(f"{b} dofs per node in {gdim}-D (the displacement components or the rigid-body modes)")
    dev = x.device
    nodes, a_s, pos, cnt = _padded_members(agg, nagg)
    cmax = int(cnt.max()) if nagg else 0
    pad = torch.zeros((nagg, cmax, gdim), dtype=torch.float64, device=dev)
    pad[a_s, pos] = x[nodes]
    xc = pad.sum(1) / cnt.to(torch.float64).clamp(min=1)[:, None]
    dead = cnt < (2 if gdim == 2 else 3)
    if gdim == 3 and nagg:
        d = torch.zeros_like(pad)
        d[a_s, pos] = x[nodes] - xc[a_s]
        eye = torch.eye(3, dtype=torch.float64, device=dev)
        M = ((d * d).sum(2)[:, :, None, None] * eye - d[:, :, :, None] * d[:, :, None, :]).sum(1)
        ev = torch.linalg.eigvalsh(M)
        dead |= ev[:, 0] < 1e-10 * ev[:, -1]
    member = agg >= 0
    idx = torch.nonzero(member).reshape(-1)
    a = agg[idx]
    dx = x[idx] - xc[a]
    blk = torch.zeros((idx.numel(), b, nr), dtype=torch.float64, device=dev)
    for k in range(b):
        blk[:, k, k] = 1.0
    if gdim == 2:
        blk[:, 0, 2] = -dx[:, 1]
        blk[:, 1, 2] = dx[:, 0]
    else:
        blk[:, 1, 3], blk[:, 2, 3] = -dx[:, 2], dx[:, 1]
        blk[:, 0, 4], blk[:, 2, 4] = dx[:, 2], -dx[:, 0]
        blk[:, 0, 5], blk[:, 1, 5] = -dx[:, 1], dx[:, 0]
    blk[:, :, gdim:] *= (~dead[a]).to(torch.float64)[:, None, None]
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(member.to(torch.int64), 0)
    return BlockCSR(indptr, a.to(torch.int32), blk, nagg), xc, dead


class ProductPlan:
    """The symbolic phase of a block product C = X Y: C's pattern (``indptr``, ``indices``, sorted columns) and,
    per block of C, the list of products that sum into it (``optr`` int64 [nout + 1] over ``xa`` / ``yb``, the
    block slots of X and Y, int32), in ascending order of X's slot, then Y's. ``keep_rows`` (bool per row of
    X) drops whole rows. ``numeric`` is fa_bcsr_product on the device and index_add in list order on the CPU."""

    def __init__(self, xptr, xidx, yptr, yidx, ncols: int, keep_rows=None):
        dev = xidx.device
        m, nx = int(xptr.numel()) - 1, int(xidx.numel())
        xrows = torch.repeat_interleave(torch.arange(m, device=dev), xptr[1:] - xptr[:-1])
        xc = xidx.to(torch.int64)
        ylen = (yptr[1:] - yptr[:-1])[xc]
        if keep_rows is not None:
            ylen = ylen * keep_rows[xrows].to(torch.int64)
        total = int(ylen.sum())
        xa = torch.repeat_interleave(torch.arange(nx, device=dev), ylen)
        yb = yptr[xc[xa]] + torch.arange(total, device=dev) - (torch.cumsum(ylen, 0) - ylen)[xa]
        key, order = torch.sort(xrows[xa] * int(ncols) + yidx.to(torch.int64)[yb], stable=True)
        self.keys, counts = torch.unique_consecutive(key, return_counts=True)
        self.xa, self.yb = xa[order].to(torch.int32).contiguous(), yb[order].to(torch.int32).contiguous()
        self.nout, self.nprod, self.nx, self.ny = int(self.keys.numel()), total, nx, int(yidx.numel())
        if max(self.nout, self.nx, self.ny) >= 2 ** 31:
            raise ValueError("block slots must fit int32")
        self.counts = counts
        self.optr = torch.zeros(self.nout + 1, dtype=torch.int64, device=dev)
        self.optr[1:] = torch.cumsum(counts, 0)
        self.indptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
        self.indptr[1:] = torch.cumsum(torch.bincount(torch.div(self.keys, int(ncols), rounding_mode="floor"),
                                                      minlength=m), 0)
        self.indices = (self.keys % int(ncols)).to(torch.int32)
        self._seg = None

    def numeric(self, X: torch.Tensor, Y: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """out[s] = sum over the list of s of X[xa] @ Y[yb]; X [nx, r, k], Y [ny, k, c], out [nout, r, c]."""
        r, k, c = int(X.shape[1]), int(X.shape[2]), int(Y.shape[2])
        for v, shape in ((X, (self.nx, r, k)), (Y, (self.ny, k, c)), (out, (self.nout, r, c))):
            if v.dtype != torch.float64 or tuple(v.shape) != shape or not v.is_contiguous() or v.device != self.xa.device:
                raise ValueError(f"product operands must be contiguous float64 blocks {shape} on {self.xa.device}")
        if X.device.type == "cuda":
            _lib.check(_lib.load().fa_bcsr_product(self.nout, r, k, c, self.optr.data_ptr(), self.nprod,
                                                   self.xa.data_ptr(), self.yb.data_ptr(), X.data_ptr(), self.nx,
                                                   Y.data_ptr(), self.ny, out.data_ptr(), _lib.stream_handle(X.device)),
                       "fa_bcsr_product")
            return out
        if self._seg is None:
            self._seg = torch.repeat_interleave(torch.arange(self.nout), self.counts)
        out.zero_()
        out.index_add_(0, self._seg, torch.bmm(X[self.xa.to(torch.int64)], Y[self.yb.to(torch.int64)]))
        return out

    def list_stats(self) -> tuple:
        """(median, maximum) products per output block."""
        if self.nout == 0:
            return 0, 0
        return int(self.counts.median()), int(self.counts.max())


def _values(A) -> torch.Tensor:
    """The blocks [nblocks, b, b] of a la.MatrixCSR (one allocation, or a concatenated copy) or la.BlockCSR."""
    return A.data.contiguous()


class Aggregation:
    """The transfer between a level and the next coarser one, and that level's matrix.

    A: the level's square block matrix (la.MatrixCSR or la.BlockCSR; its pattern is read here, its values by
    ``smooth`` and ``galerkin``); x [n, gdim]; marker: int8 per dof or None. After construction: ``agg``,
    ``nagg``, ``T``, ``xc`` (the coarse coordinates), ``dead``, ``marker_c`` (the coarse marker: the rotation
    dofs of the dead aggregates), ``P`` and ``Pt`` (la.BlockCSR, values set by ``smooth``), ``Ac`` (la.BlockCSR,
    values set by ``galerkin``) and the three product plans ``AT``, ``AP``, ``PtY``."""

    def __init__(self, A, x: torch.Tensor, marker: torch.Tensor | None):
        b, n = int(A.bs), int(A.num_block_rows)
        gdim = int(x.shape[1])
        self.b, self.n, self.gdim = b, n, gdim
        self.nr = nr = 3 if gdim == 2 else 6
        dev = A.indices.device
        self.marker = marker
        self.free = torch.ones(n, dtype=torch.bool, device=dev) if marker is None else (marker.view(n, b) == 0).any(1)
        self.agg, self.nagg = aggregate(A.indptr, A.indices, self.free)
        nagg = self.nagg
        self.T, self.xc, self.dead = tentative(x, self.agg, nagg, b)
        mc = torch.zeros((nagg, nr), dtype=torch.int8, device=dev)
        mc[:, gdim:] = self.dead.to(torch.int8)[:, None]
        self.marker_c = mc.reshape(-1).contiguous()
        T = self.T
        # P has the pattern of A T on the free rows (the others are zero rows of M_f)
        self.AT = ProductPlan(A.indptr, A.indices, T.indptr, T.indices, nagg, keep_rows=self.free)
        self.P = BlockCSR(self.AT.indptr, self.AT.indices,
                          torch.zeros((self.AT.nout, b, nr), dtype=torch.float64, device=dev), nagg)
        members = torch.nonzero(self.free).reshape(-1)
        self.tslot = torch.searchsorted(self.AT.keys, members * nagg + self.agg[members])
        if self.AT.nout == 0 or not torch.equal(self.AT.keys[self.tslot.clamp(max=max(self.AT.nout - 1, 0))],
                                                members * nagg + self.agg[members]):
            raise ValueError("the matrix pattern has a free node without a diagonal block")
        self.AT.keys = None
        # P^T, stored: the blocks of P sorted by column (then row), each transposed
        prow, pcol = self.P.block_rows(), self.P.indices.to(torch.int64)
        self.tperm = torch.sort(pcol * n + prow, stable=True).indices
        tptr = torch.zeros(nagg + 1, dtype=torch.int64, device=dev)
        tptr[1:] = torch.cumsum(torch.bincount(pcol, minlength=nagg), 0)
        self.Pt = BlockCSR(tptr, prow[self.tperm].to(torch.int32),
                           torch.zeros((self.AT.nout, nr, b), dtype=torch.float64, device=dev), n)
        self.AP = ProductPlan(A.indptr, A.indices, self.P.indptr, self.P.indices, nagg, keep_rows=self.free)
        self.AP.keys = None
        self.Y = torch.zeros((self.AP.nout, b, nr), dtype=torch.float64, device=dev)
        self.PtY = ProductPlan(self.Pt.indptr, self.Pt.indices, self.AP.indptr, self.AP.indices, nagg)
        self.PtY.keys = None
        self.Ac = BlockCSR(self.PtY.indptr, self.PtY.indices,
                           torch.zeros((self.PtY.nout, nr, nr), dtype=torch.float64, device=dev), nagg)
        # the unit diagonal of the dead rotations, as offsets into Ac's values
        I, k = torch.nonzero(mc, as_tuple=True)
        self.unit_diagonal = (self.Ac.diagonal_block_slots()[I] * nr + k) * nr + k
        self.smoothed = False

    def smooth(self, A, Dinv: torch.Tensor, lmax: float):
        """P = M_f (T - omega D^-1 A T), omega = 4 / (3 lmax), and its stored transpose."""
        P = self.P
        self.AT.numeric(_values(A), self.T.data, P.data)
        rows = P.block_rows()
        torch.bmm(Dinv[rows], P.data.clone(), out=P.data)
        P.data.mul_(-4.0 / (3.0 * float(lmax)))
        P.data[self.tslot] += self.T.data
        if self.marker is not None:
            P.data.mul_((self.marker.view(self.n, self.b)[rows] == 0).to(torch.float64)[:, :, None])
        self.Pt.data.copy_(P.data[self.tperm].transpose(1, 2))
        self.smoothed = True

    def galerkin(self, A) -> BlockCSR:
        """Ac = P^T (A P) from the current values of A, a unit diagonal on the dead rotations."""
        self.AP.numeric(_values(A), self.P.data, self.Y)
        self.PtY.numeric(self.Pt.data, self.Y, self.Ac.data)
        if self.unit_diagonal.numel():
            self.Ac.data.view(-1).index_fill_(0, self.unit_diagonal, 1.0)
        return self.Ac

    def list_bytes(self) -> int:
        """Device bytes of the three product lists (two int32 per product, one int64 per output block)."""
        return sum(8 * p.nprod + 8 * (p.nout + 1) for p in (self.AT, self.AP, self.PtY))
