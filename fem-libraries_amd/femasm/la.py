"""Global sparse matrix in torch tensors — the dolfinx.la.MatrixCSR / PETSc BAIJ role.

Storage is block CSR with block size bs = gdim (dolfinx's blocked dofmap: dof = node*bs + comp):
``indptr`` int64 [nrows+1], ``indices`` int32 [nblocks] sorted per row, ``data`` float64
[nblocks, bs, bs] row-major blocks. For config E (202 M dofs) this keeps the index arrays at
7.7 GB instead of 69 GB for scalar CSR (SURVEY.md §7 "Memory").
"""
from __future__ import annotations

import numpy as np
import torch


# Largest single values allocation by default (create_matrix(max_part_bytes=...) sets another);
# larger matrices are split into row parts (each assembled through the fa_bsr row window).
# Config E (138 GB) fits one part on a 288 GB MI355X.
MAX_PART_BYTES = 200 * (1 << 30)


class MatrixCSR:
    """Block-CSR matrix; values may be split into row parts (each its own allocation).

    ``parts``: list of (row_begin, row_end, data[indptr[row_end]-indptr[row_begin], bs, bs]).
    """

    def __init__(self, indptr: torch.Tensor, indices: torch.Tensor, bs: int, data: torch.Tensor | None = None,
                 max_part_bytes: int = MAX_PART_BYTES, window: tuple | None = None):
        self.indptr = indptr
        self.indices = indices
        self.bs = int(bs)
        nrows = int(indptr.shape[0] - 1)
        if data is not None:
            self.parts = [(0, nrows, data)]
            return
        if window is not None:  # only rows [r0, r1) are held (a rank's rows)
            r0, r1 = int(window[0]), int(window[1])
            n = int(indptr[r1]) - int(indptr[r0])
            self.parts = [(r0, r1, torch.zeros((n, self.bs, self.bs), dtype=torch.float64, device=indices.device))]
            return
        block_bytes = 8 * self.bs * self.bs
        nb = int(indices.shape[0])
        cap = max(1, max_part_bytes // block_bytes)
        bounds = [0]
        if nb > cap:
            targets = torch.arange(cap, nb, cap, device=indptr.device, dtype=torch.int64)
            cuts = torch.searchsorted(indptr, targets, right=True) - 1
            bounds += sorted({int(c) for c in cuts.cpu().tolist() if 0 < int(c) < nrows})
        bounds.append(nrows)
        self.parts = []
        for r0, r1 in zip(bounds[:-1], bounds[1:]):
            n = int(indptr[r1]) - int(indptr[r0])
            self.parts.append((r0, r1, torch.zeros((n, self.bs, self.bs), dtype=torch.float64, device=indices.device)))

    @property
    def data(self) -> torch.Tensor:
        """All values [nblocks, bs, bs] (a concatenated copy when the matrix has several parts)."""
        if len(self.parts) == 1:
            return self.parts[0][2]
        return torch.cat([p[2] for p in self.parts])

    @property
    def num_block_rows(self) -> int:
        return int(self.indptr.shape[0] - 1)

    @property
    def num_blocks(self) -> int:
        return int(self.indices.shape[0])

    @property
    def shape(self):
        n = self.num_block_rows * self.bs
        return (n, n)

    @property
    def nnz(self) -> int:
        return self.num_blocks * self.bs * self.bs

    def zero(self):
        for _, _, d in self.parts:
            d.zero_()

    def to_scipy(self):
        """scipy.sparse.bsr_matrix on the host (test / debug helper)."""
        import scipy.sparse as sp

        return sp.bsr_matrix(
            (self.data.detach().cpu().numpy(), self.indices.cpu().numpy(), self.indptr.cpu().numpy()),
            shape=self.shape)

    def to_dense(self) -> np.ndarray:
        return self.to_scipy().toarray()

    def row_blocks(self, rows) -> tuple[list, list]:
        """Column indices and value blocks of the given block rows (host numpy), across parts."""
        ip = self.indptr
        out_c, out_v = [], []
        for r in rows:
            r = int(r)
            for r0, r1, d in self.parts:
                if r0 <= r < r1:
                    b, e = int(ip[r]), int(ip[r + 1])
                    base = int(ip[r0])
                    out_c.append(self.indices[b:e].cpu().numpy())
                    out_v.append(d[b - base:e - base].cpu().numpy())
                    break
        return out_c, out_v

    def diagonal_block_slots(self) -> torch.Tensor:
        """Slot index of the diagonal block of every row (-1 if absent)."""
        rows = torch.repeat_interleave(torch.arange(self.num_block_rows, device=self.indices.device),
                                       self.indptr[1:] - self.indptr[:-1])
        hit = rows == self.indices.to(torch.int64)
        out = torch.full((self.num_block_rows,), -1, dtype=torch.int64, device=self.indices.device)
        out[rows[hit]] = torch.nonzero(hit).reshape(-1)
        return out

    def _fa_bsr(self, part: int = 0):
        """The C-ABI view (fa_bsr) of one row part."""
        from . import _lib

        r0, r1, data = self.parts[part]
        b = _lib.fa_bsr()
        b.nrows = self.num_block_rows
        b.bs = self.bs
        b.nblocks = self.num_blocks
        b.indptr = self.indptr.data_ptr()
        b.indices = self.indices.data_ptr()
        b.data = data.data_ptr()
        b.row_begin = r0
        b.row_end = r1
        return b

    def mult(self, x: torch.Tensor, y: torch.Tensor | None = None) -> torch.Tensor:
        """y = A x for a dof vector x [nrows*bs] (HIP BSR SpMV, fa_bsr_mult, per row part)."""
        import ctypes

        from . import _lib

        L = _lib.load()
        if y is None:
            y = torch.empty_like(x)
        sh = _lib.stream_handle(x.device)
        for part in range(len(self.parts)):
            fb = self._fa_bsr(part)
            _lib.check(L.fa_bsr_mult(ctypes.byref(fb), x.data_ptr(), y.data_ptr(), sh), "fa_bsr_mult")
        return y

    def block_diagonal(self) -> torch.Tensor:
        """Diagonal blocks [nrows, bs, bs] (fa_bsr_block_diag; zeros where a row has none)."""
        import ctypes

        from . import _lib

        L = _lib.load()
        out = torch.empty((self.num_block_rows, self.bs, self.bs), dtype=torch.float64, device=self.indices.device)
        sh = _lib.stream_handle(out.device)
        for part in range(len(self.parts)):
            fb = self._fa_bsr(part)
            r0 = self.parts[part][0]
            _lib.check(L.fa_bsr_block_diag(ctypes.byref(fb), out[r0:].data_ptr(), sh), "fa_bsr_block_diag")
        return out


class BlockCSR:
    """Block-CSR matrix with rectangular row-major blocks: ``indptr`` int64 [nrows+1], ``indices`` int32
    [nblocks] block columns, ``data`` float64 [nblocks, br, bc], ``num_block_cols`` block columns. Holds the
    prolongators of ``mg.SmoothedAggregation``, their stored transposes and its coarse matrices (square,
    3- or 6-dof nodes). ``mult`` is fa_bcsr_mult on the device and the same gather in torch on the CPU."""

    def __init__(self, indptr: torch.Tensor, indices: torch.Tensor, data: torch.Tensor, num_block_cols: int):
        if data.dim() != 3 or data.dtype != torch.float64 or data.shape[0] != indices.shape[0]:
            raise ValueError("data must be a float64 tensor [nblocks, br, bc]")
        self.indptr = indptr.to(torch.int64).contiguous()
        self.indices = indices.to(torch.int32).contiguous()
        self.data = data.contiguous()
        self.br, self.bc = int(data.shape[1]), int(data.shape[2])
        self.num_block_cols = int(num_block_cols)
        self._rows = self._diag = None

    @property
    def bs(self) -> int:
        if self.br != self.bc:
            raise ValueError(f"a matrix of {self.br} x {self.bc} blocks has no single block size")
        return self.br

    @property
    def num_block_rows(self) -> int:
        return int(self.indptr.shape[0] - 1)

    @property
    def num_blocks(self) -> int:
        return int(self.indices.shape[0])

    @property
    def shape(self):
        return (self.num_block_rows * self.br, self.num_block_cols * self.bc)

    @property
    def nnz(self) -> int:
        return self.num_blocks * self.br * self.bc

    def block_rows(self) -> torch.Tensor:
        """Block row of every stored block, int64 [nblocks] (cached)."""
        if self._rows is None:
            self._rows = torch.repeat_interleave(torch.arange(self.num_block_rows, device=self.indices.device),
                                                 self.indptr[1:] - self.indptr[:-1])
        return self._rows

    def to_scipy(self):
        """scipy.sparse.bsr_matrix on the host (test / debug helper)."""
        import scipy.sparse as sp

        return sp.bsr_matrix((self.data.detach().cpu().numpy(), self.indices.cpu().numpy(), self.indptr.cpu().numpy()),
                             shape=self.shape, blocksize=(self.br, self.bc))

    def mult(self, x: torch.Tensor, y: torch.Tensor | None = None, add: bool = False) -> torch.Tensor:
        """y (+)= B x; x [num_block_cols * bc], y [num_block_rows * br]."""
        if y is None:
            if add:
                raise ValueError("add needs y")
            y = torch.empty(self.shape[0], dtype=torch.float64, device=x.device)
        for v, n in ((x, self.shape[1]), (y, self.shape[0])):
            if v.dtype != torch.float64 or v.numel() != n or not v.is_contiguous() or v.device != self.data.device:
                raise ValueError(f"BlockCSR.mult vectors must be contiguous float64 of {self.shape[1]} and "
                                 f"{self.shape[0]} entries on {self.data.device}")
        if x.device.type != "cuda":
            prod = torch.bmm(self.data, x.view(-1, self.bc)[self.indices.to(torch.int64)].unsqueeze(2)).squeeze(2)
            out = y.view(-1, self.br) if add else y.view(-1, self.br).zero_()
            out.index_add_(0, self.block_rows(), prod)  # in stored order
            return y
        from . import _lib

        _lib.check(_lib.load().fa_bcsr_mult(self.num_block_rows, self.num_block_cols, self.br, self.bc,
                                            self.indptr.data_ptr(), self.indices.data_ptr(), self.data.data_ptr(),
                                            x.data_ptr(), int(bool(add)), y.data_ptr(), _lib.stream_handle(x.device)),
                   "fa_bcsr_mult")
        return y

    def diagonal_block_slots(self) -> torch.Tensor:
        """Slot of the diagonal block of every row (-1 if absent), int64 (cached)."""
        if self._diag is None:
            rows = self.block_rows()
            hit = rows == self.indices.to(torch.int64)
            out = torch.full((self.num_block_rows,), -1, dtype=torch.int64, device=self.indices.device)
            out[rows[hit]] = torch.nonzero(hit).reshape(-1)
            self._diag = out
        return self._diag

    def block_diagonal(self) -> torch.Tensor:
        """Diagonal blocks [nrows, bs, bs] (zeros where a row has none)."""
        slots = self.diagonal_block_slots()
        D = self.data[slots.clamp(min=0)]
        D[slots < 0] = 0.0
        return D
