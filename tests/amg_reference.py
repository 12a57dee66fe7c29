"""Helpers only: a scipy / numpy restatement of the smoothed-aggregation hierarchy, written from its
definition and independently of femasm.mg / femasm.amg, plus a V-cycle and PCG over it.

Definition (a level has n nodes, coordinates x, b dofs per node, matrix A, marker per dof):
1. graph = block pattern of A among the free nodes (some dof unconstrained); no edge reaches a fully
   constrained node.
2. MIS(2) with priority (((i * 2654435761) mod 2^32) << 31) + i + 1: per round the undecided nodes that hold
   the maximum over the undecided nodes within distance 2 become roots, then every undecided node within
   distance 2 of a root is removed. Roots are numbered in node order; a free node takes the largest root
   number among itself and its neighbours, else the largest aggregate number among its neighbours.
3. tentative prolongator of the rigid-body modes about the aggregate's centroid (unweighted mean).
4. aggregates with fewer than 2 (2-D) / 3 (3-D) members, or collinear members in 3-D, keep translations only:
   zero rotation columns, those coarse dofs constrained with a unit diagonal.
5. P = M_f (T - 4 / (3 lmax) D^-1 A T).  6. A_c = P^T A P.  7. stop at coarse_dofs or max_levels.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def free_nodes(marker, n, b):
    return np.ones(n, bool) if marker is None else (np.asarray(marker).reshape(n, b) == 0).any(1)


def node_graph(A, b, free):
    """Boolean node adjacency (with the diagonal) among the free nodes."""
    B = sp.bsr_matrix(A, blocksize=(b, b))
    n = B.shape[0] // b
    G = sp.csr_matrix((np.ones(B.indices.size, np.int64), B.indices, B.indptr), shape=(n, n))
    F = sp.diags(free.astype(np.int64))
    G = (F @ G @ F + F).tocsr()
    G.data[:] = 1
    return G


def aggregate(G, free):
    n = G.shape[0]
    prio = np.array([(((i * 2654435761) % 2 ** 32) << 31) + i + 1 if free[i] else 0 for i in range(n)], dtype=object)
    G2 = (G @ G).tocsr()  # distance <= 2 (G holds the diagonal)
    undecided = free.copy()
    root = np.zeros(n, bool)
    while undecided.any():
        new = []
        for i in np.nonzero(undecided)[0]:
            nb = G2.indices[G2.indptr[i]:G2.indptr[i + 1]]
            nb = nb[undecided[nb]]
            if prio[i] == max(prio[j] for j in nb):
                new.append(i)
        for i in new:
            root[i] = True
        for i in new:
            undecided[G2.indices[G2.indptr[i]:G2.indptr[i + 1]]] = False
    number = np.cumsum(root) - 1
    agg = np.full(n, -1)
    for i in np.nonzero(free)[0]:
        nb = G.indices[G.indptr[i]:G.indptr[i + 1]]
        r = [number[j] for j in nb if root[j]]
        if r:
            agg[i] = max(r)
    first = agg.copy()
    for i in np.nonzero(free & (agg < 0))[0]:
        nb = G.indices[G.indptr[i]:G.indptr[i + 1]]
        agg[i] = max(first[j] for j in nb)
    return agg, int(root.sum())


def rigid_body_modes(x, b):
    """B [n * b, nr]: translations and rotations about the origin (u = w x x in 3-D), with the extra rows of
    the nodes that carry the modes themselves (b = nr)."""
    n, gdim = x.shape
    nr = 3 if gdim == 2 else 6
    B = np.zeros((n, b, nr))
    for i in range(n):
        B[i, :gdim, :gdim] = np.eye(gdim)
        if gdim == 2:
            B[i, 0, 2], B[i, 1, 2] = -x[i, 1], x[i, 0]
        else:
            for k in range(3):
                w = np.zeros(3)
                w[k] = 1.0
                B[i, :3, 3 + k] = np.cross(w, x[i])
        if b == nr:
            B[i, gdim:, gdim:] = np.eye(nr - gdim)
    return B.reshape(n * b, nr)


def tentative(x, agg, nagg, b):
    n, gdim = x.shape
    nr = 3 if gdim == 2 else 6
    xc = np.zeros((nagg, gdim))
    dead = np.zeros(nagg, bool)
    T = sp.lil_matrix((n * b, nagg * nr))
    for I in range(nagg):
        mem = np.nonzero(agg == I)[0]
        xc[I] = x[mem].mean(0)
        dx = x[mem] - xc[I]
        if len(mem) < (2 if gdim == 2 else 3):
            dead[I] = True
        elif gdim == 3:
            M = sum(np.dot(d, d) * np.eye(3) - np.outer(d, d) for d in dx)
            ev = np.linalg.eigvalsh(M)
            dead[I] = ev[0] < 1e-10 * ev[-1]
        blocks = rigid_body_modes(dx, b).reshape(len(mem), b, nr)
        if dead[I]:
            blocks[:, :, gdim:] = 0.0
        for i, blk in zip(mem, blocks):
            T[i * b:(i + 1) * b, I * nr:(I + 1) * nr] = blk
    return T.tocsr(), xc, dead


def block_jacobi_inverse(A, b):
    n = A.shape[0] // b
    A = sp.csr_matrix(A)
    blocks = []
    for i in range(n):
        D = A[i * b:(i + 1) * b, i * b:(i + 1) * b].toarray()
        if not np.abs(D).sum():
            D = np.eye(b)
        blocks.append(np.linalg.inv(D))
    return sp.block_diag(blocks, format="csr")


def lambda_max(A, Dinv):
    """The largest eigenvalue of D^-1 A (the reference's own: a dense generalised eigenvalue up to 3000 dofs,
    Lanczos to convergence above)."""
    n = A.shape[0]
    if n <= 3000:
        D = np.linalg.inv(Dinv.toarray())
        return float(sla.eigh(A.toarray(), 0.5 * (D + D.T), eigvals_only=True, subset_by_index=[n - 1, n - 1])[0])
    op = spla.LinearOperator((n, n), matvec=lambda v: Dinv @ (A @ v))
    return float(np.real(spla.eigs(op, k=1, which="LR", tol=1e-8, return_eigenvectors=False)[0]))


def edge_prolongation(edge_verts, nverts, bs):
    """The P2 -> P1 transfer on one mesh: the identity on the vertices, 1/2 and 1/2 on an edge node."""
    ev = np.asarray(edge_verts, dtype=np.int64)
    ne = ev.shape[0]
    rows = np.concatenate([np.arange(nverts), nverts + np.arange(ne), nverts + np.arange(ne)])
    cols = np.concatenate([np.arange(nverts), ev[:, 0], ev[:, 1]])
    P = sp.coo_matrix((np.concatenate([np.ones(nverts), np.full(2 * ne, 0.5)]), (rows, cols)), shape=(nverts + ne, nverts))
    return sp.kron(P.tocsr(), sp.identity(bs), format="csr")


def preconditioner(A1, x, marker1, b, coarse_dofs, fine=None, diagonal=1.0):
    """The reference V-cycle for a degree-1 matrix A1 (fine None) or for a degree-2 matrix above it (fine =
    (A2, marker2, P21), P21 the unmasked P2 -> P1 prolongation), as a function r -> z that treats the
    constrained dofs of the finest level as the preconditioners under test do; and the levels."""
    levels = hierarchy(A1, x, marker1, b, coarse_dofs)
    marker = marker1
    if fine is not None:
        A2, marker2, P21 = fine
        L = Level()
        L.A, L.b, L.marker = sp.csr_matrix(A2), b, marker2
        keep = lambda mk, n: sp.identity(n, format="csr") if mk is None else sp.diags((np.asarray(mk) == 0).astype(float))
        L.P = (keep(marker2, A2.shape[0]) @ P21 @ keep(marker1, A1.shape[0])).tocsr()
        levels = [L] + levels
        marker = marker2
    return constrained(VCycle(levels), marker, diagonal), levels


class Level:
    pass


def coarsen(A, x, marker, b, lmax=None):
    """One step: returns (P, A_c, x_c, marker_c, agg, lmax used, Dinv)."""
    A = sp.csr_matrix(A)
    n, gdim = x.shape
    nr = 3 if gdim == 2 else 6
    free = free_nodes(marker, n, b)
    agg, nagg = aggregate(node_graph(A, b, free), free)
    T, xc, dead = tentative(x, agg, nagg, b)
    Dinv = block_jacobi_inverse(A, b)
    if lmax is None:
        lmax = lambda_max(A, Dinv)
    Mf = sp.identity(n * b, format="csr") if marker is None else sp.diags((np.asarray(marker) == 0).astype(float))
    P = (Mf @ (T - (4.0 / (3.0 * lmax)) * (Dinv @ (A @ T)))).tocsr()
    mc = np.zeros((nagg, nr), np.int8)
    mc[dead, gdim:] = 1
    mc = mc.reshape(-1)
    Ac = (P.T @ A @ P + sp.diags(mc.astype(float))).tocsr()
    return P, Ac, xc, mc, agg, lmax, Dinv


def hierarchy(A, x, marker, b, coarse_dofs, max_levels=None, lmax=None):
    """Levels from the degree-1 matrix down: each has A, b, marker, x, and, unless last, P, agg, lmax.
    lmax: per-level values to use in the prolongator smoothing instead of the reference's own."""
    levels = []
    while True:
        L = Level()
        L.A, L.x, L.marker, L.b, L.P = sp.csr_matrix(A), x, marker, b, None
        levels.append(L)
        if A.shape[0] <= coarse_dofs or (max_levels is not None and len(levels) >= max_levels):
            return levels
        given = None if lmax is None else lmax[len(levels) - 1]
        L.P, A, x, marker, L.agg, L.lmax_p, _ = coarsen(L.A, x, marker, b, given)
        b = 3 if x.shape[1] == 2 else 6


def chebyshev(A, Dinv, lmax, r, z, degree, lo=0.1, hi=1.1):
    """z <- z + p(D^-1 A) D^-1 (r - A z): Chebyshev on [lo lmax, hi lmax] (Saad, algorithm 12.1)."""
    theta, delta = 0.5 * (hi + lo) * lmax, 0.5 * (hi - lo) * lmax
    sigma = theta / delta
    rho = 1.0 / sigma
    res = Dinv @ (r - A @ z)
    d = res / theta
    for k in range(degree):
        z = z + d
        if k + 1 == degree:
            break
        res = Dinv @ (r - A @ z)
        rho_new = 1.0 / (2.0 * sigma - rho)
        d = rho_new * rho * d + (2.0 * rho_new / delta) * res
        rho = rho_new
    return z


class VCycle:
    """levels: objects with A (csr), b, P (to the next level, with the constraint masks applied; None on the
    last). Chebyshev of the given degree over block-Jacobi with the reference's own lambda_max; the last level
    is inverted densely."""

    def __init__(self, levels, degree=2):
        self.levels, self.degree = levels, degree
        for L in levels[:-1]:
            L.Dinv = block_jacobi_inverse(L.A, L.b)
            L.lmax = lambda_max(L.A, L.Dinv)
        self.Ainv = np.linalg.inv(levels[-1].A.toarray())

    def cycle(self, li, r):
        L = self.levels[li]
        if li == len(self.levels) - 1:
            return self.Ainv @ r
        z = chebyshev(L.A, L.Dinv, L.lmax, r, np.zeros_like(r), self.degree)
        z = z + L.P @ self.cycle(li + 1, L.P.T @ (r - L.A @ z))
        return chebyshev(L.A, L.Dinv, L.lmax, r, z, self.degree)

    def __call__(self, r):
        return self.cycle(0, r)


def pcg(A, b, M, rtol, max_it=5000):
    """CG with the stopping rule of nls.KrylovSolver: the preconditioned residual norm against rtol times
    its initial value. Returns (iterations, x)."""
    x = np.zeros_like(b)
    r = b.copy()
    z = M(r)
    p = z.copy()
    rz = r @ z
    tol = rtol * np.linalg.norm(z)
    for it in range(1, max_it + 1):
        Ap = A @ p
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        z = M(r)
        if np.linalg.norm(z) <= tol:
            return it, x
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    raise RuntimeError("reference PCG did not converge")


def constrained(M, marker, diagonal=1.0):
    """z = M(r) on the free dofs, r / diagonal on the constrained ones (they are decoupled from the rest)."""
    if marker is None:
        return M
    on = np.asarray(marker) != 0
    return lambda r: np.where(on, r / diagonal, M(np.where(on, 0.0, r)))


def row_rel_error(got, ref):
    """max over scalar rows i of max_j |got - ref| / max_j |ref| (the bar of tests/rowparity.py); a zero
    reference row must be reproduced exactly (inf otherwise)."""
    got, ref = sp.csr_matrix(got), sp.csr_matrix(ref)
    assert got.shape == ref.shape
    err = abs(got - ref).max(axis=1).toarray().reshape(-1)
    scale = abs(ref).max(axis=1).toarray().reshape(-1)
    if np.any(err[scale == 0] > 0):
        return float("inf")
    return float((err[scale > 0] / scale[scale > 0]).max()) if np.any(scale > 0) else 0.0
