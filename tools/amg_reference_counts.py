"""CPU run of the reference smoothed-aggregation implementation (tests/amg_reference.py) on the three PCG
problems of tests/test_gpu_amg.py, with the matrices and right-hand sides of the CPU oracle: prints the
iteration counts that profiles/amg/counts.txt records beside the device counts. No GPU, no libfemasm.

    python tools/amg_reference_counts.py
"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sps
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fem-libraries_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import amg_reference as R  # noqa: E402
import irregular_meshes as IM  # noqa: E402
from femasm import fem, mesh  # noqa: E402
from oracle import oracle as O  # noqa: E402

RTOL = 1e-12


def box(n):
    b = mesh.create_box((1.0, 1.0, 1.0), (n, n, n), mesh.CellType.tetrahedron)
    return mesh.Mesh(b.cell_type, b.x, b.cells, None, None)


def system(m, p):
    """(A, b, marker, cells E) of the linear problem: x = 0 clamped, x = 1 displaced by 1e-3, f_y = -1e3."""
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    g = m.gdim
    ct = int(m.cell_type)
    cells, geom, x = V.dofmap.numpy(), m.cells.numpy(), m.x.numpy()
    key = m.cell_tags.numpy() if m.cell_tags is not None else np.arange(m.num_cells)
    lam, mu = O.lame(O.e_range()[key % 200], 0.3)
    X = V.tabulate_dof_coordinates().numpy()
    mk = np.zeros((V.num_nodes, g), np.int8)
    gv = np.zeros((V.num_nodes, g))
    left, right = np.isclose(X[:, 0], X[:, 0].min()), np.isclose(X[:, 0], X[:, 0].max())
    mk[left | right] = 1
    gv[right, 0] = 1e-3
    mk, gv = mk.reshape(-1), gv.reshape(-1)
    ip, ix = O.sparsity(cells, V.num_nodes)
    vals = O.assemble_elasticity(ct, p, cells, geom, x, lam, mu, ip, ix, bc=mk, diag=1.0)
    A = sps.csr_matrix(sps.bsr_matrix((vals, ix, ip), shape=(V.num_dofs, V.num_dofs)))
    f = np.zeros(V.num_dofs)
    f[1::g] = -1e3
    b = O.assemble_residual(ct, p, cells, geom, x, lam, mu, u=np.zeros(V.num_dofs), f=f)
    b = O.apply_lifting(ct, p, cells, geom, x, lam, mu, b, mk, gv, x0=np.zeros(V.num_dofs), alpha=-1.0)
    b[mk != 0] = -gv[mk != 0]
    return V, A, b, mk, X


def main():
    O.build()
    cases = [("square.msh r=3 P1", IM.square_msh(refine=3), 1), ("square.msh r=2 P2", IM.square_msh(refine=2), 2),
             ("box 8^3 P1", box(8), 1)]
    for name, m, p in cases:
        t0 = time.time()
        V, A, b, mk, X = system(m, p)
        fine = None
        A1, mk1, X1 = A, mk, X
        if p == 2:
            V1, A1, _, mk1, X1 = system(m, 1)
            fine = (A, mk, R.edge_prolongation(mesh.entities(m, 1)[0].numpy(), m.num_vertices, m.gdim))
        M, levels = R.preconditioner(A1, X1, mk1, m.gdim, 300, fine=fine)
        its, x = R.pcg(A, b, M, RTOL)
        Dinv = R.block_jacobi_inverse(A, m.gdim)
        its_j, xj = R.pcg(A, b, lambda r: Dinv @ r, RTOL, max_it=20000)
        nnz = [L.A.nnz for L in levels]
        print(f"{name}: {V.num_dofs} dofs, levels {[L.A.shape[0] for L in levels]}, operator complexity "
              f"{sum(nnz) / nnz[0]:.3f}, reference AMG PCG {its} its, block-Jacobi PCG {its_j} its, solutions differ by "
              f"{np.linalg.norm(x - xj) / np.linalg.norm(xj):.2e} ({time.time() - t0:.1f} s)", flush=True)


if __name__ == "__main__":
    main()
