"""Regenerates the committed golden fixtures (run in the dev container, CPU only):

  square_p1_elasticity.npz   BSR pattern + values of the P1 linear-elasticity J on the
                             reference's common/data/square.msh (copied here as square.msh),
                             E = E_range[tag % 200] (libc srand(6575)), nu = 0.3, quadrature
                             degree 1 — computed by the CPU oracle (oracle/fa_oracle.c).
  config_a_p1_elasticity.npz config A (71x71 unit square, 2 triangles per square, right
                             diagonal, E = E_range[cell % 200]) with the reference bcs
                             (x=0 clamped, x=1 prescribed) — computed by the oracle.
  delaunay_tets_n4.npz       x [125, 3] f64, cells [426, 4] i32: Delaunay tetrahedra of a jittered
                             5 x 5 x 5 lattice on the unit cube (needs scipy; tests/irregular_meshes.py).

  python make_golden.py [name ...]   regenerates the named fixtures (default: all).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fem-libraries_amd"))

from femasm import fem, mesh  # noqa: E402
from oracle import oracle as O  # noqa: E402


def square():
    m = mesh.read_gmsh(os.path.join(HERE, "square.msh"), gdim=2)
    V = fem.functionspace(m, ("Lagrange", 1, (2,)))
    E = O.e_range()[m.cell_tags.numpy() % 200]
    lam, mu = O.lame(E, 0.3)
    cells = V.dofmap.numpy()
    indptr, indices = O.sparsity(cells, V.num_nodes)
    vals = O.assemble_elasticity(3, 1, cells, m.cells.numpy(), m.x.numpy(), lam, mu, indptr, indices, qdeg=1)
    np.savez_compressed(os.path.join(HERE, "square_p1_elasticity.npz"), indptr=indptr, indices=indices, data=vals,
                        E=E)


def config_a():
    import torch

    m = mesh.create_unit_square(71, 71)
    V = fem.functionspace(m, ("Lagrange", 1, (2,)))
    E = O.e_range()[np.arange(m.num_cells) % 200]
    lam, mu = O.lame(E, 0.3)
    left = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.zeros_like(x[0])))
    right = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.ones_like(x[0])))
    bcs = [fem.dirichletbc(0.0, left, V), fem.dirichletbc([0.01, 0.0], right, V)]
    marker, g = fem._combine_bcs(V, bcs)
    cells = V.dofmap.numpy()
    indptr, indices = O.sparsity(cells, V.num_nodes)
    vals = O.assemble_elasticity(3, 1, cells, m.cells.numpy(), m.x.numpy(), lam, mu, indptr, indices,
                                 bc=marker.numpy(), diag=1.0, qdeg=1)
    np.savez_compressed(os.path.join(HERE, "config_a_p1_elasticity.npz"), indptr=indptr, indices=indices, data=vals,
                        bc=marker.numpy(), g=g.numpy())


def delaunay_tets_n4():
    """An unstructured tetrahedral mesh of the unit cube: the 5 x 5 x 5 lattice (h = 1/4), every
    coordinate that does not lie on a boundary plane moved by 0.25 h U(-1, 1), Delaunay-triangulated;
    the vertex order of every cell as qhull returns it (both orientation signs occur). The archive is
    written with fixed member dates, so a rerun reproduces the file byte for byte."""
    import zipfile

    from scipy.spatial import Delaunay

    n = 4
    h = 1.0 / n
    ax = np.linspace(0.0, 1.0, n + 1)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")  # vertex k + 5 (j + 5 i) at (i, j, k) h
    x = np.stack([X.reshape(-1), Y.reshape(-1), Z.reshape(-1)], 1)
    rng = np.random.default_rng(1)
    jitter = 0.25 * h * rng.uniform(-1.0, 1.0, size=x.shape)
    inside = (x > 1e-12) & (x < 1.0 - 1e-12)  # per coordinate: a face vertex slides within its face
    x = np.where(inside, x + jitter, x)
    cells = Delaunay(x).simplices.astype(np.int32)
    with zipfile.ZipFile(os.path.join(HERE, "delaunay_tets_n4.npz"), "w", zipfile.ZIP_STORED) as z:
        for name, a in (("x", np.ascontiguousarray(x, dtype=np.float64)), ("cells", np.ascontiguousarray(cells))):
            with z.open(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w") as f:
                np.lib.format.write_array(f, a, allow_pickle=False)


if __name__ == "__main__":
    O.build()
    makers = dict(square=square, config_a=config_a, delaunay_tets_n4=delaunay_tets_n4)
    for name in sys.argv[1:] or list(makers):  # (all, or the ones named on the command line)
        makers[name]()
    print("golden fixtures written to", HERE)
