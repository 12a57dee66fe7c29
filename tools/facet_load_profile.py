"""The residual with a surface load, for a kernel-trace run ("Exterior-facet loads"):

    rocprofv3 --kernel-trace --stats -d OUT -o run --output-format csv -- \\
        python tools/facet_load_profile.py [--side 96] [--degree 2] [--reps 5] [--no-loads]

P2 tetrahedra on a side^3 x 6 box, linear elasticity with a random state, pressure on the face x = 1:
``--reps`` calls of ``fem.assemble_vector`` after one warm-up call (k_vector, then k_facet_load). With
``--no-loads`` the form has no loads: the kernel list must then be the one of a library without the feature
(FEMASM_LIB selects the library)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fem-libraries_amd"))

import torch  # noqa: E402

from femasm import fem, mesh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=96)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-loads", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    m = mesh.create_unit_cube(a.side, a.side, a.side, cell_type=mesh.CellType.tetrahedron, device=dev)
    V = fem.functionspace(m, ("Lagrange", a.degree, (3,)))
    g = torch.Generator().manual_seed(0)
    u = (1e-3 * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).to(dev)
    kw = {}
    nf = 0
    if not a.no_loads:
        f = mesh.locate_entities_boundary(m, 2, lambda x: torch.isclose(x[0], torch.ones_like(x[0])))
        nf = int(f.numel())
        kw["loads"] = [fem.SurfaceLoad(V, f, pressure=2.0)]
    L = fem.LinearElasticity(V, E=1.0, nu=0.3, u=u, **kw)
    b = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
    for _ in range(1 + a.reps):
        b.zero_()
        fem.assemble_vector(L, b)
    torch.cuda.synchronize()
    print(f"{m.num_cells} cells, {V.num_nodes} nodes, {nf} loaded facets, {a.reps} residuals, |b| = {float(b.norm()):.6e}")


if __name__ == "__main__":
    main()
