"""Meshes and start fields shared by test_damage_field_host.py and test_gpu_damage_field.py, with the
sequential reference (damage_reference.py) of each computed once per process and left unchanged."""
import functools
import os

import numpy as np
import torch

import damage_reference as R
from irregular_meshes import fan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SQUARE = os.path.join(GOLDEN, "square.msh")
TAG = 4  # the reference's tag_edges_damaged on square.msh (its USE_SQUARE setting)


def orphan_mesh(device=None):
    """Two triangles on vertices 0 .. 3 and a vertex 4 that no cell uses (an orphan node of a Gmsh file)."""
    from femasm import mesh

    x = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [2.0, 2.0]], dtype=torch.float64)
    cells = torch.tensor([[0, 1, 2], [1, 3, 2]], dtype=torch.int32)
    return mesh.Mesh(mesh.CellType.triangle, x.to(device), cells.to(device))


def square(device=None, refine: int = 0):
    """(mesh, edge tags) of square.msh, refined `refine` times with the tags carried along."""
    from femasm import mesh

    m = mesh.read_gmsh(SQUARE, gdim=2, device=device)
    t = mesh.read_gmsh_tags(SQUARE, m, 1)
    for _ in range(refine):
        m = mesh.refine(m)
        t = mesh.transfer_facet_tags(t, m)
    return m, t


def _mesh(name: str, device=None):
    from femasm import mesh

    CT = mesh.CellType
    if name == "square":
        return square(device)[0]
    if name == "square_r1":
        return square(device, 1)[0]
    if name == "unit16":  # 289 = 256 + 33 vertices: the last workgroup is partial
        return mesh.create_unit_square(16, 16, device=device)
    if name == "quads":
        return mesh.create_rectangle((1.0, 1.0), (3, 2), CT.quadrilateral, device=device)
    if name == "tets":
        return mesh.create_unit_cube(2, 2, 2, CT.tetrahedron, device=device)
    if name == "hexes":
        return mesh.create_unit_cube(2, 2, 1, CT.hexahedron, device=device)
    if name == "fan300":  # vertex 0 has 300 neighbours, every other vertex 3
        return fan(300, device)
    if name == "orphan":
        return orphan_mesh(device)
    raise KeyError(name)


MESHES = ("square", "square_r1", "unit16", "quads", "tets", "hexes", "fan300", "orphan")
GRAPH_MESHES = ("square", "quads", "tets", "hexes")
ITERATIONS = (0, 1, 8)
THRESHOLDS = (0.01, 0.0, float("inf"))


def make(name: str, device=None):
    return _mesh(name, device)


@functools.lru_cache(maxsize=None)
def adjacency(name: str):
    return R.mesh_adjacency(_mesh(name))


@functools.lru_cache(maxsize=None)
def start(name: str) -> np.ndarray:
    """A start field per mesh (read-only). square / square_r1: the vertices of the edges tagged 4 at 1.0;
    orphan: vertex 0 at 1.0 and the orphan at 0.25; the others: a few vertices at 1.0 and one at 0.5, spaced
    so that the gate separates vertices for several iterations."""
    from femasm import mesh

    m = _mesh(name)
    nv = m.num_vertices
    if name in ("square", "square_r1"):
        mm, t = square(None, 0 if name == "square" else 1)
        ev = mesh.entities(mm, 1)[0][t.find(TAG).to(torch.int64)]
        d = R.mark(nv, ev.numpy())
    elif name == "orphan":
        d = np.zeros(nv)
        d[0], d[4] = 1.0, 0.25
    else:
        d = np.zeros(nv)
        d[[1, nv // 3, nv - 2]] = 1.0
        d[nv // 2] = 0.5
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(name: str, iterations: int, threshold: float = 0.01) -> np.ndarray:
    d = R.spread(adjacency(name), start(name), iterations, threshold)
    d.setflags(write=False)
    return d
