"""Irregular-valence meshes for the assembly tests, and the gather planner's targets and caps restated
(test infrastructure; never imported by the product package).

The route of every hot kernel is chosen per mesh by how many cells meet at a node: fa_plan_gather cuts
rows into chunks against an entry target, a block cap and two hard caps, and one row over the entry
target moves the whole mesh off the table gather. The structured lattices of the rest of the suite have
one valence each (24 tetrahedra at an interior vertex); the meshes here vary it:

  delaunay_tets_n4   426 Delaunay tetrahedra on 125 jittered lattice points (golden fixture; recipe in
                     tests/golden/make_golden.py), vertex valence 1 .. 36, both orientation signs
  square_msh         the reference's 98-triangle Gmsh mesh, optionally refined (392 triangles)
  fan(N)             N triangles around vertex 0
  cone(nx, ny)       the 2 nx ny triangles of a structured unit square at z = 0, each joined to an apex
                     at (0.5, 0.5, 1): one tetrahedron per base triangle, apex valence 2 nx ny

tests/test_irregular_meshes_host.py holds every case to the side of each limit it is meant to sit on.
"""
from __future__ import annotations

import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TRI, TET = 3, -4

# ------------------------------------------------------------------------------------------- limits
# Restated from fem-libraries_amd/csrc/femasm.hip (line numbers of this commit). DESIGN.md section
# "Planner targets and caps" is the prose form.
GATHER_LDS = 32768        # FA_GATHER_LDS, :1416: accumulator bytes of k_gather / k_gather_lin (P2)
GATHER_LDS_NEO = 46080    # FA_GATHER_LDS_NEO, :1421: accumulator bytes of k_gather_neo
LIN_LDS_P1 = 16384        # kLinLdsP1, :1434: accumulator bytes of k_gather_lin for P1 simplices
GATHER_MAX_ADJ = 512      # kGatherMaxAdj, :1439: adjacency entries per chunk (hard: s_adj / adjrow)
GATHER_MAX_ROWS = 128     # kGatherMaxRows, :1440: rows per chunk (hard: rowoff)
OWN_LDS = 28672           # FA_OWN_LDS, :3575: output staging bytes of k_gather_own
OWN_CCAP = 256            # FA_OWN_CCAP, :3576: cells / entries per chunk of a contribution plan
SPARSITY_CAP = 2048       # kSparsityCap, :3939: (cell, node) candidates per row of k_sparsity
LIN_THREADS = 256         # lin_threads, :4584: FA_P1TET_NT = FA_P2TET_NT = 256, and 256 for triangles
NEO_THREADS = 256         # k_gather_neo's workgroup (NTH, :3305); fa_plan_gather_form, :4890
APPLY_TILE = 256          # cells per chunk of the matrix-free apply plan (femasm_apply.hip)
# column split of an item per (cell type, degree): kSimplexShapes, :4593 (linear and neo-Hookean agree
# on all four: FA_P2TET_NSPLIT = FA_NEO_NSPLIT = 2)
NSPLIT = {(TRI, 1): 1, (TRI, 2): 2, (TET, 1): 1, (TET, 2): 2}
_GDIM = {TRI: 2, TET: 3}


def gather_maxb(neo: bool, bs2: int) -> int:
    """gather_maxb, :1428: blocks of the generic / neo-Hookean accumulator."""
    return min((GATHER_LDS_NEO if neo else GATHER_LDS) // (8 * bs2), 1023)


def lin_maxb(ct: int, p: int) -> int:
    """lin_maxb, :1436: block cap of a chunk of the linear (and damage) plan, fa_plan_gather :4859."""
    gd = _GDIM[ct]
    return LIN_LDS_P1 // (8 * gd * gd) if p == 1 else gather_maxb(False, gd * gd)


def own_maxb(ct: int) -> int:
    """own_maxb, :3578: block cap of a chunk of the block-owner plan."""
    return min(OWN_LDS // (8 * _GDIM[ct] ** 2), 1023)


def entry_target(ct: int, p: int, form: str = "lin") -> int:
    """Adjacency entries per chunk the planner aims at (a row over it gets a chunk of its own,
    k_chunk_seg :4739): workgroup threads / NSPLIT. form: "lin" | "neo" | "own"."""
    if form == "own":
        return OWN_CCAP
    return (NEO_THREADS if form == "neo" else LIN_THREADS) // NSPLIT[(ct, p)]


def block_cap(ct: int, p: int, form: str = "lin") -> int:
    """Blocks per chunk; a row over it is refused (FA_E_CAPACITY ... use FA_SCATTER)."""
    if form == "own":
        return own_maxb(ct)
    return gather_maxb(True, _GDIM[ct] ** 2) if form == "neo" else lin_maxb(ct, p)


def route(ct: int, p: int, entries: int, blocks: int, form: str = "lin") -> str:
    """The route fa_assemble_matrix(FA_GATHER) takes on a mesh whose largest row has `entries`
    adjacency entries and `blocks` blocks: "table" (k_gather_lin / k_gather_neo, one item per lane),
    "generic" (k_gather's item loop; k_gather_neo in passes of 256 items), or "refused"."""
    if entries > GATHER_MAX_ADJ or blocks > block_cap(ct, p, form):
        return "refused"
    return "table" if entries <= entry_target(ct, p, form) else "generic"


# ------------------------------------------------------------------------------------------- meshes
def delaunay_tets_n4(device=None):
    from femasm import mesh

    g = np.load(os.path.join(GOLDEN, "delaunay_tets_n4.npz"))
    x, cells = g["x"], g["cells"]
    assert x.shape == (125, 3) and x.dtype == np.float64 and cells.dtype == np.int32 and cells.shape[1] == 4
    return mesh.Mesh(mesh.CellType.tetrahedron, torch.tensor(x, device=device), torch.tensor(cells, device=device))


def square_msh(device=None, refine: int = 0):
    from femasm import mesh

    m = mesh.read_gmsh(os.path.join(GOLDEN, "square.msh"), gdim=2, device=device)
    for _ in range(refine):
        m = mesh.refine(m)
    return m


def fan(ntri: int = 300, device=None):
    """ntri triangles around vertex 0 (the unit circle cut into ntri sectors)."""
    from femasm import mesh

    t = torch.arange(ntri, dtype=torch.float64) * (2 * np.pi / ntri)
    x = torch.cat([torch.zeros(1, 2, dtype=torch.float64), torch.stack([torch.cos(t), torch.sin(t)], 1)])
    i = torch.arange(ntri)
    cells = torch.stack([torch.zeros_like(i), 1 + i, 1 + (i + 1) % ntri], 1).to(torch.int32)
    return mesh.Mesh(mesh.CellType.triangle, x.to(device), cells.to(device))


def cone(nx: int, ny: int, device=None):
    """Every triangle of create_unit_square(nx, ny) at z = 0 joined to the apex (0.5, 0.5, 1). The base
    triangles alternate in orientation, so the tetrahedra do too."""
    from femasm import mesh

    base = mesh.create_unit_square(nx, ny)
    nv = base.num_vertices
    x = torch.cat([torch.cat([base.x, torch.zeros(nv, 1, dtype=torch.float64)], 1),
                   torch.tensor([[0.5, 0.5, 1.0]], dtype=torch.float64)])
    cells = torch.cat([base.cells, torch.full((base.num_cells, 1), nv, dtype=torch.int32)], 1).contiguous()
    return mesh.Mesh(mesh.CellType.tetrahedron, x.to(device), cells.to(device))


# name -> (mesh factory(device), degrees assembled). The fans and the cone put one row over a target or cap.
CASES = {
    "delaunay": (delaunay_tets_n4, (1, 2)),
    "square": (square_msh, (1, 2)),
    "square_r1": (lambda device=None: square_msh(device, 1), (1, 2)),
    "cone98": (lambda device=None: cone(9, 8, device), (1, 2)),
    "cone1212": (lambda device=None: cone(12, 12, device), (1,)),
    "fan150": (lambda device=None: fan(150, device), (2,)),
    "fan300": (lambda device=None: fan(300, device), (1, 2)),
    "fan600": (lambda device=None: fan(600, device), (1,)),
    "fan700": (lambda device=None: fan(700, device), (1,)),
}


# ------------------------------------------------------------------------------------------- statistics
def row_stats(dofmap: np.ndarray, num_nodes: int, indptr: np.ndarray) -> dict:
    """Largest-row figures of a space from its cell dofmap [nc, nn] and its pattern's indptr: adjacency
    entries (cells at the node), blocks (distinct neighbour nodes, the row's pattern length) and
    sparsity candidates (entries x nodes per cell), each the maximum over rows, and the row that holds
    the most entries."""
    ent = np.bincount(np.asarray(dofmap).reshape(-1), minlength=num_nodes)
    blk = np.diff(indptr)
    return dict(entries=int(ent.max()), blocks=int(blk.max()), candidates=int(ent.max()) * dofmap.shape[1],
                row=int(ent.argmax()), min_entries=int(ent.min()))


def signed_volumes(x: np.ndarray, cells: np.ndarray) -> np.ndarray:
    """Signed cell volumes (areas) of a simplex mesh: det[x1 - x0, ...] / tdim!."""
    X = x[cells.astype(np.int64)]
    J = X[:, 1:, :] - X[:, :1, :]
    td = cells.shape[1] - 1
    return np.linalg.det(J) / (2.0 if td == 2 else 6.0)


def min_quality(x: np.ndarray, cells: np.ndarray) -> float:
    """Smallest cell quality, 1 for the regular simplex: 6 sqrt(2) V / l_rms^3 (tetrahedra),
    4 A / (sqrt(3) l_rms^2) (triangles), l_rms the root mean square edge length."""
    X = x[cells.astype(np.int64)]
    nv = cells.shape[1]
    l2 = np.mean([((X[:, i] - X[:, j]) ** 2).sum(1) for i in range(nv) for j in range(i + 1, nv)], axis=0)
    v = np.abs(signed_volumes(x, cells))
    q = 6.0 * np.sqrt(2.0) * v / l2 ** 1.5 if nv == 4 else 4.0 * v / (np.sqrt(3.0) * l2)
    return float(q.min())


def shortest_edge(x: np.ndarray, cells: np.ndarray) -> float:
    X = x[cells.astype(np.int64)]
    nv = cells.shape[1]
    return float(min(np.sqrt(((X[:, i] - X[:, j]) ** 2).sum(1)).min() for i in range(nv) for j in range(i + 1, nv)))
