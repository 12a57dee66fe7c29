"""Meshes held in torch tensors — the dolfinx.mesh surface the reference uses.

Structured generators mirror dolfinx ``create_unit_square`` / ``create_unit_cube`` (the
synthetic inputs of BASELINE.json's configs) and the Gmsh 2.2 reader loads the
reference's own ``common/data/square.msh`` format (cell tags = physical groups, as
``gmshio``/MFEM read them: FEniCSx/mechanic2d/asym_elasto_damage_model.cc:152-162,
MFEM/mechanic2d/asym_elasto_damage_model.cc:1017-1020).

Reference-cell vertex orderings are basix's: triangle (0,0),(1,0),(0,1); tetrahedron adds
(0,0,1); quadrilateral (0,0),(1,0),(0,1),(1,1); hexahedron the tensor ordering v = i + 2j + 4k.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from enum import IntEnum

import torch


class CellType(IntEnum):
    """dolfinx.mesh.CellType values."""
    triangle = 3
    quadrilateral = 4
    tetrahedron = -4
    hexahedron = 8


GDIM = {CellType.triangle: 2, CellType.quadrilateral: 2, CellType.tetrahedron: 3, CellType.hexahedron: 3}
NVERTS = {CellType.triangle: 3, CellType.quadrilateral: 4, CellType.tetrahedron: 4, CellType.hexahedron: 8}

# basix reference sub-entities: edges as vertex pairs, faces as vertex tuples (hexahedron faces in
# the face's own tensor order v0, v1, v2, v3; tetrahedron face i is opposite vertex i)
EDGES = {
    CellType.triangle: ((1, 2), (0, 2), (0, 1)),
    CellType.tetrahedron: ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1)),
    CellType.quadrilateral: ((0, 1), (0, 2), (1, 3), (2, 3)),
    CellType.hexahedron: ((0, 1), (0, 2), (0, 4), (1, 3), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 6), (5, 7), (6, 7)),
}
HEX_FACES = ((0, 1, 2, 3), (0, 1, 4, 5), (0, 2, 4, 6), (1, 3, 5, 7), (2, 3, 6, 7), (4, 5, 6, 7))
TET_FACES = ((1, 2, 3), (0, 2, 3), (0, 1, 3), (0, 1, 2))
REF_VERTS = {
    CellType.triangle: ((0, 0), (1, 0), (0, 1)),
    CellType.tetrahedron: ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)),
    CellType.quadrilateral: ((0, 0), (1, 0), (0, 1), (1, 1)),
    CellType.hexahedron: tuple((b & 1, (b >> 1) & 1, (b >> 2) & 1) for b in range(8)),
}


def sub_entities(ct, dim: int) -> tuple:
    """Local vertex tuples of a cell's sub-entities of dimension dim (basix numbering)."""
    ct = CellType(ct)
    tdim = GDIM[ct]
    if dim == 0:
        return tuple((v,) for v in range(NVERTS[ct]))
    if dim == tdim:
        return (tuple(range(NVERTS[ct])),)
    if dim == 1:
        return EDGES[ct]
    if dim == 2 and tdim == 3:
        return TET_FACES if ct == CellType.tetrahedron else HEX_FACES
    raise ValueError(f"no sub-entities of dimension {dim} for {ct.name}")


def _facet_edges(ct):
    """Edges of each facet of a 3-D cell, as local vertex pairs (hexahedron faces: the 4 sides, not
    the diagonals)."""
    if CellType(ct) == CellType.tetrahedron:
        return tuple(((f[0], f[1]), (f[0], f[2]), (f[1], f[2])) for f in TET_FACES)
    return tuple(((f[0], f[1]), (f[0], f[2]), (f[1], f[3]), (f[2], f[3])) for f in HEX_FACES)


@dataclass
class Mesh:
    cell_type: CellType
    x: torch.Tensor  # [nverts, gdim] float64 vertex coordinates
    cells: torch.Tensor  # [ncells, nverts_per_cell] int32 geometry / topology dofmap
    cell_tags: torch.Tensor | None = None  # [ncells] int32 physical tags (E per tag)
    structured: dict | None = field(default=None, repr=False)  # lattice info for fast dofmaps
    parent: "Mesh | None" = field(default=None, repr=False)  # the mesh this one refines (refine)

    @property
    def gdim(self) -> int:
        return GDIM[self.cell_type]

    @property
    def tdim(self) -> int:
        return GDIM[self.cell_type]

    @property
    def num_cells(self) -> int:
        return int(self.cells.shape[0])

    @property
    def num_vertices(self) -> int:
        return int(self.x.shape[0])

    @property
    def device(self):
        return self.x.device

    def to(self, device) -> "Mesh":
        return Mesh(self.cell_type, self.x.to(device), self.cells.to(device),
                    None if self.cell_tags is None else self.cell_tags.to(device), self.structured,
                    None if self.parent is None else self.parent.to(device))


def _lattice_vertices(n, lengths, device):
    axes = [torch.linspace(0.0, L, k + 1, dtype=torch.float64, device=device) for k, L in zip(n, lengths)]
    grids = torch.meshgrid(*reversed(axes), indexing="ij")  # slowest = last axis
    cols = [g.reshape(-1) for g in reversed(grids)]
    return torch.stack(cols, dim=1).contiguous()


def create_unit_square(nx: int, ny: int, cell_type: CellType = CellType.triangle, diagonal: str = "right",
                       device=None) -> Mesh:
    return create_rectangle((1.0, 1.0), (nx, ny), cell_type, diagonal, device)


def create_rectangle(lengths, n, cell_type: CellType = CellType.triangle, diagonal: str = "right", device=None) -> Mesh:
    """Structured rectangle [0,Lx]x[0,Ly] with nx*ny squares; triangles split each square along
    the diagonal from (i,j) to (i+1,j+1) ("right") or (i+1,j) to (i,j+1) ("left")."""
    nx, ny = n
    cell_type = CellType(cell_type)
    x = _lattice_vertices((nx, ny), lengths, device)
    i = torch.arange(nx, device=device, dtype=torch.int64)
    j = torch.arange(ny, device=device, dtype=torch.int64)
    J, I = torch.meshgrid(j, i, indexing="ij")
    v0 = (I + (nx + 1) * J).reshape(-1)
    v1, v2, v3 = v0 + 1, v0 + nx + 1, v0 + nx + 2
    if cell_type == CellType.quadrilateral:
        cells = torch.stack([v0, v1, v2, v3], 1)
    elif cell_type == CellType.triangle:
        if diagonal == "right":
            t = torch.stack([torch.stack([v0, v1, v3], 1), torch.stack([v0, v2, v3], 1)], 1)
        else:
            t = torch.stack([torch.stack([v0, v1, v2], 1), torch.stack([v1, v2, v3], 1)], 1)
        cells = t.reshape(-1, 3)
    else:
        raise ValueError(f"2-D cell type expected, got {cell_type}")
    return Mesh(cell_type, x, cells.to(torch.int32).contiguous(), None,
                dict(kind="rect", n=(nx, ny), lengths=tuple(lengths), diagonal=diagonal))


# Kuhn subdivision of a cube into 6 tetrahedra sharing the diagonal v0-v7 (dolfinx
# create_unit_cube(..., CellType.tetrahedron)); local cube vertex v = i + 2j + 4k.
KUHN_TETS = ((0, 1, 3, 7), (0, 1, 7, 5), (0, 5, 7, 4), (0, 3, 2, 7), (0, 6, 4, 7), (0, 2, 6, 7))


def create_unit_cube(nx: int, ny: int, nz: int, cell_type: CellType = CellType.tetrahedron, device=None) -> Mesh:
    return create_box((1.0, 1.0, 1.0), (nx, ny, nz), cell_type, device)


def create_box(lengths, n, cell_type: CellType = CellType.tetrahedron, device=None, z_range=None) -> Mesh:
    """Structured box with nx*ny*nz cubes (6 Kuhn tetrahedra or 1 hexahedron each).
    ``z_range=(k0, k1)`` builds only cube layers k0..k1-1 with the GLOBAL vertex numbering
    of the full box (used to shard the mesh by slabs)."""
    nx, ny, nz = n
    cell_type = CellType(cell_type)
    x = _lattice_vertices((nx, ny, nz), lengths, device)
    k0, k1 = (0, nz) if z_range is None else z_range
    i = torch.arange(nx, device=device, dtype=torch.int64)
    j = torch.arange(ny, device=device, dtype=torch.int64)
    k = torch.arange(k0, k1, device=device, dtype=torch.int64)
    K, J, I = torch.meshgrid(k, j, i, indexing="ij")
    sx, sy = 1, nx + 1
    sz = (nx + 1) * (ny + 1)
    base = (I + sx * 0 + sy * J + sz * K).reshape(-1)
    cv = [base + (b & 1) * sx + ((b >> 1) & 1) * sy + ((b >> 2) & 1) * sz for b in range(8)]
    if cell_type == CellType.hexahedron:
        cells = torch.stack(cv, 1)
    elif cell_type == CellType.tetrahedron:
        tets = [torch.stack([cv[a] for a in t], 1) for t in KUHN_TETS]
        cells = torch.stack(tets, 1).reshape(-1, 4)
    else:
        raise ValueError(f"3-D cell type expected, got {cell_type}")
    return Mesh(cell_type, x, cells.to(torch.int32).contiguous(), None,
                dict(kind="box", n=(nx, ny, nz), lengths=tuple(lengths), z_range=(k0, k1)))


_GMSH_TYPES = {2: CellType.triangle, 3: CellType.quadrilateral, 4: CellType.tetrahedron, 5: CellType.hexahedron}


def read_gmsh(path: str, gdim: int | None = None, device=None) -> Mesh:
    """Read a Gmsh 2.2 ASCII file (the format of the reference's common/data/square.msh).
    Keeps the highest-dimension cells; cell_tags are the physical groups. Vertex order is
    converted to basix's (Gmsh quads/hexes are counter-clockwise)."""
    with open(path) as fh:
        lines = [ln.strip() for ln in fh]
    i = lines.index("$Nodes")
    nnod = int(lines[i + 1])
    ids, coords = [], []
    for ln in lines[i + 2:i + 2 + nnod]:
        p = ln.split()
        ids.append(int(p[0]))
        coords.append([float(v) for v in p[1:4]])
    i = lines.index("$Elements")
    nel = int(lines[i + 1])
    elems = {}
    for ln in lines[i + 2:i + 2 + nel]:
        p = [int(v) for v in ln.split()]
        et, ntag = p[1], p[2]
        if et in _GMSH_TYPES:
            elems.setdefault(et, []).append((p[3], p[3 + ntag:]))
    et = max(elems, key=lambda t: GDIM[_GMSH_TYPES[t]] * 10 + (1 if t in (3, 5) else 0))
    ct = _GMSH_TYPES[et]
    g = gdim or GDIM[ct]
    used = sorted({n for _, ns in elems[et] for n in ns})
    remap = {old: new for new, old in enumerate(used)}
    pos = {nid: k for k, nid in enumerate(ids)}
    x = torch.tensor([coords[pos[n]][:g] for n in used], dtype=torch.float64)
    perm = {CellType.quadrilateral: [0, 1, 3, 2], CellType.hexahedron: [0, 1, 3, 2, 4, 5, 7, 6]}.get(ct)
    cells = []
    for _, ns in elems[et]:
        c = [remap[n] for n in ns]
        if perm:
            c = [c[k] for k in perm]
        cells.append(c)
    cells = torch.tensor(cells, dtype=torch.int32)
    tags = torch.tensor([t for t, _ in elems[et]], dtype=torch.int32)
    m = Mesh(ct, x, cells, tags, None)
    return m.to(device) if device is not None else m


def _unique_rows(t: torch.Tensor):
    """(unique sorted rows of an int64 tensor [n, k], inverse index [n])."""
    if t.shape[1] == 1:
        return torch.unique(t[:, 0], return_inverse=True)
    return torch.unique(t, dim=0, return_inverse=True)


def entities(mesh: Mesh, dim: int):
    """Topology of dimension dim (dolfinx mesh.topology.create_entities): (vertex tuples of the
    entities [ne, k] int64, each cell's entity ids [ncells, n_local] int64). Entities are numbered in
    the lexicographic order of their sorted vertex tuples; dim 0 entities are the vertices themselves
    (mesh.x rows). Cached on the mesh."""
    cache = mesh.__dict__.setdefault("_entities", {})
    if dim in cache:
        return cache[dim]
    c = mesh.cells.to(torch.int64)
    if dim == 0:
        ent = torch.arange(mesh.num_vertices, device=c.device, dtype=torch.int64).reshape(-1, 1)
        out = (ent, c)
    else:
        S = torch.tensor(sub_entities(mesh.cell_type, dim), dtype=torch.int64, device=c.device)  # [nl, k]
        tup = torch.sort(c[:, S], dim=-1).values  # [nc, nl, k]
        ent, inv = _unique_rows(tup.reshape(-1, S.shape[1]))
        out = (ent.reshape(-1, S.shape[1]), inv.reshape(c.shape[0], S.shape[0]))
    cache[dim] = out
    return out


def _vertex_graph(mesh: Mesh):
    """(indptr, indices, inv_deg) of ``vertex_graph``, built once per mesh; ``inv_deg[v]`` is ``1 / deg(v)`` in
    float64 and 0 where vertex v has no neighbour (an orphan node of a Gmsh file)."""
    cached = mesh.__dict__.get("_vgraph")
    if cached is not None:
        return cached
    nv = mesh.num_vertices
    if nv > _INT32_MAX:
        raise ValueError(f"the mesh has {nv} vertices: more than the int32 indices of the vertex graph hold")
    ev, _ = entities(mesh, 1)  # rows (a, b), a < b, in lexicographic order
    dev = ev.device
    a, b = ev[:, 0], ev[:, 1]
    ne = int(ev.shape[0])
    fwd, bwd = torch.bincount(a, minlength=nv), torch.bincount(b, minlength=nv)
    deg = fwd + bwd
    indptr = torch.zeros(nv + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(deg, 0)
    # Row v is its backward neighbours (the a of the edges (a, v)) and then its forward ones (the b of the
    # edges (v, b)), each in edge order: both parts ascend, and every backward neighbour is below v, every
    # forward one above. The edges with first vertex v are consecutive; a stable sort of the second column
    # makes those with second vertex v consecutive and keeps their first vertices in edge order.
    e = torch.arange(ne, dtype=torch.int64, device=dev)
    indices = torch.empty(2 * ne, dtype=torch.int32, device=dev)
    fstart = torch.cumsum(fwd, 0) - fwd
    indices[indptr[a] + bwd[a] + (e - fstart[a])] = b.to(torch.int32)
    order = torch.argsort(b, stable=True)
    bs = b[order]
    bstart = torch.cumsum(bwd, 0) - bwd
    indices[indptr[bs] + (e - bstart[bs])] = a[order].to(torch.int32)
    degf = deg.to(torch.float64)
    inv_deg = torch.where(deg > 0, 1.0 / degf, torch.zeros_like(degf))
    out = (indptr, indices, inv_deg)
    mesh.__dict__["_vgraph"] = out
    return out


def vertex_graph(mesh: Mesh):
    """The vertex graph of the mesh as CSR, ``(indptr [nv + 1] int64, indices [nnz] int32)``: vertices v and w
    are neighbours when they share an edge of ``entities(mesh, 1)`` (any cell type; a quadrilateral's or a
    hexahedron face's diagonal is no edge). Row v lists the neighbours of v in ascending index, without
    duplicates or self loops, so ``nnz = 2 * num_edges``; a vertex no cell uses has an empty row. Built with
    torch ops on the mesh's device and cached on the mesh, as ``entities`` is."""
    indptr, indices, _ = _vertex_graph(mesh)
    return indptr, indices


def exterior_facets(mesh: Mesh) -> torch.Tensor:
    """Facet ids (entities(mesh, tdim - 1)) that belong to exactly one cell (dolfinx
    exterior_facet_indices on one process)."""
    _, cf = entities(mesh, mesh.tdim - 1)
    cnt = torch.bincount(cf.reshape(-1), minlength=int(cf.max()) + 1 if cf.numel() else 0)
    return torch.nonzero(cnt == 1, as_tuple=False).reshape(-1)


def locate_entities_boundary(mesh: Mesh, dim: int, marker) -> torch.Tensor:
    """dolfinx.mesh.locate_entities_boundary: the entities of dimension dim attached to an exterior
    facet (the facets themselves, or their edges / vertices) whose vertices ALL satisfy
    marker(x[gdim, n]). Returns sorted entity ids (int32) of entities(mesh, dim); for dim 0 these are
    vertex indices. The reference calls it with dim 0 (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:627-636,
    :651-660)."""
    tdim = mesh.tdim
    if not 0 <= dim < tdim:
        raise ValueError(f"boundary entities have dimension 0 .. {tdim - 1}, not {dim}")
    fverts, _ = entities(mesh, tdim - 1)
    ext = exterior_facets(mesh)
    dev = mesh.x.device
    if dim == tdim - 1:
        cand = ext
        cand_verts = fverts[ext]
    elif dim == 0:
        cand = torch.unique(fverts[ext].reshape(-1))
        cand_verts = cand.reshape(-1, 1)
    else:  # dim 1 of a 3-D mesh: the edges of the exterior facets
        # an exterior facet's vertices in its cell's local order give its edges (hexahedron faces:
        # the sides only); locate each exterior facet in one of its cells
        _, cf = entities(mesh, tdim - 1)
        c = mesh.cells.to(torch.int64)
        flat = cf.reshape(-1)
        is_ext = torch.zeros(fverts.shape[0], dtype=torch.bool, device=dev)
        is_ext[ext] = True
        hit = torch.nonzero(is_ext[flat], as_tuple=False).reshape(-1)
        cell, lf = hit // cf.shape[1], hit % cf.shape[1]
        FE = torch.tensor(_facet_edges(mesh.cell_type), dtype=torch.int64, device=dev)  # [nf, ne, 2]
        ev = c[cell[:, None, None], FE[lf]]  # [n, ne, 2]
        ev = torch.sort(ev.reshape(-1, 2), dim=-1).values
        everts, _ = entities(mesh, 1)
        # ids of these edges in entities(mesh, 1): search the sorted unique tuples
        key_all = everts[:, 0] * mesh.num_vertices + everts[:, 1]
        key = torch.unique(ev[:, 0] * mesh.num_vertices + ev[:, 1])
        cand = torch.searchsorted(key_all, key)
        cand_verts = everts[cand]
    ok = marker(mesh.x.T)
    ok = torch.as_tensor(ok, device=dev).to(torch.bool)
    keep = ok[cand_verts].all(dim=1)
    return cand[keep].to(torch.int32)


def locate_vertices(mesh: Mesh, marker) -> torch.Tensor:
    """Vertices whose coordinates satisfy marker(x) (x as [gdim, n], dolfinx convention)."""
    keep = marker(mesh.x.T)
    return torch.nonzero(keep, as_tuple=False).reshape(-1).to(torch.int32)


# ---------------------------------------------------------------------------------- uniform refinement
# Local vertex codes of a parent cell: its vertices 0 .. nv - 1, then the midpoints m01, m02, (m03,) m12,
# (m13, m23); with the edge order of EDGES code nv + k is local edge n_local - 1 - k.
_REFINE_TRI = ((0, 3, 4), (3, 1, 5), (4, 5, 2), (3, 5, 4))
_REFINE_TET_CORNER = ((0, 4, 5, 6), (4, 1, 7, 8), (5, 7, 2, 9), (6, 8, 9, 3))
# the four children around each diagonal of the inner octahedron (m01-m23, m02-m13, m03-m12); each child
# is the diagonal plus one edge of the cycle through the other four midpoints, its vertices ordered so
# that it keeps the parent's orientation sign
_REFINE_TET_INNER = (
    ((4, 5, 6, 9), (4, 6, 8, 9), (4, 7, 9, 8), (4, 5, 9, 7)),
    ((4, 5, 6, 8), (4, 5, 8, 7), (5, 6, 8, 9), (5, 7, 9, 8)),
    ((4, 5, 6, 7), (5, 6, 7, 9), (6, 7, 9, 8), (4, 6, 8, 7)),
)
_TET_DIAGONALS = (((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2)))
_INT32_MAX = 2 ** 31 - 1


def _refine_host(m: Mesh, ev: torch.Tensor, ce: torch.Tensor):
    """Plain-torch refinement (the definition; any device): (x, cells, tags) of refine(m)."""
    nv, nl = m.num_vertices, ce.shape[1]
    c = m.cells.to(torch.int64)
    x = torch.cat([m.x, 0.5 * (m.x[ev[:, 0]] + m.x[ev[:, 1]])], 0)
    local = torch.cat([c, nv + ce.flip(1)], 1)  # [nc, nv_cell + nl] by local vertex code
    if m.cell_type == CellType.triangle:
        cells = local[:, torch.tensor(_REFINE_TRI, dtype=torch.int64, device=c.device)]
    else:
        X = m.x[c]  # [nc, 4, 3]
        best, choice = None, torch.zeros(c.shape[0], dtype=torch.int64, device=c.device)
        for g, ((a, b), (p, q)) in enumerate(_TET_DIAGONALS):
            # every product and sum rounded on its own, in this order: fa_refine_cells computes the same bits
            df = 0.5 * (X[:, a] + X[:, b]) - 0.5 * (X[:, p] + X[:, q])
            sq = df * df
            l2 = sq[:, 0] + sq[:, 1] + sq[:, 2]
            if best is None:
                best = l2
            else:
                less = l2 < best  # ties stay with the earlier diagonal
                choice = torch.where(less, torch.full_like(choice, g), choice)
                best = torch.where(less, l2, best)
        table = torch.tensor([_REFINE_TET_CORNER + inner for inner in _REFINE_TET_INNER], dtype=torch.int64,
                             device=c.device)  # [3, 8, 4]
        cells = torch.gather(local[:, None, :].expand(-1, 8, -1), 2, table[choice])
    nchild = cells.shape[1]
    cells = cells.reshape(-1, c.shape[1]).to(torch.int32).contiguous()
    tags = None if m.cell_tags is None else m.cell_tags.repeat_interleave(nchild).contiguous()
    return x.contiguous(), cells, tags


def refine(m: Mesh) -> Mesh:
    """Regular ("red") refinement of a triangle or tetrahedron mesh (the reference scales its Gmsh mesh
    this way: MAX_REFINE with refine, -r with UniformRefinement).

    The parent's vertices keep their indices and coordinates; vertex ``nv + e`` is the midpoint of edge
    ``e`` of ``entities(m, 1)``, which is the numbering of the degree-2 nodes of ``m``: the P1 space on
    the result has the nodes of the P2 space on ``m``, in the same order. The children of cell ``c`` are
    the cells ``c * 2^tdim + k`` (the parent of child ``j`` is ``j >> tdim``), with m_ij the midpoint of
    local vertices i and j:

      triangle     (v0,m01,m02) (m01,v1,m12) (m02,m12,v2) (m01,m12,m02)
      tetrahedron  (v0,m01,m02,m03) (m01,v1,m12,m13) (m02,m12,v2,m23) (m03,m13,m23,v3), then the inner
                   octahedron split along the shortest of its diagonals (lengths from the vertex
                   coordinates, ties to the first):
        m01-m23:   (m01,m02,m03,m23) (m01,m03,m13,m23) (m01,m12,m23,m13) (m01,m02,m23,m12)
        m02-m13:   (m01,m02,m03,m13) (m01,m02,m13,m12) (m02,m03,m13,m23) (m02,m12,m23,m13)
        m03-m12:   (m01,m02,m03,m12) (m02,m03,m12,m23) (m03,m12,m23,m13) (m01,m03,m13,m12)

    Every child keeps its parent's orientation sign. ``cell_tags`` are inherited, ``structured`` is None,
    ``parent`` is ``m``. A mesh on the GPU is refined by fa_refine_cells / fa_edge_midpoints, one on the
    CPU by the same definition in torch; the two agree bit for bit."""
    if m.cell_type not in (CellType.triangle, CellType.tetrahedron):
        raise ValueError(f"refine serves triangles and tetrahedra, not {CellType(m.cell_type).name} cells")
    ev, ce = entities(m, 1)
    nv, ne, nc = m.num_vertices, int(ev.shape[0]), m.num_cells
    nchild = 2 ** m.tdim
    if nv + ne > _INT32_MAX:
        raise ValueError(f"the refined mesh has {nv + ne} vertices: more than int32 holds")
    if nc * nchild > _INT32_MAX:
        raise ValueError(f"the refined mesh has {nc * nchild} cells: more than int32 holds")
    if m.device.type != "cuda":
        x, cells, tags = _refine_host(m, ev, ce)
        return Mesh(m.cell_type, x, cells, tags, None, m)
    from . import _lib

    L = _lib.load()
    dev = m.device
    sh = _lib.stream_handle(dev)
    gdim = m.gdim
    ev32 = ev.to(torch.int32).contiguous()
    ce32 = ce.to(torch.int32).contiguous()
    mx, mc = m.x.contiguous(), m.cells.contiguous()
    x = torch.empty((nv + ne, gdim), dtype=torch.float64, device=dev)
    x[:nv] = mx
    _lib.check(L.fa_edge_midpoints(ne, gdim, ev32.data_ptr(), mx.data_ptr(), x[nv:].data_ptr(), sh),
               "fa_edge_midpoints")
    cells = torch.empty((nc * nchild, mc.shape[1]), dtype=torch.int32, device=dev)
    mt = None if m.cell_tags is None else m.cell_tags.to(torch.int32).contiguous()
    tags = None if mt is None else torch.empty(nc * nchild, dtype=torch.int32, device=dev)
    _lib.check(L.fa_refine_cells(int(m.cell_type), nc, nv, mc.data_ptr(), ce32.data_ptr(), mx.data_ptr(),
                                 _lib.ptr(mt), cells.data_ptr(), _lib.ptr(tags), sh), "fa_refine_cells")
    return Mesh(m.cell_type, x, cells, tags, None, m)


# ---------------------------------------------------------------------------------- facet tags
def _find_rows(ent: torch.Tensor, rows: torch.Tensor, what: str) -> torch.Tensor:
    """Ids in ``ent`` (the sorted unique vertex tuples of ``entities``) of the sorted vertex tuples ``rows``:
    the union's unique rows are ``ent`` again exactly when every row is one of its entities."""
    if rows.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64, device=ent.device)
    uniq, inv = _unique_rows(torch.cat([ent, rows], 0))
    if uniq.shape[0] != ent.shape[0]:
        raise ValueError(f"{what}: not an entity of the mesh")
    return inv[ent.shape[0]:]


_GMSH_SUB = {0: {15: 1}, 1: {1: 2}, 2: {2: 3, 3: 4}}  # dim -> Gmsh element type -> vertices


def read_gmsh_tags(path: str, mesh: Mesh, dim: int):
    """The lower-dimensional physical groups of a Gmsh 2.2 ASCII file as an ``io.MeshTags`` of dimension
    ``dim`` < tdim on ``mesh = read_gmsh(path)``: lines (dim 1), triangles and quadrilaterals (dim 2) or
    points (dim 0), each mapped to its id in ``entities(mesh, dim)`` (vertex indices for dim 0) and tagged
    with its physical group — the facet markers gmshio hands dolfinx next to the cell tags, which
    ``read_gmsh`` drops. Indices sorted (int32), values int32, on the mesh's device."""
    from .io import MeshTags

    if not 0 <= dim < mesh.tdim or dim not in _GMSH_SUB:
        raise ValueError(f"tags of dimension 0 .. {mesh.tdim - 1} of a {mesh.cell_type.name} mesh, not {dim}")
    with open(path) as fh:
        lines = [ln.strip() for ln in fh]
    i = lines.index("$Nodes")
    nnod = int(lines[i + 1])
    coords = {}
    for ln in lines[i + 2:i + 2 + nnod]:
        p = ln.split()
        coords[int(p[0])] = [float(v) for v in p[1:4]]
    i = lines.index("$Elements")
    nel = int(lines[i + 1])
    top = {2: CellType.triangle, 3: CellType.quadrilateral, 4: CellType.tetrahedron, 5: CellType.hexahedron}
    cell_et = {v: k for k, v in top.items()}[mesh.cell_type]
    used, sub = set(), []
    for ln in lines[i + 2:i + 2 + nel]:
        p = [int(v) for v in ln.split()]
        et, ntag = p[1], p[2]
        if et == cell_et:
            used.update(p[3 + ntag:])
        elif et in _GMSH_SUB[dim]:
            sub.append((p[3], p[3 + ntag:]))
    # read_gmsh's vertex numbering: the cells' nodes in ascending file id
    used = sorted(used)
    remap = {old: new for new, old in enumerate(used)}
    x = torch.tensor([coords[n][:mesh.gdim] for n in used], dtype=torch.float64)
    if x.shape[0] != mesh.num_vertices or not torch.equal(x, mesh.x.cpu()):
        raise ValueError(f"{path}: its cells' vertices are not the mesh's (pass the mesh read_gmsh built from it)")
    dev = mesh.device
    if not sub:
        z = torch.zeros(0, dtype=torch.int32, device=dev)
        return MeshTags(dim, z, z.clone())
    if any(n not in remap for _, ns in sub for n in ns):
        raise ValueError(f"{path}: a tagged entity of dimension {dim} has a node no cell uses")
    width = {len(ns) for _, ns in sub}
    ent, _ = entities(mesh, dim)
    if len(width) != 1 or width.pop() != ent.shape[1]:
        raise ValueError(f"{path}: tagged entities of dimension {dim} do not match the mesh's cell type")
    rows = torch.sort(torch.tensor([[remap[n] for n in ns] for _, ns in sub], dtype=torch.int64, device=dev), dim=1).values
    ids = _find_rows(ent, rows, f"{path}: a tagged entity of dimension {dim}")
    vals = torch.tensor([t for t, _ in sub], dtype=torch.int32, device=dev)
    order = torch.argsort(ids, stable=True)
    ids, vals = ids[order], vals[order]
    if ids.numel() > 1 and bool((ids[1:] == ids[:-1]).any()):
        raise ValueError(f"{path}: an entity of dimension {dim} is tagged twice")
    return MeshTags(dim, ids.to(torch.int32), vals)


def transfer_facet_tags(tags, fine: Mesh):
    """Facet tags of ``fine.parent`` carried to ``fine = refine(fine.parent)``, as an ``io.MeshTags`` of the
    same dimension: with ``refine``'s numbering (vertex ``nv + e`` is the midpoint of parent edge ``e``) a
    tagged edge (a, b) becomes its two child edges (a, m_ab), (m_ab, b), a tagged triangle (a, b, c) its
    four child triangles (a, m_ab, m_ac), (b, m_ab, m_bc), (c, m_ac, m_bc), (m_ab, m_ac, m_bc), each with the
    parent's value. ``refine`` inherits cell tags only; this keeps boundary markers through the
    refine-then-multigrid workflow. Torch only, on the meshes' device."""
    from .io import MeshTags

    coarse = fine.parent
    if coarse is None:
        raise ValueError("transfer_facet_tags needs a refined mesh (fine.parent is None)")
    if tags.dim != coarse.tdim - 1:
        raise ValueError(f"facet tags have dimension {coarse.tdim - 1}, not {tags.dim}")
    dev = fine.device
    nv = coarse.num_vertices
    ev, _ = entities(coarse, 1)
    idx = tags.indices.to(dev).to(torch.int64)
    vals = tags.values.to(dev).to(torch.int32)
    fent, _ = entities(coarse, tags.dim)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= fent.shape[0]):
        raise ValueError(f"tagged facet ids outside [0, {fent.shape[0]})")
    if tags.dim == 1:
        a, b = ev[idx, 0], ev[idx, 1]
        mid = nv + idx
        kids = torch.stack([torch.stack([a, mid], 1), torch.stack([b, mid], 1)], 1)  # [n, 2, 2]
    else:
        a, b, c = fent[idx, 0], fent[idx, 1], fent[idx, 2]  # ascending: the pairs below are sorted too
        mab = nv + _find_rows(ev, torch.stack([a, b], 1), "a tagged triangle's edge")
        mac = nv + _find_rows(ev, torch.stack([a, c], 1), "a tagged triangle's edge")
        mbc = nv + _find_rows(ev, torch.stack([b, c], 1), "a tagged triangle's edge")
        kids = torch.stack([torch.stack([a, mab, mac], 1), torch.stack([b, mab, mbc], 1),
                            torch.stack([c, mac, mbc], 1), torch.stack([mab, mac, mbc], 1)], 1)  # [n, 4, 3]
    nchild, k = kids.shape[1], kids.shape[2]
    rows = torch.sort(kids.reshape(-1, k), dim=1).values
    ids = _find_rows(entities(fine, tags.dim)[0], rows, "a child facet")
    cvals = vals.repeat_interleave(nchild)
    order = torch.argsort(ids, stable=True)
    return MeshTags(tags.dim, ids[order].to(torch.int32), cvals[order].contiguous(), getattr(tags, "name", "mesh_tags"))
