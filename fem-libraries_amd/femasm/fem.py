"""dolfinx.fem-shaped host API over the femasm C ABI.

Mirrors the calls the reference makes on its hot path (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:
``create_functionspace`` :275-285, ``Function`` / ``Constant`` :253-262, :506-546,
``locate_dofs_topological`` + ``DirichletBC`` :620-669, ``create_form`` :679-685,
``petsc::create_matrix`` :688, ``assemble_matrix`` + ``set_diagonal`` :847-862), with the
same argument meaning: bcs zero the rows/columns of constrained dofs and ``diagonal`` is
inserted on them. Mesh, dofmaps, coefficients and the global BSR matrix are torch tensors
on the GPU; every numeric step runs in hand-written HIP kernels (libfemasm.so). There is no
CPU fallback.
"""
from __future__ import annotations

import ctypes
import weakref
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .la import MatrixCSR
from .mesh import CellType, Mesh, NVERTS

from .mesh import EDGES as _EDGES, HEX_FACES as _HEX_FACES, REF_VERTS as _REF_VERTS  # basix sub-entities

_HEX_FACE_SPAN = ((0, 1, 2), (0, 1, 4), (0, 2, 4), (1, 3, 5), (2, 3, 6), (4, 5, 6))


def is_simplex(ct) -> bool:
    return CellType(ct) in (CellType.triangle, CellType.tetrahedron)


def num_nodes_of(ct, p: int) -> int:
    ct = CellType(ct)
    return {CellType.triangle: (p + 1) * (p + 2) // 2, CellType.tetrahedron: (p + 1) * (p + 2) * (p + 3) // 6,
            CellType.quadrilateral: (p + 1) ** 2, CellType.hexahedron: (p + 1) ** 3}[ct]


def element_info(ct, degree: int, qdeg: int | None = None) -> tuple[int, int]:
    """(nodes per cell, quadrature points) of the library's element tables (fa_element_info);
    qdeg None = the degree UFL estimates for the elasticity form."""
    nn, nq = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(_lib.load().fa_element_info(int(CellType(ct)), int(degree), -1 if qdeg is None else int(qdeg),
                                           ctypes.byref(nn), ctypes.byref(nq)), "fa_element_info")
    return nn.value, nq.value


def line_points(p: int) -> np.ndarray:
    """1-D node positions: equispaced (p <= 2) or GLL (p = 3; basix gll_warped)."""
    if p == 3:
        return np.array([0.0, 0.5 * (1 - 1 / np.sqrt(5)), 0.5 * (1 + 1 / np.sqrt(5)), 1.0])
    return np.linspace(0.0, 1.0, p + 1)


def node_lattice(ct, p: int) -> np.ndarray:
    """basix local node -> integer lattice position (units of 1/p of the cell) [nn, tdim].
    For tensor cells the entries are 1-D lattice indices (GLL positions at p = 3)."""
    ct = CellType(ct)
    V = np.array(_REF_VERTS[ct]) * p
    out = [tuple(v) for v in V]
    for a, b in _EDGES[ct]:
        for s in range(1, p):
            out.append(tuple(V[a] + s * (V[b] - V[a]) // p))
    if ct == CellType.quadrilateral:
        for i in range(1, p):
            for j in range(1, p):
                out.append((i, j))
    if ct == CellType.hexahedron:
        for f in _HEX_FACE_SPAN:
            for s in range(1, p):
                for t in range(1, p):
                    out.append(tuple(V[f[0]] + s * (V[f[1]] - V[f[0]]) // p + t * (V[f[2]] - V[f[0]]) // p))
        for i in range(1, p):
            for j in range(1, p):
                for k in range(1, p):
                    out.append((i, j, k))
    if is_simplex(ct) and p > 2:
        raise NotImplementedError("simplex degree > 2")
    return np.array(out, dtype=np.int64)


def reference_nodes(ct, p: int) -> np.ndarray:
    L = node_lattice(ct, p)
    if is_simplex(ct):
        return L.astype(np.float64) / p
    return line_points(p)[L]


def _geometry_basis(ct, X: np.ndarray) -> np.ndarray:
    """P1 / Q1 geometry basis values at reference points X [n, tdim] -> [n, nverts]."""
    ct = CellType(ct)
    if is_simplex(ct):
        return np.concatenate([1.0 - X.sum(1, keepdims=True), X], axis=1)
    cols = []
    for v in _REF_VERTS[ct]:
        f = np.ones(X.shape[0])
        for d, bit in enumerate(v):
            f = f * (X[:, d] if bit else 1.0 - X[:, d])
        cols.append(f)
    return np.stack(cols, 1)


class FunctionSpace:
    """Vector (bs = gdim) or scalar Lagrange space, or DG0 (per-cell) space."""

    _prepared_builds = 0  # builds of the static part of a prepared cell state on this space (_prepared_state)

    def __init__(self, mesh: Mesh, family: str, degree: int, shape: tuple | None):
        self.mesh = mesh
        self.family = family
        self.degree = int(degree)
        self.bs = int(np.prod(shape)) if shape else 1
        self._adjacency = None
        self._pattern = None
        if family in ("DG", "Discontinuous Lagrange"):
            if degree != 0:
                raise NotImplementedError("only DG0 coefficient spaces")
            self.dofmap = torch.arange(mesh.num_cells, dtype=torch.int32, device=mesh.device).reshape(-1, 1)
            self.num_nodes = mesh.num_cells
            self.nn = 1
            return
        if family not in ("Lagrange", "P", "Q", "CG"):
            raise ValueError(f"unsupported family {family}")
        self.nn = num_nodes_of(mesh.cell_type, self.degree)
        if self.degree == 1:
            self.dofmap = mesh.cells
            self.num_nodes = mesh.num_vertices
        elif mesh.structured is not None:
            self.dofmap, self.num_nodes = _structured_dofmap(mesh, self.degree)
        else:
            self.dofmap, self.num_nodes = _generic_dofmap(mesh, self.degree)
        self._x = None

    @classmethod
    def from_dofmap(cls, mesh: Mesh, degree: int, bs: int, dofmap: torch.Tensor, num_nodes: int) -> "FunctionSpace":
        """A Lagrange space with a caller-supplied node numbering (e.g. a rank-local numbering
        of a slab of a larger mesh: femasm.parallel)."""
        V = cls.__new__(cls)
        V.mesh, V.family, V.degree, V.bs = mesh, "Lagrange", int(degree), int(bs)
        V.nn = num_nodes_of(mesh.cell_type, int(degree))
        V.dofmap = dofmap.to(torch.int32).contiguous()
        V.num_nodes = int(num_nodes)
        V._adjacency, V._pattern, V._x = None, None, None
        return V

    @property
    def num_dofs(self) -> int:
        return self.num_nodes * self.bs

    def tabulate_dof_coordinates(self) -> torch.Tensor:
        """Node coordinates [num_nodes, gdim] (the geometry map applied to the reference nodes)."""
        if self._x is None and self.mesh.structured is not None and self.degree > 1:
            self._x = _structured_node_coordinates(self.mesh, self.degree)
        if self._x is None:
            self._x = self._mapped_node_coordinates()
        return self._x

    def _mapped_node_coordinates(self) -> torch.Tensor:
        """The geometry map of the mesh's CURRENT vertices applied to the reference nodes [num_nodes, gdim]
        (not cached; the lattice shortcut of ``tabulate_dof_coordinates`` describes the generator's box, not
        a mesh whose vertices were moved afterwards)."""
        m = self.mesh
        X = reference_nodes(m.cell_type, self.degree)
        Psi = torch.tensor(_geometry_basis(m.cell_type, X), dtype=torch.float64, device=m.device)  # [nn, nv]
        xv = m.x[m.cells.to(torch.int64)]  # [nc, nv, gdim]
        xn = torch.einsum("kv,cvd->ckd", Psi, xv)
        out = torch.zeros((self.num_nodes, m.gdim), dtype=torch.float64, device=m.device)
        out[self.dofmap.to(torch.int64).reshape(-1)] = xn.reshape(-1, m.gdim)
        return out

    # native objects -------------------------------------------------------------------
    def _fa_mesh(self) -> _lib.fa_mesh:
        m = self.mesh
        s = _lib.fa_mesh()
        s.cell_type = int(m.cell_type)
        s.degree = self.degree
        s.gdim = m.gdim
        s.nn = self.nn
        s.ncells = m.num_cells
        s.nnodes = self.num_nodes
        s.cells = self.dofmap.data_ptr()
        s.nv = NVERTS[m.cell_type]
        s.geom = m.cells.data_ptr()
        s.x = m.x.data_ptr()
        return s

    def adjacency(self):
        """Node -> cell adjacency (built once on the GPU: fa_build_adjacency)."""
        if self._adjacency is None:
            L = _lib.load()
            dev = self.mesh.device
            ptr = torch.empty(self.num_nodes + 1, dtype=torch.int64, device=dev)
            idx = torch.empty(self.mesh.num_cells * self.nn, dtype=torch.int32, device=dev)
            fm = self._fa_mesh()
            _lib.check(L.fa_build_adjacency(ctypes.byref(fm), ptr.data_ptr(), idx.data_ptr(), _lib.stream_handle(dev)),
                       "fa_build_adjacency")
            self._adjacency = (ptr, idx)
        return self._adjacency

    def _fa_adjacency(self) -> _lib.fa_adjacency:
        ptr, idx = self.adjacency()
        a = _lib.fa_adjacency()
        a.ptr = ptr.data_ptr()
        a.idx = idx.data_ptr()
        return a


def _structured_dofmap(mesh: Mesh, p: int, chunk: int = 1 << 22):
    """Lattice numbering of a structured mesh's degree-p nodes: node index of lattice point
    (I, J[, K]) is I + (p nx + 1)(J + (p ny + 1) K) — neighbours stay close in memory.
    Processed in cell chunks to bound temporaries (config E has 50 M cells)."""
    st = mesh.structured
    n = st["n"]
    tdim = len(n)
    dims = [p * k + 1 for k in n]
    vdims = [k + 1 for k in n]
    dev = mesh.device
    L = torch.tensor(node_lattice(mesh.cell_type, p), dtype=torch.int64, device=dev)  # [nn, tdim]
    out = torch.empty((mesh.num_cells, L.shape[0]), dtype=torch.int32, device=dev)
    simplex = is_simplex(mesh.cell_type)
    for c0 in range(0, mesh.num_cells, chunk):
        v = mesh.cells[c0:c0 + chunk].to(torch.int64)
        vlat = []
        for d in range(tdim):
            stride = int(np.prod(vdims[:d]))
            vlat.append((v // stride) % vdims[d])
        vlat = torch.stack(vlat, -1)  # [nc, nv, tdim]
        v0 = vlat[:, 0, :]
        nl = p * v0[:, None, :]
        if simplex:
            # node lattice = p v0 + sum_k L[node, k] (v_k - v0)   (L in units of 1/p)
            for k in range(tdim):
                nl = nl + L[None, :, k, None] * (vlat[:, k + 1, :] - v0)[:, None, :]
        else:
            nl = nl + L[None, :, :]
        idx = torch.zeros(nl.shape[:2], dtype=torch.int64, device=dev)
        for d in range(tdim - 1, -1, -1):
            idx = idx * dims[d] + nl[:, :, d]
        out[c0:c0 + chunk] = idx.to(torch.int32)
    return out.contiguous(), int(np.prod(dims))


def _structured_node_coordinates(mesh: Mesh, p: int) -> torch.Tensor:
    """Node coordinates of the lattice numbering (uniform box, GLL-graded inside cells at p = 3)."""
    st = mesh.structured
    n, lengths = st["n"], st["lengths"]
    r = torch.tensor(line_points(p), dtype=torch.float64, device=mesh.device)
    axes = []
    for k, Lk in zip(n, lengths):
        i = torch.arange(p * k + 1, device=mesh.device)
        cell, loc = torch.div(i, p, rounding_mode="floor"), i % p
        cell = torch.where(i == p * k, torch.full_like(cell, k - 1), cell)
        loc = torch.where(i == p * k, torch.full_like(loc, p), loc)
        axes.append((cell.to(torch.float64) + r[loc]) * (Lk / k))
    grids = torch.meshgrid(*reversed(axes), indexing="ij")
    return torch.stack([g.reshape(-1) for g in reversed(grids)], 1).contiguous()


def _generic_dofmap(mesh: Mesh, p: int):
    """Degree-2 numbering of an unstructured mesh: vertices, then one node per edge (and per
    hex face and quad/hex cell), edges identified by their sorted vertex pair."""
    if p != 2:
        raise NotImplementedError("unstructured meshes: degree <= 2 (Q3 needs a structured mesh)")
    ct = mesh.cell_type
    c = mesh.cells.to(torch.int64)
    nv = mesh.num_vertices
    parts = [c]
    E = torch.tensor(_EDGES[ct], dtype=torch.int64, device=c.device)
    ev = c[:, E]  # [nc, ne, 2]
    lo, hi = ev.min(-1).values, ev.max(-1).values
    key = lo * nv + hi
    uniq, inv = torch.unique(key.reshape(-1), return_inverse=True)
    parts.append(nv + inv.reshape(key.shape))
    nxt = nv + uniq.numel()
    if ct == CellType.hexahedron:
        F = torch.tensor(_HEX_FACES, dtype=torch.int64, device=c.device)
        fv = torch.sort(c[:, F], dim=-1).values  # [nc, 6, 4]
        fu, finv = torch.unique(fv.reshape(-1, 4), dim=0, return_inverse=True)
        parts.append(nxt + finv.reshape(fv.shape[:2]))
        nxt += fu.shape[0]
    if ct in (CellType.quadrilateral, CellType.hexahedron):
        parts.append(nxt + torch.arange(mesh.num_cells, device=c.device).reshape(-1, 1))
        nxt += mesh.num_cells
    return torch.cat(parts, 1).to(torch.int32).contiguous(), int(nxt)


def functionspace(mesh: Mesh, element) -> FunctionSpace:
    """dolfinx.fem.functionspace(mesh, ("Lagrange", p, (gdim,))) / ("DG", 0)."""
    family, degree = element[0], element[1]
    shape = element[2] if len(element) > 2 else None
    return FunctionSpace(mesh, family, degree, shape)


class Function:
    def __init__(self, V: FunctionSpace, name: str = "f", x: torch.Tensor | None = None):
        self.function_space = V
        self.name = name
        n = V.num_nodes * V.bs
        self.x = x if x is not None else torch.zeros(n, dtype=torch.float64, device=V.mesh.device)

    @property
    def array(self) -> torch.Tensor:
        return self.x

    def eval(self, x, cells=None, grad: bool = False):
        """dolfinx ``Function.eval(x, cells)``: values [n, bs] at the physical points x [n, gdim] (``eval_points``;
        cells None: the points are located first)."""
        return eval_points(self, x, cells=cells, grad=grad)

    def interpolate(self, fn, missing: str = "raise"):
        """Nodal interpolation: fn(x[gdim, n]) -> values [bs, n] (dolfinx convention), or an
        ``Expression`` evaluated at the single interpolation point of a DG0 space
        (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:926-927: ``stress->interpolate(expr)``), or a
        ``Function`` on another mesh or space of the same block size: this space's nodes (a DG0 space: its
        cell midpoints) are located in the other function's mesh and take its values there. missing: what a
        node outside that mesh does, "raise" (ValueError with their number), "keep" (its value stays) or
        "nan"."""
        V = self.function_space
        if isinstance(fn, Function):
            return self._interpolate_function(fn, missing)
        if isinstance(fn, Expression):
            if V.family not in ("DG", "Discontinuous Lagrange") or V.degree != 0:
                raise ValueError("interpolating an Expression needs a DG0 space")
            if V.mesh is not fn.form.V.mesh:
                raise ValueError("the Expression's form lives on another mesh")
            if V.bs != fn.value_size:
                raise ValueError(f"space block size {V.bs} != the expression's value size {fn.value_size}")
            if fn.X.shape[0] != 1 or not np.array_equal(fn.X, interpolation_points(V.mesh.cell_type)):
                raise ValueError("the Expression's points must be the DG0 space's single interpolation point")
            if self.x.dtype != torch.float64 or not self.x.is_contiguous() or self.x.numel() != V.num_dofs:
                self.x = torch.empty(V.num_dofs, dtype=torch.float64, device=V.mesh.device)
            evaluate(fn.form, (fn.quantity,), X=fn.X, out={fn.quantity: self.x.view(V.num_nodes, V.bs)})
            return
        xn = V.tabulate_dof_coordinates()
        vals = fn(xn.T)
        vals = torch.as_tensor(vals, dtype=torch.float64, device=xn.device).reshape(V.bs, -1)
        self.x = vals.T.contiguous().reshape(-1)

    def _interpolate_function(self, other: "Function", missing: str):
        if missing not in ("raise", "keep", "nan"):
            raise ValueError(f"missing must be 'raise', 'keep' or 'nan', not {missing!r}")
        V, W = self.function_space, other.function_space
        if V.bs != W.bs:
            raise ValueError(f"block size {V.bs} != the other function's {W.bs}")
        if V.mesh.device != W.mesh.device:
            raise ValueError("the two functions live on different devices")
        if V.mesh.gdim != W.mesh.gdim:
            raise ValueError("the two meshes have different dimensions")
        if V.family in ("DG", "Discontinuous Lagrange"):
            m = V.mesh
            Psi = torch.tensor(_geometry_basis(m.cell_type, interpolation_points(m.cell_type)), dtype=torch.float64,
                               device=m.device)
            xn = torch.einsum("qv,cvd->cqd", Psi, m.x[m.cells.to(torch.int64)]).reshape(-1, m.gdim)
        else:
            xn = V._mapped_node_coordinates()  # (the mesh's current vertices, whatever generated it)
        from . import geometry

        cells, X = geometry.locate_points(W.mesh, xn)
        vals = eval_points(other, xn, cells=cells, X=X)
        found = cells >= 0
        nmiss = int((~found).sum())
        if nmiss and missing == "raise":
            raise ValueError(f"interpolate: {nmiss} of {xn.shape[0]} nodes lie outside the other function's mesh")
        if nmiss and missing == "keep":
            vals = torch.where(found[:, None], vals, self.x.view(-1, V.bs))
        self.x = vals.contiguous().reshape(-1)


class Constant:
    def __init__(self, mesh_or_value, value=None):
        self.value = float(mesh_or_value if value is None else value)

    def __float__(self):
        return self.value


@dataclass
class DirichletBC:
    """Constrained dofs of V with their prescribed values (blocked dof = node*bs + comp)."""
    V: FunctionSpace
    dofs: torch.Tensor  # int64 dof indices
    g: torch.Tensor  # float64 [num_dofs] prescribed values (0 elsewhere)

    def marker(self) -> torch.Tensor:
        m = torch.zeros(self.V.num_dofs, dtype=torch.int8, device=self.dofs.device)
        m[self.dofs] = 1
        return m


def locate_dofs_geometrical(V: FunctionSpace, marker) -> torch.Tensor:
    """Nodes whose coordinates satisfy marker(x[gdim, n]); returns node indices (int64)."""
    xn = V.tabulate_dof_coordinates()
    return torch.nonzero(marker(xn.T), as_tuple=False).reshape(-1)


def _closure_nodes(ct, p: int, S) -> list:
    """Local nodes (basix order) in the closure of the reference sub-entity with local vertices S:
    simplices, barycentric coordinates of the vertices outside S vanish; tensor cells, the node lies
    on every coordinate plane all vertices of S share."""
    ct = CellType(ct)
    X = reference_nodes(ct, p)
    RV = np.array(_REF_VERTS[ct], dtype=np.float64)
    on = np.ones(X.shape[0], dtype=bool)
    if is_simplex(ct):
        lam = np.concatenate([1.0 - X.sum(1, keepdims=True), X], axis=1)  # [nn, nv]
        for v in range(RV.shape[0]):
            if v not in S:
                on &= np.abs(lam[:, v]) < 1e-12
    else:
        for d in range(RV.shape[1]):
            vals = {RV[v, d] for v in S}
            if len(vals) == 1:
                on &= np.abs(X[:, d] - vals.pop()) < 1e-12
    return [int(j) for j in np.nonzero(on)[0]]


def locate_dofs_topological(V: FunctionSpace, entity_dim: int, entities) -> torch.Tensor:
    """dolfinx.fem.locate_dofs_topological: the nodes (block dofs) in the closure of the given
    entities of dimension entity_dim (ids of femasm.mesh.entities; vertex indices for dim 0).
    Closure semantics as dolfinx: a vertex carries only its own node, an edge its vertices' and its
    interior nodes, a facet every node on it. The reference selects with entity_dim 0
    (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:637-638, :661-662), which for P >= 2 constrains
    the vertex nodes of the plane only. Returns sorted node indices (int64)."""
    from . import mesh as fmesh

    m = V.mesh
    ents = torch.as_tensor(entities, device=m.device).to(torch.int64).reshape(-1)
    _, cell_ents = fmesh.entities(m, entity_dim) if entity_dim < m.tdim else \
        (None, torch.arange(m.num_cells, device=m.device, dtype=torch.int64).reshape(-1, 1))
    nent = int(cell_ents.max()) + 1 if cell_ents.numel() else 0
    mark = torch.zeros(max(nent, int(ents.max()) + 1 if ents.numel() else 0), dtype=torch.bool, device=m.device)
    mark[ents] = True
    dm = V.dofmap.to(torch.int64)
    out = []
    for i, S in enumerate(fmesh.sub_entities(m.cell_type, entity_dim)):
        loc = torch.tensor(_closure_nodes(m.cell_type, V.degree, S), dtype=torch.int64, device=m.device)
        hit = mark[cell_ents[:, i]]
        if bool(hit.any()):
            out.append(dm[hit][:, loc].reshape(-1))
    if not out:
        return torch.zeros(0, dtype=torch.int64, device=m.device)
    return torch.unique(torch.cat(out))


def dirichletbc(value, nodes: torch.Tensor, V: FunctionSpace, components=None) -> DirichletBC:
    """Constrain all (or the given) components of `nodes` to `value` (a scalar or a bs-vector)."""
    bs = V.bs
    comps = list(range(bs)) if components is None else list(components)
    val = torch.as_tensor(value, dtype=torch.float64, device=nodes.device).reshape(-1)
    if val.numel() == 1:
        val = val.expand(bs)
    nodes = nodes.to(torch.int64)
    dofs = torch.cat([nodes * bs + c for c in comps]) if nodes.numel() else nodes
    g = torch.zeros(V.num_dofs, dtype=torch.float64, device=nodes.device)
    for c in comps:
        g[nodes * bs + c] = val[c]
    return DirichletBC(V, dofs, g)


def _bc_state(bc, with_g: bool):
    # the exact tensor objects a bc holds (weakly) and their in-place versions: a hit needs the same
    # objects at the same versions, so a reassigned bc.dofs / bc.g (even one the caching allocator
    # put at a freed tensor's address) or an edited one misses the cache
    st = [weakref.ref(bc), weakref.ref(bc.dofs), bc.dofs._version]
    if with_g:
        st += [weakref.ref(bc.g), bc.g._version]
    return st


def _bc_state_ok(st, bc, with_g: bool) -> bool:
    if st[0]() is not bc or st[1]() is not bc.dofs or st[2] != bc.dofs._version:
        return False
    return not with_g or (st[3]() is bc.g and st[4] == bc.g._version)


def _combine_bcs(V: FunctionSpace, bcs, with_g: bool = True):
    """(marker int8 [num_dofs], g f64 [num_dofs] or None) of a bcs list, cached on V per bcs set
    (a Newton loop assembles with the same bcs every iteration: the marker is built once, not in
    every timed assembly). with_g=False: the matrix assembly needs the marker only."""
    if not bcs:
        return None, None
    cache = V.__dict__.setdefault("_bc_cache", {})
    key = (with_g,) + tuple(id(bc) for bc in bcs)
    hit = cache.get(key)
    if hit is not None and all(_bc_state_ok(st, bc, with_g) for st, bc in zip(hit[2], bcs)):
        return hit[0], hit[1]
    marker = torch.zeros(V.num_dofs, dtype=torch.int8, device=V.mesh.device)
    g = torch.zeros(V.num_dofs, dtype=torch.float64, device=V.mesh.device) if with_g else None
    for bc in bcs:
        marker[bc.dofs] = 1
        if with_g:
            g[bc.dofs] = bc.g[bc.dofs]
    cache.pop(key, None)
    if len(cache) >= 8:  # a handful of bcs sets per space; drop the oldest
        cache.pop(next(iter(cache)))
    # weak references only (a bc refers to V: strong ones would make a cycle that keeps V's tensors
    # alive until a GC pass); a hit is checked against them, so a reused id cannot match
    cache[key] = (marker, g, [_bc_state(bc, with_g) for bc in bcs])
    return marker, g


# ---------------------------------------------------------------------------------- forms
class LinearElasticity:
    """J of the reference form with damage d = 0:
    inner(sigma(du), eps(v)) dx, sigma = lmbda tr(eps) I + 2 mu eps, mu = E/(2(1+nu)),
    lmbda = E nu/((1+nu)(1-2nu))  (FEniCSx/mechanic2d/asym_ufl.py:22-34, :78-83).
    E: DG0 Function / per-cell tensor / float; nu: Constant / float. Alternatively lam & mu per cell.
    loads: ``SurfaceLoad`` objects on V; ``assemble_vector`` subtracts each after the cell term (dead loads:
    the matrix and the Jacobian action do not see them)."""
    kind = _lib.FA_LINEAR_ELASTICITY

    def __init__(self, V: FunctionSpace, E=None, nu=0.3, lam=None, mu=None, quadrature_degree: int | None = None,
                 u=None, f=None, loads=None):
        self.V = V
        self.loads = _check_loads(V, loads)
        nc = V.mesh.num_cells
        dev = V.mesh.device
        self.nu = float(nu)
        self.E = self.lam = self.mu = None
        if E is not None:
            self.E = _cellwise(E, nc, dev)
        else:
            self.lam, self.mu = _cellwise(lam, nc, dev), _cellwise(mu, nc, dev)
        self.qdeg = -1 if quadrature_degree is None else int(quadrature_degree)
        self.d = None
        # state (residual / nonlinear tangents) and body force, per dof; Functions or tensors
        self.u = None if u is None else (u.x if isinstance(u, Function) else u)
        self.f = None if f is None else (f.x if isinstance(f, Function) else f)


class AsymDamage(LinearElasticity):
    """The reference mechanic2d J: derivative of inner(sigma(u), eps(v)) dxx with the
    asymmetric tension/compression damage law, P1 triangles, one quadrature point
    (FEniCSx/mechanic2d/asym_ufl.py:36-81; MFEM/mechanic2d/asym_elasto_damage_model.cc:639-916).
    u: displacement Function, d: damage (P1 scalar Function or per-node tensor)."""
    kind = _lib.FA_ASYM_DAMAGE

    def __init__(self, V: FunctionSpace, E=None, nu=0.3, u=None, d=None, lam=None, mu=None, f=None,
                 tangent: str = "hand", loads=None):
        """tangent: "hand" (the reference's default build: eigen-decomposition tangent and stress,
        :207-329, :766-881) or "ad" (its USE_AD build: forward-over-forward AD of the damage
        potential, :100-204, :752-763)."""
        super().__init__(V, E=E, nu=nu, lam=lam, mu=mu, quadrature_degree=1, u=u, f=f, loads=loads)
        self.d = None if d is None else (d.x if isinstance(d, Function) else d)
        if tangent not in ("hand", "ad"):
            raise ValueError(f"tangent must be 'hand' or 'ad', not {tangent!r}")
        self.tangent = tangent
        if tangent == "ad":
            self.kind = _lib.FA_ASYM_DAMAGE_AD


class NeoHookean(LinearElasticity):
    """Compressible neo-Hookean tangent (BASELINE config E): psi = mu/2 (I_C - 3) - mu ln J +
    lmbda/2 (ln J)^2, F = I + grad u; J = derivative of the first Piola stress, taken on the
    GPU by forward-over-forward automatic differentiation of psi (the pattern of the reference's
    MFEM AD, MFEM/mechanic2d/autodiff/admfem.hpp:672-700). u: the state (required)."""
    kind = _lib.FA_NEO_HOOKEAN

    def __init__(self, V: FunctionSpace, E=None, nu=0.3, u=None, lam=None, mu=None, quadrature_degree=None, f=None,
                 loads=None):
        if u is None:
            raise ValueError("NeoHookean needs the state u")
        super().__init__(V, E=E, nu=nu, lam=lam, mu=mu, quadrature_degree=quadrature_degree, u=u, f=f, loads=loads)


def _check_loads(V: FunctionSpace, loads):
    """The loads list of a form on V (None when there is none)."""
    if not loads:
        return None
    loads = [loads] if isinstance(loads, SurfaceLoad) else list(loads)
    for ld in loads:
        if not isinstance(ld, SurfaceLoad):
            raise TypeError(f"loads holds a {type(ld).__name__}, not a SurfaceLoad")
        if ld.V is not V and (ld.V.mesh is not V.mesh or ld.V.degree != V.degree or ld.V.num_dofs != V.num_dofs):
            raise ValueError("a SurfaceLoad of another function space")
    return loads


def _cellwise(v, nc, dev):
    if isinstance(v, Function):
        v = v.x
    t = torch.as_tensor(v, dtype=torch.float64, device=dev)
    if t.numel() == 1:
        t = t.reshape(1).expand(nc)
    return t.contiguous()


def form(a):
    """dolfinx.fem.form analogue: forms are ready-made descriptors here (no code generation);
    returns the argument after validating it."""
    if not isinstance(a, LinearElasticity):
        raise TypeError("expected a femasm form descriptor (LinearElasticity, AsymDamage, ...)")
    return a


def _fa_form(a) -> _lib.fa_form:
    f = _lib.fa_form()
    f.kind = a.kind
    f.qdeg = a.qdeg
    f.E = _lib.ptr(a.E)
    f.nu = a.nu
    f.lam = _lib.ptr(a.lam)
    f.mu = _lib.ptr(a.mu)
    f.u = _lib.ptr(a.u)
    f.d = _lib.ptr(a.d)
    f.f = _lib.ptr(a.f)
    return f


def check_pattern(V: FunctionSpace, indptr: torch.Tensor, indices: torch.Tensor):
    """Validate a pattern of V and V's adjacency on the device (fa_check_pattern): sorted unique
    in-range columns, monotone indptr, exactly the node pairs of the cells. Raises FemasmError."""
    fm = V._fa_mesh()
    adj = V._fa_adjacency()
    _lib.check(_lib.load().fa_check_pattern(ctypes.byref(fm), ctypes.byref(adj), indptr.data_ptr(), indices.data_ptr(),
                                            int(indices.numel()), _lib.stream_handle(V.mesh.device)),
               "fa_check_pattern")


def sparsity_pattern(V: FunctionSpace):
    """The BSR pattern (indptr, indices) of V's cell node pairs, built on the GPU once and cached on V
    (dolfinx.fem.create_sparsity_pattern; create_matrix uses it)."""
    if V._pattern is None:
        L = _lib.load()
        dev = V.mesh.device
        fm = V._fa_mesh()
        adj = V._fa_adjacency()
        indptr = torch.empty(V.num_nodes + 1, dtype=torch.int64, device=dev)
        nb = ctypes.c_int64(0)
        sh = _lib.stream_handle(dev)
        _lib.check(L.fa_sparsity_count(ctypes.byref(fm), ctypes.byref(adj), indptr.data_ptr(), ctypes.byref(nb), sh),
                   "fa_sparsity_count")
        indices = torch.empty(nb.value, dtype=torch.int32, device=dev)
        _lib.check(L.fa_sparsity_fill(ctypes.byref(fm), ctypes.byref(adj), indptr.data_ptr(), indices.data_ptr(), sh),
                   "fa_sparsity_fill")
        V._pattern = (indptr, indices)
    return V._pattern


def create_matrix(a, max_part_bytes: int | None = None, check: bool = False) -> MatrixCSR:
    """Sparsity pattern of the bilinear form (all node pairs of every cell), built on the GPU
    (dolfinx.fem.petsc.create_matrix, FEniCSx/mechanic2d/asym_elasto_damage_model.cc:688), and the
    matrix's value array. check: validate the pattern and adjacency on the device (fa_check_pattern)."""
    V = a.V
    indptr, indices = sparsity_pattern(V)
    if check:
        check_pattern(V, indptr, indices)
    if max_part_bytes is None:
        return MatrixCSR(indptr, indices, V.bs)
    return MatrixCSR(indptr, indices, V.bs, max_part_bytes=max_part_bytes)


def _fa_bsr(A: MatrixCSR, part: int = 0) -> _lib.fa_bsr:
    return A._fa_bsr(part)


def _plan_order(V, fm, adj, fb, plan, sh, eadj=None, order: str = "positional", search: bool = False):
    """Bank-conflict-aware LDS order of the affine-simplex gather (fa_plan_order). order:
    "positional" (default) also balances which entries share a 16-lane quarter (one int32 per
    adjacency entry), "steps" orders each lane's blocks only, "none" keeps the plain slot map.
    Every quarter gets the aligned order of csrc/plan_order.h: the pairwise descent, then Kempe swaps
    that bring the over-full residues' extra steps together (the equitable colouring where no residue
    holds more than a lane has blocks). search (FA_PLAN_ORDER_SEARCH): also the descent's
    alternating-path chain search and a second start from the equitable colouring (config E: 2 % fewer
    LDS passes for a ~4x longer plan); DESIGN.md §3.2b has the counts."""
    if order not in ("positional", "steps", "none"):
        raise ValueError(f"unknown slot order {order!r}")
    if order == "none":
        return None
    if search:
        plan.cell_flags |= _lib.FA_PLAN_ORDER_SEARCH
    if order == "positional" and eadj is None:
        eadj = torch.empty(V.mesh.num_cells * V.nn, dtype=torch.int32, device=V.mesh.device)
    if order != "positional":
        eadj = None
    _lib.check(_lib.load().fa_plan_order(ctypes.byref(fm), ctypes.byref(adj), ctypes.byref(fb),
                                         eadj.data_ptr() if eadj is not None else None, ctypes.byref(plan), sh),
               "fa_plan_order")
    return eadj if plan.eadj else None


def _plan_locality(V, fm, adj, plan, sh, locality=True):
    """Chunk visiting order of the gather (the kernels' XCD x walks positions [x per, (x + 1) per) of
    it). True / "morton": fa_plan_locality, Morton order of the chunks' positions, so chunks that share
    cells run close in time on one XCD and the cells' records are re-read from its L2. "deal": row
    order dealt to the XCDs in pairs of chunks (chunk c to XCD (c // 2) mod 8): every XCD works in one
    compact window of the matrix at any time (the neo-Hookean gather, round 6: 62.1-62.2 vs 63.2-63.3 ms
    Morton on config E-neo, profiles/r6/order_variants_Eneo.txt). False / "row": row order, XCD x
    taking the contiguous eighth x of the chunks."""
    if locality in (False, "row") or plan.nchunks <= 1:
        return None
    if locality == "deal":
        nch = int(plan.nchunks)
        c = torch.arange(nch, device=V.mesh.device, dtype=torch.int64)
        corder = torch.argsort(((c // 2) % 8) * nch + c).to(torch.int32).contiguous()
        plan.corder = corder.data_ptr()
        return corder
    if locality not in (True, "morton"):
        raise ValueError(f"unknown chunk order {locality!r}")
    corder = torch.empty(plan.nchunks, dtype=torch.int32, device=V.mesh.device)
    _lib.check(_lib.load().fa_plan_locality(ctypes.byref(fm), ctypes.byref(adj), corder.data_ptr(),
                                            ctypes.byref(plan), sh), "fa_plan_locality")
    return corder if plan.corder else None


def _use_contrib(V, kind, owner) -> bool:
    """Block-owner gather (fa_plan_contrib) for linear elasticity on P1/P2 triangles and
    tetrahedra. owner=None (default) uses it for triangles, where it measured faster (config A
    0.136 vs 0.220 ms), and keeps the LDS-atomic gather for tetrahedra, where that one is faster
    (C 1.72 vs 2.07 ms, E 46.8 vs 53.1 ms); True / False force it."""
    if owner is False or kind != _lib.FA_LINEAR_ELASTICITY or V.degree not in (1, 2):
        return False
    if owner:
        return V.mesh.cell_type in (_lib.FA_TRIANGLE, _lib.FA_TETRAHEDRON)
    return V.mesh.cell_type == _lib.FA_TRIANGLE


def _plan_contrib(V, fm, adj, fb, rs, plan, sh):
    """Chunking + contribution plan of the block-owner gather; None when a chunk cannot hold a row's
    blocks or entries (then the caller plans the LDS-atomic gather, whose block cap is the larger one:
    a row of 897 .. 1023 blocks of a P2 triangle mesh is over own_maxb only)."""
    L = _lib.load()
    rc = L.fa_plan_gather_contrib(ctypes.byref(fm), ctypes.byref(adj), ctypes.byref(fb), rs.data_ptr(),
                                  ctypes.byref(plan), sh)
    if rc == _lib.FA_E_CAPACITY:  # a row over the block-owner chunk's caps
        return None
    _lib.check(rc, "fa_plan_gather_contrib")
    if plan.nchunks == 0:
        return None
    nbytes = ctypes.c_int64(0)
    _lib.check(L.fa_plan_contrib_bytes(ctypes.byref(fm), ctypes.byref(adj), ctypes.byref(fb), ctypes.byref(plan),
                                       ctypes.byref(nbytes), sh), "fa_plan_contrib_bytes")
    buf = torch.empty(max(int(nbytes.value), 16), dtype=torch.uint8, device=V.mesh.device)
    rc = L.fa_plan_contrib(ctypes.byref(fm), ctypes.byref(adj), ctypes.byref(fb), buf.data_ptr(), buf.numel(),
                           ctypes.byref(plan), sh)
    if rc != _lib.FA_OK:
        if rc == _lib.FA_E_CAPACITY:  # rows with more entries than a chunk holds
            return None
        _lib.check(rc, "fa_plan_contrib")
    return buf


def gather_plan(V: FunctionSpace, A: MatrixCSR, part: int = 0, kind: int = _lib.FA_LINEAR_ELASTICITY,
                deterministic: bool = False, owner: bool | None = None, slots: bool = True,
                order: str = "positional", locality: bool | None = None, search: bool = False):
    """Row-chunk plan of the gather kernel of a form kind for one row part of A's pattern (cached
    on V per options). Neo-Hookean forms get their own chunking (fa_plan_gather_form); the other
    kinds share one. deterministic: the LDS-atomic gather's plan (no contribution plan), for
    FA_DETERMINISTIC. owner: the block-owner contribution plan (None: for triangles). slots: the
    per-entry slot map (fa_plan_slots; False: the kernels search the pattern in LDS). order: the
    slot map's LDS order (_plan_order). search: the order's alternating-path moves (opt-in).
    locality: the chunk visiting order (_plan_locality: "morton" / True, "deal", "row" / False); None
    (default): "deal" for the neo-Hookean gather (62.1 vs 63.2 ms Morton on E-neo), "row" for the others
    (config E: 35.8 vs 36.3, 36.0 vs 36.2, 35.13 vs 35.29 ms Morton on three boxes; C 0.99 vs 1.01 ms;
    DESIGN.md §4)."""
    if deterministic and owner:
        raise ValueError("deterministic assembly runs the LDS-atomic gather: owner=True (block-owner plan) "
                         "cannot be combined with deterministic=True")
    neo = kind == _lib.FA_NEO_HOOKEAN
    if locality is None:
        locality = "deal" if neo else "row"
    if neo and not (slots and order == "positional"):
        raise ValueError("the neo-Hookean gather needs positional plans (slots=True, order='positional')")
    plans = V.__dict__.setdefault("_plans", {})
    contrib = _use_contrib(V, kind, owner) and not deterministic
    key = (A.indptr.data_ptr(), A.parts[part][0], A.parts[part][1], neo, contrib, slots, order, locality, search)
    if key not in plans:
        L = _lib.load()
        fm = V._fa_mesh()
        adj = V._fa_adjacency()
        fb = _fa_bsr(A, part)
        rs = torch.empty(A.parts[part][1] - A.parts[part][0] + 1, dtype=torch.int64, device=V.mesh.device)
        plan = _lib.fa_plan()
        sh = _lib.stream_handle(V.mesh.device)
        if contrib:
            buf = _plan_contrib(V, fm, adj, fb, rs, plan, sh)
            if buf is not None:
                plans[key] = (plan, rs, A.indptr, buf)
                return plan
        _lib.check(L.fa_plan_gather_form(ctypes.byref(fm), int(kind), ctypes.byref(adj), ctypes.byref(fb),
                                         rs.data_ptr(), ctypes.byref(plan), sh), "fa_plan_gather_form")
        smap = eadj = None
        # Per (adjacency entry, column node) block position in its row: no LDS search in the
        # kernel, for 2 B x nn^2 extra reads per cell. Measured with the interleaved-search
        # kernel: config E 64.5 -> 61.0 ms, C 2.22 -> 2.15 ms, Q2 quads +21 % (profiles/r1/
        # slots.md) -> on by default.
        if slots:
            smap = torch.empty(V.mesh.num_cells * V.nn * V.nn, dtype=torch.int16, device=V.mesh.device)
            _lib.check(L.fa_plan_slots(ctypes.byref(fm), ctypes.byref(adj), ctypes.byref(fb), smap.data_ptr(),
                                       ctypes.byref(plan), sh), "fa_plan_slots")
            # bank-balanced positional order of the LDS adds (affine-simplex elasticity and, with the
            # same column split, the neo-Hookean gather)
            eadj = _plan_order(V, fm, adj, fb, plan, sh, order=order, search=search)
        corder = _plan_locality(V, fm, adj, plan, sh, locality)
        # the gathers' chunk arrays in the visiting order, once per plan (fa_plan_chunk_desc; a launch
        # had rebuilt them: config E 0.21 ms of its ~35)
        cdesc = None
        if plan.nchunks > 0 and hasattr(L, "fa_plan_chunk_desc"):  # (an older measurement build lacks it)
            cdesc = torch.empty(3 * (int(plan.nchunks) + 1), dtype=torch.int64, device=V.mesh.device)
            _lib.check(L.fa_plan_chunk_desc(ctypes.byref(fm), ctypes.byref(adj), ctypes.byref(fb), ctypes.byref(plan),
                                            cdesc.data_ptr(), sh), "fa_plan_chunk_desc")
        plans[key] = (plan, rs, A.indptr, smap, eadj, corder, cdesc)
        V.__dict__.setdefault("_plan_xver", {})[key] = _coords_version(V.mesh)
    plan = plans[key][0]
    _recheck_affine(V, key, plan)
    return plan


def _coords_version(m) -> tuple:
    return (m.x.data_ptr(), m.x._version)


def _recheck_affine(V: FunctionSpace, key, plan):
    """The plan's FA_PLAN_AFFINE flag describes the coordinates it was planned on: the affine tensor
    gather builds each cell's Jacobian from three edges, so vertices moved in place since then
    (mesh.x is a public tensor) re-run the library's per-cell affinity check before assembling."""
    if V.mesh.cell_type not in (CellType.quadrilateral, CellType.hexahedron):
        return
    vers = V.__dict__.setdefault("_plan_xver", {})
    now = _coords_version(V.mesh)
    if vers.get(key) == now:
        return
    fm = V._fa_mesh()
    _lib.check(_lib.load().fa_plan_check_affine(ctypes.byref(fm), ctypes.byref(plan),
                                                _lib.stream_handle(V.mesh.device)), "fa_plan_check_affine")
    vers[key] = now


class _Prepared:
    """Prepared cell state of one (form kind, coordinates, dofmap, bc marker) on a space: the static
    records (fa_prepare_cells), and per row window of a pattern its Dirichlet diagonal list
    (fa_prepare_diag). The coefficient array is the space's (rewritten by every assembly)."""

    def __init__(self, rec, coef, marker, has_bc):
        self.rec, self.coef, self.marker, self.has_bc = rec, coef, marker, has_bc
        self.windows = {}  # (indptr pointer, row_begin, row_end) -> (fa_prepared, offsets, indptr)

    def window(self, V, fm, fb, indptr, sh):
        key = (indptr.data_ptr(), int(fb.row_begin), int(fb.row_end))
        hit = self.windows.get(key)
        if hit is None:
            L = _lib.load()
            pp = _lib.fa_prepared(rec=self.rec.data_ptr(), coef=self.coef.data_ptr(), diag_off=None, ndiag=0,
                                  has_bc=self.has_bc)
            off = None
            if self.has_bc:
                n = ctypes.c_int64(0)
                _lib.check(L.fa_prepare_diag_count(ctypes.byref(fm), ctypes.byref(fb), self.marker.data_ptr(),
                                                   ctypes.byref(n), sh), "fa_prepare_diag_count")
                if n.value > 0:
                    off = torch.empty(n.value, dtype=torch.int64, device=V.mesh.device)
                    _lib.check(L.fa_prepare_diag(ctypes.byref(fm), ctypes.byref(fb), self.marker.data_ptr(),
                                                 off.data_ptr(), n.value, sh), "fa_prepare_diag")
                    pp.diag_off, pp.ndiag = off.data_ptr(), n.value
            if len(self.windows) >= 64:  # (row parts and split ranges of a few matrices)
                self.windows.pop(next(iter(self.windows)))
            hit = self.windows[key] = (pp, off, indptr)
        return hit[0]


def _prepared_state(V: FunctionSpace, a, marker, plan, fm, ff, sh):
    """The prepared cell state for assembling `a` with this marker, built on a miss, or None when the
    library does not take the form, element or plan (the caller then assembles as before). Held on V
    like the plans; a hit needs the same form kind and quadrature, coordinates (tensor and version),
    dofmap and marker (the tensor _combine_bcs returned, at the same version)."""
    L = _lib.load()
    if not hasattr(L, "fa_assemble_matrix_prepared"):  # (an older measurement build)
        return None
    if plan.contrib or not plan.eadj:  # the block-owner gather / a plan without positional items
        return None
    xver = _coords_version(V.mesh)
    states = V.__dict__.setdefault("_prepared", {})
    key = (a.kind, a.qdeg, a.E is not None, bool(plan.cell_flags & _lib.FA_PLAN_AFFINE), xver,
           V.dofmap.data_ptr(), V.mesh.cells.data_ptr(),
           None if marker is None else (id(marker), marker._version))
    if key in states:
        return states[key]
    # A form the library does not prepare is remembered with its Poisson ratio, which decides that (the
    # uniform-nu kernels' interval); the records themselves do not depend on nu, so a state serves every nu.
    refused = V.__dict__.setdefault("_unprepared", set())
    if (key, a.nu) in refused:
        return None
    for k in [k for k in states if k[4] != xver]:  # records of coordinates that are gone
        del states[k]
    while len(states) >= 3:
        states.pop(next(iter(states)))
    nrec, ncoef = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = L.fa_prepared_bytes(ctypes.byref(fm), ctypes.byref(ff), ctypes.byref(plan), ctypes.byref(nrec),
                             ctypes.byref(ncoef))
    st = None
    if rc != _lib.FA_E_UNSUPPORTED:
        _lib.check(rc, "fa_prepared_bytes")
        dev = V.mesh.device
        coef = V.__dict__.get("_prepared_coef")
        if coef is None or coef.numel() * 8 != max(ncoef.value, 8):
            coef = V.__dict__["_prepared_coef"] = torch.empty(max(ncoef.value // 8, 1), dtype=torch.float64, device=dev)
        rec = torch.empty(max(nrec.value // 8, 2), dtype=torch.float64, device=dev)
        pp = _lib.fa_prepared(rec=rec.data_ptr(), coef=coef.data_ptr(), diag_off=None, ndiag=0, has_bc=0)
        adj = V._fa_adjacency()
        rc = L.fa_prepare_cells(ctypes.byref(fm), ctypes.byref(ff), ctypes.byref(adj), ctypes.byref(plan),
                                _lib.ptr(marker), ctypes.byref(pp), sh)
        if rc != _lib.FA_E_UNSUPPORTED:
            _lib.check(rc, "fa_prepare_cells")
            st = _Prepared(rec, coef, marker, int(pp.has_bc))
            V._prepared_builds = V._prepared_builds + 1
    if st is None:
        if len(refused) >= 16:
            refused.clear()
        refused.add((key, a.nu))
        return None
    states[key] = st
    return st


def assemble_matrix(a, bcs=None, diagonal: float = 1.0, A: MatrixCSR | None = None, method: str = "gather",
                    deterministic: bool = False, plan: dict | None = None, check: bool = False) -> MatrixCSR:
    """Assemble the bilinear form into a BSR matrix (dolfinx.fem.assemble_matrix + set_diagonal).

    bcs: list of DirichletBC — their rows and columns receive no cell contribution and their
    diagonal entries are set to `diagonal`. method: "gather" (row-gather, default) or
    "scatter" (element scatter with FP64 atomics; zeroes A first like MatZeroEntries).
    deterministic: bit-identical values run to run (FA_DETERMINISTIC: exact 64-bit fixed-point
    sums in the gather; linear elasticity with E per cell and one Poisson ratio -0.99 < nu < 0.49, at the
    default quadrature rule, on affine simplices, affine Q1 / Q2 quadrilaterals and Q1 hexahedra). Any
    other form, Poisson ratio or rule raises FemasmError: their kernels sum in floating point.
    The Poisson ratio also picks the kernel of the default mode: -0.99 < nu < 0.49 (with E per cell) runs the
    uniform-nu kernels and the prepared cell state, any other nu in (-1, 0.5), or lam / mu per cell, the
    general lam/mu kernels. A quadrature_degree other than the element's default runs the element scatter
    (FP64 atomics) under either method. All of them meet the same per-row accuracy.
    plan: gather_plan options (owner, slots, order, locality). check: synchronise and raise if a
    kernel found a pattern entry missing (FA_CHECK_ERRORS).
    """
    V = a.V
    if method not in ("gather", "scatter"):
        raise ValueError(f"unknown method {method}")
    if deterministic and method != "gather":
        raise ValueError("deterministic assembly is a gather mode")
    if A is None:
        A = create_matrix(a)
    L = _lib.load()
    marker, _ = _combine_bcs(V, bcs, with_g=False)
    fm = V._fa_mesh()
    ff = _fa_form(a)
    sh = _lib.stream_handle(V.mesh.device)
    prep, coef_done = None, False
    for part in range(len(A.parts)):
        fb = _fa_bsr(A, part)
        if method == "gather":
            adj = V._fa_adjacency()
            gp = gather_plan(V, A, part, a.kind, deterministic=deterministic, **(plan or {}))
            flags = _lib.FA_GATHER | (_lib.FA_DETERMINISTIC if deterministic else 0) | \
                (_lib.FA_CHECK_ERRORS if check else 0)
            # the prepared cell state (static records and diagonal lists kept on V; the coefficient pass
            # once per assembly, not per part), where the library takes the form and the plan
            if part == 0:
                prep = _prepared_state(V, a, marker, gp, fm, ff, sh)
            if prep is not None:
                pp = prep.window(V, fm, fb, A.indptr, sh)
                rc = L.fa_assemble_matrix_prepared(ctypes.byref(fm), ctypes.byref(ff), ctypes.byref(adj),
                                                   ctypes.byref(gp), ctypes.byref(pp), float(diagonal), ctypes.byref(fb),
                                                   flags | (_lib.FA_KEEP_COEF if coef_done else 0), sh)
                if rc != _lib.FA_E_UNSUPPORTED:
                    _lib.check(rc, "fa_assemble_matrix_prepared")
                    coef_done = True
                    continue
                prep = None  # (a plan or a coefficient the prepared gather does not take: as before)
            rc = L.fa_assemble_matrix(ctypes.byref(fm), ctypes.byref(ff), ctypes.byref(adj), ctypes.byref(gp),
                                      _lib.ptr(marker), float(diagonal), ctypes.byref(fb), flags, sh)
        else:
            flags = _lib.FA_SCATTER | _lib.FA_ZERO_FIRST | (_lib.FA_CHECK_ERRORS if check else 0)
            rc = L.fa_assemble_matrix(ctypes.byref(fm), ctypes.byref(ff), None, None, _lib.ptr(marker),
                                      float(diagonal), ctypes.byref(fb), flags, sh)
        _lib.check(rc, "fa_assemble_matrix")
    A._keepalive = (marker, a)
    return A


class JacobianOperator:
    """The Jacobian of a form at its current state, applied without assembling it: ``mult(x)`` is
    ``assemble_matrix(a, bcs, diagonal).mult(x)`` (fa_apply_jacobian) and ``block_diagonal()`` that
    matrix's diagonal blocks (fa_jacobian_block_diag), with ``MatrixCSR``'s signatures, so it drops into
    ``nls.KrylovSolver``. The form's ``u`` is read live (same storage): the operator always acts at the
    current state and needs no re-assembly between Newton steps.

    method: "auto" runs the planned kernel where the element has one (P1 / P2 triangles and tetrahedra)
    and the generic node-parallel kernel elsewhere, or when a node has more cells than a chunk's tile
    holds (FA_E_CAPACITY); "planned" raises instead of falling back; "generic" always runs the generic
    kernel. The apply plan is built once per space and cached on V (like the adjacency).
    ``num_chunks`` / ``plan_bytes``: the plan's chunks and device bytes (0 for the generic kernel);
    ``redundancy``: cell visits per launch / cells (1.0 when no cell straddles chunks; nodes per cell
    for the generic kernel, which visits a cell once per node). Single GPU: ``parallel.SlabProblem``
    keeps assembling."""

    def __init__(self, a, bcs=None, diagonal: float = 1.0, method: str = "auto"):
        if not isinstance(a, LinearElasticity):
            raise TypeError("expected a femasm form descriptor (LinearElasticity, AsymDamage, ...)")
        if method not in ("auto", "planned", "generic"):
            raise ValueError(f"unknown method {method!r}: 'auto', 'planned' or 'generic'")
        V = a.V
        if V.family in ("DG", "Discontinuous Lagrange") or V.bs != V.mesh.gdim:
            raise ValueError("the form's space must be a vector Lagrange space (bs = gdim)")
        self.a, self.V = a, V
        self.bcs = list(bcs or [])
        self.diagonal = float(diagonal)
        self.method = method
        self.bs = V.bs
        self._plan = None  # (buffer | None, chunks, bytes, cell visits), resolved on the first device use
        if V.mesh.device.type == "cuda":
            self._resolve()

    @property
    def shape(self):
        return (self.V.num_dofs, self.V.num_dofs)

    @staticmethod
    def has_plan(V: FunctionSpace) -> bool:
        """Whether V's element has a planned kernel (P1 / P2 triangles and tetrahedra)."""
        return is_simplex(V.mesh.cell_type) and V.degree in (1, 2)

    def _resolve(self):
        if self._plan is not None:
            return self._plan
        V = self.V
        generic = (None, 0, 0, V.mesh.num_cells * V.nn)
        if self.method == "generic" or (self.method == "auto" and not self.has_plan(V)):
            self._plan = generic
            return self._plan
        if not self.has_plan(V):
            raise ValueError("method='planned': the planned kernel serves P1 / P2 triangles and tetrahedra only")
        cached = V.__dict__.get("_apply_plan")
        if cached is None:
            L = _lib.load()
            fm, adj = V._fa_mesh(), V._fa_adjacency()
            sh = _lib.stream_handle(V.mesh.device)
            nbytes, nch = ctypes.c_int64(0), ctypes.c_int64(0)
            rc = L.fa_apply_plan_bytes(ctypes.byref(fm), ctypes.byref(adj), ctypes.byref(nbytes), ctypes.byref(nch), sh)
            if rc == _lib.FA_OK:
                buf = torch.empty(max(int(nbytes.value) // 8, 4), dtype=torch.int64, device=V.mesh.device)
                rc = L.fa_apply_plan(ctypes.byref(fm), ctypes.byref(adj), buf.data_ptr(), buf.numel() * 8, sh)
            if rc == _lib.FA_E_CAPACITY:
                cached = ("capacity", L.fa_last_error().decode(errors="replace"))
            else:
                _lib.check(rc, "fa_apply_plan")
                cached = (buf, int(nch.value), int(nbytes.value), int(buf[3]))
            V.__dict__["_apply_plan"] = cached
        if cached[0] == "capacity":
            if self.method == "planned":
                raise _lib.FemasmError(f"fa_apply_plan failed ({_lib.FA_E_CAPACITY}): {cached[1]}")
            self._plan = generic
        else:
            self._plan = cached
        return self._plan

    @property
    def num_chunks(self) -> int:
        return self._resolve()[1]

    @property
    def plan_bytes(self) -> int:
        return self._resolve()[2]

    @property
    def redundancy(self) -> float:
        nc = self.V.mesh.num_cells
        return self._resolve()[3] / nc if nc else 1.0

    def _check_vector(self, t, name: str):
        V = self.V
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise ValueError(f"{name} must be a float64 tensor")
        if t.dim() != 1 or t.numel() != V.num_dofs:
            raise ValueError(f"{name} must have {V.num_dofs} entries (V.num_dofs), not {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if t.device != V.mesh.device:
            raise ValueError(f"{name} is on {t.device}, the mesh on {V.mesh.device}")

    def mult(self, x: torch.Tensor, y: torch.Tensor | None = None) -> torch.Tensor:
        """y = J(u) x for a dof vector x [num_dofs]; y (optional, not aliasing x) is overwritten. With y
        given the call allocates no device memory."""
        self._check_vector(x, "x")
        if y is not None:
            self._check_vector(y, "y")
            n = 8 * x.numel()
            if x.data_ptr() < y.data_ptr() + n and y.data_ptr() < x.data_ptr() + n:
                raise ValueError("x and y must not alias")
        else:
            y = torch.empty_like(x)
        V = self.V
        plan = self._resolve()[0]
        marker, _ = _combine_bcs(V, self.bcs, with_g=False)
        fm, ff, adj = V._fa_mesh(), _fa_form(self.a), V._fa_adjacency()
        _lib.check(_lib.load().fa_apply_jacobian(
            ctypes.byref(fm), ctypes.byref(ff), ctypes.byref(adj), None if plan is None else plan.data_ptr(),
            _lib.ptr(marker), self.diagonal, x.data_ptr(), y.data_ptr(), _lib.stream_handle(V.mesh.device)),
            "fa_apply_jacobian")
        return y

    def block_diagonal(self) -> torch.Tensor:
        """Diagonal blocks [num_nodes, bs, bs] of J(u) (the block-Jacobi preconditioner)."""
        V = self.V
        out = torch.empty((V.num_nodes, V.bs, V.bs), dtype=torch.float64, device=V.mesh.device)
        marker, _ = _combine_bcs(V, self.bcs, with_g=False)
        fm, ff, adj = V._fa_mesh(), _fa_form(self.a), V._fa_adjacency()
        _lib.check(_lib.load().fa_jacobian_block_diag(
            ctypes.byref(fm), ctypes.byref(ff), ctypes.byref(adj), _lib.ptr(marker), self.diagonal, out.data_ptr(),
            _lib.stream_handle(V.mesh.device)), "fa_jacobian_block_diag")
        return out


class SplitGather:
    """fa_assemble_matrix(FA_GATHER) split into ``prepare()`` (per-cell records of all cells, once)
    and ``rows(i)`` (the rows of ``ranges[i]`` of one row part of A), via fa_gather_prepare /
    fa_gather_rows on a work buffer it owns. Each range is its own gather plan; every row of the
    part must be in exactly one range for a complete assembly. femasm.parallel uses it to start
    the interface exchange of a rank's slab while its interior rows assemble."""

    def __init__(self, a, bcs, A: MatrixCSR, ranges, part: int = 0, diagonal: float = 1.0,
                 deterministic: bool = False, slots: bool = True, order: str = "positional"):
        V = a.V
        if a.kind == _lib.FA_NEO_HOOKEAN and not (slots and order == "positional"):
            raise ValueError("the neo-Hookean gather needs positional plans (slots=True, order='positional')")
        L = _lib.load()
        self.L, self.a, self.A, self.diagonal = L, a, A, float(diagonal)
        self.marker, _ = _combine_bcs(V, bcs, with_g=False)
        self.fm, self.ff, self.adj = V._fa_mesh(), _fa_form(a), V._fa_adjacency()
        dev = V.mesh.device
        self.sh = _lib.stream_handle(dev)
        nbytes = ctypes.c_int64(0)
        _lib.check(L.fa_gather_work_bytes(ctypes.byref(self.fm), ctypes.byref(self.ff), ctypes.byref(nbytes)),
                   "fa_gather_work_bytes")
        # the per-step records' buffer: allocated by the first prepare() that does not run on the
        # prepared cell state (which keeps its static records on V instead)
        self._work_bytes, self.work, self._prep = max(int(nbytes.value), 16), None, None
        pr0, pr1, data = A.parts[part]
        base = int(A.indptr[pr0])
        bs2 = A.bs * A.bs
        self.slots = None
        if slots:
            self.slots = torch.empty(V.mesh.num_cells * V.nn * V.nn, dtype=torch.int16, device=dev)
        self.subs, self.plans, self._keep = [], [], []
        self._xver = _coords_version(V.mesh)
        for r0, r1 in ranges:
            if not (pr0 <= r0 <= r1 <= pr1):
                raise ValueError(f"row range [{r0}, {r1}) outside part [{pr0}, {pr1})")
            fb = _fa_bsr(A, part)
            fb.row_begin, fb.row_end = r0, r1
            fb.data = data.data_ptr() + 8 * bs2 * (int(A.indptr[r0]) - base)
            rs = torch.empty(r1 - r0 + 1, dtype=torch.int64, device=dev)
            plan = _lib.fa_plan()
            if r1 > r0:
                _lib.check(L.fa_plan_gather_form(ctypes.byref(self.fm), int(a.kind), ctypes.byref(self.adj),
                                                 ctypes.byref(fb), rs.data_ptr(), ctypes.byref(plan), self.sh),
                           "fa_plan_gather_form")
            if deterministic:
                plan.cell_flags |= _lib.FA_PLAN_DETERMINISTIC
            self.subs.append(fb)
            self.plans.append(plan)
            self._keep.append(rs)
            if r1 > r0:
                self._keep.append(_plan_locality(V, self.fm, self.adj, plan, self.sh,  # (gather_plan's default)
                                                 locality="deal" if a.kind == _lib.FA_NEO_HOOKEAN else "row"))
        if self.slots is not None:
            # one slot map for all rows (fa_plan_slots writes every row), then each plan's order
            live = [i for i, (r0, r1) in enumerate(ranges) if r1 > r0]
            for i in live[:1]:
                _lib.check(L.fa_plan_slots(ctypes.byref(self.fm), ctypes.byref(self.adj), ctypes.byref(self.subs[i]),
                                           self.slots.data_ptr(), ctypes.byref(self.plans[i]), self.sh), "fa_plan_slots")
            self.eadj = None  # one positional entry buffer: the plans' entries are disjoint
            for i in live:
                self.plans[i].slots = self.slots.data_ptr()
                self.plans[i].slot_order = 0
                e = _plan_order(V, self.fm, self.adj, self.subs[i], self.plans[i], self.sh, self.eadj, order)
                self.eadj = e if e is not None else self.eadj

    def prepare(self):
        # the plans' FA_PLAN_AFFINE flags describe the coordinates they were planned on: vertices
        # moved in place since then re-run the library's per-cell affinity check (as gather_plan does)
        m = self.a.V.mesh
        now = _coords_version(m)
        if now != self._xver:
            self.fm = self.a.V._fa_mesh()  # mesh.x may be a new tensor
            if m.cell_type in (CellType.quadrilateral, CellType.hexahedron):
                for plan in self.plans:
                    _lib.check(self.L.fa_plan_check_affine(ctypes.byref(self.fm), ctypes.byref(plan), self.sh),
                               "fa_plan_check_affine")
            self._xver = now
        # the prepared cell state of the space (shared with assemble_matrix): only the coefficient pass
        # runs per step; the records and constrained-dof bits are rebuilt when the mesh or the marker change
        live = [p for p in self.plans if p.nchunks > 0]
        V = self.a.V
        st = _prepared_state(V, self.a, self.marker, live[0], self.fm, self.ff, self.sh) if live else None
        if st is not None:
            pp = [st.window(V, self.fm, fb, self.A.indptr, self.sh) if p.nchunks > 0 else None
                  for fb, p in zip(self.subs, self.plans)]
            rc = self.L.fa_prepare_coef(ctypes.byref(self.fm), ctypes.byref(self.ff),
                                        ctypes.byref(next(p for p in pp if p is not None)), self.sh)
            if rc != _lib.FA_E_UNSUPPORTED:
                _lib.check(rc, "fa_prepare_coef")
                self._prep = pp
                return
        self._prep = None
        self._prepare_records()

    def _prepare_records(self):
        if self.work is None:
            self.work = torch.empty(self._work_bytes, dtype=torch.uint8, device=self.a.V.mesh.device)
        _lib.check(self.L.fa_gather_prepare(ctypes.byref(self.fm), ctypes.byref(self.ff), _lib.ptr(self.marker),
                                            self.work.data_ptr(), self.sh), "fa_gather_prepare")

    def rows(self, i: int):
        if self.plans[i].nchunks == 0:
            return
        if self._prep is not None:
            rc = self.L.fa_gather_rows_prepared(ctypes.byref(self.fm), ctypes.byref(self.ff), ctypes.byref(self.adj),
                                                ctypes.byref(self.plans[i]), ctypes.byref(self._prep[i]), self.diagonal,
                                                ctypes.byref(self.subs[i]), self.sh)
            if rc != _lib.FA_E_UNSUPPORTED:
                _lib.check(rc, "fa_gather_rows_prepared")
                return
            self._prep = None  # (a plan the prepared gather does not take: this step's records, as before)
            self._prepare_records()
        _lib.check(self.L.fa_gather_rows(ctypes.byref(self.fm), ctypes.byref(self.ff), ctypes.byref(self.adj),
                                         ctypes.byref(self.plans[i]), _lib.ptr(self.marker), self.diagonal,
                                         self.work.data_ptr(), ctypes.byref(self.subs[i]), self.sh), "fa_gather_rows")


def tabulate_cells(a, c0: int = 0, ncells: int | None = None) -> torch.Tensor:
    """Element matrices [nc, nn*bs, nn*bs] (batched ffcx tabulate_tensor / AssembleElementGrad)."""
    V = a.V
    nc = V.mesh.num_cells - c0 if ncells is None else ncells
    nd = V.nn * V.bs
    Ae = torch.empty((nc, nd, nd), dtype=torch.float64, device=V.mesh.device)
    L = _lib.load()
    fm = V._fa_mesh()
    ff = _fa_form(a)
    _lib.check(L.fa_tabulate_cells(ctypes.byref(fm), ctypes.byref(ff), c0, nc, Ae.data_ptr(),
                                   _lib.stream_handle(V.mesh.device)), "fa_tabulate_cells")
    return Ae


def assemble_vector(L, b: torch.Tensor | None = None) -> torch.Tensor:
    """Residual of the form's constitutive law: b += int sigma(u):eps(v) dxx - int f.v dx
    - sum over the form's loads of int (t - p n).v ds
    (dolfinx.fem.assemble_vector of the reference F, FEniCSx/mechanic2d/asym_elasto_damage_model.cc:825;
    MFEM damIntegrator::AssembleElementVector :559-637). u, f are the form's `u` / `f` (None = 0); each
    ``SurfaceLoad`` of the form's `loads` is subtracted after the cell term (``assemble_surface_load``
    with alpha = -1). Without loads the launches are the cell term's alone."""
    V = L.V
    if b is None:
        b = torch.zeros(V.num_dofs, dtype=torch.float64, device=V.mesh.device)
    Lb = _lib.load()
    fm = V._fa_mesh()
    ff = _fa_form(L)
    adj = V._fa_adjacency()
    _lib.check(Lb.fa_assemble_vector(ctypes.byref(fm), ctypes.byref(ff), ctypes.byref(adj), b.data_ptr(),
                                     _lib.stream_handle(V.mesh.device)), "fa_assemble_vector")
    for ld in getattr(L, "loads", None) or ():
        assemble_surface_load(ld, b, alpha=-1.0)
    return b


def apply_lifting(b: torch.Tensor, a: list, bcs: list, x0: list | None = None, alpha: float = 1.0, scale=None):
    """dolfinx apply_lifting: b -= alpha * A (g - x0) over constrained columns, with the cell
    matrices of a[0] (the reference calls it with alpha = -1, :827)."""
    if scale is not None:
        alpha = scale
    form_ = a[0]
    V = form_.V
    marker, g = _combine_bcs(V, bcs[0])
    if marker is None:
        return b
    x = None if not x0 else (x0[0].x if isinstance(x0[0], Function) else x0[0])
    Lb = _lib.load()
    fm = V._fa_mesh()
    ff = _fa_form(form_)
    adj = V._fa_adjacency()
    _lib.check(Lb.fa_apply_lifting(ctypes.byref(fm), ctypes.byref(ff), ctypes.byref(adj), b.data_ptr(),
                                   marker.data_ptr(), g.data_ptr(), _lib.ptr(x), float(alpha),
                                   _lib.stream_handle(V.mesh.device)), "fa_apply_lifting")
    return b


def set_bc(b: torch.Tensor, bcs: list, x0=None, alpha: float = 1.0, scale=None):
    """dolfinx set_bc: b[bc dofs] = alpha * (g - x0) (the reference: alpha = -1, x0 = u, :836)."""
    if scale is not None:
        alpha = scale
    if not bcs:
        return b
    V = bcs[0].V
    marker, g = _combine_bcs(V, bcs)
    x = None if x0 is None else (x0.x if isinstance(x0, Function) else x0)
    Lb = _lib.load()
    _lib.check(Lb.fa_set_bc(b.data_ptr(), b.numel(), marker.data_ptr(), g.data_ptr(), _lib.ptr(x), float(alpha),
                            _lib.stream_handle(V.mesh.device)), "fa_set_bc")
    return b


# ---------------------------------------------------------------------------------- exterior-facet loads
def _space_basis(ct, p: int, X: np.ndarray) -> np.ndarray:
    """Degree-p Lagrange basis (basix node order) at reference points X [n, tdim] -> [n, nn]."""
    ct = CellType(ct)
    if is_simplex(ct):
        lam = np.concatenate([1.0 - X.sum(1, keepdims=True), X], axis=1)
        if p == 1:
            return lam
        if p != 2:
            raise NotImplementedError("simplex degree > 2")
        return np.concatenate([lam * (2.0 * lam - 1.0)] + [4.0 * lam[:, [i]] * lam[:, [j]] for i, j in _EDGES[ct]], axis=1)
    r = line_points(p)
    l1 = []  # per direction, the 1-D Lagrange polynomials at the points [n, p + 1]
    for d in range(X.shape[1]):
        cols = []
        for i in range(p + 1):
            v = np.ones(X.shape[0])
            for k in range(p + 1):
                if k != i:
                    v = v * (X[:, d] - r[k]) / (r[i] - r[k])
            cols.append(v)
        l1.append(np.stack(cols, 1))
    L = node_lattice(ct, p)
    out = np.ones((X.shape[0], L.shape[0]))
    for d in range(X.shape[1]):
        out = out * l1[d][:, L[:, d]]
    return out


def _geometry_gradients(ct, X: np.ndarray) -> np.ndarray:
    """Reference gradients of the P1 / Q1 geometry basis at X [n, tdim] -> [n, nverts, tdim]."""
    ct = CellType(ct)
    n, td = X.shape
    if is_simplex(ct):
        g = np.concatenate([-np.ones((1, td)), np.eye(td)], 0)
        return np.broadcast_to(g, (n, td + 1, td)).copy()
    out = np.empty((n, len(_REF_VERTS[ct]), td))
    for v, bits in enumerate(_REF_VERTS[ct]):
        f = [X[:, d] if bits[d] else 1.0 - X[:, d] for d in range(td)]
        for k in range(td):
            gk = np.full(n, 1.0 if bits[k] else -1.0)
            for d in range(td):
                if d != k:
                    gk = gk * f[d]
            out[:, v, k] = gk
    return out


def _gauss_01(n: int):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def _facet_rule(ct, qdeg: int):
    """(points [nq, tdim - 1], weights [nq]) on the reference facet of a cell type, the library's rules:
    Gauss on [0, 1]; on a triangle the 1- and 3-point rules up to degree 2, a collapsed Gauss product above;
    a Gauss product with (qdeg + 2) // 2 points per direction on a quadrilateral."""
    ct = CellType(ct)
    if ct in (CellType.triangle, CellType.quadrilateral):
        x, w = _gauss_01((qdeg + 2) // 2)
        return x.reshape(-1, 1), w
    if ct == CellType.hexahedron:
        x, w = _gauss_01((qdeg + 2) // 2)
        return np.array([[a, b] for a in x for b in x]), np.array([u * v for u in w for v in w])
    if qdeg == 1:
        return np.array([[1.0 / 3.0, 1.0 / 3.0]]), np.array([0.5])
    if qdeg == 2:
        a, b = 1.0 / 6.0, 2.0 / 3.0
        return np.array([[a, a], [a, b], [b, a]]), np.full(3, 1.0 / 6.0)
    x, w = _gauss_01((qdeg + 2) // 2 + 1)
    return (np.array([[a * (1.0 - b), b] for a in x for b in x]),
            np.array([u * v * (1.0 - b) for u in w for v, b in zip(w, x)]))


_FACET_TABLES = {}


def _facet_tables(ct, p: int, qdeg: int) -> dict:
    """Facet tables of an element, per local facet (mesh.sub_entities(ct, tdim - 1)): the facet rule mapped
    into the cell through the facet's reference vertices, X = V0 + xi (V1 - V0) + eta (V2 - V0); wq [nq],
    phi [nl, nq, nn], gdphi [nl, nq, nv, td], nref [nl, td] = the outward N_ref dS_ref of that
    parametrisation, closure [nl, nk] = _closure_nodes of each local facet."""
    ct = CellType(ct)
    key = (ct, p, qdeg)
    if key in _FACET_TABLES:
        return _FACET_TABLES[key]
    from .mesh import sub_entities

    RV = np.array(_REF_VERTS[ct], dtype=np.float64)
    td = RV.shape[1]
    pts, wq = _facet_rule(ct, qdeg)
    phi, gd, nref, closure = [], [], [], []
    for S in sub_entities(ct, td - 1):
        V0, A = RV[S[0]], RV[S[1]] - RV[S[0]]
        X = V0 + pts[:, [0]] * A
        if td == 3:
            B = RV[S[2]] - RV[S[0]]
            X = X + pts[:, [1]] * B
            N = np.cross(A, B)
        else:
            N = np.array([A[1], -A[0]])
        if N @ (X.mean(0) - RV.mean(0)) < 0.0:
            N = -N
        phi.append(_space_basis(ct, p, X))
        gd.append(_geometry_gradients(ct, X))
        nref.append(N)
        closure.append(_closure_nodes(ct, p, S))
    T = dict(wq=wq, phi=np.stack(phi), gdphi=np.stack(gd), nref=np.stack(nref), closure=np.array(closure, dtype=np.int64))
    _FACET_TABLES[key] = T
    return T


class SurfaceLoad:
    """A dead load on exterior facets of V's mesh: ``int (t - p n).v ds`` on the reference configuration,
    the reference's ``dot(t*n, delta_u)*ds(0)`` term (FEniCSx/mechanic2d/asym_ufl.py:81; its scalar t is -p).

    facets: ids of ``mesh.entities(m, tdim - 1)`` (what ``mesh.locate_entities_boundary``,
    ``mesh.exterior_facets`` and ``io.MeshTags.find`` return), each exterior and given once.
    traction ``t``, a force per reference area: one gdim-vector; a ``[len(facets), gdim]`` tensor of
    per-facet values in the order of ``facets``; or nodal values, a ``Function`` on V or a ``[num_dofs]``
    tensor, interpolated with the cell basis at the facet points.
    pressure ``p``, along the reference OUTWARD unit normal n (the traction is -p n): a scalar; a
    ``[len(facets)]`` tensor; or nodal values, a ``Function`` on a scalar space with V's nodes or a
    ``[num_nodes]`` tensor. A plain tensor of ``len(facets)`` entries is per-facet: where that count equals
    ``num_nodes``, nodal values have to come as a Function.
    Both may be given and add. Tensors (and Functions) are read at every assembly, like a form's ``E``:
    changing them in place costs nothing. quadrature_degree: None = 2 * degree, the rule of the f.v dx term.

    The plan is built here, once, in torch: the facets sorted by id (slots), each slot's cell and local facet
    (``mesh.sub_entities`` numbering) from ``entities()``'s cell -> facet table, and a node-parallel
    adjacency over the loaded nodes only: ``nodes`` (ascending), a CSR ``node_ptr`` and entries
    ``slot * nk + k`` with k indexing ``_closure_nodes(ct, p, S_local_facet)``, a node's entries in
    ascending slot order. The sum order is therefore fixed: results are bit-identical run to run and under
    any permutation of ``facets`` (per-facet values following their facets).

    Out of scope: follower (deformation-dependent) pressure and its unsymmetric tangent, interior-facet and
    Robin terms, and ``parallel.SlabProblem`` (a slab's cut planes are exterior facets of the slab mesh)."""

    def __init__(self, V: FunctionSpace, facets, traction=None, pressure=None, quadrature_degree: int | None = None):
        from . import mesh as fmesh

        m = V.mesh
        if V.family in ("DG", "Discontinuous Lagrange") or V.bs != m.gdim:
            raise ValueError("a SurfaceLoad needs a vector Lagrange space (bs = gdim)")
        if traction is None and pressure is None:
            raise ValueError("a SurfaceLoad needs a traction, a pressure or both")
        if quadrature_degree is not None and not 1 <= int(quadrature_degree) <= 12:
            raise ValueError(f"quadrature_degree {quadrature_degree} outside 1 .. 12")
        self.V = V
        self.qdeg = -1 if quadrature_degree is None else int(quadrature_degree)
        dev = m.device
        f = torch.as_tensor(facets, device=dev)
        if f.dim() != 1 or f.dtype.is_floating_point or f.dtype == torch.bool:
            raise ValueError("facets must be a 1-D tensor of facet ids")
        f = f.to(torch.int64)
        _, cf = fmesh.entities(m, m.tdim - 1)
        nfac = int(cf.max()) + 1 if cf.numel() else 0
        if f.numel() and (int(f.min()) < 0 or int(f.max()) >= nfac):
            raise ValueError(f"facet ids outside [0, {nfac})")
        order = torch.argsort(f, stable=True)
        fs = f[order]
        if fs.numel() > 1 and bool((fs[1:] == fs[:-1]).any()):
            raise ValueError("a facet is given twice")
        flat = cf.reshape(-1)
        cnt = torch.bincount(flat, minlength=nfac)
        if bool((cnt[fs] != 1).any()):
            bad = fs[cnt[fs] != 1]
            raise ValueError(f"{bad.numel()} of the facets are not exterior (first: facet {int(bad[0])})")
        self.facets = f
        nf, nl = int(f.numel()), int(cf.shape[1])
        # slot -> (cell, local facet): an exterior facet has one position in the cell -> facet table
        pos = torch.zeros(nfac, dtype=torch.int64, device=dev)
        pos[flat] = torch.arange(flat.numel(), device=dev)
        hit = pos[fs]
        cell, lf = hit // nl, hit % nl
        CL = torch.tensor([_closure_nodes(m.cell_type, V.degree, S) for S in fmesh.sub_entities(m.cell_type, m.tdim - 1)],
                          dtype=torch.int64, device=dev)  # [nl, nk]
        nk = int(CL.shape[1])
        if nf * nk > 2 ** 31 - 1:
            raise ValueError(f"{nf} facets of {nk} nodes: more entries than int32 holds")
        fnodes = torch.gather(V.dofmap.to(torch.int64)[cell], 1, CL[lf])  # [nf, nk]
        # entries slot * nk + k by node; the stable sort keeps a node's entries in ascending slot order
        flatn = fnodes.reshape(-1)
        perm = torch.argsort(flatn, stable=True)
        nodes, counts = torch.unique_consecutive(flatn[perm], return_counts=True)
        ptr = torch.zeros(nodes.numel() + 1, dtype=torch.int64, device=dev)
        ptr[1:] = torch.cumsum(counts, 0)
        self.nk = nk
        self.facet_cell = cell.to(torch.int32).contiguous()
        self.facet_local = lf.to(torch.int32).contiguous()
        self.facet_value = order.to(torch.int32).contiguous()  # slot -> row of the per-facet values as given
        self.nodes = nodes.to(torch.int32).contiguous()
        self.node_ptr = ptr
        self.entries = perm.to(torch.int32).contiguous()
        self._traction = self._value_source(traction, "traction", m.gdim)
        self._pressure = self._value_source(pressure, "pressure", 1)

    def _value_source(self, v, name: str, width: int):
        """(mode, holder) of a value argument: the holder is a device tensor, or the Function whose ``x`` is
        read at every assembly."""
        V = self.V
        if v is None:
            return (_lib.FA_LOAD_NONE, None)
        if isinstance(v, Function):
            W = v.function_space
            if W.mesh is not V.mesh or W.bs != width or W.num_nodes != V.num_nodes or W.degree != V.degree or \
                    W.family in ("DG", "Discontinuous Lagrange"):
                raise ValueError(f"the {name} Function must live on V's nodes with {width} value(s) per node")
            return (_lib.FA_LOAD_NODAL, v)
        if isinstance(v, Constant):
            v = v.value
        t = torch.as_tensor(v, dtype=torch.float64, device=V.mesh.device).contiguous()
        nf = int(self.facets.numel())
        if width == 1:
            if t.numel() == 1 and t.dim() <= 1:
                return (_lib.FA_LOAD_CONSTANT, t.reshape(1))
            if t.dim() == 1 and t.numel() == nf:
                return (_lib.FA_LOAD_FACET, t)
            if t.dim() == 1 and t.numel() == V.num_nodes:
                return (_lib.FA_LOAD_NODAL, t)
            raise ValueError(f"pressure of shape {tuple(t.shape)}: a scalar, [{nf}] per facet or [{V.num_nodes}] per node")
        if t.dim() == 1 and t.numel() == width:
            return (_lib.FA_LOAD_CONSTANT, t)
        if t.dim() == 2 and tuple(t.shape) == (nf, width):
            return (_lib.FA_LOAD_FACET, t)
        if t.dim() == 1 and t.numel() == V.num_dofs:
            return (_lib.FA_LOAD_NODAL, t)
        raise ValueError(f"traction of shape {tuple(t.shape)}: [{width}], [{nf}, {width}] per facet or [{V.num_dofs}] per dof")

    def _values(self, src, name: str, nodal_size: int):
        mode, h = src
        if h is None:
            return mode, None
        t = h.x if isinstance(h, Function) else h
        if isinstance(h, Function) and (t.dtype != torch.float64 or t.numel() != nodal_size or not t.is_contiguous()
                                        or t.device != self.V.mesh.device):
            raise ValueError(f"the {name} Function's values changed shape, type or device")
        return mode, t

    def values(self):
        """((traction mode, tensor | None), (pressure mode, tensor | None)) as this assembly reads them."""
        V = self.V
        return self._values(self._traction, "traction", V.num_dofs), self._values(self._pressure, "pressure", V.num_nodes)

    def _fa_facet_load(self, tv, pv) -> _lib.fa_facet_load:
        s = _lib.fa_facet_load()
        s.nfacets, s.nloaded, s.nvalues = int(self.facets.numel()), int(self.nodes.numel()), int(self.facets.numel())
        s.nk, s.qdeg = self.nk, self.qdeg
        s.facet_cell, s.facet_local, s.facet_value = (self.facet_cell.data_ptr(), self.facet_local.data_ptr(),
                                                      self.facet_value.data_ptr())
        s.nodes, s.node_ptr, s.entries = self.nodes.data_ptr(), self.node_ptr.data_ptr(), self.entries.data_ptr()
        s.traction_mode, s.traction = tv[0], _lib.ptr(tv[1])
        s.pressure_mode, s.pressure = pv[0], _lib.ptr(pv[1])
        return s


def _surface_load_host(load: SurfaceLoad, alpha: float, b: torch.Tensor) -> torch.Tensor:
    """Plain-torch definition of ``assemble_surface_load`` (any device; what a mesh on the CPU runs). Per slot
    and facet point: J = sum_v x_v (x) gdphi_v, n dS = sign(det J) cof(J) N_ref dS_ref (the cofactor's columns
    are cross products of J's columns: no inverse), dS = |n dS|; then each node's entries summed in the
    plan's order."""
    V = load.V
    m = V.mesh
    gd, dev = m.gdim, m.device
    qd = 2 * V.degree if load.qdeg < 0 else load.qdeg
    Tn = _facet_tables(m.cell_type, V.degree, qd)
    T = {k: torch.as_tensor(v, device=dev) for k, v in Tn.items()}
    cell, lf = load.facet_cell.to(torch.int64), load.facet_local.to(torch.int64)
    nf, nk = int(cell.numel()), load.nk
    if nf == 0:
        return b
    (tmode, tval), (pmode, pval) = load.values()
    xv = m.x[m.cells.to(torch.int64)[cell]]  # [nf, nv, gd]
    J = torch.einsum("fvi,fqvk->fqik", xv, T["gdphi"][lf])  # [nf, nq, gd, gd]
    N = T["nref"][lf][:, None, :]  # [nf, 1, gd]
    if gd == 2:
        det = J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
        nds = torch.stack([J[..., 1, 1] * N[..., 0] - J[..., 1, 0] * N[..., 1],
                           J[..., 0, 0] * N[..., 1] - J[..., 0, 1] * N[..., 0]], -1)
    else:
        j0, j1, j2 = J[..., 0], J[..., 1], J[..., 2]
        c0, c1, c2 = torch.cross(j1, j2, dim=-1), torch.cross(j2, j0, dim=-1), torch.cross(j0, j1, dim=-1)
        det = (j0 * c0).sum(-1)
        nds = c0 * N[..., 0:1] + c1 * N[..., 1:2] + c2 * N[..., 2:3]
    sign = torch.where(det < 0.0, -torch.ones_like(det), torch.ones_like(det))
    nds = sign[..., None] * nds  # [nf, nq, gd]
    dS = torch.sqrt((nds * nds).sum(-1))  # [nf, nq]
    phi = T["phi"][lf]  # [nf, nq, nn]
    nq = phi.shape[1]
    rows = load.facet_value.to(torch.int64)
    dm = V.dofmap.to(torch.int64)[cell]  # [nf, nn]
    g = torch.zeros((nf, nq, gd), dtype=torch.float64, device=dev)
    if tmode != _lib.FA_LOAD_NONE:
        if tmode == _lib.FA_LOAD_CONSTANT:
            tq = tval.reshape(1, 1, gd)
        elif tmode == _lib.FA_LOAD_FACET:
            tq = tval[rows][:, None, :]
        else:
            tq = torch.einsum("fqb,fbi->fqi", phi, tval.reshape(-1, gd)[dm])
        g = g + tq * dS[..., None]
    if pmode != _lib.FA_LOAD_NONE:
        if pmode == _lib.FA_LOAD_CONSTANT:
            pq = pval.reshape(1, 1)
        elif pmode == _lib.FA_LOAD_FACET:
            pq = pval[rows][:, None]
        else:
            pq = torch.einsum("fqb,fb->fq", phi, pval[dm])
        g = g - pq[..., None] * nds
    aloc = T["closure"][lf]  # [nf, nk]
    pha = torch.gather(phi, 2, aloc[:, None, :].expand(nf, nq, nk))  # [nf, nq, nk]
    contrib = torch.einsum("q,fqk,fqi->fki", T["wq"], pha, g).reshape(nf * nk, gd)
    # a node's entries in the plan's order: pass j adds every node's j-th entry
    ptr, ent = load.node_ptr, load.entries.to(torch.int64)
    counts = ptr[1:] - ptr[:-1]
    r = torch.zeros((int(load.nodes.numel()), gd), dtype=torch.float64, device=dev)
    for j in range(int(counts.max())):
        sel = counts > j
        r[sel] += contrib[ent[ptr[:-1][sel] + j]]
    bv = b.view(-1, gd)
    nodes = load.nodes.to(torch.int64)
    bv[nodes] = bv[nodes] + float(alpha) * r
    return b


def assemble_surface_load(load: SurfaceLoad, b: torch.Tensor | None = None, alpha: float = 1.0) -> torch.Tensor:
    """b += alpha * int (t - p n).v ds over the load's facets; returns b (zeros when None). The linear form
    of a linear problem A u = b (dolfinx.fem.assemble_vector of ``dot(t, v)*ds - p*dot(n, v)*ds``); a form
    with ``loads`` subtracts it in ``assemble_vector``. A mesh on the GPU runs k_facet_load
    (fa_facet_load_apply: one thread per loaded node, no atomics, bit-identical run to run), one on the CPU
    the same definition in torch (``_surface_load_host``)."""
    if not isinstance(load, SurfaceLoad):
        raise TypeError("expected a SurfaceLoad")
    V = load.V
    dev = V.mesh.device
    if b is None:
        b = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
    elif b.dtype != torch.float64 or b.dim() != 1 or b.numel() != V.num_dofs or not b.is_contiguous() or b.device != dev:
        raise ValueError(f"b must be a contiguous float64 vector of {V.num_dofs} entries on {dev}")
    if dev.type != "cuda":
        return _surface_load_host(load, alpha, b)
    tv, pv = load.values()
    fm = V._fa_mesh()
    fl = load._fa_facet_load(tv, pv)
    _lib.check(_lib.load().fa_facet_load_apply(ctypes.byref(fm), ctypes.byref(fl), float(alpha), b.data_ptr(),
                                              _lib.stream_handle(dev)), "fa_facet_load_apply")
    return b


# ---------------------------------------------------------------------------------- expressions
QUANTITIES =("grad", "strain", "stress", "energy")


def interpolation_points(ct) -> np.ndarray:
    """The DG0 interpolation point of a cell type, [1, tdim]: its midpoint (1/3, 1/3),
    (1/4, 1/4, 1/4), (1/2, 1/2) or (1/2, 1/2, 1/2) (basix DG0 ``element.points``)."""
    ct = CellType(ct)
    td = len(_REF_VERTS[ct][0])
    return np.full((1, td), 1.0 / (td + 1) if is_simplex(ct) else 0.5)


def value_size(form, quantity: str) -> int:
    """Values per point of a quantity: grad gd*gd; strain and the small-strain stress gd(gd+1)/2
    (reduced: (xx, xy, yy) / (xx, xy, xz, yy, yz, zz)); the neo-Hookean stress (first Piola) gd*gd;
    energy 1."""
    gd = form.V.mesh.gdim
    if quantity not in QUANTITIES:
        raise ValueError(f"unknown quantity {quantity!r}: one of {QUANTITIES}")
    if quantity == "energy":
        return 1
    if quantity == "grad" or (quantity == "stress" and form.kind == _lib.FA_NEO_HOOKEAN):
        return gd * gd
    return gd * (gd + 1) // 2


def _check_expression(form, quantities, X) -> np.ndarray:
    """Host-side argument checks of evaluate / Expression (no device call); returns X [npts, tdim]."""
    if not isinstance(form, LinearElasticity):
        raise TypeError("expected a femasm form descriptor (LinearElasticity, AsymDamage, ...)")
    V = form.V
    if not quantities:
        raise ValueError("no quantity requested")
    for q in quantities:
        value_size(form, q)
    if len(set(quantities)) != len(quantities):
        raise ValueError(f"repeated quantity in {tuple(quantities)}")
    if form.u is None:
        raise ValueError("evaluating an expression needs the form's state u")
    if V.family in ("DG", "Discontinuous Lagrange") or V.bs != V.mesh.gdim:
        raise ValueError("the form's space must be a vector Lagrange space (bs = gdim)")
    if form.kind in (_lib.FA_ASYM_DAMAGE, _lib.FA_ASYM_DAMAGE_AD) and \
            (CellType(V.mesh.cell_type) != CellType.triangle or V.degree != 1):
        raise ValueError("the damage law is the reference's P1-triangle law: its space must be P1 on triangles")
    td = V.mesh.tdim
    X = interpolation_points(V.mesh.cell_type) if X is None else np.ascontiguousarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != td or X.shape[0] < 1:
        raise ValueError(f"X must be reference points [npts >= 1, {td}]")
    return X


def evaluate(form, quantities, X=None, cells=None, out=None) -> dict:
    """Per-cell expressions of the form's state u at reference points, one fa_eval_cells launch for
    all of them (dolfinx ``fem.Expression(...).eval``; the reference evaluates reps(u) and rsig(u) in
    two passes, FEniCSx/mechanic2d/asym_elasto_damage_model.cc:909-942).

    quantities: names from ``QUANTITIES``; "stress" is the form's own law (linear, damage, first Piola
    of NeoHookean), "energy" = inner(eps, sigma). X: reference points [npts, tdim] (None: the cell's
    midpoint, the DG0 interpolation point). cells: cell ids (None: every cell). out: optional
    {name: preallocated float64 tensor of ncells * npts * value_size elements}, contiguous (offset views
    are fine). Returns {name: tensor [ncells, npts * value_size]}."""
    quantities = (quantities,) if isinstance(quantities, str) else tuple(quantities)
    X = _check_expression(form, quantities, X)
    V = form.V
    dev = V.mesh.device
    if cells is None:
        nc, cptr = V.mesh.num_cells, None
    else:
        cells = torch.as_tensor(cells, device=dev).to(torch.int32).contiguous().reshape(-1)
        nc, cptr = int(cells.numel()), cells.data_ptr()
        if nc and (int(cells.min()) < 0 or int(cells.max()) >= V.mesh.num_cells):
            raise ValueError(f"cells outside [0, {V.mesh.num_cells})")
    npts = int(X.shape[0])
    res, ptrs = {}, {}
    for q in quantities:
        w = npts * value_size(form, q)
        t = None if out is None else out.get(q)
        if t is None:
            t = torch.empty((nc, w), dtype=torch.float64, device=dev)
        elif t.dtype != torch.float64 or t.device != dev or not t.is_contiguous() or t.numel() != nc * w:
            raise ValueError(f"out[{q!r}] must be a contiguous float64 tensor of {nc * w} elements on {dev}")
        res[q] = t.view(nc, w)
        ptrs[q] = t.data_ptr()
    # (the neo-Hookean energy goes to the library, which refuses it with FA_E_UNSUPPORTED)
    if nc == 0 and not (form.kind == _lib.FA_NEO_HOOKEAN and "energy" in quantities):
        return res  # nothing to launch
    fm = V._fa_mesh()
    ff = _fa_form(form)
    _lib.check(_lib.load().fa_eval_cells(
        ctypes.byref(fm), ctypes.byref(ff), npts, X.ctypes.data, cptr, nc, ptrs.get("grad"), ptrs.get("strain"),
        ptrs.get("stress"), ptrs.get("energy"), _lib.stream_handle(dev)), "fa_eval_cells")
    return res


class Expression:
    """dolfinx.fem.Expression for the expressions the reference's UFL files end with
    (FEniCSx/mechanic2d/asym_manual.py:103-116: ``(reps(u), centre), (rsig(u), centre), (energ(u),
    centre)``): one quantity of a form's state at the reference points X (None: the cell midpoint)."""

    def __init__(self, form, quantity: str, X=None):
        self.X = _check_expression(form, (quantity,), X)
        self.form = form
        self.quantity = quantity
        self.value_size = value_size(form, quantity)

    def eval(self, mesh=None, cells=None) -> torch.Tensor:
        """Values [ncells, npts * value_size] (dolfinx ``Expression.eval(mesh, cells)``)."""
        if mesh is not None and mesh is not self.form.V.mesh:
            raise ValueError("the Expression's form lives on another mesh")
        return evaluate(self.form, (self.quantity,), X=self.X, cells=cells)[self.quantity]


# ---------------------------------------------------------------------------------- scalar functionals
def quadrature(cell_type, qdeg: int):
    """(points [nq, tdim], weights [nq]) of the library's rule of degree qdeg on the reference cell, as numpy
    arrays (fa_quadrature: host only; the rule every kernel integrates with, not a copy of it)."""
    L = _lib.load()
    ct = int(CellType(cell_type))
    nq = ctypes.c_int32(0)
    _lib.check(L.fa_quadrature(ct, int(qdeg), ctypes.byref(nq), None, None), "fa_quadrature")
    td = len(_REF_VERTS[CellType(cell_type)][0])
    pts, wts = np.empty((nq.value, td)), np.empty(nq.value)
    _lib.check(L.fa_quadrature(ct, int(qdeg), ctypes.byref(nq), pts.ctypes.data, wts.ctypes.data), "fa_quadrature")
    return pts, wts


def quadrature_points(V: FunctionSpace, qdeg: int) -> torch.Tensor:
    """Physical coordinates [ncells, nq, gdim] of the degree-qdeg rule's points in every cell (the geometry
    map applied to ``quadrature(...)[0]``): ``g = exact(xq)`` for ``L2Norm2``."""
    m = V.mesh
    X, _ = quadrature(m.cell_type, qdeg)
    Psi = torch.tensor(_geometry_basis(m.cell_type, X), dtype=torch.float64, device=m.device)  # [nq, nv]
    return torch.einsum("qv,cvd->cqd", Psi, m.x[m.cells.to(torch.int64)])


def _space_basis_gradients(ct, p: int, X: np.ndarray) -> np.ndarray:
    """Reference gradients of the degree-p Lagrange basis (basix node order) at X [n, tdim] -> [n, nn, tdim]."""
    ct = CellType(ct)
    n, td = X.shape
    if is_simplex(ct):
        lam = np.concatenate([1.0 - X.sum(1, keepdims=True), X], axis=1)  # [n, nv]
        gl = np.concatenate([-np.ones((1, td)), np.eye(td)], 0)  # [nv, td]
        if p == 1:
            return np.broadcast_to(gl, (n, td + 1, td)).copy()
        if p != 2:
            raise NotImplementedError("simplex degree > 2")
        out = [(4.0 * lam[:, :, None] - 1.0) * gl[None]]
        for i, j in _EDGES[ct]:
            out.append(4.0 * (lam[:, [i], None] * gl[None, [j]] + lam[:, [j], None] * gl[None, [i]]))
        return np.concatenate(out, axis=1)
    r = line_points(p)
    v1, d1 = [], []  # per direction, the 1-D Lagrange polynomials and derivatives at the points [n, p + 1]
    for d in range(td):
        vc, dc = [], []
        for i in range(p + 1):
            v = np.ones(n)
            dv = np.zeros(n)
            for k in range(p + 1):
                if k != i:
                    t = (X[:, d] - r[k]) / (r[i] - r[k])
                    dv = dv * t + v / (r[i] - r[k])
                    v = v * t
            vc.append(v)
            dc.append(dv)
        v1.append(np.stack(vc, 1))
        d1.append(np.stack(dc, 1))
    L = node_lattice(ct, p)
    out = np.ones((n, L.shape[0], td))
    for k in range(td):
        for d in range(td):
            out[:, :, k] *= (d1 if d == k else v1)[d][:, L[:, d]]
    return out


def _field(w):
    return w.x if isinstance(w, Function) else w


# ---------------------------------------------------------------------------------- evaluation at points
def _eval_points_host(V: FunctionSpace, w: torch.Tensor, cells: torch.Tensor, X: torch.Tensor, grad: bool):
    """k_eval_points in torch (what a mesh on the CPU runs): (val [n, bs], grad [n, bs, gdim] or None)."""
    m = V.mesh
    bs, gd = V.bs, m.gdim
    found = cells >= 0
    c = cells.to(torch.int64).clamp(min=0)
    Xs = torch.where(found[:, None], X, torch.zeros_like(X))
    Xn = Xs.cpu().numpy()
    dev = m.device
    phi = torch.as_tensor(_space_basis(m.cell_type, V.degree, Xn), device=dev)  # [n, nn]
    wc = w.view(-1, bs)[V.dofmap.to(torch.int64)[c]]  # [n, nn, bs]
    nan = float("nan")
    val = torch.einsum("na,nar->nr", phi, wc)
    val = torch.where(found[:, None], val, torch.full_like(val, nan))
    if not grad:
        return val, None
    dphi = torch.as_tensor(_space_basis_gradients(m.cell_type, V.degree, Xn), device=dev)  # [n, nn, td]
    gg = torch.as_tensor(_geometry_gradients(m.cell_type, Xn), device=dev)  # [n, nv, td]
    xv = m.x[m.cells.to(torch.int64)[c]]
    xv = xv - xv[:, :1]
    J = torch.einsum("nvi,nvk->nik", xv, gg)
    R = torch.einsum("nar,nak->nrk", wc, dphi)
    g = torch.einsum("nrk,nkj->nrj", R, torch.linalg.inv(J)) if J.shape[0] else R
    return val, torch.where(found[:, None, None], g, torch.full_like(g, nan))


def eval_points(u, x=None, cells=None, X=None, grad: bool = False, V: FunctionSpace | None = None):
    """A finite-element field at arbitrary physical points: values [n, bs], and with ``grad=True`` also the
    gradients [n, bs, gdim] (d u_r / d x_j), at the points x [n, gdim]. u: a ``Function``, or a nodal tensor
    with its space ``V``; block size 1 to 3. The points are located with ``geometry.locate_points`` unless
    ``cells`` and ``X`` (its two results) are given; ``cells`` alone pulls the points back into those cells
    (dolfinx ``Function.eval(x, cells)``). Rows whose point no cell holds (cell -1) are NaN.
    A GPU mesh runs k_eval_points (fa_eval_points: the basis evaluated on the device at each point's own
    reference coordinates, one lane per point); a CPU mesh the same definition in torch. A DG0 space returns
    ``u.x[cell]``; its gradient raises."""
    from . import geometry

    if isinstance(u, Function):
        V, w = u.function_space, u.x
    else:
        if V is None:
            raise ValueError("a nodal tensor needs its space: eval_points(w, x, V=V)")
        w = u
    m = V.mesh
    dev, gd, bs = m.device, m.gdim, V.bs
    if not 1 <= bs <= 3:
        raise ValueError(f"eval_points: block size {bs} outside 1 .. 3")
    if w.dtype != torch.float64 or w.numel() != V.num_dofs or not w.is_contiguous() or w.device != dev:
        raise ValueError(f"u must be a contiguous float64 vector of {V.num_dofs} entries on {dev}")
    if cells is None or X is None:
        if x is None:
            raise ValueError("eval_points needs the points x, or cells and X")
        x = torch.as_tensor(x, dtype=torch.float64, device=dev).reshape(-1, gd).contiguous()
        if cells is None:
            cells, X = geometry.locate_points(m, x)
        else:
            cells = torch.as_tensor(cells, device=dev).to(torch.int32).reshape(-1).contiguous()
            X = geometry.pull_back(m, x, cells)
    cells = torch.as_tensor(cells, device=dev).to(torch.int32).reshape(-1).contiguous()
    X = torch.as_tensor(X, dtype=torch.float64, device=dev).reshape(-1, gd).contiguous()
    n = cells.numel()
    if X.shape[0] != n:
        raise ValueError(f"{n} cells but {X.shape[0]} reference points")
    if V.family in ("DG", "Discontinuous Lagrange"):
        if grad:
            raise ValueError("a DG0 function has no gradient to evaluate")
        found = cells >= 0
        val = w.view(-1, bs)[cells.to(torch.int64).clamp(min=0)]
        return torch.where(found[:, None], val, torch.full_like(val, float("nan")))
    if dev.type != "cuda":
        val, g = _eval_points_host(V, w, cells, X, grad)
        return (val, g) if grad else val
    val = torch.empty((n, bs), dtype=torch.float64, device=dev)
    g = torch.empty((n, bs, gd), dtype=torch.float64, device=dev) if grad else None
    if n:
        fm = V._fa_mesh()
        _lib.check(_lib.load().fa_eval_points(ctypes.byref(fm), w.data_ptr(), bs, n, cells.data_ptr(), X.data_ptr(),
                                              val.data_ptr(), _lib.ptr(g), _lib.stream_handle(dev)), "fa_eval_points")
    return (val, g) if grad else val


class Measure:
    """int 1 dx over V's mesh (any rule is exact on affine cells)."""
    kind = _lib.FA_FUNC_MEASURE

    def __init__(self, V: FunctionSpace, qdeg: int | None = None):
        self.V, self.qdeg = V, qdeg


class StrainEnergy:
    """int psi(grad u) dx of the form's law at its state ``form.u``, on the form's own rule: the potential
    whose gradient is ``assemble_vector``'s sigma term. Linear: lam/2 tr(eps)^2 + mu eps:eps; NeoHookean:
    mu/2 (I_C - 3) - mu ln J + lam/2 (ln J)^2 (non-finite when a cell is inverted); AsymDamage: the
    reference's damage potential with the mean nodal damage of the cell."""
    kind = _lib.FA_FUNC_STRAIN_ENERGY

    def __init__(self, form):
        if not isinstance(form, LinearElasticity):
            raise TypeError("expected a femasm form descriptor (LinearElasticity, AsymDamage, NeoHookean)")
        self.form, self.V, self.qdeg = form, form.V, None


class L2Norm2:
    """int |w - g|^2 dx: w a Function or nodal tensor on V, g [ncells, nq, bs] values at
    ``quadrature_points(V, qdeg)`` (None: zero); qdeg None = 2 * degree."""
    kind = _lib.FA_FUNC_L2

    def __init__(self, w, g=None, qdeg: int | None = None, V: FunctionSpace | None = None):
        self.V = w.function_space if isinstance(w, Function) else V
        if self.V is None:
            raise ValueError("a nodal tensor needs its space: L2Norm2(w, V=V)")
        self.w, self.g, self.qdeg = w, g, qdeg


class H1Semi2(L2Norm2):
    """int |grad w - G|^2 dx: G [ncells, nq, bs, gdim] values at the rule's points (None: zero)."""
    kind = _lib.FA_FUNC_H1

    def __init__(self, w, G=None, qdeg: int | None = None, V: FunctionSpace | None = None):
        super().__init__(w, G, qdeg, V)


class TotalEnergy:
    """Pi(u) = StrainEnergy(form) - dot(u, b_ext) with b_ext = -assemble_vector(the form without its state):
    the body force on the degree-2p rule and every ``SurfaceLoad``, from the residual's own kernels, so that
    grad Pi(u) is exactly ``assemble_vector(form)``. b_ext is held by the object; ``refresh()`` rebuilds it
    after the force or a load's values changed."""

    def __init__(self, form):
        self.strain = StrainEnergy(form)
        self.form, self.V = form, form.V
        self.b_ext = None
        self.refresh()

    def refresh(self):
        import copy

        ext = copy.copy(self.form)
        # no state: the sigma term vanishes whatever the law, so the copy is a plain linear form (the
        # library refuses a neo-Hookean form without u)
        ext.u, ext.d, ext.kind = None, None, _lib.FA_LINEAR_ELASTICITY
        V = self.V
        if V.mesh.device.type == "cuda":
            self.b_ext = assemble_vector(ext).neg_()
        else:
            b = _body_force_host(ext)
            for ld in getattr(ext, "loads", None) or ():
                assemble_surface_load(ld, b, alpha=1.0)
            self.b_ext = b
        return self


def _func_qdeg(M) -> int:
    """The rule's degree as the library resolves it (fa_assemble_scalar)."""
    V = M.V
    ct, p = V.mesh.cell_type, V.degree
    est = 2 * (p - 1) if is_simplex(ct) else 2 * p
    if M.kind == _lib.FA_FUNC_STRAIN_ENERGY:
        if M.form.kind in (_lib.FA_ASYM_DAMAGE, _lib.FA_ASYM_DAMAGE_AD):
            return 1
        q = M.form.qdeg
        return est if q < 0 else q
    if M.qdeg is not None and M.qdeg >= 0:
        return int(M.qdeg)
    return max(1, est) if M.kind == _lib.FA_FUNC_MEASURE else 2 * p


def _host_geometry(V: FunctionSpace, qdeg: int):
    """(wd [nc, nq], gphys [nc, nq, nn, gd], |dphi| |J^-1| majorant of gphys, phi [nq, nn]) on any device."""
    m = V.mesh
    dev = m.device
    X, wq = quadrature(m.cell_type, qdeg)
    phi = torch.as_tensor(_space_basis(m.cell_type, V.degree, X), device=dev)
    dphi = torch.as_tensor(_space_basis_gradients(m.cell_type, V.degree, X), device=dev)
    gd = torch.as_tensor(_geometry_gradients(m.cell_type, X), device=dev)
    xv = m.x[m.cells.to(torch.int64)]  # [nc, nv, gd]
    J = torch.einsum("cvi,qvk->cqik", xv, gd)
    if J.shape[0] == 0:
        z = torch.zeros((0, len(wq)), dtype=torch.float64, device=dev)
        g0 = torch.zeros((0, len(wq), phi.shape[1], m.gdim), dtype=torch.float64, device=dev)
        return z, g0, g0, phi
    Ji = torch.linalg.inv(J)
    wd = torch.as_tensor(wq, device=dev)[None, :] * torch.linalg.det(J).abs()
    gphys = torch.einsum("qbk,cqkd->cqbd", dphi, Ji)
    gabs = torch.einsum("qbk,cqkd->cqbd", dphi.abs(), Ji.abs())
    return wd, gphys, gabs, phi


def _body_force_host(form) -> torch.Tensor:
    """int f.v dx on the degree-2p rule in torch (the load term of k_vector with the sign of a right-hand side)."""
    V = form.V
    dev = V.mesh.device
    b = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
    if form.f is None:
        return b
    bs = V.bs
    wd, _, _, phi = _host_geometry(V, 2 * V.degree)
    dm = V.dofmap.to(torch.int64)
    fq = torch.einsum("qb,cbi->cqi", phi, form.f.view(-1, bs)[dm])
    contrib = torch.einsum("cq,qa,cqi->cai", wd, phi, fq)
    b.view(-1, bs).index_add_(0, dm.reshape(-1), contrib.reshape(-1, bs))
    return b


def _perm_abs(Fa: torch.Tensor) -> torch.Tensor:
    """The determinant's expansion with every product taken in absolute value (Fa >= 0), [..., gd, gd]."""
    if Fa.shape[-1] == 2:
        return Fa[..., 0, 0] * Fa[..., 1, 1] + Fa[..., 0, 1] * Fa[..., 1, 0]
    a = Fa
    return (a[..., 0, 0] * (a[..., 1, 1] * a[..., 2, 2] + a[..., 1, 2] * a[..., 2, 1])
            + a[..., 0, 1] * (a[..., 1, 0] * a[..., 2, 2] + a[..., 1, 2] * a[..., 2, 0])
            + a[..., 0, 2] * (a[..., 1, 0] * a[..., 2, 1] + a[..., 1, 1] * a[..., 2, 0]))


def _det(F: torch.Tensor) -> torch.Tensor:
    if F.shape[-1] == 2:
        return F[..., 0, 0] * F[..., 1, 1] - F[..., 0, 1] * F[..., 1, 0]
    return (F[..., 0, 0] * (F[..., 1, 1] * F[..., 2, 2] - F[..., 1, 2] * F[..., 2, 1])
            - F[..., 0, 1] * (F[..., 1, 0] * F[..., 2, 2] - F[..., 1, 2] * F[..., 2, 0])
            + F[..., 0, 2] * (F[..., 1, 0] * F[..., 2, 1] - F[..., 1, 1] * F[..., 2, 0]))


def assemble_scalar_host(M):
    """The functionals' definitions in differentiable torch, on the mesh's device (what a mesh on the CPU
    runs): (cell integrals [nc], magnitudes [nc]). A cell's magnitude is its integral evaluated with every
    product replaced by its absolute value and every difference by a sum (for ln J and the principal strains,
    whose arguments cancel, the first-order bound of their error): rounding moves the cell integral by a
    few units of 1.1e-16 times it, which is what the device parity bars are stated in. ``TotalEnergy`` has
    no per-cell split: use its ``strain`` part."""
    if isinstance(M, TotalEnergy):
        raise ValueError("TotalEnergy has no per-cell split: pass M.strain")
    V = M.V
    bs = V.bs
    if V.family in ("DG", "Discontinuous Lagrange") or bs != V.mesh.gdim:
        raise ValueError("functionals live on a vector Lagrange space (bs = gdim)")
    wd, gp, ga, phi = _host_geometry(V, _func_qdeg(M))
    dm = V.dofmap.to(torch.int64)
    if M.kind == _lib.FA_FUNC_MEASURE:
        v = wd.sum(1)
        return v, v.detach().abs()
    if M.kind in (_lib.FA_FUNC_L2, _lib.FA_FUNC_H1):
        wc = _field(M.w).view(-1, bs)[dm]  # [nc, nn, bs]
        if M.kind == _lib.FA_FUNC_L2:
            val = torch.einsum("qb,cbi->cqi", phi, wc)
            mag = torch.einsum("qb,cbi->cqi", phi.abs(), wc.abs())
        else:
            val = torch.einsum("cbi,cqbk->cqik", wc, gp)
            mag = torch.einsum("cbi,cqbk->cqik", wc.abs(), ga)
        if M.g is not None:
            g = M.g.reshape(val.shape)
            val, mag = val - g, mag + g.abs()
        s = (val * val).reshape(val.shape[0], val.shape[1], -1).sum(2)
        sm = (mag * mag).reshape(val.shape[0], val.shape[1], -1).sum(2)
        return (wd * s).sum(1), (wd * sm).sum(1).detach()
    form = M.form
    if form.u is None:
        raise ValueError("the strain energy needs the form's state u")
    if form.E is not None:
        mu = form.E / (2.0 * (1.0 + form.nu))
        lam = form.E * form.nu / ((1.0 + form.nu) * (1.0 - 2.0 * form.nu))
    else:
        lam, mu = form.lam, form.mu
    lam, mu = lam[:, None], mu[:, None]
    uc = form.u.view(-1, bs)[dm]
    gu = torch.einsum("cbi,cqbk->cqik", uc, gp)
    gua = torch.einsum("cbi,cqbk->cqik", uc.detach().abs(), ga)
    eye = torch.eye(bs, dtype=torch.float64, device=gu.device)

    def lin(g):
        tr = g.diagonal(dim1=-2, dim2=-1).sum(-1)
        eps = 0.5 * (g + g.transpose(-1, -2))
        return tr, (eps * eps).sum((-1, -2))

    if form.kind == _lib.FA_NEO_HOOKEAN:
        F, Fa = gu + eye, gua + eye
        Jd = _det(F)
        lnJ = torch.log(Jd)
        psi = 0.5 * mu * ((F * F).sum((-1, -2)) - bs) - mu * lnJ + 0.5 * lam * lnJ * lnJ
        with torch.no_grad():
            ln = lnJ.abs()
            pm = (0.5 * mu.abs() * ((Fa * Fa).sum((-1, -2)) + bs) + mu.abs() * ln + 0.5 * lam.abs() * ln * ln
                  + (mu.abs() + lam.abs() * ln) * _perm_abs(Fa) / Jd.abs())
    else:
        tr, ee = lin(gu)
        psi = 0.5 * lam * tr * tr + mu * ee
        tra, eea = lin(gua)
        pm = 0.5 * lam.abs() * tra * tra + mu.abs() * eea
        if form.kind in (_lib.FA_ASYM_DAMAGE, _lib.FA_ASYM_DAMAGE_AD) and form.d is not None:
            d = form.d[dm].sum(1, keepdim=True) * (1.0 / 3.0)  # [nc, 1]: the mean nodal damage, unclamped
            e11, e22, e12 = gu[..., 0, 0], gu[..., 1, 1], 0.5 * (gu[..., 0, 1] + gu[..., 1, 0])
            I1, I2 = e11 + e22, e12 * e12 - e11 * e22
            with torch.no_grad():
                nz = (I1.abs() > 1e-12) | (I2.abs() > 1e-12)
            dl = I1 * I1 + 4.0 * I2
            with torch.no_grad():
                # the double eigenvalue (the hand hook's r < 1e-12): sqrt has no derivative at 0, psi has
                # (dl cancels to +-ulp(I1^2) there on a strain with roundoff: the test also takes the form that does not)
                dl2 = (e11 - e22) * (e11 - e22) + 4.0 * e12 * e12
                dbl = nz & (torch.sqrt(torch.minimum(dl, dl2).clamp_min(0.0)) < 1e-12)
                gen = nz & ~dbl
            r = torch.sqrt(torch.where(gen, dl, torch.ones_like(I1)))
            ev1, ev2 = 0.5 * (I1 + r), 0.5 * (I1 - r)
            with torch.no_grad():
                a1, a2 = (ev1 >= 0).to(gu.dtype), (ev2 >= 0).to(gu.dtype)
                al = ((ev1 + ev2) >= 0).to(gu.dtype)
                ai = (I1 >= 0).to(gu.dtype)
            p_dam = 0.5 * (1.0 - al * d) * lam * (I1 * I1) + mu * ((1.0 - a1 * d) * ev1 * ev1 + (1.0 - a2 * d) * ev2 * ev2)
            # |I1| > 1e-12 > r there: ev1, ev2 and I1 share a sign and ev1^2 + ev2^2 = (I1^2 + delta) / 2
            p_dbl = (1.0 - ai * d) * (0.5 * lam * (I1 * I1) + 0.5 * mu * (I1 * I1 + dl))
            p_null = (1.0 - d) * (0.5 * lam * (I1 * I1) + mu * (e11 * e11 + e22 * e22 + 2.0 * e12 * e12))
            psi = torch.where(d > 0, torch.where(gen, p_dam, torch.where(dbl, p_dbl, p_null)), psi)
            with torch.no_grad():
                I1a = gua[..., 0, 0] + gua[..., 1, 1]
                e12a = 0.5 * (gua[..., 0, 1] + gua[..., 1, 0])
                da = I1a * I1a + 4.0 * (e12a * e12a + gua[..., 0, 0] * gua[..., 1, 1])
                eva = 0.5 * (I1a + da / r)  # r's error is bounded by eps * da / (2 r), and r <= da / r
                pd = 0.5 * lam.abs() * I1a * I1a + 2.0 * mu.abs() * eva * eva
                pb = 0.5 * lam.abs() * I1a * I1a + 0.5 * mu.abs() * (I1a * I1a + da)
                pm = torch.where(d > 0, torch.where(gen, pd, torch.where(dbl, pb, pm)), pm)
    return (wd * psi).sum(1), (wd * pm).sum(1).detach()


def _functional_work(V: FunctionSpace, fm) -> torch.Tensor:
    """The reduction's workspace, cached on V (the library allocates nothing per call)."""
    nb = ctypes.c_int64(0)
    _lib.check(_lib.load().fa_functional_work_bytes(ctypes.byref(fm), ctypes.byref(nb)), "fa_functional_work_bytes")
    wk = V.__dict__.get("_functional_work")
    if wk is None or wk.numel() < nb.value or wk.device != V.mesh.device:
        wk = torch.empty(nb.value, dtype=torch.uint8, device=V.mesh.device)
        V.__dict__["_functional_work"] = wk
    return wk


def assemble_scalar(M, cellwise: bool = False, out: torch.Tensor | None = None) -> torch.Tensor:
    """dolfinx.fem.assemble_scalar for a functional descriptor (``Measure``, ``StrainEnergy``, ``L2Norm2``,
    ``H1Semi2``, ``TotalEnergy``): a 0-d float64 tensor on the mesh's device (nothing is synchronised: the
    caller's ``float()`` does), or with ``cellwise=True`` the [ncells] cell integrals. A mesh on the GPU runs
    k_functional_cells (every cell once, one lane per cell) and k_functional_reduce (fixed-order sums, no
    atomics: bit-identical run to run); a mesh on the CPU runs ``assemble_scalar_host``, differentiable with
    respect to a state that requires grad. out: optional preallocated result (GPU meshes; every entry is
    written)."""
    if isinstance(M, TotalEnergy):
        if cellwise:
            raise ValueError("TotalEnergy has no per-cell split: pass M.strain")
        return assemble_scalar(M.strain) - torch.dot(M.form.u, M.b_ext)
    if not isinstance(M, (Measure, StrainEnergy, L2Norm2)):
        raise TypeError("expected a functional descriptor (Measure, StrainEnergy, L2Norm2, H1Semi2, TotalEnergy)")
    V = M.V
    dev = V.mesh.device
    if dev.type != "cuda":
        cells, _ = assemble_scalar_host(M)
        return cells if cellwise else cells.sum()
    nc = V.mesh.num_cells
    if V.family in ("DG", "Discontinuous Lagrange") or V.bs != V.mesh.gdim:
        raise ValueError("functionals live on a vector Lagrange space (bs = gdim)")
    w = g = None
    ff = None
    if M.kind == _lib.FA_FUNC_STRAIN_ENERGY:
        if M.form.u is None:
            raise ValueError("the strain energy needs the form's state u")
        ff = _fa_form(M.form)
    elif M.kind != _lib.FA_FUNC_MEASURE:
        w = _field(M.w)
        if w.dtype != torch.float64 or w.numel() != V.num_dofs or not w.is_contiguous() or w.device != dev:
            raise ValueError(f"w must be a contiguous float64 vector of {V.num_dofs} entries on {dev}")
        if M.g is not None:
            nq = len(quadrature(V.mesh.cell_type, _func_qdeg(M))[1])
            per = V.bs * (V.mesh.gdim if M.kind == _lib.FA_FUNC_H1 else 1)
            g = M.g
            if g.dtype != torch.float64 or g.numel() != nc * nq * per or not g.is_contiguous() or g.device != dev:
                raise ValueError(f"g must be a contiguous float64 tensor of {nc} x {nq} x {per} values on {dev}")
    fm = V._fa_mesh()
    wk = _functional_work(V, fm)
    if out is None:
        out = torch.empty(nc if cellwise else (), dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or out.device != dev or not out.is_contiguous() or \
            out.shape != ((nc,) if cellwise else ()):
        raise ValueError(f"out must be a contiguous float64 tensor of shape {(nc,) if cellwise else ()} on {dev}")
    qd = -1 if getattr(M, "qdeg", None) is None else int(M.qdeg)
    _lib.check(_lib.load().fa_assemble_scalar(
        ctypes.byref(fm), None if ff is None else ctypes.byref(ff), int(M.kind), _lib.ptr(w), _lib.ptr(g), qd,
        out.data_ptr() if cellwise else None, wk.data_ptr(), wk.numel(), None if cellwise else out.data_ptr(),
        _lib.stream_handle(dev)), "fa_assemble_scalar")
    return out


# ---------------------------------------------------------------------------------- damage field
# The reference's second step: mark the vertices of tagged entities and spread the marks over the vertex
# graph (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:315-475, MFEM/mechanic2d/asym_elasto_damage_model.cc:
# 1159-1315). One process owns every vertex here, so the reference's scatter_rev / scatter_fwd exchanges
# between the passes collapse to nothing.
def mark_vertices(m: Mesh, dim: int, entities, value: float = 1.0, out: torch.Tensor | None = None) -> torch.Tensor:
    """A per-vertex float64 field [nv] with ``value`` at every vertex of the given entities of dimension
    ``dim`` (0 .. tdim) and 0 elsewhere; with ``out`` the values are written into that field instead, the
    rest of it stays, and it is returned. Entity ids are those of ``mesh.entities(m, dim)`` (vertex indices
    for dim 0, cell ids for dim = tdim): what ``io.MeshTags.find``, ``read_gmsh_tags(...).find`` and
    ``locate_entities_boundary`` return. Order and duplicates in ``entities`` do not matter (every writer of
    a vertex writes the same value). An id outside the mesh's entities raises ValueError before anything is
    indexed."""
    from . import mesh as _mesh

    dim = int(dim)
    if not 0 <= dim <= m.tdim:
        raise ValueError(f"entities of dimension 0 .. {m.tdim}, not {dim}")
    dev = m.device
    nv = m.num_vertices
    ids = torch.as_tensor(entities, device=dev).reshape(-1)
    if ids.numel() and (ids.dtype.is_floating_point or ids.dtype in (torch.bool, torch.complex64, torch.complex128)):
        raise ValueError(f"entity ids are integers, not {ids.dtype}")
    ids = ids.to(torch.int64)
    if dim == 0:
        count, verts = nv, None
    elif dim == m.tdim:
        count, verts = m.num_cells, m.cells
    else:
        verts = _mesh.entities(m, dim)[0]
        count = int(verts.shape[0])
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= count):
        raise ValueError(f"entity ids outside [0, {count}) of dimension {dim}")
    if out is None:
        out = torch.zeros(nv, dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or out.shape != (nv,) or out.device != dev:
        raise ValueError(f"out must be a float64 tensor of {nv} entries on {dev}")
    v = ids if verts is None else verts[ids].reshape(-1).to(torch.int64)
    out[v] = float(value)
    return out


def _spread_host(indptr: torch.Tensor, indices: torch.Tensor, inv_deg: torch.Tensor, d: torch.Tensor,
                 iterations: int, threshold: float) -> torch.Tensor:
    """The spread in torch ops (any device; the definition's arithmetic). Rows are padded to the largest degree
    with an index that points at an appended 0.0 and summed column by column: x + 0.0 == x exactly for x >= 0,
    so every row's sum is the sequential one, bit for bit."""
    nv = int(d.shape[0])
    deg = indptr[1:] - indptr[:-1]
    width = int(deg.max()) if nv else 0
    row = torch.repeat_interleave(torch.arange(nv, dtype=torch.int64, device=d.device), deg)
    col = torch.arange(indices.shape[0], dtype=torch.int64, device=d.device) - indptr[:-1][row]
    padded = torch.full((nv, width), nv, dtype=torch.int64, device=d.device)
    padded[row, col] = indices.to(torch.int64)

    def row_sums(f):
        fz = torch.cat([f, torch.zeros(1, dtype=f.dtype, device=f.device)])
        s = torch.zeros_like(f)
        for k in range(width):
            s = s + fz[padded[:, k]]
        return s

    for _ in range(iterations):
        s = torch.where(d < threshold, row_sums(d), torch.zeros_like(d))
        d = torch.maximum(s * inv_deg, d)
        d = torch.maximum(row_sums(d) * inv_deg, d)
    return d


def spread(m: Mesh, d0: torch.Tensor, iterations: int, threshold: float = 0.01) -> torch.Tensor:
    """``iterations`` spreading iterations of the per-vertex field ``d0`` [nv] (float64, finite, >= 0) on the
    vertex graph of ``m`` (``mesh.vertex_graph``); ``d0`` is left untouched. With N(v) the neighbours of v in
    ascending index and r(v) = 1 / |N(v)| (0 for a vertex without neighbours, which keeps its value), one
    iteration is two Jacobi passes, each reading the previous field only:

      gated   s(v) = sum of d(w), w in N(v), where d(v) < threshold, else 0;   d'(v)  = max(s(v) r(v), d(v))
      full    s(v) = sum of d'(w), w in N(v);                                  d''(v) = max(s(v) r(v), d'(v))

    The sum starts at 0.0 and adds the neighbours one by one in ascending index, is multiplied by the stored
    reciprocal and compared: a mesh on the GPU (fa_vertex_spread, one lane per vertex, no atomics), one on
    the CPU (the same passes in torch ops) and a sequential loop agree bit for bit. ``threshold`` may be
    ``inf`` (every vertex takes the gated pass) or 0 (none does)."""
    from . import mesh as _mesh

    nv = m.num_vertices
    dev = m.device
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f"iterations must not be negative ({iterations})")
    threshold = float(threshold)
    if threshold != threshold:
        raise ValueError("threshold is NaN")
    if not isinstance(d0, torch.Tensor) or d0.dtype != torch.float64 or d0.shape != (nv,) or d0.device != dev:
        raise ValueError(f"d0 must be a float64 tensor of {nv} entries on {dev}")
    if nv and not bool((torch.isfinite(d0) & (d0 >= 0)).all()):
        raise ValueError("d0 must be finite and >= 0")
    indptr, indices, inv_deg = _mesh._vertex_graph(m)
    if iterations == 0 or nv == 0 or indices.numel() == 0:
        return d0.clone()
    if dev.type != "cuda":
        return _spread_host(indptr, indices, inv_deg, d0, iterations, threshold)
    d = d0.contiguous().clone()
    tmp = torch.empty_like(d)
    _lib.check(_lib.load().fa_vertex_spread(nv, indptr.data_ptr(), indices.data_ptr(), inv_deg.data_ptr(),
                                            d.data_ptr(), tmp.data_ptr(), iterations, threshold,
                                            _lib.stream_handle(dev)), "fa_vertex_spread")
    return d


def damage_field(S: FunctionSpace, entities=None, dim: int = 1, tags=None, values=None, d_max: float = 1.0,
                 iterations: int | None = None, threshold: float = 0.01, name: str = "d") -> Function:
    """The reference's damage field on the scalar degree-1 Lagrange space ``S``: ``d_max`` at the vertices of
    the selected entities (``mark_vertices``), spread over the vertex graph (``spread``); the Function that
    ``AsymDamage(V, ..., d=d)`` takes. Select either ``entities`` of dimension ``dim`` (ids of
    ``mesh.entities``), or ``tags`` (an ``io.MeshTags``, whose ``dim`` is used) with ``values``, the list of tag
    values whose entities are damaged (the reference's ``tag_edges_damaged``).

    ``iterations`` defaults to ``8 * (R + 1)``, the reference's ``8 * (MAX_REFINE + 1)``, with R the length of
    the mesh's ``parent`` chain: the number of ``mesh.refine`` calls that produced it. A mesh whose parents
    were dropped (rebuilt from its arrays, or moved without them) has R = 0.

    One process owns every vertex; ``parallel.SlabProblem`` and multi-rank ownership are not served."""
    if not isinstance(S, FunctionSpace) or S.family in ("DG", "Discontinuous Lagrange"):
        raise ValueError("the damage field lives on a scalar degree-1 Lagrange space, not a DG space")
    if S.bs != 1:
        raise ValueError(f"the damage field lives on a scalar space (block size 1, not {S.bs})")
    if S.degree != 1:
        raise ValueError(f"the damage field lives on a degree-1 space (node i is vertex i), not degree {S.degree}")
    m = S.mesh
    if S.dofmap is not m.cells:
        raise ValueError("the space's dofmap is not the mesh's cells: its nodes are not the mesh's vertices")
    if (entities is None) == (tags is None):
        raise ValueError("pass either entities or tags (with values), not both and not neither")
    d_max = float(d_max)
    if not d_max > 0 or d_max == float("inf"):
        raise ValueError(f"d_max must be positive and finite ({d_max})")
    if iterations is None:
        R, p = 0, m.parent
        while p is not None:
            R, p = R + 1, p.parent
        iterations = 8 * (R + 1)
    elif int(iterations) < 0:
        raise ValueError(f"iterations must not be negative ({iterations})")
    if tags is not None:
        if values is None:
            raise ValueError("tags need values: the tag values whose entities are damaged")
        dim = tags.dim
        vals = [values] if isinstance(values, int) else list(values)
        found = [tags.find(v).to(m.device).to(torch.int64) for v in vals]
        entities = torch.cat(found) if found else torch.zeros(0, dtype=torch.int64, device=m.device)
    elif values is not None:
        raise ValueError("values select among tags: pass tags with them")
    d0 = mark_vertices(m, dim, entities, d_max)
    return Function(S, name, spread(m, d0, int(iterations), threshold))
