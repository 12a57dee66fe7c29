"""Dirichlet sets of the constraint-set tests (tests/test_dirichlet_sets_host.py on the CPU,
tests/test_gpu_dirichlet_sets.py on the device): tables and set builders, no device work.

Every other suite constrains all components on the planes x0 = 0 and x0 = 1, which sets a fraction of the
per-cell bit positions (local node, component) the kernels read. The sets here are constructed so that every
position of every cell is set by one set and clear under another, cell-interior nodes are constrained, a
node has exactly one of its components constrained, whole cells are constrained, and nothing is.

build(name, V, seed) runs on the CPU (numpy on the node coordinates) and returns
    (bcs, marker, g):  the list of fem.DirichletBC on V's device, and the expected marker (int8) and
                       prescribed values (float64) per dof as numpy arrays,
the two arrays written from the node indices alone: neither reads bc.dofs, bc.g or fem._combine_bcs.
The prescribed values are distinct per dof and per bc (order 1e-2), written into bc.g[bc.dofs] in place
after dirichletbc(): a wrong index into g shows.

Element tables are tests/form_parameters.py's; routes are test_gpu_irregular.ROUTES for simplices and
test_gpu_invariance.routes_of for tensor cells (the GPU file imports those; this file stays importable
without a device)."""
import numpy as np
import torch

from form_parameters import (DAMAGE, DETERMINISTIC, ELEMENTS, HEX, MESHES, NEO, OPERATOR,  # noqa: F401
                             PERTURB, QUAD, TET, TRI, VECTOR_CASES)

SETS = ["scatter", "scatter-complement", "last-component", "interior", "single", "all", "empty", "overlap"]

# Cells per axis of this suite where a coverage condition of test_dirichlet_sets_host.py fails on
# form_parameters.ELEMENTS' own mesh: none does (every mesh there has a node strictly inside the domain
# and a plane x0 = 0), so the table is empty and mesh_of() returns ELEMENTS' sizes.
N_OVERRIDE = {}

G_AMP = 1e-2  # order of the prescribed values
EDGE = 1e-9   # a node is on the boundary of the unit square / cube within this


def mesh_of(elem, table=None):
    """(cell type, degree, cells per axis) of an element id."""
    ct, p, n = (ELEMENTS if table is None else table)[elem]
    return ct, p, N_OVERRIDE.get(elem, n)


def node_coordinates(V) -> np.ndarray:
    return V.tabulate_dof_coordinates().detach().cpu().numpy()


def interior_nodes(xn: np.ndarray) -> np.ndarray:
    """Nodes strictly inside the unit square / cube (bool per node)."""
    return ((xn > EDGE) & (xn < 1.0 - EDGE)).all(1)


def scatter_mask(V, seed) -> np.ndarray:
    """[num_nodes, bs] bool: every dof independently with probability 0.5."""
    return np.random.default_rng(seed).random((V.num_nodes, V.bs)) < 0.5


def _specs(name, V, seed):
    """The set as a list of (node indices int64, components), in bc order. Node lists may repeat a node."""
    xn = node_coordinates(V)
    nn, bs = V.num_nodes, V.bs
    every = np.arange(nn, dtype=np.int64)
    comps = list(range(bs))
    inside = interior_nodes(xn)
    if name in ("scatter", "scatter-complement"):
        m = scatter_mask(V, seed)
        if name == "scatter-complement":
            m = ~m
        return [(np.nonzero(m[:, c])[0].astype(np.int64), [c]) for c in comps]
    if name == "last-component":
        on = np.isclose(xn[:, 0], 0.0) | inside
        return [(every[on], [bs - 1])]
    if name == "interior":
        return [(every[inside], comps)]
    if name == "single":
        pool = every[inside] if inside.any() else every
        k = pool[np.argmin(((xn[pool] - xn.mean(0)) ** 2).sum(1))]
        return [(np.array([k], dtype=np.int64), [1])]
    if name == "all":
        return [(every, comps)]
    if name == "empty":
        return [(np.zeros(0, dtype=np.int64), comps)]
    if name == "overlap":
        # two bcs share the band 0.25 <= x0 <= 0.5 (the later one wins there); the third constrains
        # component 0 on x0 = 1 and names its first node twice
        low = every[xn[:, 0] <= 0.5 + EDGE]
        mid = every[(xn[:, 0] >= 0.25 - EDGE) & (xn[:, 0] <= 0.75 + EDGE)]
        right = every[np.isclose(xn[:, 0], 1.0)]
        return [(low, comps), (mid, comps), (np.concatenate([right, right[:1]]), [0])]
    raise KeyError(name)


def build(name, V, seed=0):
    """(bcs, marker, g) of the set `name` on V: see the module docstring."""
    from femasm import fem

    dev = V.mesh.device
    bs, nd = V.bs, V.num_dofs
    rng = np.random.default_rng(1000 + seed)
    marker = np.zeros(nd, dtype=np.int8)
    g = np.zeros(nd, dtype=np.float64)
    bcs = []
    for nodes, comps in _specs(name, V, seed):
        gb = G_AMP * (0.25 + 0.75 * rng.random(nd)) * rng.choice([-1.0, 1.0], nd)  # this bc's value per dof
        bc = fem.dirichletbc(0.0, torch.as_tensor(nodes, dtype=torch.int64).to(dev), V,
                             components=None if len(comps) == bs else comps)
        if bc.dofs.numel():
            bc.g[bc.dofs] = torch.as_tensor(gb, dtype=torch.float64).to(dev)[bc.dofs]
        bcs.append(bc)
        dofs = (nodes[:, None] * bs + np.asarray(comps, dtype=np.int64)[None, :]).reshape(-1)
        marker[dofs] = 1
        g[dofs] = gb[dofs]  # a later bc overwrites an earlier one
    return bcs, marker, g


def overlap_band(V) -> np.ndarray:
    """Nodes both of the first two bcs of `overlap` hold."""
    xn = node_coordinates(V)
    return np.nonzero((xn[:, 0] >= 0.25 - EDGE) & (xn[:, 0] <= 0.5 + EDGE))[0]


def cell_positions(V, marker: np.ndarray) -> np.ndarray:
    """[num_cells, nn, bs] bool: the constrained (local node, component) positions of every cell."""
    dm = V.dofmap.detach().cpu().numpy().astype(np.int64)
    return marker.reshape(-1, V.bs).astype(bool)[dm]


def cell_masks(V, marker: np.ndarray) -> np.ndarray:
    """The 32-bit mask per cell as the kernels define it (bit b * bs + j for local node b, component j),
    for elements of at most 32 dofs per cell."""
    pos = cell_positions(V, marker)
    nc, nn, bs = pos.shape
    assert nn * bs <= 32
    w = (np.uint64(1) << np.arange(nn * bs, dtype=np.uint64))
    return (pos.reshape(nc, -1).astype(np.uint64) * w[None, :]).sum(1).astype(np.uint64)


def swap_one_dof(V, bc, marker: np.ndarray):
    """In place on bc.dofs: its first constrained dof that no other position of the marker needs becomes
    the first free dof of the same component. Returns (dropped dof, added dof)."""
    bs = V.bs
    dofs = bc.dofs.detach().cpu().numpy()
    drop = int(dofs[0])
    free = np.nonzero(marker == 0)[0]
    add = int(free[free % bs == drop % bs][0])
    bc.dofs[0] = add
    return drop, add
