"""The damage field's definition, restated sequentially in plain Python / NumPy: the yardstick of
test_damage_field_host.py and test_gpu_damage_field.py.

G is the vertex graph of the mesh: v and w are neighbours iff they share an edge of the mesh. N(v) lists the
neighbours of v in ascending index, r(v) = 1 / |N(v)| and r(v) = 0 where N(v) is empty. Marking sets d0 = d_max
at every vertex of every selected entity and 0 elsewhere. One iteration is two Jacobi passes, each reading
only the previous field and writing a new one:

  gated   s(v) = sum of d(w), w in N(v), if d(v) < threshold, else s(v) = 0;   d'(v)  = max(s(v) r(v), d(v))
  full    s(v) = sum of d'(w), w in N(v), for every v;                          d''(v) = max(s(v) r(v), d'(v))

The arithmetic is part of the definition: the sum starts at 0.0 and adds the neighbours one by one in
ascending index, is multiplied by the stored reciprocal (never divided by the degree), then the maximum is
taken. Everything here is scalar float64 arithmetic in that order; nothing is vectorised, so nothing can
reorder a sum. The edges come from the cells and a table of local edges written out here, not from the
package's entity numbering.
"""
import numpy as np

# local edges of a cell as pairs of local vertices (triangle 3, quadrilateral 4 in tensor order v = i + 2j,
# tetrahedron -4, hexahedron 8 in tensor order v = i + 2j + 4k); the keys are the package's CellType values
LOCAL_EDGES = {
    3: ((0, 1), (1, 2), (0, 2)),
    4: ((0, 1), (0, 2), (1, 3), (2, 3)),
    -4: ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)),
    8: ((0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)),
}


def adjacency(cell_type: int, cells, nv: int) -> list:
    """N(v) for every vertex: sorted lists of neighbours."""
    nb = [set() for _ in range(nv)]
    for c in np.asarray(cells).tolist():
        for a, b in LOCAL_EDGES[int(cell_type)]:
            nb[c[a]].add(c[b])
            nb[c[b]].add(c[a])
    return [sorted(s) for s in nb]


def mesh_adjacency(m) -> list:
    return adjacency(int(m.cell_type), m.cells.cpu().numpy(), m.num_vertices)


def num_edges(adj: list) -> int:
    return sum(len(a) for a in adj) // 2


def mark(nv: int, entity_vertices, d_max: float = 1.0) -> np.ndarray:
    """d0: d_max at every vertex of every entity (rows of vertex indices), 0 elsewhere."""
    d = np.zeros(nv, dtype=np.float64)
    for row in np.asarray(entity_vertices).reshape(len(entity_vertices), -1).tolist():
        for v in row:
            d[v] = d_max
    return d


def _pass(adj, r, d, threshold, gated):
    out = [0.0] * len(d)
    for v in range(len(d)):
        s = 0.0
        if not gated or d[v] < threshold:
            for w in adj[v]:
                s = s + d[w]
        a = s * r[v]
        out[v] = a if a > d[v] else d[v]
    return out


def spread(adj: list, d0, iterations: int, threshold: float = 0.01) -> np.ndarray:
    """The sequential loop on Python floats (IEEE binary64, one rounding per operation)."""
    r = [1.0 / len(a) if a else 0.0 for a in adj]
    d = [float(x) for x in np.asarray(d0, dtype=np.float64)]
    for _ in range(iterations):
        d = _pass(adj, r, d, threshold, True)
        d = _pass(adj, r, d, threshold, False)
    return np.array(d, dtype=np.float64)
