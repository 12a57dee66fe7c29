"""Host side of uniform refinement and of the multigrid over a refined hierarchy, no GPU: mesh.refine
(counts, tags, parent, measures, orientation, conformity, the shortest-diagonal rule), the identity
between the P1 nodes of refine(m) and the P2 nodes of m that the edge transfer rests on,
mg.plan_refined_hierarchy and mg.edge_transfer_matrix."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = os.path.join(ROOT, "tests", "golden", "square.msh")


def _single(ct):
    from femasm import mesh

    if ct == 3:
        x = torch.tensor([[0.1, 0.0], [1.3, 0.2], [0.4, 0.9]], dtype=torch.float64)
        return mesh.Mesh(mesh.CellType.triangle, x, torch.tensor([[0, 1, 2]], dtype=torch.int32),
                         torch.tensor([7], dtype=torch.int32))
    x = torch.tensor([[0.0, 0.1, 0.0], [1.2, 0.0, 0.1], [0.3, 0.9, 0.0], [0.2, 0.3, 1.1]], dtype=torch.float64)
    return mesh.Mesh(mesh.CellType.tetrahedron, x, torch.tensor([[0, 1, 2, 3]], dtype=torch.int32),
                     torch.tensor([5], dtype=torch.int32))


def _unstructured_box(n, lengths=(1.0, 1.0, 1.0)):
    from femasm import mesh

    b = mesh.create_box(lengths, n, mesh.CellType.tetrahedron)
    return mesh.Mesh(b.cell_type, b.x, b.cells, None, None)


def _square():
    from femasm import mesh

    return mesh.read_gmsh(SQUARE)


MESHES = {"triangle": lambda: _single(3), "tetrahedron": lambda: _single(-4), "square": _square,
          "box": lambda: _unstructured_box((2, 1, 2), (1.0, 0.7, 1.3))}


def _signed_measures(m):
    x = m.x.numpy()[m.cells.numpy().astype(np.int64)]
    J = x[:, 1:] - x[:, :1]
    return np.linalg.det(J) / (2.0 if m.tdim == 2 else 6.0)


@pytest.mark.parametrize("name", list(MESHES))
def test_counts_tags_parent_measures_orientation(name):
    from femasm import mesh

    m = MESHES[name]()
    ne = int(mesh.entities(m, 1)[0].shape[0])
    r = mesh.refine(m)
    nchild = 2 ** m.tdim
    assert r.cell_type == m.cell_type and r.structured is None and r.parent is m
    assert r.num_vertices == m.num_vertices + ne and r.num_cells == nchild * m.num_cells
    assert r.cells.dtype == torch.int32 and r.x.dtype == torch.float64
    assert torch.equal(r.x[:m.num_vertices], m.x)
    ev = mesh.entities(m, 1)[0]
    assert torch.equal(r.x[m.num_vertices:], 0.5 * (m.x[ev[:, 0]] + m.x[ev[:, 1]]))
    if m.cell_tags is None:
        assert r.cell_tags is None
    else:
        assert torch.equal(r.cell_tags, m.cell_tags[torch.arange(r.num_cells) >> m.tdim])
    vp, vc = _signed_measures(m), _signed_measures(r)
    parent = np.arange(r.num_cells) >> m.tdim
    # each child has measure parent / 2^tdim with the parent's sign (a determinant of 2 or 3 differences
    # of coordinates of size 1: a few ulp of the coordinate scale)
    assert np.abs(vc - vp[parent] / nchild).max() <= 1e-14
    assert (np.sign(vc) == np.sign(vp[parent])).all() and (vc != 0).all()
    assert np.abs(np.bincount(parent, weights=vc) - vp).max() <= 1e-14
    # to() carries the parent along
    r2 = r.to("cpu")
    assert r2.parent is not None and torch.equal(r2.parent.cells, m.cells)


def test_square_twice_and_unsupported_cells():
    from femasm import mesh

    m = _square()
    assert (m.num_cells, m.num_vertices) == (98, 62)
    r1 = mesh.refine(m)
    r2 = mesh.refine(r1)
    ne0 = int(mesh.entities(m, 1)[0].shape[0])
    ne1 = int(mesh.entities(r1, 1)[0].shape[0])
    assert ne0 == 62 + 98 - 1  # Euler: V - E + F = 1 on a disc
    assert (r1.num_cells, r1.num_vertices) == (392, 62 + ne0)
    assert (r2.num_cells, r2.num_vertices) == (1568, 62 + ne0 + ne1)
    assert r2.parent is r1 and r1.parent is m and m.parent is None
    assert set(np.unique(r2.cell_tags.numpy())) == set(np.unique(m.cell_tags.numpy()))
    for ct, n in ((mesh.CellType.quadrilateral, (2, 2)), (mesh.CellType.hexahedron, (1, 1, 1))):
        q = mesh.create_rectangle((1, 1), n, ct) if len(n) == 2 else mesh.create_box((1, 1, 1), n, ct)
        with pytest.raises(ValueError, match="triangles and tetrahedra"):
            mesh.refine(q)


@pytest.mark.parametrize("name", list(MESHES))
def test_refined_mesh_is_conforming(name):
    from femasm import mesh

    m = MESHES[name]()
    r = mesh.refine(m)
    _, cf = mesh.entities(r, r.tdim - 1)
    cnt = np.bincount(cf.reshape(-1).numpy())
    assert cnt.min() >= 1 and cnt.max() <= 2
    assert int(mesh.exterior_facets(r).numel()) == 2 ** (m.tdim - 1) * int(mesh.exterior_facets(m).numel())
    # no hanging node: every vertex is used, and no vertex lies in the interior of a refined edge
    assert np.array_equal(np.unique(r.cells.numpy()), np.arange(r.num_vertices))


@pytest.mark.parametrize("name", list(MESHES))
@pytest.mark.parametrize("g", [1, 2])
def test_p1_on_refined_is_p2_on_parent(name, g):
    from femasm import fem, mesh

    m = MESHES[name]()
    r = mesh.refine(m)
    V2 = fem.functionspace(m, ("Lagrange", 2, (g,)))
    V1 = fem.functionspace(r, ("Lagrange", 1, (g,)))
    assert V1.num_nodes == V2.num_nodes and V1.num_dofs == V2.num_dofs
    x2, x1 = V2.tabulate_dof_coordinates().numpy(), V1.tabulate_dof_coordinates().numpy()
    scale = np.abs(m.x.numpy()).max()
    assert np.abs(x1 - x2).max() <= np.spacing(scale)
    # each parent's P2 node set is the union of its children's vertices
    nchild = 2 ** m.tdim
    kids = r.cells.numpy().reshape(m.num_cells, nchild * r.cells.shape[1])
    p2 = V2.dofmap.numpy()
    for c in range(m.num_cells):
        assert set(kids[c]) == set(p2[c]), c


def test_refined_rectangle_is_the_doubled_rectangle():
    from femasm import mesh

    r = mesh.refine(mesh.create_rectangle((1, 1), (3, 2)))
    d = mesh.create_rectangle((1, 1), (6, 4))
    assert r.structured is None and r.num_cells == d.num_cells and r.num_vertices == d.num_vertices

    def cell_set(m):
        x = np.round(m.x.numpy()[m.cells.numpy().astype(np.int64)] * 12).astype(np.int64)  # lattice units
        return sorted(tuple(sorted(map(tuple, tri))) for tri in x)

    assert cell_set(r) == cell_set(d)


def _inner_diagonal(r):
    """The edge of refine(one tetrahedron) that joins two midpoints of opposite parent edges."""
    from femasm import mesh

    m = r.parent
    ev = mesh.entities(m, 1)[0].numpy()
    mid = {tuple(e): 4 + k for k, e in enumerate(map(tuple, ev))}
    pairs = {((0, 1), (2, 3)): 0, ((0, 2), (1, 3)): 1, ((0, 3), (1, 2)): 2}
    redges = {tuple(e) for e in mesh.entities(r, 1)[0].numpy()}
    found = [g for (a, b), g in pairs.items() if tuple(sorted((mid[a], mid[b]))) in redges]
    assert len(found) == 1
    return found[0]


def test_shortest_diagonal_rule():
    from femasm import mesh

    base = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    # reference tetrahedron: m01-m23 has length^2 3/4 (d = (1/2, -1/2, -1/2)), as have the other two: a tie
    # in exact binary arithmetic, which goes to the first diagonal
    cases = [(base, 0)]
    diagonals = (((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2)))
    # the two edges of one diagonal moved apart (stretched: the other two diagonals keep their midpoints
    # and still tie, the first of them wins) or together (shrunk: it is the shortest); the factors keep
    # every coordinate a multiple of 1/16, so the arithmetic is exact
    for g, ((a, b), (p, q)) in enumerate(diagonals):
        d = 0.5 * (base[a] + base[b]) - 0.5 * (base[p] + base[q])
        for f, expect in ((0.75, 1 if g == 0 else 0), (-0.25, g)):
            x = base.copy()
            x[[a, b]] += f * d
            x[[p, q]] -= f * d
            cases.append((x, expect))
    # random tetrahedra, the three lengths computed independently below
    rng = np.random.default_rng(4)
    for _ in range(12):
        cases.append((base + 0.3 * rng.standard_normal((4, 3)), None))
    seen = set()
    for x, expect in cases:
        m = mesh.Mesh(mesh.CellType.tetrahedron, torch.tensor(x), torch.tensor([[0, 1, 2, 3]], dtype=torch.int32))
        r = mesh.refine(m)
        l2 = [float(np.sum((0.5 * (x[a] + x[b]) - 0.5 * (x[p] + x[q])) ** 2))
              for (a, b), (p, q) in (((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2)))]
        g = _inner_diagonal(r)
        if expect is not None:
            assert g == expect
        else:
            assert l2[g] == min(l2) and sorted(l2)[1] > min(l2) * (1 + 1e-9), l2  # no near-tie among these
        seen.add(g)
        v = _signed_measures(r)
        assert np.abs(v - _signed_measures(m)[0] / 8).max() <= 1e-14
    assert seen == {0, 1, 2}  # every diagonal has been the shortest one, every child table exercised


def _space(m, p, bs=None):
    from femasm import fem

    return fem.functionspace(m, ("Lagrange", p, (bs or m.gdim,)))


def test_refined_level_table_and_errors():
    from femasm import fem, mesh, mg

    m0 = _square()
    m1 = mesh.refine(m0)
    m2 = mesh.refine(m1)
    V = _space(m2, 2)
    full = mg.plan_refined_hierarchy(V, coarse_dofs=0)
    assert [p for p, _ in full] == [2, 1, 1, 1]
    assert [k for _, k in full] == [m2, m2, m1, m0] and full[3][1] is m0
    assert mg.plan_refined_hierarchy(V, coarse_dofs=0, max_levels=2) == full[:2]
    assert mg.plan_refined_hierarchy(V, coarse_dofs=10 ** 9) == full[:1]
    assert mg.plan_refined_hierarchy(V, coarse_dofs=m1.num_vertices * 2) == full[:3]  # stops where a level fits
    assert mg.plan_refined_hierarchy(V) == full[:2]  # default coarse_dofs: P1 on m2 has 1714 dofs
    assert [p for p, _ in mg.plan_refined_hierarchy(_space(m1, 1), coarse_dofs=0)] == [1, 1]
    # a degree-1 space on a mesh nobody refined: nothing to coarsen to
    with pytest.raises(ValueError, match="structured") as ei:
        mg.plan_refined_hierarchy(_space(m0, 1), coarse_dofs=0)
    assert "mesh.refine" in str(ei.value)
    assert mg.plan_refined_hierarchy(_space(m0, 1)) == [(1, m0)]  # small enough to factor
    assert [p for p, _ in mg.plan_refined_hierarchy(_space(m0, 2), coarse_dofs=0)] == [2, 1]
    with pytest.raises(ValueError, match="plan_hierarchy"):
        mg.plan_refined_hierarchy(_space(mesh.create_rectangle((1, 1), (4, 4)), 2))
    q = mesh.create_rectangle((1, 1), (4, 4), mesh.CellType.quadrilateral)
    with pytest.raises(ValueError, match="triangles or tetrahedra"):
        mg.plan_refined_hierarchy(_space(mesh.Mesh(q.cell_type, q.x, q.cells, None, None), 2))
    with pytest.raises(ValueError, match="degree"):
        mg.plan_refined_hierarchy(fem.functionspace(m1, ("DG", 0, (2,))))
    with pytest.raises(ValueError, match="max_levels"):
        mg.plan_refined_hierarchy(V, max_levels=0)
    # the constructor raises the same error before it touches the device, and plan_hierarchy is unchanged
    with pytest.raises(ValueError, match="mesh.refine"):
        mg.GeometricMultigrid(fem.LinearElasticity(_space(m0, 1), E=1.0), coarse_dofs=0)
    with pytest.raises(ValueError, match="structured"):
        mg.plan_hierarchy(V)


@pytest.mark.parametrize("name", list(MESHES))
def test_edge_transfer_matrix(name):
    from femasm import fem, mesh, mg

    m = MESHES[name]()
    ev = mesh.entities(m, 1)[0]
    t = mg.EdgeTransfer(ev, m.num_vertices, 1)
    assert (t.num_coarse_dofs, t.num_fine_dofs) == (m.num_vertices, m.num_vertices + ev.shape[0])
    P = mg.edge_transfer_matrix(t)
    assert P.shape == (t.num_fine_dofs, t.num_coarse_dofs)
    assert np.abs(np.asarray(P.sum(1)).reshape(-1) - 1.0).max() == 0.0
    # a linear function at the coarse nodes goes to itself at the fine nodes, both as the P2 nodes of m
    # and as the vertices of refine(m)
    w = np.array([2.0, -3.0, 0.5])[:m.gdim]
    Xc = m.x.numpy()
    for Xf in (fem.functionspace(m, ("Lagrange", 2, (1,))).tabulate_dof_coordinates().numpy(),
               mesh.refine(m).x.numpy()):
        assert np.abs(P @ (1.0 + Xc @ w) - (1.0 + Xf @ w)).max() <= 1e-14
    # the CSR of the restriction: each node's edges, ascending
    vptr, vedges, evn = t.vptr.numpy(), t.vedges.numpy(), ev.numpy()
    assert vptr[0] == 0 and vptr[-1] == 2 * ev.shape[0]
    for v in range(m.num_vertices):
        mine = vedges[vptr[v]:vptr[v + 1]]
        assert list(mine) == sorted(np.nonzero((evn == v).any(1))[0])
    # blocked dofs: node * bs + comp
    P3 = mg.edge_transfer_matrix(mg.EdgeTransfer(ev, m.num_vertices, 3)).toarray()
    for c in range(3):
        np.testing.assert_array_equal(P3[c::3, c::3], P.toarray())
    assert np.count_nonzero(P3) == 3 * P.nnz
    with pytest.raises(ValueError):
        mg.EdgeTransfer(ev, m.num_vertices - 1, 1)  # an edge names a node past the coarse ones
    with pytest.raises(ValueError):
        mg.EdgeTransfer(ev, m.num_vertices, 4)
