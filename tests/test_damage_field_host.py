"""fem.damage_field on the CPU: the vertex graph, the marking and the torch host path of the spread against
the sequential restatement of the definition (damage_reference.py). Every comparison with the reference is
exact equality: the arithmetic (sum from 0.0 in ascending neighbour order, times the stored reciprocal, then
max) is part of the definition, so nothing may differ in the last bit."""
import math

import numpy as np
import pytest
import torch

import damage_cases as C
import damage_reference as R

INF = float("inf")


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def _space(m):
    from femasm import fem

    return fem.functionspace(m, ("Lagrange", 1))


# ------------------------------------------------------------------------------------------------ graph
@pytest.mark.parametrize("name", C.GRAPH_MESHES)
def test_vertex_graph(name):
    from femasm import mesh

    m = C.make(name)
    indptr, indices = mesh.vertex_graph(m)
    nv, ne = m.num_vertices, int(mesh.entities(m, 1)[0].shape[0])
    assert indptr.dtype == torch.int64 and indptr.shape == (nv + 1,)
    assert indices.dtype == torch.int32 and indices.shape == (2 * ne,)
    assert int(indptr[0]) == 0 and int(indptr[-1]) == 2 * ne
    rows = [indices[int(indptr[v]):int(indptr[v + 1])].tolist() for v in range(nv)]
    pairs = set()
    for v, row in enumerate(rows):
        assert row == sorted(set(row)), f"row {v} not ascending or with duplicates"
        assert v not in row, f"self loop at {v}"
        pairs.update((v, w) for w in row)
    assert all((w, v) in pairs for v, w in pairs), "not symmetric"
    assert rows == C.adjacency(name)
    assert mesh.vertex_graph(m)[1] is indices, "not cached on the mesh"


def test_vertex_graph_square_msh():
    from femasm import mesh

    m = C.make("square")
    indptr, indices = mesh.vertex_graph(m)
    deg = indptr[1:] - indptr[:-1]
    assert m.num_vertices == 62
    assert int(deg.min()) == 3 and int(deg.max()) == 7
    assert indices.numel() == 2 * mesh.entities(m, 1)[0].shape[0]


def test_orphan_vertex_keeps_its_value():
    from femasm import fem, mesh

    m = C.make("orphan")
    indptr, _ = mesh.vertex_graph(m)
    assert int(indptr[5] - indptr[4]) == 0
    d0 = _t(C.start("orphan"))
    d = fem.spread(m, d0, 8)
    assert bool(torch.isfinite(d).all())
    assert float(d[4]) == 0.25
    assert np.array_equal(d.numpy(), C.reference("orphan", 8))
    z = fem.spread(m, torch.zeros(5, dtype=torch.float64), 3)
    assert bool((z == 0).all())


# ------------------------------------------------------------------------------------------------ reference case
def test_square_msh_tag4_reference_case():
    from femasm import fem, mesh

    m, t = C.square()
    edges = t.find(C.TAG)
    assert edges.numel() == 7
    d0 = fem.mark_vertices(m, 1, edges)
    assert int((d0 > 0).sum()) == 8
    assert np.array_equal(d0.numpy(), C.start("square"))
    ref = C.reference("square", 8)
    assert (ref > 0).sum() == 62
    assert math.isclose(ref.min(), 0.0554786685439930, rel_tol=1e-12)
    assert ref.max() == 1.0
    assert math.isclose(math.fsum(ref), 33.8126894005934, rel_tol=1e-12)
    d = fem.damage_field(_space(m), tags=t, values=[C.TAG])
    assert isinstance(d, fem.Function) and d.name == "d"
    assert np.array_equal(d.x.numpy(), ref)
    one = C.reference("square", 1)
    assert (one > 0).sum() == 41 and (one < 0.01).sum() == 21
    assert np.array_equal(fem.spread(m, d0, 1).numpy(), one)
    ev = mesh.entities(m, 1)[0][edges.to(torch.int64)]
    by_entities = fem.damage_field(_space(m), entities=edges, dim=1)
    assert torch.equal(by_entities.x, d.x) and ev.shape == (7, 2)


@pytest.mark.parametrize("name", C.MESHES)
@pytest.mark.parametrize("iterations", C.ITERATIONS)
@pytest.mark.parametrize("threshold", C.THRESHOLDS)
def test_host_path_equals_sequential_loop(name, iterations, threshold):
    from femasm import fem

    m = C.make(name)
    d = fem.spread(m, _t(C.start(name)), iterations, threshold)
    assert np.array_equal(d.numpy(), C.reference(name, iterations, threshold))


def test_gate():
    from femasm import fem

    m = C.make("square")
    d0 = _t(C.start("square"))
    gated, every, none = (fem.spread(m, d0, 8, th).numpy() for th in (0.01, INF, 0.0))
    assert np.array_equal(every, C.reference("square", 8, INF))
    assert np.array_equal(none, C.reference("square", 8, 0.0))
    assert not np.array_equal(every, gated)
    # threshold 0: the gated pass changes nothing, an iteration is the full pass alone
    adj = C.adjacency("square")
    r = [1.0 / len(a) for a in adj]
    full_only = R._pass(adj, r, list(C.start("square")), 0.0, False)
    assert np.array_equal(fem.spread(m, d0, 1, 0.0).numpy(), np.array(full_only))


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("d_max", [1.0, 0.75])
def test_properties(d_max):
    from femasm import fem

    m, t = C.square()
    S = _space(m)
    edges = t.find(C.TAG)
    marks = fem.mark_vertices(m, 1, edges, d_max)
    prev = None
    for it in (0, 1, 2, 8, 16):
        d = fem.damage_field(S, entities=edges, dim=1, d_max=d_max, iterations=it).x
        assert bool((d >= 0).all()) and bool((d <= d_max).all())
        assert bool((d[marks > 0] == d_max).all())
        if it == 0:
            assert torch.equal(d, marks)
        else:
            assert bool((d >= prev).all())
        prev = d
    shuffled = torch.cat([edges.flip(0), edges, edges[:3]])
    assert torch.equal(fem.damage_field(S, entities=shuffled, dim=1, d_max=d_max).x,
                       fem.damage_field(S, entities=edges, dim=1, d_max=d_max).x)
    assert torch.equal(fem.mark_vertices(m, 1, shuffled.tolist(), d_max), marks)
    keep = marks.clone()
    fem.spread(m, marks, 8)
    assert torch.equal(marks, keep), "d0 was modified"


def test_mark_vertices_dimensions_and_out():
    from femasm import fem, mesh

    m = C.make("square")
    nv = m.num_vertices
    v = fem.mark_vertices(m, 0, [3, 5, 3])
    assert v.dtype == torch.float64 and v.shape == (nv,)
    assert sorted(torch.nonzero(v).reshape(-1).tolist()) == [3, 5]
    c = fem.mark_vertices(m, 2, torch.tensor([7]), 0.5)
    assert sorted(torch.nonzero(c).reshape(-1).tolist()) == sorted(m.cells[7].tolist())
    assert bool((c[c > 0] == 0.5).all())
    b = mesh.locate_entities_boundary(m, 1, lambda x: torch.isclose(x[0], torch.zeros_like(x[0])))
    on_left = fem.mark_vertices(m, 1, b)
    assert bool((m.x[on_left > 0, 0].abs() < 1e-12).all()) and int((on_left > 0).sum()) == b.numel() + 1
    out = torch.full((nv,), 0.125, dtype=torch.float64)
    got = fem.mark_vertices(m, 0, [0], 2.0, out=out)
    assert got is out and float(out[0]) == 2.0 and bool((out[1:] == 0.125).all())
    t = C.make("tets")
    f = fem.mark_vertices(t, 2, [0])
    assert sorted(torch.nonzero(f).reshape(-1).tolist()) == mesh.entities(t, 2)[0][0].tolist()


# ------------------------------------------------------------------------------------------------ defaults
def test_default_iterations_follow_the_parent_chain():
    from femasm import fem, mesh

    m, t = C.square()
    S = _space(m)
    assert torch.equal(fem.damage_field(S, tags=t, values=[C.TAG]).x,
                       fem.damage_field(S, tags=t, values=[C.TAG], iterations=8).x)
    m1, t1 = C.square(refine=1)
    assert m1.num_vertices == 221 and m1.parent is not None
    d1 = fem.damage_field(_space(m1), tags=t1, values=[C.TAG]).x
    assert np.array_equal(d1.numpy(), C.reference("square_r1", 16))
    assert not np.array_equal(d1.numpy(), C.reference("square_r1", 8))
    # a mesh whose parents were dropped counts no refinement
    flat = mesh.Mesh(m1.cell_type, m1.x, m1.cells, m1.cell_tags, None)
    d8 = fem.damage_field(_space(flat), tags=t1, values=[C.TAG]).x
    assert np.array_equal(d8.numpy(), C.reference("square_r1", 8))


# ------------------------------------------------------------------------------------------------ errors
def test_value_errors():
    from femasm import fem, mesh

    m, t = C.square()
    S = _space(m)
    edges = t.find(C.TAG)
    ne = int(mesh.entities(m, 1)[0].shape[0])
    for bad in ([ne], [-1], [0, ne + 5]):
        with pytest.raises(ValueError):
            fem.mark_vertices(m, 1, bad)
    with pytest.raises(ValueError):
        fem.mark_vertices(m, 0, [m.num_vertices])
    with pytest.raises(ValueError):
        fem.mark_vertices(m, 2, [m.num_cells])
    with pytest.raises(ValueError):
        fem.mark_vertices(m, 3, [0])
    with pytest.raises(ValueError):
        fem.damage_field(fem.functionspace(m, ("Lagrange", 1, (2,))), entities=edges)  # vector space
    with pytest.raises(ValueError):
        fem.damage_field(fem.functionspace(m, ("Lagrange", 2)), entities=edges)  # degree 2
    with pytest.raises(ValueError):
        fem.damage_field(fem.functionspace(m, ("DG", 0)), entities=edges)  # DG
    own = fem.FunctionSpace.from_dofmap(m, 1, 1, m.cells.clone(), m.num_vertices)
    with pytest.raises(ValueError):
        fem.damage_field(own, entities=edges)  # a dofmap that is not the mesh's cells
    for d_max in (0.0, -1.0):
        with pytest.raises(ValueError):
            fem.damage_field(S, entities=edges, d_max=d_max)
    with pytest.raises(ValueError):
        fem.damage_field(S, entities=edges, iterations=-1)
    with pytest.raises(ValueError):
        fem.damage_field(S, entities=edges, tags=t, values=[C.TAG])  # both
    with pytest.raises(ValueError):
        fem.damage_field(S)  # neither
    with pytest.raises(ValueError):
        fem.damage_field(S, tags=t)  # tags without values
    d0 = fem.mark_vertices(m, 1, edges)
    with pytest.raises(ValueError):
        fem.spread(m, d0, -1)
    for bad in (-0.5, float("nan"), INF):
        x = d0.clone()
        x[5] = bad
        with pytest.raises(ValueError):
            fem.spread(m, x, 1)
    with pytest.raises(ValueError):
        fem.spread(m, d0[:-1], 1)
    with pytest.raises(ValueError):
        fem.spread(m, d0.to(torch.float32), 1)
