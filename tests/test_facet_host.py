"""CPU checks of the exterior-facet loads: the facet plan and the plain-torch definition of
``fem.assemble_surface_load`` (what a mesh on the CPU runs; the GPU kernel is held to it and to the same
reference in tests/test_gpu_facet_load.py), ``mesh.read_gmsh_tags`` and ``mesh.transfer_facet_tags``.

Bar: max|b - ref| <= 1e-12 max|ref|, the project's vector bar (tests/test_gpu_vector.py RTOL): the values
are O(1) sums of at most a few dozen terms. The reference (tests/facet_reference.py) uses p + 2 Gauss points
per direction. On simplices, quadrilaterals and planar faces the integrands are polynomials that both that
rule and the library's default (degree 2p) integrate exactly. The area element of a warped (bilinear)
hexahedron face is no polynomial, so no rule is exact there: those cases pass quadrature_degree = 2p + 2,
which is the same p + 2 point Gauss rule, and compare the two quadrature sums."""
import os

import numpy as np
import pytest
import torch

import facet_reference as FR
from femasm import fem, mesh
from femasm.io import MeshTags
from femasm.mesh import CellType, Mesh

RTOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MSH = os.path.join(ROOT, "tests", "golden", "square.msh")


def _close(b, ref):
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else b
    err, scale = np.abs(b - ref).max(), np.abs(ref).max()
    print(f"max|b - ref| = {err:.3e}, max|ref| = {scale:.3e}, ratio {err / scale:.3e}")
    assert err <= RTOL * scale


def _space(m, p):
    return fem.functionspace(m, ("Lagrange", p, (m.gdim,)))


def _facets_at(m, axis, value):
    return mesh.locate_entities_boundary(m, m.tdim - 1, lambda x: torch.isclose(x[axis], torch.full_like(x[axis], value)))


# ------------------------------------------------------------------------------------ 1. closed-form weights
def _weights_on_face(m, p, axis, value):
    """x-components of the load of a unit constant traction e_x on the single facet of the plane
    x_axis = value, as {rounded node coordinates on the facet: weight}."""
    V = _space(m, p)
    f = _facets_at(m, axis, value)
    assert f.numel() == 1
    b = fem.assemble_surface_load(fem.SurfaceLoad(V, f, traction=[1.0] + [0.0] * (m.gdim - 1)))
    bv = b.view(-1, m.gdim)
    assert float(bv[:, 1:].abs().max()) == 0.0
    xn = V.tabulate_dof_coordinates()
    on = torch.isclose(xn[:, axis], torch.full_like(xn[:, axis], value))
    assert float(bv[~on].abs().max()) == 0.0
    return {tuple(np.round(xn[i].numpy(), 9)): float(bv[i, 0]) for i in torch.nonzero(on).reshape(-1)}


def _check_weights(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        assert abs(got[k] - v) <= RTOL * max(abs(w) for w in want.values()), (k, got[k], v)


def test_weights_p1_p2_edge():
    L = 0.7  # the edge x = 1.5 of one rectangle cut into two triangles
    for p, want in ((1, {(1.5, 0.0): L / 2, (1.5, L): L / 2}),
                    (2, {(1.5, 0.0): L / 6, (1.5, L): L / 6, (1.5, L / 2): 4 * L / 6})):
        m = mesh.create_rectangle((1.5, L), (1, 1), CellType.triangle)
        _check_weights(_weights_on_face(m, p, 0, 1.5), want)


def test_weights_q3_edge_are_gll():
    L = 0.7
    m = mesh.create_rectangle((1.5, L), (1, 1), CellType.quadrilateral)
    r = fem.line_points(3)
    want = {(1.5, round(L * r[i], 9)): w * L for i, w in enumerate((1 / 12, 5 / 12, 5 / 12, 1 / 12))}
    _check_weights(_weights_on_face(m, 3, 0, 1.5), want)


def test_weights_p1_p2_triangle_face():
    m = mesh.create_box((1.0, 0.8, 0.6), (1, 1, 1), CellType.tetrahedron)
    # the plane z = 0.6 holds two triangles: load one of them
    for p in (1, 2):
        V = _space(m, p)
        f = _facets_at(m, 2, 0.6)[:1]
        area = float(FR.facet_measure(m, f.numpy())[0])
        assert abs(area - 0.4) < 1e-14
        b = fem.assemble_surface_load(fem.SurfaceLoad(V, f, traction=[0.0, 0.0, 1.0])).view(-1, 3)
        fv = mesh.entities(m, 2)[0][f.long()][0]
        nodes = fem.locate_dofs_topological(V, 2, f)
        assert float(b[:, :2].abs().max()) == 0.0
        rest = torch.ones(V.num_nodes, dtype=torch.bool)
        rest[nodes] = False
        assert float(b[rest].abs().max()) == 0.0
        xn = V.tabulate_dof_coordinates()
        for n in nodes.tolist():
            vertex = bool((m.x[fv] == xn[n]).all(1).any())  # (a node at one of the facet's vertices)
            want = area / 3 if (p == 1 or not vertex) else 0.0
            assert abs(float(b[n, 2]) - want) <= RTOL * area / 3, (p, n, float(b[n, 2]), want)


def test_weights_q2_face_is_tensor_simpson():
    Ly, Lz = 0.8, 0.6
    m = mesh.create_box((1.0, Ly, Lz), (1, 1, 1), CellType.hexahedron)
    s = (1 / 6, 4 / 6, 1 / 6)
    want = {(1.0, round(Ly * i / 2, 9), round(Lz * j / 2, 9)): s[i] * s[j] * Ly * Lz for i in range(3) for j in range(3)}
    _check_weights(_weights_on_face(m, 2, 0, 1.0), want)


# ------------------------------------------------------------------------------------ 2. one-cell meshes
def _one_cell(ct, flip, seed):
    """One cell with randomly moved vertices; flip: reordered so that det J < 0 everywhere (simplices: two
    vertices swapped; tensor cells: mirrored in the first reference direction, v <-> v ^ 1 -- swapping just
    two vertices of a quadrilateral or hexahedron would fold the cell, not turn it over)."""
    ct = CellType(ct)
    rng = np.random.default_rng(seed)
    x = np.array(mesh.REF_VERTS[ct], dtype=np.float64)
    x = x + 0.15 * (rng.random(x.shape) - 0.5)
    order = list(range(x.shape[0]))
    if flip:
        order = [1, 0] + order[2:] if fem.is_simplex(ct) else [v ^ 1 for v in order]
    # vertex k of the cell is point order[k]: the same body, another orientation
    return Mesh(ct, torch.tensor(x), torch.tensor([order], dtype=torch.int32))


ONE_CELL = [(3, 1), (3, 2), (4, 1), (4, 2), (-4, 1), (-4, 2), (8, 1), (8, 2)]


def _jacobian_sign(m):
    c = m.cells[0].long()
    X = m.x[c]
    if fem.is_simplex(m.cell_type):
        return float(torch.sign(torch.linalg.det((X[1:] - X[0]).T)))
    k = [1, 2] if m.gdim == 2 else [1, 2, 4]
    return float(torch.sign(torch.linalg.det((X[k] - X[0]).T)))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("ct,p", ONE_CELL)
def test_one_cell_all_facets(ct, p, flip):
    m = _one_cell(ct, flip, seed=3 + p)
    assert _jacobian_sign(m) == (-1.0 if flip else 1.0)
    V = _space(m, p)
    f = mesh.exterior_facets(m)
    nf, gd = int(f.numel()), m.gdim
    assert nf == len(mesh.sub_entities(ct, m.tdim - 1))  # every local facet is on the boundary
    qd = None if fem.is_simplex(ct) else 2 * p + 2
    g = torch.Generator().manual_seed(11)
    tc, pc = torch.rand(gd, generator=g, dtype=torch.float64) - 0.5, 0.7
    tf, pf = torch.rand((nf, gd), generator=g, dtype=torch.float64) - 0.5, torch.rand(nf, generator=g, dtype=torch.float64)
    tn = torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5
    pn = torch.rand(V.num_nodes + 1, generator=g, dtype=torch.float64)[:V.num_nodes]
    if V.num_nodes == nf:  # a plain tensor of len(facets) entries is per-facet: nodal values come as a Function
        Q = fem.functionspace(m, ("Lagrange", p))
        pn_arg = fem.Function(Q, x=pn)
    else:
        pn_arg = pn
    for kw, ref_kw in ((dict(traction=tc, pressure=pc), dict(t_const=tc.numpy(), p_const=pc)),
                       (dict(traction=tf, pressure=pf), dict(t_facet=tf.numpy(), p_facet=pf.numpy())),
                       (dict(traction=tn, pressure=pn_arg), dict(t_nodal=tn.numpy(), p_nodal=pn.numpy()))):
        ld = fem.SurfaceLoad(V, f, quadrature_degree=qd, **kw)
        _close(fem.assemble_surface_load(ld), FR.reference_load(V, f.numpy(), **ref_kw))
    # closed surface: the resultant of a constant pressure vanishes (the closed integral of n dS is 0)
    b = fem.assemble_surface_load(fem.SurfaceLoad(V, f, pressure=pc, quadrature_degree=qd)).view(-1, gd)
    area = float(np.abs(FR.reference_load(V, f.numpy(), t_const=np.eye(gd)[0]).reshape(-1, gd)[:, 0]).sum())
    assert float(b.sum(0).abs().max()) <= 1e-12 * pc * area


def test_alpha_and_accumulation():
    m = _one_cell(3, False, seed=1)
    V = _space(m, 2)
    ld = fem.SurfaceLoad(V, mesh.exterior_facets(m), traction=[0.3, -0.2], pressure=1.5)
    b1 = fem.assemble_surface_load(ld)
    b0 = torch.ones(V.num_dofs, dtype=torch.float64)
    out = fem.assemble_surface_load(ld, b0, alpha=-2.0)
    assert out is b0
    assert torch.allclose(b0, 1.0 - 2.0 * b1, rtol=0, atol=1e-15)


def test_values_are_read_live():
    m = _one_cell(4, False, seed=2)
    V = _space(m, 1)
    t = torch.tensor([1.0, 0.0], dtype=torch.float64)
    ld = fem.SurfaceLoad(V, mesh.exterior_facets(m), traction=t)
    b1 = fem.assemble_surface_load(ld).clone()
    t.mul_(3.0)
    assert torch.allclose(fem.assemble_surface_load(ld), 3.0 * b1, rtol=0, atol=1e-15)


def test_argument_errors():
    m = mesh.create_unit_square(2, 2)
    V = _space(m, 1)
    ext = mesh.exterior_facets(m)
    interior = [i for i in range(mesh.entities(m, 1)[0].shape[0]) if i not in ext.tolist()]
    with pytest.raises(ValueError, match="not exterior"):
        fem.SurfaceLoad(V, [int(ext[0]), interior[0]], pressure=1.0)
    with pytest.raises(ValueError, match="twice"):
        fem.SurfaceLoad(V, [int(ext[0]), int(ext[1]), int(ext[0])], pressure=1.0)
    with pytest.raises(ValueError):
        fem.SurfaceLoad(V, ext, traction=[1.0, 0.0, 0.0])  # a 3-vector on a 2-D mesh
    with pytest.raises(ValueError):
        fem.SurfaceLoad(V, ext, pressure=torch.ones(int(ext.numel()) + 2, dtype=torch.float64))  # 8 facets, 9 nodes
    with pytest.raises(ValueError):
        fem.SurfaceLoad(V, ext, traction=torch.ones((int(ext.numel()), 3), dtype=torch.float64))
    with pytest.raises(ValueError):
        fem.SurfaceLoad(V, ext)  # nothing to apply
    with pytest.raises(ValueError, match="bs = gdim"):
        fem.SurfaceLoad(fem.functionspace(m, ("Lagrange", 1)), ext, pressure=1.0)
    with pytest.raises(ValueError, match="outside"):
        fem.SurfaceLoad(V, [10 ** 6], pressure=1.0)
    W = _space(mesh.create_unit_square(2, 2), 1)
    with pytest.raises(ValueError, match="another function space"):
        fem.LinearElasticity(W, E=1.0, loads=[fem.SurfaceLoad(V, ext, pressure=1.0)])


# ------------------------------------------------------------------------------------ 3. the Gmsh file's line groups
EXPECTED_COUNTS = {1: 2, 2: 6, 3: 6, 4: 7, 5: 4, 6: 6}


def test_read_gmsh_tags_of_square():
    m = mesh.read_gmsh(MSH)
    tags = mesh.read_gmsh_tags(MSH, m, 1)
    assert isinstance(tags, MeshTags) and tags.dim == 1
    assert int(tags.indices.numel()) == 31
    assert bool((tags.indices[1:] > tags.indices[:-1]).all())
    assert {v: int((tags.values == v).sum()) for v in EXPECTED_COUNTS} == EXPECTED_COUNTS
    ext = set(mesh.exterior_facets(m).tolist())
    for v in (1, 2, 3, 5, 6):
        assert set(tags.find(v).tolist()) <= ext, v
    assert not set(tags.find(4).tolist()) & ext  # the 7 edges of group 4 are all interior
    V = _space(m, 1)
    with pytest.raises(ValueError, match="not exterior"):
        fem.SurfaceLoad(V, tags.find(4), pressure=1.0)
    # group 2 is the side x = 1 (length 1): a unit pressure pushes with (-1, 0)
    ev = mesh.entities(m, 1)[0][tags.find(2).long()]
    assert bool((m.x[ev.reshape(-1), 0] == 1.0).all())
    for p in (1, 2):
        Vp = _space(m, p)
        b = fem.assemble_surface_load(fem.SurfaceLoad(Vp, tags.find(2), pressure=1.0)).view(-1, 2)
        assert float((b.sum(0) - torch.tensor([-1.0, 0.0], dtype=torch.float64)).abs().max()) <= 1e-12


def test_read_gmsh_tags_rejects_another_mesh():
    with pytest.raises(ValueError):
        mesh.read_gmsh_tags(MSH, mesh.create_unit_square(3, 3), 1)
    with pytest.raises(ValueError):
        mesh.read_gmsh_tags(MSH, mesh.read_gmsh(MSH), 2)


# ------------------------------------------------------------------------------------ 4. tags through refine
EXPECTED_LENGTH = {1: 0.341949388655, 2: 1.0, 3: 1.0, 5: 0.658050611345, 6: 1.0}


def test_transfer_facet_tags_2d():
    m = mesh.read_gmsh(MSH)
    tags = mesh.read_gmsh_tags(MSH, m, 1)
    fine = mesh.refine(m)
    ft = mesh.transfer_facet_tags(tags, fine)
    assert ft.dim == 1 and bool((ft.indices[1:] > ft.indices[:-1]).all())
    cev, fev = mesh.entities(m, 1)[0], mesh.entities(fine, 1)[0]
    for v, n in EXPECTED_COUNTS.items():
        kids = ft.find(v)
        assert int(kids.numel()) == 2 * n
        seg = fine.x[fev[kids.long()]]  # [2n, 2, 2]
        if v in EXPECTED_LENGTH:
            assert abs(float((seg[:, 1] - seg[:, 0]).norm(dim=1).sum()) - EXPECTED_LENGTH[v]) <= 1e-12
        # every child's vertices lie on a parent edge of the same tag
        par = m.x[cev[tags.find(v).long()]]  # [n, 2, 2]
        a, d = par[:, 0], par[:, 1] - par[:, 0]
        for pt in seg.reshape(-1, 2):
            r = pt - a
            s = (r * d).sum(1) / (d * d).sum(1)
            off = (r - s[:, None] * d).norm(dim=1)
            assert bool(((off <= 1e-14) & (s >= -1e-14) & (s <= 1 + 1e-14)).any())
    assert set(ft.find(2).tolist()) <= set(mesh.exterior_facets(fine).tolist())


def test_transfer_facet_tags_3d():
    m = mesh.create_unit_cube(1, 1, 1)
    ext = mesh.exterior_facets(m)
    fv = mesh.entities(m, 2)[0][ext]
    side = torch.where((m.x[fv][:, :, 0] == 1.0).all(1), 7, 3).to(torch.int32)  # the face x = 1 and the rest
    tags = MeshTags(2, ext.to(torch.int32), side)
    fine = mesh.refine(m)
    ft = mesh.transfer_facet_tags(tags, fine)
    assert int(ft.indices.numel()) == 4 * int(ext.numel())
    assert set(ft.indices.tolist()) == set(mesh.exterior_facets(fine).tolist())
    for v in (3, 7):
        assert int(ft.find(v).numel()) == 4 * int(tags.find(v).numel())
        assert abs(FR.facet_measure(fine, ft.find(v).numpy()).sum() - FR.facet_measure(m, tags.find(v).numpy()).sum()) <= 1e-12
    kids = mesh.entities(fine, 2)[0][ft.find(7).long()]
    assert bool((fine.x[kids.reshape(-1), 0] == 1.0).all())
    with pytest.raises(ValueError):
        mesh.transfer_facet_tags(tags, m)  # not a refined mesh


# ------------------------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("ct,p,n", [(3, 2, (4, 3)), (-4, 1, (2, 3, 2)), (8, 2, (2, 1, 2))])
def test_bit_identical_under_permutation(ct, p, n):
    m = mesh.create_unit_square(*n, cell_type=ct) if len(n) == 2 else mesh.create_unit_cube(*n, cell_type=ct)
    V = _space(m, p)
    f = mesh.exterior_facets(m)
    g = torch.Generator().manual_seed(5)
    nf = int(f.numel())
    tf = torch.rand((nf, m.gdim), generator=g, dtype=torch.float64) - 0.5
    pf = torch.rand(nf, generator=g, dtype=torch.float64)
    b0 = fem.assemble_surface_load(fem.SurfaceLoad(V, f, traction=tf, pressure=pf))
    perm = torch.randperm(nf, generator=g)
    ld = fem.SurfaceLoad(V, f[perm], traction=tf[perm], pressure=pf[perm])
    assert torch.equal(fem.assemble_surface_load(ld), b0)
    assert torch.equal(fem.assemble_surface_load(ld), b0)
    # the plan: ascending nodes, each node's entries in ascending slot order
    assert bool((ld.nodes[1:] > ld.nodes[:-1]).all())
    slot = ld.entries.long() // ld.nk
    same = torch.ones(slot.numel() - 1, dtype=torch.bool)
    same[ld.node_ptr[1:-1] - 1] = False
    assert bool((slot[1:] > slot[:-1])[same].all())
    _close(b0, FR.reference_load(V, f.numpy(), t_facet=tf.numpy(), p_facet=pf.numpy()))
