"""CPU checks of point location and evaluation at points (femasm.geometry, fem.eval_points,
Function.interpolate across meshes): the host path, which runs the kernels' definition in torch with the same
grid and the same acceptance rule. tests/test_gpu_points.py holds the kernels to the same checks.

Bars. Round trip: |x(X) - x|_inf <= 1e-12 (|x|_inf + max vertex |x_v|_inf of the cell), the project's 1e-12 on
the magnitude of the quantities subtracted. Values: 1e-12 * sum_a |phi_a| |w_a|; gradients: 1e-12 *
sum_a |w_a| sum_k |d_k phi_a| |Jinv_kj| (every product of the sum taken in absolute value). The affine field
u = A x + b: 1e-12 (|A| |x| + |b|) as the issue states it, its gradient against A on the magnitude bar above."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import irregular_meshes as IM  # noqa: E402
import points_cases as PC  # noqa: E402
import transformed_meshes as TM  # noqa: E402

FAMILIES = list(TM.FAMILIES)
DEV = None  # the host path


def _irregular():
    return {"fan": IM.fan(300), "delaunay": IM.delaunay_tets_n4(), "square_msh": IM.square_msh()}


# ------------------------------------------------------------------------------------------- 1, 2, 3
@pytest.mark.parametrize("family", FAMILIES)
def test_interior_points(family):
    for tr in TM.PARITY + TM.SHIFTS:
        PC.check_interior(PC.family_mesh(family, tr), DEV)


@pytest.mark.parametrize("family", FAMILIES)
def test_points_on_shared_entities(family):
    for tr in TM.PARITY:
        PC.check_entities(PC.family_mesh(family, tr), DEV)


@pytest.mark.parametrize("name", ["fan", "delaunay", "square_msh"])
def test_irregular_meshes(name):
    m = _irregular()[name]
    PC.check_interior(m, DEV)
    PC.check_entities(m, DEV)


@pytest.mark.parametrize("family", FAMILIES)
def test_outside_points(family):
    for tr in TM.PARITY:
        m = PC.family_mesh(family, tr)
        PC.check_rejected(m, PC.outside_queries(family, tr), DEV)
        x = m.x.numpy()
        size = np.abs(x.max(0) - x.min(0)).max()
        far = x.mean(0) + 1e6 * size * np.array([[1.0, -1.0, 1.0][:m.gdim], [-1.0, 0.0, 0.0][:m.gdim]])
        PC.check_rejected(m, far, DEV)
        bad = np.repeat(x.mean(0)[None], m.gdim + 1, 0)
        for d in range(m.gdim):
            bad[d, d] = np.nan
        bad[m.gdim, 0] = np.inf
        PC.check_rejected(m, bad, DEV)


def test_hole():
    m, pts = PC.hole_mesh()
    PC.check_rejected(m, pts, DEV)
    PC.check_interior(m, DEV)


def test_degenerate_queries():
    from femasm import geometry, mesh

    m = PC.family_mesh("tet-P1", "rot")
    c, X = geometry.locate_points(m, torch.zeros((0, 3), dtype=torch.float64))
    assert c.shape == (0,) and c.dtype == torch.int32 and X.shape == (0, 3)
    for ct, x in ((mesh.CellType.triangle, [[0.0, 0.0], [2.0, 0.5], [0.5, 1.5]]),
                  (mesh.CellType.hexahedron, mesh.create_unit_cube(1, 1, 1, mesh.CellType.hexahedron).x.tolist())):
        one = mesh.Mesh(ct, torch.tensor(x, dtype=torch.float64), torch.arange(len(x), dtype=torch.int32)[None])
        tree = geometry.bb_tree(one)
        assert tree.dims == (1, 1, 1) and tree.num_pairs == 1
        PC.check_interior(one, DEV, per_cell=70)
        PC.check_entities(one, DEV)
    # points exactly on the upper faces of the grid's box (the bin-index clamp) and on the mesh's upper faces
    m = PC.family_mesh("quad-Q1", None)
    tree = geometry.bb_tree(m)
    hi = np.array([tree.lo[d] + tree.dims[d] / tree.inv_h[d] for d in range(2)])
    PC.check_rejected(m, np.array([[hi[0], 0.5], [0.5, hi[1]], hi]), DEV)  # in the padding: listed, held by no cell
    c, _ = PC.locate(m, np.array([[1.0, 0.5], [0.5, 1.0], [1.0, 1.0]]), DEV)
    assert np.array_equal(c, PC.brute_force(m, np.array([[1.0, 0.5], [0.5, 1.0], [1.0, 1.0]]))) and (c >= 0).all()


# ------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("family", ["tri-P1", "tet-P2", "quad-Q2-warp", "hex-Q1-warp", "hex-Q3"])
def test_grid_independence_and_brute_force(family):
    from femasm import geometry

    for tr in ("rotmirror", "stretch"):
        m = PC.family_mesh(family, tr)
        x = np.concatenate([PC.interior_queries(m, 2)[0], PC.entity_queries(m)[0], PC.outside_queries(family, tr)])
        t0 = geometry.bb_tree(m)
        gd = m.gdim
        c0, X0 = PC.locate(m, x, DEV)
        c1, _ = PC.locate(m, x, DEV, tree=geometry.bb_tree(m, dims=(1,) * gd))
        c4, _ = PC.locate(m, x, DEV, tree=geometry.bb_tree(m, dims=tuple(4 * d for d in t0.dims[:gd])))
        assert np.array_equal(c0, c1) and np.array_equal(c0, c4)
        assert np.array_equal(c0, PC.brute_force(m, x))


def test_tree_sizing_and_cache():
    from femasm import geometry

    m = PC.family_mesh("tet-P1", None)
    t = geometry.bb_tree(m)
    assert t is geometry.bb_tree(m)
    assert 0.25 * m.num_cells <= t.num_bins <= 4 * m.num_cells and t.num_pairs <= geometry.PAIR_CAP * m.num_cells
    per = (t.bin_ptr[1:] - t.bin_ptr[:-1]).numpy()
    bc = t.bin_cells.numpy()
    for b in np.nonzero(per > 1)[0]:
        seg = bc[t.bin_ptr[b]:t.bin_ptr[b + 1]]
        assert (np.diff(seg) > 0).all()  # ascending cell ids per bin
    m.x[0, 0] += 0.0  # an in-place write bumps the coordinates' version
    assert geometry.bb_tree(m) is not t
    # aspect 256 (stretch of a box mesh): the pair cap halves the bin counts
    from femasm import mesh

    s = TM.apply(mesh.create_unit_cube(4, 4, 4), "stretch")
    ts = geometry.bb_tree(s)
    assert ts.num_pairs <= geometry.PAIR_CAP * s.num_cells and ts.num_bins < s.num_cells / 2
    with pytest.raises(ValueError):
        geometry.locate_points(m, torch.zeros((1, 3), dtype=torch.float64), tol=1e-3)


# ------------------------------------------------------------------------------------------- 5, 6
@pytest.mark.parametrize("family", FAMILIES)
def test_affine_field_end_to_end(family):
    for tr in ("rot", "mirror", "shear", "stretch", "shift1e4"):
        PC.check_affine_field(family, tr, DEV)
    if TM.is_affine(family) and TM.FAMILIES[family][1] >= 2:
        PC.check_affine_field(family, "rotmirror", DEV, quadratic=True)


def test_eval_points_arguments():
    from femasm import fem

    m = PC.family_mesh("tri-P2", None)
    V = PC.space_of(m, "tri-P2", 2)
    u = fem.Function(V)
    u.x = torch.arange(V.num_dofs, dtype=torch.float64)
    x = torch.tensor([[0.3, 0.2], [5.0, 5.0]])
    v = fem.eval_points(u, x)
    assert v.shape == (2, 2) and torch.isfinite(v[0]).all() and torch.isnan(v[1]).all()
    v2, g2 = u.eval(x, grad=True), fem.eval_points(u.x, x, V=V, grad=True)[1]
    assert torch.equal(v2[0][0], v[0]) and g2.shape == (2, 2, 2) and torch.isnan(g2[1]).all()
    from femasm import geometry

    c, X = geometry.locate_points(m, x)
    assert torch.equal(fem.eval_points(u, cells=c, X=X)[0], v[0])
    assert torch.allclose(fem.eval_points(u, x, cells=c)[0], v[0], rtol=1e-13)  # cells alone: pulled back
    with pytest.raises(ValueError):
        fem.eval_points(u.x, x)
    W = fem.functionspace(m, ("Lagrange", 1, (4,)))
    with pytest.raises(ValueError):
        fem.eval_points(fem.Function(W), x)


# ------------------------------------------------------------------------------------------- 7
def test_across_meshes():
    PC.check_across_meshes(DEV)


def test_missing_and_dg0():
    PC.check_missing_and_dg0(DEV)


# ------------------------------------------------------------------------------------------- 8, 9
def test_determinism_host():
    m = PC.family_mesh("hex-Q2-warp", "rot")
    x = np.concatenate([PC.interior_queries(m, 3)[0], PC.entity_queries(m)[0]])
    c0, X0 = PC.locate(m, x, DEV)
    c1, X1 = PC.locate(m, x, DEV)
    assert np.array_equal(c0, c1) and np.array_equal(X0, X1)
    perm = np.random.default_rng(0).permutation(x.shape[0])
    cp, Xp = PC.locate(m, x[perm], DEV)
    assert np.array_equal(cp, c0[perm]) and np.array_equal(Xp, X0[perm], equal_nan=True)


def test_abi_symbols_and_argument_checks():
    from femasm import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfemasm.so not built (run __graft_entry__.build())")
    L = _lib.load()
    assert L.fa_version() >= 108
    for name in ("fa_locate_points", "fa_eval_points"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.fa_cell_grid) == 80
    # argument checks return before any device call
    fm = _lib.fa_mesh()
    fm.cell_type, fm.degree, fm.gdim, fm.nn, fm.nv, fm.ncells, fm.nnodes = 3, 1, 2, 3, 3, 1, 3
    g = _lib.fa_cell_grid()
    assert L.fa_locate_points(ctypes.byref(fm), ctypes.byref(g), 1, None, 1e-10, None, None, None) == _lib.FA_E_ARG
    assert L.fa_eval_points(ctypes.byref(fm), None, 1, 1, None, None, None, None, None) == _lib.FA_E_ARG
    buf = (ctypes.c_double * 8)()
    fm.cells = fm.geom = fm.x = ctypes.addressof(buf)  # (never dereferenced: the calls below are refused first)
    assert L.fa_locate_points(ctypes.byref(fm), None, 1, None, 1e-10, None, None, None) == _lib.FA_E_ARG
    assert L.fa_locate_points(ctypes.byref(fm), ctypes.byref(g), 1, None, 1e-10, None, None, None) == _lib.FA_E_ARG
    p = ctypes.addressof(buf)
    assert L.fa_eval_points(ctypes.byref(fm), p, 4, 1, p, p, p, None, None) == _lib.FA_E_ARG
    assert L.fa_eval_points(ctypes.byref(fm), p, 0, 1, p, p, p, None, None) == _lib.FA_E_ARG
    assert L.fa_eval_points(ctypes.byref(fm), None, 2, 1, p, p, p, None, None) == _lib.FA_E_ARG
    assert L.fa_eval_points(ctypes.byref(fm), p, 2, 1, p, p, None, None, None) == _lib.FA_E_ARG
    assert L.fa_eval_points(ctypes.byref(fm), p, 2, 1, None, p, p, None, None) == _lib.FA_E_ARG
    fm.degree, fm.nn = 3, 10  # P3 triangles: no such element
    assert L.fa_eval_points(ctypes.byref(fm), p, 2, 1, p, p, p, None, None) == _lib.FA_E_UNSUPPORTED
    assert L.fa_locate_points(ctypes.byref(fm), ctypes.byref(g), 1, p, 1e-10, p, p, None) == _lib.FA_E_UNSUPPORTED
    assert b"unsupported" in L.fa_last_error()
