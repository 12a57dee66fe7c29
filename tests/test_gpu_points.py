"""GPU checks of k_locate_points and k_eval_points (fa_locate_points / fa_eval_points through
femasm.geometry.locate_points and fem.eval_points): the checks of tests/test_points_host.py run on the device,
the device against the host path, and fa_eval_points against the host basis at the device's own (cell, X).

Bars (tests/test_points_host.py states them): round trip 1e-12 (|x|_inf + max |x_v|_inf); values
1e-12 sum_a |phi_a| |w_a|; gradients 1e-12 sum_a |w_a| sum_k |d_k phi_a| |Jinv_kj|."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import irregular_meshes as IM  # noqa: E402
import points_cases as PC  # noqa: E402
import transformed_meshes as TM  # noqa: E402

pytestmark = pytest.mark.gpu
FAMILIES = list(TM.FAMILIES)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _irregular(name):
    return {"fan": lambda: IM.fan(300), "delaunay": IM.delaunay_tets_n4, "square_msh": IM.square_msh}[name]()


def _same_as_host(m, x, dev):
    """Test 8, GPU against the CPU path: equal cells, X within the round-trip bar."""
    c, X = PC.locate(m, x, dev)
    ch, Xh = PC.locate(m, x, None)
    assert np.array_equal(c, ch)
    hit = c >= 0
    assert np.isnan(X[~hit]).all() and np.isnan(Xh[~hit]).all()
    cells = c[hit].astype(np.int64)
    d = np.abs(PC.map_points(m, cells, X[hit]) - PC.map_points(m, cells, Xh[hit])).max(1) if hit.any() else np.zeros(0)
    assert (d <= PC.round_trip_bar(m, x[hit], cells)).all()


# ------------------------------------------------------------------------------------------- 1, 2, 3
@pytest.mark.parametrize("family", FAMILIES)
def test_interior_points(family, dev):
    for tr in TM.PARITY + TM.SHIFTS:
        m = PC.family_mesh(family, tr)
        x, _ = PC.check_interior(m, dev)
        _same_as_host(m, x, dev)


@pytest.mark.parametrize("family", FAMILIES)
def test_points_on_shared_entities(family, dev):
    for tr in TM.PARITY:
        m = PC.family_mesh(family, tr)
        x, _ = PC.check_entities(m, dev)
        _same_as_host(m, x, dev)


@pytest.mark.parametrize("name", ["fan", "delaunay", "square_msh"])
def test_irregular_meshes(name, dev):
    m = _irregular(name)
    PC.check_interior(m, dev)
    x, _ = PC.check_entities(m, dev)
    _same_as_host(m, x, dev)


@pytest.mark.parametrize("family", FAMILIES)
def test_outside_points(family, dev):
    for tr in TM.PARITY:
        m = PC.family_mesh(family, tr)
        out = PC.outside_queries(family, tr)
        PC.check_rejected(m, out, dev)
        x = m.x.numpy()
        size = np.abs(x.max(0) - x.min(0)).max()
        far = x.mean(0) + 1e6 * size * np.array([[1.0, -1.0, 1.0][:m.gdim], [-1.0, 0.0, 0.0][:m.gdim]])
        PC.check_rejected(m, far, dev)
        bad = np.repeat(x.mean(0)[None], m.gdim + 1, 0)
        for d in range(m.gdim):
            bad[d, d] = np.nan
        bad[m.gdim, 0] = np.inf
        PC.check_rejected(m, bad, dev)
        _same_as_host(m, np.concatenate([out, far, bad]), dev)


def test_hole(dev):
    m, pts = PC.hole_mesh()
    PC.check_rejected(m, pts, dev)
    PC.check_interior(m, dev)


def test_degenerate_queries(dev):
    from femasm import geometry, mesh

    m = PC.on_device(PC.family_mesh("tet-P1", "rot"), dev)
    c, X = geometry.locate_points(m, torch.zeros((0, 3), dtype=torch.float64, device=dev))
    assert c.shape == (0,) and c.dtype == torch.int32 and X.shape == (0, 3) and c.device.type == "cuda"
    for ct, x in ((mesh.CellType.triangle, [[0.0, 0.0], [2.0, 0.5], [0.5, 1.5]]),
                  (mesh.CellType.hexahedron, mesh.create_unit_cube(1, 1, 1, mesh.CellType.hexahedron).x.tolist())):
        one = mesh.Mesh(ct, torch.tensor(x, dtype=torch.float64), torch.arange(len(x), dtype=torch.int32)[None])
        assert geometry.bb_tree(PC.on_device(one, dev)).dims == (1, 1, 1)
        PC.check_interior(one, dev, per_cell=70)
        PC.check_entities(one, dev)
    m = PC.family_mesh("quad-Q1", None)
    tree = geometry.bb_tree(PC.on_device(m, dev))
    hi = np.array([tree.lo[d] + tree.dims[d] / tree.inv_h[d] for d in range(2)])
    PC.check_rejected(m, np.array([[hi[0], 0.5], [0.5, hi[1]], hi]), dev)
    top = np.array([[1.0, 0.5], [0.5, 1.0], [1.0, 1.0]])
    c, _ = PC.locate(m, top, dev)
    assert np.array_equal(c, PC.brute_force(m, top)) and (c >= 0).all()


# ------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("family", ["tri-P1", "tet-P2", "quad-Q2-warp", "hex-Q1-warp", "hex-Q3"])
def test_grid_independence_and_brute_force(family, dev):
    from femasm import geometry

    for tr in ("rotmirror", "stretch"):
        m = PC.family_mesh(family, tr)
        md = PC.on_device(m, dev)
        x = np.concatenate([PC.interior_queries(m, 2)[0], PC.entity_queries(m)[0], PC.outside_queries(family, tr)])
        gd = m.gdim
        t0 = geometry.bb_tree(md)
        c0, X0 = PC.locate(m, x, dev)
        c1, X1 = PC.locate(m, x, dev, tree=geometry.bb_tree(md, dims=(1,) * gd))
        c4, X4 = PC.locate(m, x, dev, tree=geometry.bb_tree(md, dims=tuple(4 * d for d in t0.dims[:gd])))
        assert np.array_equal(c0, c1) and np.array_equal(c0, c4)
        assert np.array_equal(X0, X1, equal_nan=True) and np.array_equal(X0, X4, equal_nan=True)
        assert np.array_equal(c0, PC.brute_force(m, x))


# ------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("family", FAMILIES)
def test_eval_against_host_basis(family, dev):
    """fa_eval_points at the device's own (cell, X) against the host basis, gradients and Jacobian there."""
    from femasm import fem, geometry

    for tr in ("rotmirror", "shear"):
        m = PC.family_mesh(family, tr)
        md = PC.on_device(m, dev)
        x = np.concatenate([PC.interior_queries(m, 3)[0], PC.entity_queries(m)[0], PC.outside_queries(family, tr)])
        cells, X = geometry.locate_points(md, torch.tensor(x, device=dev))
        ch = cells.cpu().numpy().astype(np.int64)
        hit = ch >= 0
        assert hit.any() and (~hit).any()
        for bs in (1, 2, 3):
            V = PC.space_of(md, family, bs)
            # random signs, magnitudes in [0.5, 1]: at a vertex query the bar is 1e-12 |w_vertex| while both
            # sides round lambda_0 = 1 - sum X to eps, an error of eps |w_b| at the other nodes; a field with
            # entries near zero would make that a test of the field's smallest entry, not of the kernel
            gen = torch.Generator().manual_seed(40 + bs)
            w = torch.rand(V.num_dofs, generator=gen, dtype=torch.float64)
            w = ((0.5 + 0.5 * w) * torch.where(torch.rand(V.num_dofs, generator=gen) < 0.5, -1.0, 1.0)).to(dev)
            val, g = fem.eval_points(w, cells=cells, X=X, grad=True, V=V)
            only = fem.eval_points(w, cells=cells, X=X, V=V)
            val, g, only = val.cpu().numpy(), g.cpu().numpy(), only.cpu().numpy()
            assert val.shape == (x.shape[0], bs) and g.shape == (x.shape[0], bs, m.gdim)
            assert np.array_equal(val, only, equal_nan=True)
            assert np.isnan(val[~hit]).all() and np.isnan(g[~hit]).all()
            rv, rg, vmag, gmag = PC.host_reference(V, w.cpu(), ch[hit], X.cpu().numpy()[hit])
            ev, eg = np.abs(val[hit] - rv) / vmag, np.abs(g[hit] - rg) / gmag
            print(f"{family} {tr} bs {bs}: value {ev.max():.3e}, gradient {eg.max():.3e} of the magnitudes")
            assert (ev <= 1e-12).all() and (eg <= 1e-12).all(), (ev.max(), eg.max())


# ------------------------------------------------------------------------------------------- 6, 7
@pytest.mark.parametrize("family", FAMILIES)
def test_affine_field_end_to_end(family, dev):
    for tr in ("rot", "mirror", "shear", "stretch", "shift1e4"):
        PC.check_affine_field(family, tr, dev)
    if TM.is_affine(family) and TM.FAMILIES[family][1] >= 2:
        PC.check_affine_field(family, "rotmirror", dev, quadratic=True)


def test_across_meshes(dev):
    PC.check_across_meshes(dev)


def test_missing_and_dg0(dev):
    PC.check_missing_and_dg0(dev)


# ------------------------------------------------------------------------------------------- 8, 9
@pytest.mark.parametrize("family", ["tri-P2", "hex-Q2-warp"])
def test_determinism(family, dev):
    from femasm import fem, geometry

    m = PC.family_mesh(family, "rot")
    md = PC.on_device(m, dev)
    x = np.concatenate([PC.interior_queries(m, 3)[0], PC.entity_queries(m)[0], PC.outside_queries(family, "rot")])
    c0, X0 = PC.locate(m, x, dev)
    c1, X1 = PC.locate(m, x, dev)
    assert np.array_equal(c0, c1) and np.array_equal(X0, X1, equal_nan=True)
    perm = np.random.default_rng(0).permutation(x.shape[0])
    cp, Xp = PC.locate(m, x[perm], dev)
    assert np.array_equal(cp, c0[perm]) and np.array_equal(Xp, X0[perm], equal_nan=True)
    V = PC.space_of(md, family, 2)
    w = (torch.rand(V.num_dofs, generator=torch.Generator().manual_seed(1), dtype=torch.float64) - 0.5).to(dev)
    cd, Xd = geometry.locate_points(md, torch.tensor(x, device=dev))
    v0, g0 = fem.eval_points(w, cells=cd, X=Xd, grad=True, V=V)
    v1, g1 = fem.eval_points(w, cells=cd, X=Xd, grad=True, V=V)
    pt = torch.tensor(perm, device=dev)
    vp, gp = fem.eval_points(w, cells=cd[pt], X=Xd[pt], grad=True, V=V)
    for a, b in ((v0, v1), (g0, g1), (vp, v0[pt]), (gp, g0[pt])):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def test_abi_on_device(dev):
    import ctypes

    from femasm import _lib, geometry

    L = _lib.load()
    assert L.fa_version() >= 108
    m = PC.on_device(PC.family_mesh("tri-P1", None), dev)
    fm = geometry._fa_geometry_mesh(m)
    g = geometry.bb_tree(m)._fa_cell_grid()
    x = torch.rand((5, 2), dtype=torch.float64, device=dev)
    c = torch.empty(5, dtype=torch.int32, device=dev)
    X = torch.empty((5, 2), dtype=torch.float64, device=dev)
    w = torch.rand(m.num_vertices * 2, dtype=torch.float64, device=dev)
    v = torch.empty((5, 2), dtype=torch.float64, device=dev)
    E = _lib.FA_E_ARG
    assert L.fa_locate_points(ctypes.byref(fm), ctypes.byref(g), 5, None, 1e-10, c.data_ptr(), X.data_ptr(), None) == E
    assert L.fa_locate_points(ctypes.byref(fm), ctypes.byref(g), 5, x.data_ptr(), 1e-10, None, X.data_ptr(), None) == E
    assert L.fa_locate_points(ctypes.byref(fm), None, 5, x.data_ptr(), 1e-10, c.data_ptr(), X.data_ptr(), None) == E
    assert L.fa_locate_points(ctypes.byref(fm), ctypes.byref(g), -1, x.data_ptr(), 1e-10, c.data_ptr(), X.data_ptr(), None) == E
    assert L.fa_locate_points(ctypes.byref(fm), ctypes.byref(g), 0, None, 1e-10, None, None, None) == 0
    assert L.fa_locate_points(ctypes.byref(fm), ctypes.byref(g), 5, x.data_ptr(), 1e-10, c.data_ptr(), X.data_ptr(), None) == 0
    assert L.fa_eval_points(ctypes.byref(fm), w.data_ptr(), 4, 5, c.data_ptr(), X.data_ptr(), v.data_ptr(), None, None) == E
    assert L.fa_eval_points(ctypes.byref(fm), None, 2, 5, c.data_ptr(), X.data_ptr(), v.data_ptr(), None, None) == E
    assert L.fa_eval_points(ctypes.byref(fm), w.data_ptr(), 2, 5, c.data_ptr(), X.data_ptr(), None, None, None) == E
    assert L.fa_eval_points(ctypes.byref(fm), w.data_ptr(), 2, 0, None, None, v.data_ptr(), None, None) == 0
    assert L.fa_eval_points(ctypes.byref(fm), w.data_ptr(), 2, 5, c.data_ptr(), X.data_ptr(), v.data_ptr(), None, None) == 0
    fm.degree, fm.nn = 3, 10
    assert L.fa_eval_points(ctypes.byref(fm), w.data_ptr(), 2, 5, c.data_ptr(), X.data_ptr(), v.data_ptr(), None,
                            None) == _lib.FA_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isfinite(v).all() and (c >= 0).all()
