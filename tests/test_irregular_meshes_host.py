"""Host checks of the irregular-valence meshes (tests/irregular_meshes.py) and of which side of every
planner target and cap each of them sits on: the executable form of DESIGN.md's "Planner targets and
caps" table. Everything here comes from the cell dofmap, oracle.sparsity and the node -> cell adjacency
(a bincount of the dofmap); no device is used. tests/test_gpu_irregular.py assembles these cases.

Printed per case: largest-row entries / blocks / candidates and the minimum cell quality.
"""
import numpy as np
import pytest

import irregular_meshes as im
from irregular_meshes import TET, TRI

# (case, degree) -> largest row (entries, blocks, candidates), and the routes of the three plans:
# linear (fa_plan_gather), neo-Hookean (fa_plan_gather_form) and block-owner (fa_plan_gather_contrib).
# Entries of a row = cells at its node; blocks = its distinct neighbour nodes + itself; candidates =
# entries x nodes per cell. fan(N): N / N + 1 / 3 N at P1, N / 3 N + 1 / 6 N at P2 (row 0);
# cone(nx, ny), c = 2 nx ny cells, v = (nx + 1)(ny + 1) base vertices, e = base edges = c + v - 1 (Euler):
# c / v + 1 / 4 c at P1, c / v + e + v + 1 / 10 c at P2 (the apex row).
EXPECT = {
    ("delaunay", 1): ((36, 21, 144), "table", "table", "table"),
    ("delaunay", 2): ((36, 95, 360), "table", "table", "table"),
    ("square", 1): ((7, 8, 21), "table", "table", "table"),
    ("square", 2): ((7, 22, 42), "table", "table", "table"),
    ("square_r1", 1): ((7, 8, 21), "table", "table", "table"),
    ("square_r1", 2): ((7, 22, 42), "table", "table", "table"),
    # 144 entries: under the P1 target of 256, over the P2 target of 128; 414 blocks: under the linear
    # P2 cap (455) and the neo-Hookean one (640), over the block-owner one (398)
    ("cone98", 1): ((144, 91, 576), "table", "table", "table"),
    ("cone98", 2): ((144, 414, 1440), "generic", "generic", "refused"),
    # 288 entries over the P1 target of 256; 170 blocks under the P1 cap of 227
    ("cone1212", 1): ((288, 170, 1152), "generic", "generic", "generic"),
    # 150 entries: over the P2 target of 128, inside a block-owner chunk (256): the default plan of a
    # triangle mesh (owner) takes it, owner=False sends it to the generic gather
    ("fan150", 2): ((150, 451, 900), "generic", "generic", "table"),
    # 300 entries: over every target; 901 blocks over the block-owner cap (896) too
    ("fan300", 2): ((300, 901, 1800), "generic", "generic", "refused"),
    ("fan300", 1): ((300, 301, 900), "generic", "generic", "generic"),
    ("fan600", 1): ((600, 601, 1800), "refused", "refused", "refused"),
    ("fan700", 1): ((700, 701, 2100), "refused", "refused", "refused"),
}
CASES = im.CASES

_mesh_cache = {}


def _mesh(name):
    if name not in _mesh_cache:
        _mesh_cache[name] = CASES[name][0]()
    return _mesh_cache[name]


def test_every_case_is_listed():
    assert {(n, p) for n, (_, ps) in CASES.items() for p in ps} == set(EXPECT)


def test_limits_are_the_kernels():
    """The named limits, per element, as fa_plan_gather / fa_plan_gather_form / fa_plan_gather_contrib
    pass them to plan_gather."""
    assert [im.entry_target(*e) for e in ((TRI, 1), (TRI, 2), (TET, 1), (TET, 2))] == [256, 128, 256, 128]
    assert [im.entry_target(*e, "neo") for e in ((TRI, 1), (TRI, 2), (TET, 1), (TET, 2))] == [256, 128, 256, 128]
    assert [im.block_cap(*e) for e in ((TRI, 1), (TRI, 2), (TET, 1), (TET, 2))] == [512, 1023, 227, 455]
    assert [im.block_cap(*e, "neo") for e in ((TRI, 1), (TRI, 2), (TET, 1), (TET, 2))] == [1023, 1023, 640, 640]
    assert [im.block_cap(ct, 2, "own") for ct in (TRI, TET)] == [896, 398]
    assert (im.GATHER_MAX_ADJ, im.GATHER_MAX_ROWS, im.OWN_CCAP, im.SPARSITY_CAP) == (512, 128, 256, 2048)


@pytest.mark.parametrize("name,p", sorted(EXPECT))
def test_largest_row_and_route(oracle, name, p):
    from femasm import fem

    m = _mesh(name)
    ct = int(m.cell_type)
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    dm = V.dofmap.numpy()
    indptr, _ = oracle.sparsity(dm, V.num_nodes)
    st = im.row_stats(dm, V.num_nodes, indptr)
    x, cells = m.x.numpy(), m.cells.numpy()
    q = im.min_quality(x, cells)
    print(f"{name} P{p}: {m.num_cells} cells, {V.num_nodes} nodes; largest row {st['row']}: entries "
          f"{st['entries']} / blocks {st['blocks']} / candidates {st['candidates']}; min quality {q:.4f}")
    (entries, blocks, cand), lin, neo, own = EXPECT[(name, p)]
    assert (st["entries"], st["blocks"], st["candidates"]) == (entries, blocks, cand)
    assert st["min_entries"] >= 1  # every node belongs to a cell
    assert im.route(ct, p, entries, blocks, "lin") == lin
    assert im.route(ct, p, entries, blocks, "neo") == neo
    assert im.route(ct, p, entries, blocks, "own") == own
    # each side stated on its own, so that a changed constant shows which comparison moved
    if lin == "generic":
        assert im.entry_target(ct, p) < entries <= im.GATHER_MAX_ADJ and blocks <= im.block_cap(ct, p)
        assert blocks <= im.block_cap(ct, p, "neo")
    if name == "fan600":  # over both hard caps of the gather, under the sparsity kernel's
        assert entries > im.GATHER_MAX_ADJ and blocks > im.block_cap(ct, p) and cand <= im.SPARSITY_CAP
    if name == "fan700":
        assert cand > im.SPARSITY_CAP
    else:
        assert cand <= im.SPARSITY_CAP


def _fan_quality(n):
    """fan(n): legs 1, 1, base 2 sin(pi / n), area sin(2 pi / n) / 2."""
    l2 = (2.0 + 4.0 * np.sin(np.pi / n) ** 2) / 3.0
    return 4.0 * (0.5 * np.sin(2.0 * np.pi / n)) / (np.sqrt(3.0) * l2)


@pytest.mark.parametrize("name", sorted(CASES))
def test_geometry(name):
    """Volume sum, orientation signs and minimum cell quality 6 sqrt(2) V / l_rms^3 (tetrahedra),
    4 A / (sqrt(3) l_rms^2) (triangles). The quality floor 0.05 makes the 1e-12 bar of the GPU tests a
    statement about the kernels, not about slivers; it holds wherever the valence allows it. A planar
    fan of N cells has the apex angle 2 pi / N and with it the quality _fan_quality(N) (0.036 at N = 300),
    and the cone's tetrahedra stand on a base of 1 / (nx ny) under a unit height: those cases are held to
    that closed form / bound instead."""
    m = _mesh(name)
    x, cells = m.x.numpy(), m.cells.numpy()
    sv = im.signed_volumes(x, cells)
    q = im.min_quality(x, cells)
    npos, nneg = int((sv > 0).sum()), int((sv < 0).sum())
    print(f"{name}: volume {np.abs(sv).sum():.15f}, {npos} positive / {nneg} negative cells, min quality {q:.4f}, "
          f"shortest edge {im.shortest_edge(x, cells):.4f}")
    assert npos + nneg == len(sv)  # no flat cell
    if name == "delaunay":
        assert cells.shape == (426, 4)
        assert abs(np.abs(sv).sum() - 1.0) <= 1e-14  # the cells tile the unit cube
        assert npos > 0 and nneg > 0
        val = np.bincount(cells.reshape(-1), minlength=125)
        assert (int(val.min()), int(val.max())) == (1, 36)
        assert q >= 0.05
    elif name.startswith("square"):
        assert abs(np.abs(sv).sum() - 1.0) <= 1e-14
        assert q >= 0.05
    elif name.startswith("cone"):
        nx, ny = (9, 8) if name == "cone98" else (12, 12)
        assert abs(np.abs(sv).sum() - 1.0 / 3.0) <= 1e-14  # a pyramid over the unit square, height 1
        assert npos == nneg == nx * ny
        # V = 1 / (6 nx ny) for every cell; apex edges <= sqrt(1 + 1 / 2): l_rms^2 <= (2 (a^2 + b^2) + 4.5) / 6
        a, b = 1.0 / nx, 1.0 / ny
        bound = 6.0 * np.sqrt(2.0) / (6.0 * nx * ny) / ((2.0 * (a * a + b * b) + 4.5) / 6.0) ** 1.5
        assert bound <= q
    else:
        n = int(name[3:])
        assert abs(np.abs(sv).sum() - 0.5 * n * np.sin(2.0 * np.pi / n)) <= 1e-12
        assert nneg == 0
        assert abs(q - _fan_quality(n)) <= 1e-12
        if n <= 150:
            assert q >= 0.05
