"""The inputs and the oracle of tests/test_gpu_dirichlet_sets.py, pinned on the CPU so that a failure there
points at a device kernel and not at a set builder or the reference.

1. Coverage: on every element of form_parameters.ELEMENTS the sets of tests/dirichlet_sets.py reach what
   they are aimed at (every (local node, component) position set and clear, full masks, cell-interior
   nodes, a node with only its last component constrained, an empty marker).
2. The oracle's constrained matrix against an independent model: its own unconstrained matrix with the
   constrained rows and columns zeroed and `d` on the constrained diagonals. The oracle zeroes entries of
   the cell matrix and adds the cell matrices in the same order either way, so every untouched entry is
   held to exact equality (it proved true: no entry needs the per-row bar).
3. The oracle's lifting followed by the set-bc overwrite against  b - alpha A0 (mk * (g - x0))  with A0
   the unconstrained matrix in scipy, at the suite's vector bar 1e-12 max|ref|.
4. fem._combine_bcs on a CPU mesh against the builders' independent arrays, the later bc winning in
   `overlap`, and the cache never serving a stale marker or g after an edit or a reassignment.

`python tests/test_dirichlet_sets_host.py` writes the coverage table profiles/dirichlet_sets/host_model.txt."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import dirichlet_sets as DS
import form_parameters as FP
from rowparity import RTOL
from test_form_parameters_host import host_mesh

SEED = 0
_cache = {}


class HostCase:
    def __init__(self, oracle, ct, p, n, perturb=0.0):
        from femasm import fem

        self.ct, self.p, self.n = ct, p, n
        m = self.m = host_mesh(ct, n, perturb)
        self.V = V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
        self.cells, self.geom, self.x = V.dofmap.numpy(), m.cells.numpy(), m.x.numpy()
        self.ip, self.ix = oracle.sparsity(self.cells, V.num_nodes)
        self.lam, self.mu = oracle.lame(oracle.e_range()[np.arange(m.num_cells) % 200], 0.3)
        g = torch.Generator().manual_seed(1)
        self.u = (1e-3 * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).numpy()
        d = torch.rand(V.num_nodes, generator=g, dtype=torch.float64)
        d[d < 0.4] = 0.0
        self.d = d.numpy()
        self.u_neo = (0.05 * torch.sin(torch.pi * V.tabulate_dof_coordinates())).reshape(-1).numpy()
        self._sets, self._mat = {}, {}

    def set(self, name):
        if name not in self._sets:
            self._sets[name] = DS.build(name, self.V, SEED)
        return self._sets[name]

    def args(self):
        return (self.ct, self.p, self.cells, self.geom, self.x, self.lam, self.mu)

    def matrix(self, oracle, law, bc=None, diag=1.0):
        if law == "lin":
            return oracle.assemble_elasticity(*self.args(), self.ip, self.ix, bc=bc, diag=diag)
        if law == "neo":
            return oracle.assemble_neohookean(*self.args(), self.u_neo, self.ip, self.ix, bc=bc, diag=diag)
        return oracle.assemble_damage(self.cells, self.geom, self.x, self.lam, self.mu, self.u, self.d, self.ip, self.ix,
                                      bc=bc, diag=diag)

    def free(self, oracle, law):
        if law not in self._mat:
            self._mat[law] = self.matrix(oracle, law)
        return self._mat[law]


def _case(oracle, elem, table=None):
    ct, p, n = DS.mesh_of(elem, table) if isinstance(elem, str) else elem
    key = (ct, p, n)
    if key not in _cache:
        _cache[key] = HostCase(oracle, ct, p, n)
    return _cache[key]


# ------------------------------------------------------------------------------------------ 1. coverage
def coverage(C):
    """Per set: (positions set in some cell, positions clear in some cell, cells with every position set),
    and the number of positions of the element."""
    rows = {}
    for name in DS.SETS:
        pos = DS.cell_positions(C.V, C.set(name)[1])
        flat = pos.reshape(pos.shape[0], -1)
        rows[name] = (int(flat.any(0).sum()), int((~flat).any(0).sum()), int(flat.all(1).sum()))
    return rows, C.V.nn * C.V.bs


@pytest.mark.parametrize("elem", list(FP.ELEMENTS))
def test_coverage(oracle, elem):
    from femasm import fem

    C = _case(oracle, elem)
    V = C.V
    ct, p, _ = DS.mesh_of(elem)
    npos = V.nn * V.bs
    pa = DS.cell_positions(V, C.set("scatter")[1]).reshape(-1, npos)
    pb = DS.cell_positions(V, C.set("scatter-complement")[1]).reshape(-1, npos)
    assert np.array_equal(pa, ~pb)  # the complement, dof by dof
    assert (pa.any(0) | pb.any(0)).all() and ((~pa).any(0) | (~pb).any(0)).all()
    full = DS.cell_positions(V, C.set("all")[1]).reshape(-1, npos)
    assert full.all()
    if npos <= 32:
        want = (1 << npos) - 1
        assert (DS.cell_masks(V, C.set("all")[1]) == np.uint64(want)).all()
        if elem == "quad-Q3":
            assert want == 0xFFFFFFFF
        if elem == "tet-P2":
            assert want == (1 << 30) - 1
        assert (DS.cell_masks(V, C.set("empty")[1]) == 0).all()
    if ct in (FP.QUAD, FP.HEX) and p >= 2:
        X = fem.reference_nodes(ct, p)
        inner = np.nonzero(((X > 1e-12) & (X < 1 - 1e-12)).all(1))[0]
        assert inner.size == (p - 1) ** V.mesh.gdim
        assert DS.cell_positions(V, C.set("interior")[1])[:, inner, :].any()
    mk = C.set("interior")[1].reshape(-1, V.bs).astype(bool)
    xn = DS.node_coordinates(V)
    assert mk.any() and not mk[~DS.interior_nodes(xn)].any()
    last = C.set("last-component")[1].reshape(-1, V.bs).astype(bool)
    assert (last[:, -1] & ~last[:, :-1].any(1)).any() and not last[:, :-1].any()
    assert last[np.isclose(xn[:, 0], 0.0), -1].all() and last[DS.interior_nodes(xn), -1].all()
    assert int(C.set("empty")[1].sum()) == 0 and len(C.set("empty")[0]) == 1
    single = C.set("single")[1]
    assert int(single.sum()) == 1 and int(np.nonzero(single)[0][0]) % V.bs == 1
    assert DS.interior_nodes(xn)[np.nonzero(single)[0][0] // V.bs]
    assert DS.overlap_band(V).size > 0 and len(C.set("overlap")[0]) == 3


@pytest.mark.parametrize("elem", list(FP.VECTOR_CASES))
def test_vector_meshes_hold_the_sets(oracle, elem):
    """The smaller meshes of VECTOR_CASES: the band two bcs of `overlap` share exists, `single` has its
    interior node, and the prescribed values are distinct per dof."""
    C = _case(oracle, elem, FP.VECTOR_CASES)
    xn = DS.node_coordinates(C.V)
    assert DS.overlap_band(C.V).size > 0 and DS.interior_nodes(xn).any()
    for name in DS.SETS:
        _, mk, g = C.set(name)
        on = mk.astype(bool)
        assert np.unique(g[on]).size == on.sum() and (np.abs(g[on]) >= 0.25 * DS.G_AMP).all() and not g[~on].any()


# ------------------------------------------------------------------------------------------ 2. the oracle's matrix
def _model(C, free, marker, d):
    """The unconstrained values with constrained rows and columns zeroed and d on constrained diagonals."""
    bs = free.shape[1]
    rows = np.repeat(np.arange(len(C.ip) - 1), np.diff(C.ip))
    mk = marker.reshape(-1, bs).astype(bool)
    mr, mc = mk[rows], mk[C.ix]
    out = free.copy()
    out[mr[:, :, None] | mc[:, None, :]] = 0.0
    out[(rows == C.ix)[:, None, None] & np.eye(bs, dtype=bool)[None] & mr[:, :, None]] = d
    return out


def _oracle_vs_model(oracle, C, law):
    free = C.free(oracle, law)
    assert np.isfinite(free).all() and np.abs(free).max() > 0
    for name in DS.SETS:
        marker = C.set(name)[1]
        for d in (1.0, 0.0, 2.5):
            got = C.matrix(oracle, law, bc=marker, diag=d)
            np.testing.assert_array_equal(got, _model(C, free, marker, d), err_msg=f"{law} {name} diag={d}")


@pytest.mark.parametrize("elem", list(FP.ELEMENTS))
def test_oracle_matrix_is_the_zeroed_unconstrained_one(oracle, elem):
    _oracle_vs_model(oracle, _case(oracle, elem), "lin")


@pytest.mark.parametrize("elem", list(FP.NEO))
def test_oracle_neohookean_matrix(oracle, elem):
    _oracle_vs_model(oracle, _case(oracle, elem, FP.NEO), "neo")


def test_oracle_damage_matrix(oracle):
    _oracle_vs_model(oracle, _case(oracle, FP.DAMAGE), "dam")


# ------------------------------------------------------------------------------------------ 3. the oracle's lifting
def _oracle_lifting(oracle, C, law):
    kind = {"lin": 0, "dam": 1, "neo": 2}[law]
    u = {"lin": C.u, "dam": C.u, "neo": C.u_neo}[law]
    A0 = sp.bsr_matrix((C.free(oracle, law), C.ix, C.ip)).tocsr()
    b = np.random.default_rng(5).standard_normal(C.V.num_dofs) * np.abs(A0).max() * DS.G_AMP
    worst = 0.0
    for name in DS.SETS:
        _, marker, g = C.set(name)
        mk = marker.astype(bool)
        for x0 in (None, u):
            for alpha in (-1.0, 1.0):
                got = oracle.apply_lifting(*C.args(), b, marker, g, x0=x0, alpha=alpha, u=u if kind else None,
                                           d=C.d if kind == 1 else None, kind=kind)
                v = np.where(mk, g - (0.0 if x0 is None else x0), 0.0)
                ref = b - alpha * (A0 @ v)
                got[mk] = alpha * v[mk]  # set_bc
                ref[mk] = alpha * v[mk]
                rel = float(np.abs(got - ref).max() / np.abs(ref).max())
                worst = max(worst, rel)
                assert rel <= RTOL, f"{law} {name} x0={'u' if x0 is not None else None} alpha={alpha}: {rel:.3e}"
    return worst


@pytest.mark.parametrize("elem", list(FP.VECTOR_CASES))
def test_oracle_lifting(oracle, elem):
    _oracle_lifting(oracle, _case(oracle, elem, FP.VECTOR_CASES), "lin")


@pytest.mark.parametrize("elem", list(FP.NEO))
def test_oracle_lifting_neohookean(oracle, elem):
    _oracle_lifting(oracle, _case(oracle, elem, FP.NEO), "neo")


def test_oracle_lifting_damage(oracle):
    _oracle_lifting(oracle, _case(oracle, FP.DAMAGE), "dam")


# ------------------------------------------------------------------------------------------ 4. _combine_bcs
@pytest.mark.parametrize("elem", list(FP.ELEMENTS))
def test_combine_bcs_matches_the_builders(oracle, elem):
    from femasm import fem

    C = _case(oracle, elem)
    for name in DS.SETS:
        bcs, marker, g = C.set(name)
        mk, gv = fem._combine_bcs(C.V, bcs)
        assert mk.dtype == torch.int8
        np.testing.assert_array_equal(mk.numpy(), marker, err_msg=name)
        np.testing.assert_array_equal(gv.numpy(), g, err_msg=name)
        mk2, none = fem._combine_bcs(C.V, bcs, with_g=False)
        np.testing.assert_array_equal(mk2.numpy(), marker)
        assert none is None


def test_overlap_later_bc_wins(oracle):
    from femasm import fem

    C = _case(oracle, "quad-Q2")
    V = C.V
    bcs, marker, g = C.set("overlap")
    band = DS.overlap_band(V)
    dofs = (band[:, None] * V.bs + np.arange(V.bs)[None, :]).reshape(-1)
    first, second = bcs[0].g.numpy()[dofs], bcs[1].g.numpy()[dofs]
    assert (first != second).all() and (first != 0).all()
    _, gv = fem._combine_bcs(V, bcs)
    np.testing.assert_array_equal(gv.numpy()[dofs], second)
    np.testing.assert_array_equal(g[dofs], second)
    _, gr = fem._combine_bcs(V, bcs[::-1])  # the other order: the other value
    np.testing.assert_array_equal(gr.numpy()[dofs], first)
    d3 = bcs[2].dofs.numpy()
    assert np.unique(d3).size == d3.size - 1  # the repeated node


def test_combine_bcs_never_serves_stale_state(oracle):
    from femasm import fem

    ct, p, n = DS.mesh_of("tri-P2")
    C = HostCase(oracle, ct, p, n)  # its own space: its own cache
    V = C.V
    bcs, marker, g = DS.build("scatter", V, SEED)

    def check(what):
        mk, gv = fem._combine_bcs(V, bcs)
        np.testing.assert_array_equal(mk.numpy(), marker, err_msg=what)
        np.testing.assert_array_equal(gv.numpy(), g, err_msg=what)
        mk2, _ = fem._combine_bcs(V, bcs, with_g=False)
        np.testing.assert_array_equal(mk2.numpy(), marker, err_msg=what)

    check("as built")
    hit = fem._combine_bcs(V, bcs)[0]
    assert fem._combine_bcs(V, bcs)[0] is hit  # (the cache does serve an unchanged set)
    k = int(bcs[0].dofs[0])
    bcs[0].g[k] = 0.5  # g edited in place
    g[k] = 0.5
    check("g edited in place")
    drop, add = DS.swap_one_dof(V, bcs[0], marker)  # dofs edited in place
    marker[drop], marker[add] = 0, 1
    g[drop], g[add] = 0.0, float(bcs[0].g[add])
    check("dofs edited in place")
    new_g = bcs[1].g.clone()
    new_g[bcs[1].dofs] *= -2.0
    bcs[1].g = new_g  # g reassigned
    on = bcs[1].dofs.numpy()
    g[on] = new_g.numpy()[on]
    check("g reassigned")
    keep = bcs[1].dofs[1:].clone()
    gone = int(bcs[1].dofs[0])
    bcs[1].dofs = keep  # dofs reassigned
    marker[gone], g[gone] = 0, 0.0
    check("dofs reassigned")


# ------------------------------------------------------------------------------------------ the table
def _write_table():
    from oracle import oracle

    oracle.build()
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dirichlet_sets")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "host_model.txt"), "w") as fh:
        fh.write("# Per element of form_parameters.ELEMENTS and set of tests/dirichlet_sets.py (seed 0): the per-cell\n"
                 "# bit positions (local node, component) set in at least one cell / clear in at least one cell, of the\n"
                 "# element's positions, and the cells whose every position is set, of the mesh's cells.\n"
                 "# planes: the reference's set of every other suite (all components on x0 = 0 and x0 = 1).\n")
        for elem in FP.ELEMENTS:
            C = _case(oracle, elem)
            rows, npos = coverage(C)
            xn = DS.node_coordinates(C.V)
            on = np.isclose(xn[:, 0], 0.0) | np.isclose(xn[:, 0], 1.0)
            flat = DS.cell_positions(C.V, np.repeat(on, C.V.bs).astype(np.int8)).reshape(C.m.num_cells, -1)
            rows = {"planes": (int(flat.any(0).sum()), int((~flat).any(0).sum()), int(flat.all(1).sum())), **rows}
            for name, (s, c, f) in rows.items():
                fh.write(f"{elem:8s} {name:18s} set {s:3d}/{npos:<3d} clear {c:3d}/{npos:<3d} full cells {f:3d}/{C.m.num_cells}\n")
    print(open(os.path.join(out, "host_model.txt")).read())


if __name__ == "__main__":
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "fem-libraries_amd")]
    _write_table()
