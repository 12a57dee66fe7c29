"""GPU: the prepared cell state of the table gather (fa_prepare_cells / fa_prepare_diag /
fa_assemble_matrix_prepared behind fem.assemble_matrix and fem.SplitGather): static records and
Dirichlet diagonal lists kept on the space across assemblies, the coefficient pass per call.
Against the CPU oracle at the project's per-row bar (tests/rowparity: 1e-12 of each row's scale),
identical patterns. Meshes: small, but many chunks and partly filled last waves."""
import numpy as np
import pytest
import torch

from rowparity import assert_rows_close

pytestmark = pytest.mark.gpu

# (cell type, cells per axis, gather_plan options): triangles default to the block-owner plan, which
# the prepared gather does not take -- owner=False plans the LDS-atomic table gather for them
MESHES = [("tetrahedron", (6, 5, 4), None), ("triangle", (9, 7), dict(owner=False)),
          ("quadrilateral", (8, 6), None)]
IDS = ["P2tet", "P2tri", "Q2quad"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


class Problem:
    def __init__(self, dev, oracle, ct_name, n, degree=2):
        from femasm import fem, mesh

        self.oracle = oracle
        ct = mesh.CellType[ct_name]
        if len(n) == 3:
            m = mesh.create_box((1.0, 1.0, 1.0), n, cell_type=ct, device=dev)
        else:
            m = mesh.create_rectangle((1.0, 1.0), n, cell_type=ct, device=dev)
        self.m, self.gd, self.degree = m, m.gdim, degree
        self.V = V = fem.functionspace(m, ("Lagrange", degree, (m.gdim,)))
        self.E = torch.tensor(oracle.e_range()[np.arange(m.num_cells) % 200], dtype=torch.float64, device=dev)
        self.a = fem.LinearElasticity(V, E=self.E, nu=0.3)
        gd = m.gdim

        def face(axis, value):
            return fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[axis], torch.full_like(x[axis], value)))

        # one face clamped and one face prescribed; and another set on another face
        self.bcs = [fem.dirichletbc(0.0, face(0, 0.0), V), fem.dirichletbc([0.01] + [0.0] * (gd - 1), face(0, 1.0), V)]
        self.bcs2 = [fem.dirichletbc(0.0, face(1, 0.0), V)]
        self.cells = V.dofmap.cpu().numpy()
        self.indptr, self.indices = oracle.sparsity(self.cells, V.num_nodes)

    def marker(self, bcs):
        from femasm import fem

        mk, _ = fem._combine_bcs(self.V, bcs)
        return None if mk is None else mk.cpu().numpy()

    def ref(self, bcs=None, diag=1.0):
        """The oracle's matrix for the CURRENT E and coordinates."""
        lam, mu = self.oracle.lame(self.E.cpu().numpy(), 0.3)
        return self.oracle.assemble_elasticity(int(self.m.cell_type), self.degree, self.cells, self.m.cells.cpu().numpy(),
                                               self.m.x.cpu().numpy(), lam, mu, self.indptr, self.indices,
                                               bc=self.marker(bcs), diag=diag)

    def check(self, A, bcs=None, diag=1.0, what=""):
        torch.cuda.synchronize()
        assert np.array_equal(A.indices.cpu().numpy(), self.indices), "sparsity pattern mismatch"
        got = A.data.cpu().numpy()
        assert np.isfinite(got).all(), what
        assert_rows_close(got, self.ref(bcs, diag), self.indptr, what=what)
        check_bc_structure(got, self.indptr, self.indices, self.marker(bcs), diag, self.gd)
        return got


def check_bc_structure(vals, indptr, indices, marker, diag, bs):
    """Every constrained row holds `diag` on its diagonal and zeros elsewhere; every constrained column
    holds zeros (exactly)."""
    if marker is None:
        return
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    mk = marker.reshape(-1, bs).astype(bool)
    mr, mc = mk[rows], mk[indices]  # [nb, bs]: the block's constrained rows / columns
    expect = np.zeros_like(vals)
    on_diag = (rows == indices)[:, None, None] & np.eye(bs, dtype=bool)[None] & mr[:, :, None]
    expect[on_diag] = diag
    con = mr[:, :, None] | mc[:, None, :]
    assert on_diag.sum() == mk.sum(), "a constrained dof has no diagonal entry"
    assert np.array_equal(vals[con], expect[con]), "constrained rows / columns"


def assemble(P, plan, bcs=None, **kw):
    from femasm import fem

    return fem.assemble_matrix(P.a, bcs=bcs, plan=plan, **kw)


@pytest.mark.parametrize("with_bcs", [True, False], ids=["bcs", "nobcs"])
@pytest.mark.parametrize("ct,n,plan", MESHES, ids=IDS)
def test_prepared_matches_oracle(dev, oracle, ct, n, plan, with_bcs):
    P = Problem(dev, oracle, ct, n)
    bcs = P.bcs if with_bcs else None
    A = assemble(P, plan, bcs)
    assert P.V._prepared_builds == 1, "the prepared path did not run"
    P.check(A, bcs)
    st = next(iter(P.V._prepared.values()))
    pp = next(iter(st.windows.values()))[0]
    assert bool(pp.has_bc) == with_bcs and (pp.ndiag > 0) == with_bcs  # no bcs: no bits, no list


@pytest.mark.parametrize("ct,n,plan", MESHES, ids=IDS)
def test_repeated_assemblies_build_once(dev, oracle, ct, n, plan):
    P = Problem(dev, oracle, ct, n)
    ref = P.ref(P.bcs)
    A = None
    for k in range(3):
        A = assemble(P, plan, P.bcs, A=A)
        torch.cuda.synchronize()
        assert_rows_close(A.data.cpu().numpy(), ref, P.indptr, what=f"assembly {k}")
    assert P.V._prepared_builds == 1


@pytest.mark.parametrize("ct,n,plan", MESHES, ids=IDS)
def test_coefficient_changed_in_place(dev, oracle, ct, n, plan):
    """E scaled in place on a random half of the cells, then one cell's E negated (the sign taken from
    the coefficient): the next matrices are the oracle's for the new E; nothing static is rebuilt."""
    P = Problem(dev, oracle, ct, n)
    A = assemble(P, plan, P.bcs)
    P.check(A, P.bcs, what="first")
    g = torch.Generator(device="cpu").manual_seed(3)
    half = (torch.rand(P.m.num_cells, generator=g) < 0.5).to(dev)
    P.E.mul_(torch.where(half, torch.full_like(P.E, 3.7), torch.ones_like(P.E)))
    A = assemble(P, plan, P.bcs, A=A)
    P.check(A, P.bcs, what="E scaled")
    P.E[P.m.num_cells // 3].neg_()
    A = assemble(P, plan, P.bcs, A=A)
    P.check(A, P.bcs, what="one E negated")
    assert P.V._prepared_builds == 1


@pytest.mark.parametrize("ct,n,plan", MESHES, ids=IDS)
def test_coordinates_moved_in_place(dev, oracle, ct, n, plan):
    P = Problem(dev, oracle, ct, n)
    A = assemble(P, plan, P.bcs)
    P.check(A, P.bcs, what="before the move")
    x = P.m.x
    if ct == "quadrilateral":  # a shear keeps the parallelograms (the affine table route)
        x[:, 0] += 0.2 * x[:, 1]
    else:  # a smooth shift of the interior vertices: simplices stay affine
        interior = ((x > 1e-9) & (x < 1 - 1e-9)).all(1)
        x[interior] += 0.03 * torch.sin(5.0 * x[interior])
    A = assemble(P, plan, P.bcs, A=A)
    P.check(A, P.bcs, what="after the move")
    assert P.V._prepared_builds == 2


def test_quadrilaterals_moved_off_affine_fall_back(dev, oracle):
    """Quadrilaterals that stop being parallelograms leave the table gather: the next assembly runs
    the general path on the moved mesh (no stale static record is read)."""
    P = Problem(dev, oracle, "quadrilateral", (8, 6))
    A = assemble(P, None, P.bcs)
    x = P.m.x
    interior = ((x > 1e-9) & (x < 1 - 1e-9)).all(1)
    x[interior] += 0.03 * torch.sin(5.0 * x[interior])
    A = assemble(P, None, P.bcs, A=A)
    P.check(A, P.bcs, what="non-affine quadrilaterals")
    assert P.V._prepared_builds == 1


@pytest.mark.parametrize("ct,n,plan", MESHES, ids=IDS)
def test_other_bcs_sets(dev, oracle, ct, n, plan):
    """Another bcs list, then none: bits and diagonals follow, into a fresh matrix and into the same
    matrix (no diagonal or zeroed column left from the previous set)."""
    P = Problem(dev, oracle, ct, n)
    A = assemble(P, plan, P.bcs)
    P.check(A, P.bcs, what="first set")
    for bcs, name in ((P.bcs2, "second set"), (None, "no bcs"), (P.bcs, "first set again")):
        P.check(assemble(P, plan, bcs), bcs, what=name + ", fresh matrix")
        A = assemble(P, plan, bcs, A=A)
        P.check(A, bcs, what=name + ", same matrix")
    assert P.V._prepared_builds == 3  # one static part per marker; the first set's is found again


def test_diagonal_value_follows(dev, oracle):
    P = Problem(dev, oracle, "tetrahedron", (6, 5, 4))
    A = assemble(P, None, P.bcs, diagonal=1.0)
    P.check(A, P.bcs, 1.0)
    A = assemble(P, None, P.bcs, diagonal=2.0, A=A)
    P.check(A, P.bcs, 2.0)
    assert P.V._prepared_builds == 1


@pytest.mark.parametrize("ct,n,plan", MESHES, ids=IDS)
def test_deterministic(dev, oracle, ct, n, plan):
    P = Problem(dev, oracle, ct, n)
    A1 = assemble(P, plan, P.bcs, deterministic=True)
    g1 = P.check(A1, P.bcs, what="deterministic")
    A2 = assemble(P, plan, P.bcs, deterministic=True)
    torch.cuda.synchronize()
    assert np.array_equal(g1, A2.data.cpu().numpy()), "deterministic assemblies differ"
    assert P.V._prepared_builds == 1


def test_several_row_parts(dev, oracle):
    from femasm import fem

    P = Problem(dev, oracle, "tetrahedron", (6, 5, 4))
    nb = len(P.indices)
    A = fem.create_matrix(P.a, max_part_bytes=(nb // 3) * 8 * 9)
    assert len(A.parts) >= 3
    for _ in range(2):
        A = assemble(P, None, P.bcs, A=A)
    got = P.check(A, P.bcs)
    ref = P.ref(P.bcs)
    for r0, r1, d in A.parts:  # parity on every part
        b0, b1 = P.indptr[r0], P.indptr[r1]
        assert_rows_close(got[b0:b1], ref[b0:b1], P.indptr[r0:r1 + 1] - b0, what=f"part [{r0}, {r1})")
    assert P.V._prepared_builds == 1
    st = next(iter(P.V._prepared.values()))
    assert len(st.windows) == len(A.parts)  # one diagonal list per part


@pytest.mark.parametrize("ct,n,plan", MESHES, ids=IDS)
def test_split_gather_equals_assemble(dev, oracle, ct, n, plan):
    from femasm import fem

    P = Problem(dev, oracle, ct, n)
    N = P.V.num_nodes
    A = fem.create_matrix(P.a)
    sg = fem.SplitGather(P.a, P.bcs, A, [(0, N // 3), (N // 3, N)])
    for k in range(2):
        A.parts[0][2].fill_(np.nan)  # every value written by the two ranges
        sg.prepare()
        sg.rows(1)
        sg.rows(0)
        assert sg._prep is not None, "the split gather did not run on the prepared state"
        got = P.check(A, P.bcs, what=f"split gather, step {k}")
        full = assemble(P, plan, P.bcs)
        torch.cuda.synchronize()
        assert_rows_close(got, full.data.cpu().numpy(), P.indptr, what=f"split vs assemble_matrix, step {k}")
        P.E.mul_(1.0 + 0.5 * torch.sin(torch.arange(P.m.num_cells, device=dev, dtype=torch.float64)))
    assert P.V._prepared_builds == 1  # shared by the split gather and assemble_matrix


def test_forms_outside_the_scope_fall_back(dev, oracle):
    """P1 tetrahedra (the fused records) and the neo-Hookean tangent assemble as before."""
    from femasm import fem

    P = Problem(dev, oracle, "tetrahedron", (5, 4, 3), degree=1)
    P.check(assemble(P, None, P.bcs), P.bcs, what="P1 tetrahedra")
    assert P.V._prepared_builds == 0 and not any(P.V.__dict__.get("_prepared", {}).values())
    Q = Problem(dev, oracle, "tetrahedron", (3, 3, 2))
    g = torch.Generator(device="cpu").manual_seed(5)
    u = (0.01 * torch.rand(Q.V.num_dofs, generator=g, dtype=torch.float64)).to(dev)
    a = fem.NeoHookean(Q.V, E=Q.E, nu=0.3, u=u)
    A = fem.assemble_matrix(a, bcs=Q.bcs)
    torch.cuda.synchronize()
    lam, mu = oracle.lame(Q.E.cpu().numpy(), 0.3)
    ref = oracle.assemble_neohookean(int(Q.m.cell_type), 2, Q.cells, Q.m.cells.cpu().numpy(), Q.m.x.cpu().numpy(), lam,
                                     mu, u.cpu().numpy(), Q.indptr, Q.indices, bc=Q.marker(Q.bcs), diag=1.0)
    assert_rows_close(A.data.cpu().numpy(), ref, Q.indptr, what="neo-Hookean")
    assert Q.V._prepared_builds == 0
