"""Smoothed-aggregation multigrid on the GPU (mg.SmoothedAggregation over femasm.amg and femasm_amg.hip):
the four kernels against dense torch / scipy, the device Galerkin products against the independent
restatement in tests/amg_reference.py, the V-cycle as a symmetric positive definite operator, AMG-preconditioned
CG against block-Jacobi CG and against the reference implementation's iteration count, and the Newton driver
with the preconditioner set. Every mesh here is parentless and without a lattice as far as the package knows.

Measured figures are in profiles/amg/counts.txt and DESIGN.md section 3.13.
"""
import numpy as np
import pytest
import scipy.sparse as sps
import torch

import amg_reference as R
import irregular_meshes as IM

pytestmark = pytest.mark.gpu

MULT_SHAPES = [(2, 3), (3, 2), (3, 3), (3, 6), (6, 3), (6, 6)]
PRODUCT_SHAPES = [(2, 2, 3), (3, 3, 3), (3, 3, 6), (6, 6, 6), (3, 2, 3), (6, 3, 6)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _dev(a, dev, dtype=torch.float64):
    return torch.tensor(a, dtype=dtype, device=dev)


def _parentless(m):
    from femasm import mesh

    return mesh.Mesh(m.cell_type, m.x, m.cells, m.cell_tags, None)


def _square(dev, r):
    """square.msh refined r times, parents dropped."""
    return _parentless(IM.square_msh(refine=r)).to(dev)


def _box(dev, n):
    """A tetrahedral box without its lattice record (tests/test_gpu_refine_mg.py::_box)."""
    from femasm import mesh

    b = mesh.create_box((1.0, 1.0, 1.0), (n, n, n), mesh.CellType.tetrahedron)
    return mesh.Mesh(b.cell_type, b.x, b.cells, None, None).to(dev)


def _cell_E(oracle, m):
    key = m.cell_tags.cpu().numpy() if m.cell_tags is not None else np.arange(m.num_cells)
    return torch.tensor(oracle.e_range()[key % 200], device=m.device)


def _bcs(V, comps_right=None, disp=1e-3):
    from femasm import fem

    g = V.mesh.gdim
    x0, x1 = float(V.mesh.x[:, 0].min()), float(V.mesh.x[:, 0].max())
    left = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.full_like(x[0], x0)))
    right = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.full_like(x[0], x1)))
    return [fem.dirichletbc(0.0, left, V), fem.dirichletbc([disp] + [0.0] * (g - 1), right, V, components=comps_right)]


# ------------------------------------------------------------------------------------ 1. kernels
def _random_bcsr(rng, nrows, ncols, br, bc, dev):
    """Rows of 0 .. 5 blocks, every fifth row empty, one row of 70 blocks."""
    from femasm import la

    counts = rng.integers(1, 6, nrows)
    counts[::5] = 0
    if nrows:
        counts[min(3, nrows - 1)] = 70
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(ncols, k, replace=False)) for k in counts] + [np.zeros(0, np.int64)])
    data = rng.standard_normal((int(indptr[-1]), br, bc))
    return la.BlockCSR(_dev(indptr, dev, torch.int64), _dev(indices, dev, torch.int32), _dev(data, dev), ncols)


@pytest.mark.parametrize("br,bc", MULT_SHAPES)
def test_bcsr_mult_matches_dense_torch(dev, br, bc):
    rng = np.random.default_rng(100 * br + bc)
    ncols = 80
    for nrows in (0, 1, 65, 257):
        B = _random_bcsr(rng, nrows, ncols, br, bc, dev)
        if nrows:
            assert int((B.indptr[1:] - B.indptr[:-1]).max()) == 70
            assert nrows == 1 or int((B.indptr[1:] - B.indptr[:-1]).min()) == 0
        M = torch.zeros((nrows, br, ncols, bc), dtype=torch.float64)
        M[B.block_rows().cpu(), :, B.indices.cpu().to(torch.int64), :] = B.data.cpu()
        M = M.reshape(nrows * br, ncols * bc)
        x = torch.tensor(rng.standard_normal(ncols * bc))
        for add in (False, True):
            y0 = torch.tensor(rng.standard_normal(nrows * br)) if add else torch.full((nrows * br,), float("nan"),
                                                                                      dtype=torch.float64)
            y = y0.to(dev)
            B.mult(x.to(dev), y, add=add)
            ref = M @ x + (y0 if add else 0.0)
            bound = 1e-14 * (M.abs() @ x.abs() + (y0.abs() if add else 0.0))
            err = (y.cpu() - ref).abs()
            assert bool(torch.isfinite(err).all()) and bool((err <= bound).all()), (nrows, add, float(err.max()))
            again = y0.to(dev)
            B.mult(x.to(dev), again, add=add)
            assert torch.equal(y, again)  # bit-identical


def test_bcsr_argument_errors(dev):
    from femasm import _lib

    L = _lib.load()
    sh = _lib.stream_handle(dev)
    x = torch.full((64,), float("nan"), dtype=torch.float64, device=dev)
    ip = torch.zeros(8, dtype=torch.int64, device=dev)
    ix = torch.zeros(8, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()
    # outputs poisoned: an error must return before anything is launched
    assert L.fa_bcsr_mult(2, 2, 4, 4, p(ip), p(ix), p(x), p(x), 0, p(x), sh) == _lib.FA_E_UNSUPPORTED
    assert L.fa_bcsr_mult(2, 2, 2, 2, p(ip), p(ix), p(x), p(x), 0, p(x), sh) == _lib.FA_E_UNSUPPORTED
    assert L.fa_bcsr_mult(-1, 2, 3, 3, p(ip), p(ix), p(x), p(x), 0, p(x), sh) == _lib.FA_E_ARG
    assert L.fa_bcsr_mult(2, 2, 3, 3, None, p(ix), p(x), p(x), 0, p(x), sh) == _lib.FA_E_ARG
    assert L.fa_bcsr_mult(2, 2, 3, 3, p(ip), p(ix), p(x), None, 0, p(x), sh) == _lib.FA_E_ARG
    assert b"null" in L.fa_last_error()
    assert L.fa_bcsr_mult(2, 2, 3, 3, p(ip), p(ix), p(x), p(x), 0, None, sh) == _lib.FA_E_ARG
    assert L.fa_bcsr_product(2, 2, 3, 3, p(ip), 0, p(ix), p(ix), p(x), 1, p(x), 1, p(x), sh) == _lib.FA_E_UNSUPPORTED
    assert L.fa_bcsr_product(2, 4, 4, 4, p(ip), 0, p(ix), p(ix), p(x), 1, p(x), 1, p(x), sh) == _lib.FA_E_UNSUPPORTED
    assert L.fa_bcsr_product(-1, 3, 3, 3, p(ip), 0, p(ix), p(ix), p(x), 1, p(x), 1, p(x), sh) == _lib.FA_E_ARG
    assert L.fa_bcsr_product(2, 3, 3, 3, None, 0, p(ix), p(ix), p(x), 1, p(x), 1, p(x), sh) == _lib.FA_E_ARG
    assert L.fa_bcsr_product(2, 3, 3, 3, p(ip), 4, None, p(ix), p(x), 1, p(x), 1, p(x), sh) == _lib.FA_E_ARG
    assert L.fa_bcsr_product(2, 3, 3, 3, p(ip), 0, p(ix), p(ix), p(x), 1, p(x), 1, None, sh) == _lib.FA_E_ARG
    assert L.fa_csr_row_max(-1, p(ip), p(ix), None, p(ip), 8, p(ip), sh) == _lib.FA_E_ARG
    assert L.fa_csr_row_max(2, None, p(ix), None, p(ip), 8, p(ip), sh) == _lib.FA_E_ARG
    assert L.fa_cheb_step6(-1, p(x), p(x), None, 0.0, 1.0, p(x), p(x), sh) == _lib.FA_E_ARG
    assert L.fa_cheb_step6(2, None, p(x), None, 0.0, 1.0, p(x), p(x), sh) == _lib.FA_E_ARG
    # fa_cheb_step itself keeps refusing more than 3 dofs per node
    for bs in (4, 6):
        assert L.fa_cheb_step(2, bs, p(x), p(x), None, 0.0, 1.0, p(x), p(x), sh) == _lib.FA_E_UNSUPPORTED
    assert L.fa_version() >= 109
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all()) and bool((ip == 0).all())


@pytest.mark.parametrize("r,k,c", PRODUCT_SHAPES)
def test_bcsr_product_matches_scipy(dev, r, k, c):
    """Lists of 0, 1, 63, 64, 65 and 200 products per output block in one call (both sides of the 64 lanes
    of a wave, and a list several strides long), against scipy's block product of the list written out as two
    matrices, per row relative to sum |X| |Y|. A second call with short lists only takes the quarter-wave
    kernel (at most 8 products per block on average)."""
    from femasm import _lib

    rng = np.random.default_rng(r * 100 + k * 10 + c)
    nx, ny = 50, 40
    X, Y = rng.standard_normal((nx, r, k)), rng.standard_normal((ny, k, c))
    for counts in ([0, 1, 63, 64, 65, 200] * 3, [0, 1, 2, 5, 9, 3, 0, 7] * 9):
        counts = np.array(counts)
        nout, nprod = len(counts), int(counts.sum())
        optr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        xa, yb = rng.integers(0, nx, nprod), rng.integers(0, ny, nprod)
        left = sps.bsr_matrix((X[xa], np.arange(nprod), optr), shape=(nout * r, nprod * k))
        right = sps.bsr_matrix((Y[yb], np.zeros(nprod, np.int64), np.arange(nprod + 1)), shape=(nprod * k, c))
        ref = (left @ right).toarray().reshape(nout, r, c)
        mag = (abs(left) @ abs(right)).toarray().reshape(nout, r, c)
        args = [_dev(a, dev, t) for a, t in ((optr, torch.int64), (xa, torch.int32), (yb, torch.int32),
                                             (X, torch.float64), (Y, torch.float64))]
        outs = []
        for _ in range(2):
            out = torch.full((nout, r, c), float("nan"), dtype=torch.float64, device=dev)
            _lib.check(_lib.load().fa_bcsr_product(nout, r, k, c, args[0].data_ptr(), nprod, args[1].data_ptr(),
                                                   args[2].data_ptr(), args[3].data_ptr(), nx, args[4].data_ptr(), ny,
                                                   out.data_ptr(), _lib.stream_handle(dev)), "fa_bcsr_product")
            outs.append(out)
        assert torch.equal(outs[0], outs[1])  # bit-identical
        err = np.abs(_np(outs[0]) - ref)
        assert np.isfinite(err).all()
        assert (err.max(axis=2) <= 1e-14 * mag.max(axis=2)).all(), float((err.max(2) / np.maximum(mag.max(2), 1e-300)).max())
        assert (_np(outs[0])[counts == 0] == 0.0).all()


def test_cheb_step6_matches_torch(dev):
    from femasm import mg

    bs = 6
    g = torch.Generator().manual_seed(11 + bs)
    nn = 1037  # several workgroups, not a multiple of the block
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(dev)
    Dinv, b, Ax, d0, x0 = rnd(nn, bs, bs), rnd(nn * bs), rnd(nn * bs), rnd(nn * bs), rnd(nn * bs)
    absmv = lambda v: torch.bmm(Dinv.abs(), v.view(-1, bs, 1)).reshape(-1)
    for c_d, c_r, use_Ax in ((0.37, -1.3, True), (0.0, 0.8, True), (0.21, 0.6, False)):
        res = b - Ax if use_Ax else b
        d_ref = c_d * d0 + c_r * torch.bmm(Dinv, res.view(-1, bs, 1)).reshape(-1)
        x_ref = x0 + d_ref
        d = torch.full_like(d0, float("nan")) if c_d == 0.0 else d0.clone()  # c_d == 0 must not read d
        x = x0.clone()
        mg.cheb_step(Dinv, b, Ax if use_Ax else None, c_d, c_r, d, x)
        mag = abs(c_d) * d0.abs() + abs(c_r) * absmv(b.abs() + (Ax.abs() if use_Ax else 0))
        assert bool((torch.abs(d - d_ref) <= 1e-14 * mag).all()), float(torch.abs(d - d_ref).max())
        assert bool((torch.abs(x - x_ref) <= 1e-14 * (mag + x0.abs())).all())


def test_row_max_matches_torch(dev, oracle):
    """The fan (a row of 71 entries) and a graph with empty rows, with and without the free mask; the device
    aggregation equals the host one."""
    from femasm import amg

    m = IM.fan(70)
    ip, ix = oracle.sparsity(m.cells.numpy(), m.num_vertices)
    assert int(np.diff(ip).max()) == 71
    graphs = [(torch.tensor(ip), torch.tensor(ix)),
              (torch.tensor([0, 2, 2, 5, 6, 6]), torch.tensor([1, 3, 0, 1, 2, 3], dtype=torch.int32))]
    g = torch.Generator().manual_seed(5)
    for indptr, indices in graphs:
        n = indptr.numel() - 1
        v = torch.randint(-2 ** 62, 2 ** 62, (n,), generator=g)
        free = (torch.rand(n, generator=g) < 0.7).to(torch.int8)
        for f in (None, free):
            ref = amg.csr_row_max(indptr, indices, v, f)
            got = amg.csr_row_max(indptr.to(dev), indices.to(dev), v.to(dev), None if f is None else f.to(dev))
            assert torch.equal(got.cpu(), ref)
        a_h, n_h = amg.aggregate(indptr, indices, free)
        a_d, n_d = amg.aggregate(indptr.to(dev), indices.to(dev), free.to(dev))
        assert n_h == n_d and torch.equal(a_d.cpu(), a_h)


# ------------------------------------------------------------------------------------ 2. Galerkin on the device
def _problem(oracle, dev, name, p, single_component=True):
    from femasm import fem

    m = {"square2": lambda: _square(dev, 2), "square3": lambda: _square(dev, 3), "delaunay": lambda: IM.delaunay_tets_n4(dev),
         "box3": lambda: _box(dev, 3), "box8": lambda: _box(dev, 8)}[name]()
    assert m.structured is None and m.parent is None
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    a = fem.LinearElasticity(V, E=_cell_E(oracle, m), nu=0.3)
    return m, V, a, _bcs(V, comps_right=[0] if single_component else None)


def _p1_level(M):
    return M._levels[[L.degree for L in M._levels].index(1)]


@pytest.mark.parametrize("name,p,coarse_dofs,algebraic", [("square2", 1, 60, 2), ("delaunay", 1, 60, 1), ("box3", 2, 60, 1)])
def test_device_galerkin_equals_the_reference(oracle, dev, name, p, coarse_dofs, algebraic):
    """Every algebraic level's A_c against the reference's P^T A P (+ the unit diagonals), per row at 1e-12,
    and the aggregates node for node. The reference smooths its prolongators with the device's lambda_max
    estimates: the two hierarchies are then the same operator up to rounding."""
    from femasm import fem, mg

    m, V, a, bcs = _problem(oracle, dev, name, p)
    M = mg.SmoothedAggregation(a, bcs, coarse_dofs=coarse_dofs)
    M.update()
    assert M.updates == 1 and M.rebuilds == 1
    L1 = _p1_level(M)
    lv = M.levels
    assert [l[0] for l in lv] == ([2] if p == 2 else []) + [1] + [0] * algebraic and all(l[1] is None for l in lv)
    assert lv[0][2:] == (V.num_dofs, "matrix-free") and lv[-1][3] == "direct" and lv[-1][2] <= coarse_dofs < lv[-2][2]
    assert all(l[3] == "galerkin" for l in lv[1 + (p == 2):-1])
    trs = M.transfers
    assert len(trs) == algebraic
    marker1 = None if L1.marker is None else _np(L1.marker)
    assert marker1 is not None and 0 < (marker1.reshape(-1, m.gdim).sum(1) == 1).sum()  # a single-component constraint
    A1 = sps.csr_matrix(L1.entries.to_scipy())
    i1 = M._levels.index(L1)
    ref = R.hierarchy(A1, _np(L1.x), marker1, m.gdim, coarse_dofs, lmax=[L.lmax for L in M._levels[i1:-1]])
    assert len(ref) == algebraic + 1
    for k, tr in enumerate(trs):
        assert np.array_equal(_np(tr.agg), ref[k].agg), k
        rel = R.row_rel_error(tr.Ac.to_scipy(), ref[k + 1].A)
        relP = R.row_rel_error(tr.P.to_scipy(), ref[k].P)
        print(f"{name} P{p} level {k}: {tr.n} -> {tr.nagg} nodes, A_c per-row error {rel:.3e}, P {relP:.3e}, "
              f"lists (median, max) A.P {tr.AP.list_stats()} Pt.Y {tr.PtY.list_stats()}")
        assert relP <= 1e-12 and rel <= 1e-12
    assert 1.0 < M.operator_complexity < 2.0
    # the numeric products are bit-identical run to run ...
    for tr, L in zip(trs, M._levels[i1:]):
        first = tr.galerkin(L.entries).data.clone()
        assert torch.equal(tr.galerkin(L.entries).data, first)
    # ... and a second update() rebuilds nothing: the prolongators keep their bits, and so do the coarse
    # matrices whenever the re-assembled degree-1 matrix does (the default assembly sums with FP64 atomics,
    # whose order is not fixed)
    before = [tr.Ac.data.clone() for tr in trs]
    Pbefore = [tr.P.data.clone() for tr in trs]
    A1before = L1.entries.data.clone()
    M.update()
    assert M.updates == 2 and M.rebuilds == 1
    assert all(torch.equal(b, tr.P.data) for b, tr in zip(Pbefore, trs))
    same = torch.equal(A1before, L1.entries.data)
    print(f"{name} P{p}: re-assembled degree-1 matrix bitwise equal: {same}")
    if same:
        assert all(torch.equal(b, tr.Ac.data) for b, tr in zip(before, trs))


# ------------------------------------------------------------------------------------ 3. V-cycle
@pytest.mark.parametrize("name,p,coarse_dofs", [("square2", 2, 60), ("box3", 1, 30), ("delaunay", 1, 60)])
def test_vcycle_is_symmetric_positive_definite(oracle, dev, name, p, coarse_dofs):
    """Mixed bcs: x = 0 clamped, x = 1 constrained in its first component only. Two freshly built
    preconditioners give bitwise equal results from the same matrix entries: at degree 1 they share one
    assembled matrix; at degree 2 each assembles its own degree-1 level, with FP64 atomics in no fixed order,
    so there the comparison is made when the two matrices came out bitwise equal."""
    from femasm import fem, mg

    diagonal = 2.0
    m, V, a, bcs = _problem(oracle, dev, name, p)
    A = fem.assemble_matrix(a, bcs=bcs, diagonal=diagonal) if p == 1 else None
    g = torch.Generator().manual_seed(3)
    r1, r2 = (torch.randn(V.num_dofs, generator=g, dtype=torch.float64).to(dev) for _ in range(2))
    zs, entries = [], []
    for _ in range(2):
        M = mg.SmoothedAggregation(a, bcs, diagonal=diagonal, fine_operator=A, coarse_dofs=coarse_dofs)
        M.update()
        zs.append((M.apply(r1).clone(), M.apply(r2, torch.empty_like(r2))))
        entries.append(_p1_level(M).entries.data.clone())
    (z1, z2), (y1, y2) = zs
    same = torch.equal(entries[0], entries[1])
    print(f"{name} P{p}: degree-1 matrices of the two preconditioners bitwise equal: {same}")
    assert same or p == 2
    if same:
        assert torch.equal(z1, y1) and torch.equal(z2, y2)  # bit-identical
    z1, z2 = y1, y2  # (M is the second preconditioner from here on)
    assert len(M.levels) >= 2 + (p == 2) and M.levels[-1][3] == "direct"
    asym = abs(float(torch.dot(z1, r2) - torch.dot(r1, z2))) / float(z1.norm() * r2.norm())
    print(f"{name} P{p}: V-cycle asymmetry {asym:.3e} ({M.levels})")
    assert asym <= 1e-8
    assert float(torch.dot(z1, r1)) > 0 and float(torch.dot(z2, r2)) > 0
    marker, _ = fem._combine_bcs(V, bcs, with_g=False)
    on = marker != 0
    assert int(on.sum()) > 0
    assert torch.equal(z1[on], r1[on] / diagonal)
    torch.cuda.synchronize()
    n0 = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    M.apply(r1, z2)
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == n0
    assert torch.equal(z2, z1)


# ------------------------------------------------------------------------------------ 4. PCG
RTOL = 1e-12


def _solve_pair(oracle, dev, name, p, coarse_dofs):
    """Linear elasticity, E per tag / per cell, x = 0 clamped, x = 1 prescribed, body force along y:
    block-Jacobi PCG, AMG PCG, and the reference implementation's PCG on the same matrices (CPU)."""
    from femasm import fem, mesh, mg, nls

    m, V, a0, _ = _problem(oracle, dev, name, p)
    u = fem.Function(V)
    f = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
    f[1::m.gdim] = -1e3
    a = fem.LinearElasticity(V, E=a0.E, nu=0.3, u=u, f=f)
    bcs = _bcs(V)
    problem = nls.NonlinearProblem(a, u, bcs, matrix_free=False)
    b = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
    problem.F(u.x, b)
    A = problem.matrix()
    problem.J(u.x, A)
    out = []
    for use_mg in (False, True):
        ks = nls.KrylovSolver(rtol=RTOL, max_it=20000)
        if use_mg:
            M = mg.SmoothedAggregation(a, bcs, fine_operator=A, coarse_dofs=coarse_dofs)
            ks.set_preconditioner(M)
        ks.set_operator(A)
        x = torch.zeros_like(b)
        out.append((ks.solve(x, b), x))
    # the reference, from the same matrices
    marker = _np(fem._combine_bcs(V, bcs, with_g=False)[0])
    L1 = _p1_level(M)
    A1 = sps.csr_matrix(L1.entries.to_scipy())
    fine = None
    if p == 2:
        ev = _np(mesh.entities(m, 1)[0])
        fine = (sps.csr_matrix(A.to_scipy()), marker, R.edge_prolongation(ev, m.num_vertices, m.gdim))
    Mref, ref_levels = R.preconditioner(A1, _np(L1.x), _np(L1.marker), m.gdim, coarse_dofs, fine=fine)
    its_ref, x_ref = R.pcg(sps.csr_matrix(A.to_scipy()), _np(b), Mref, RTOL)
    return out, (its_ref, x_ref, ref_levels), M


@pytest.mark.parametrize("name,p,coarse_dofs,min_algebraic", [("square3", 1, 300, 2), ("square2", 2, 300, 1), ("box8", 1, 300, 1)])
def test_amg_pcg_matches_jacobi_pcg_and_the_reference_count(oracle, dev, name, p, coarse_dofs, min_algebraic):
    """Both solvers stop at rtol 1e-12 on their preconditioned residual; the error left is at most rtol times
    the condition number of the preconditioned operator. For block-Jacobi that is about 32 / (pi h)^2 for the
    Laplacian with one clamped side, times the spread of E (2.7 between the two tags of square.msh, 20 per cell
    in the box) and a factor of about 3 for elasticity at nu = 0.3: 1e5 on square.msh at h = 1 / 56 (P1 refined
    three times, or P2 refined twice: the same nodes), 1.2e4 on the 8^3 box; a degree-2 basis adds less than a
    factor of 10. So the solutions agree to 1e-6 (= rtol x 1e6) in every case.

    The iteration count is below block-Jacobi's and at most the reference implementation's on the same
    matrices plus a quarter of it (at least plus 3): the two hierarchies differ in the lambda_max estimate
    only (10 seeded Lanczos steps here, the reference's own eigenvalue there)."""
    ((its_j, x_j), (its_mg, x_mg)), (its_ref, x_ref, ref_levels), M = _solve_pair(oracle, dev, name, p, coarse_dofs)
    rel = float((x_mg - x_j).norm() / x_j.norm())
    rel_ref = float(np.linalg.norm(_np(x_mg) - x_ref) / np.linalg.norm(x_ref))
    print(f"{name} P{p}: block-Jacobi {its_j} its, AMG {its_mg} its, reference {its_ref} its; solutions differ by "
          f"{rel:.3e} (reference {rel_ref:.3e}); levels {M.levels}, operator complexity {M.operator_complexity:.3f}")
    assert len(M.transfers) >= min_algebraic and len(ref_levels) == len(M.levels)
    assert [L.A.shape[0] for L in ref_levels] == [l[2] for l in M.levels]
    assert rel <= 1e-6 and rel_ref <= 1e-6
    assert its_mg < its_j
    assert its_mg <= its_ref + max(its_ref / 4.0, 3.0)


# ------------------------------------------------------------------------------------ 5. Newton
@pytest.mark.parametrize("kind", ["damage-p1-triangles", "neo-p2-tetrahedra"])
def test_newton_with_amg_matches_newton(oracle, dev, kind):
    """AsymDamage on P1 triangles (square.msh refined twice, parents dropped, E per tag, damage 0.5 on the nodes
    of the cells of tag 2; assembled mode: the problem's matrix is the resident degree-1 matrix) and NeoHookean
    on P2 tetrahedra (the parentless 3^3 box, matrix-free) against Newton with block-Jacobi."""
    from femasm import fem, mg, nls

    results = []
    for use_mg in (False, True):
        if kind == "damage-p1-triangles":
            m = _square(dev, 2)
            V = fem.functionspace(m, ("Lagrange", 1, (2,)))
            coarse_dofs, disp, matrix_free = 100, 1e-3, False
        else:
            m = _box(dev, 3)
            V = fem.functionspace(m, ("Lagrange", 2, (3,)))
            coarse_dofs, disp, matrix_free = 60, 0.05, True
        E = _cell_E(oracle, m)
        u = fem.Function(V)
        f = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
        f[1::m.gdim] = -1e3
        if kind == "damage-p1-triangles":
            d = torch.zeros(V.num_nodes, dtype=torch.float64, device=dev)
            d[m.cells[m.cell_tags == 2].to(torch.int64).reshape(-1)] = 0.5
            assert 0 < int((d > 0).sum()) < V.num_nodes
            form = fem.AsymDamage(V, E=E, nu=0.3, u=u, d=d, f=f)
        else:
            form = fem.NeoHookean(V, E=E, nu=0.3, u=u, f=f)
        bcs = _bcs(V, disp=disp)
        problem = nls.NonlinearProblem(form, u, bcs, matrix_free=matrix_free and use_mg)
        solver = nls.NewtonSolver(None, problem)
        solver.rtol, solver.atol, solver.max_it = 1e-7, 5e-8, 10
        M = None
        if use_mg:
            M = mg.SmoothedAggregation(form, bcs, fine_operator=problem.matrix(), coarse_dofs=coarse_dofs)
            solver.krylov_solver.set_preconditioner(M)
        it, conv = solver.solve(u)
        assert conv
        results.append((it, u.x.clone(), solver.krylov_iterations, M))
    (it0, u0, k0, _), (it1, u1, k1, M) = results
    print(f"{kind}: Newton {it0} / {it1} steps, Krylov iterations block-Jacobi {k0}, AMG {k1} ({M.levels})")
    assert len(M.transfers) >= 1 and M.levels[-1][3] == "direct"
    assert M.levels[0][3] == ("matrix-free" if kind == "neo-p2-tetrahedra" else "operator")
    assert float((u1 - u0).norm() / u0.norm()) <= 1e-8
    assert abs(it1 - it0) <= 1
    assert M.rebuilds == 1 and M.updates == it1  # prolongators frozen: one update per Newton step
    assert k1 < k0
    # re-smoothing the prolongators at the converged state, and the solve from zero again
    M.update(rebuild=True)
    assert M.rebuilds == 2 and M.updates == it1 + 1
    u.x.zero_()
    it2, conv2 = solver.solve(u)
    assert conv2 and M.rebuilds == 2 and M.updates == it1 + 1 + it2
    assert float((u.x - u0).norm() / u0.norm()) <= 1e-8
