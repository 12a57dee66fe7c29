"""fem.damage_field on the GPU: fa_vertex_spread against the sequential restatement of the definition
(damage_reference.py), bit for bit. The meshes are the smallest at which the ping-pong parity (iterations 0,
1, 8), the gate (thresholds 0.01, 0, inf), the row bounds (degrees 0 .. 300) and the tail workgroup (62, 221
and 289 = 256 + 33 vertices) can go wrong."""
import ctypes

import numpy as np
import pytest
import torch

import damage_cases as C

pytestmark = pytest.mark.gpu
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _dev_start(name, dev):
    return torch.tensor(np.asarray(C.start(name)), dtype=torch.float64, device=dev)


@pytest.mark.parametrize("name", C.MESHES)
def test_spread_equals_sequential_reference(dev, name):
    from femasm import fem

    m = C.make(name, dev)
    d0 = _dev_start(name, dev)
    for iterations in C.ITERATIONS:
        for threshold in C.THRESHOLDS:
            d = fem.spread(m, d0, iterations, threshold)
            assert d.device.type == "cuda" and d.dtype == torch.float64
            ref = torch.tensor(np.asarray(C.reference(name, iterations, threshold)))
            assert torch.equal(d.cpu(), ref), (name, iterations, threshold)


@pytest.mark.parametrize("refine", [0, 1])
def test_damage_field_equals_sequential_reference(dev, refine):
    from femasm import fem

    m, t = C.square(dev, refine)
    name = "square_r1" if refine else "square"
    d = fem.damage_field(fem.functionspace(m, ("Lagrange", 1)), tags=t, values=[C.TAG])
    assert m.num_vertices == (221 if refine else 62)
    ref = torch.tensor(np.asarray(C.reference(name, 8 * (refine + 1))))
    assert torch.equal(d.x.cpu(), ref)


@pytest.mark.parametrize("name", ["unit16", "fan300"])
def test_deterministic_and_start_field_untouched(dev, name):
    from femasm import fem

    m = C.make(name, dev)
    d0 = _dev_start(name, dev)
    keep = d0.clone()
    a = fem.spread(m, d0, 8)
    b = fem.spread(m, d0, 8)
    assert torch.equal(a, b)
    assert torch.equal(d0, keep)
    assert a.data_ptr() != d0.data_ptr()
    assert fem.spread(m, d0, 0).data_ptr() != d0.data_ptr()


@pytest.mark.parametrize("name", C.MESHES)
def test_device_equals_host_path(dev, name):
    from femasm import fem, mesh

    m = C.make(name, dev)
    host = m.to("cpu")
    for a, b in zip(mesh.vertex_graph(m), mesh.vertex_graph(host)):
        assert a.device.type == "cuda" and torch.equal(a.cpu(), b)
    d0 = _dev_start(name, dev)
    for threshold in C.THRESHOLDS:
        assert torch.equal(fem.spread(m, d0, 8, threshold).cpu(), fem.spread(host, d0.cpu(), 8, threshold))


def test_assembly_with_the_damage_field(dev):
    """End to end on P1 triangles: the damage law assembled with fem.damage_field's d equals, value for value,
    the assembly given the sequential reference's d, and differs from the d = 0 matrix.

    Value for value means two things here, because the default gather of a damage form adds a block's cell
    contributions with LDS FP64 atomics in no fixed order ("Reproducibility"; only
    linear forms have FA_DETERMINISTIC), so two assemblies of the SAME inputs differ in their last bits:
    torch.equal(A.data, A_ref.data) failed on the MI355X with every test of d itself passing. (1) What the
    assembly sums, the element matrices of every cell (fa_tabulate_cells: per cell, no sum across cells), is
    bitwise equal. (2) Every assembled value agrees up to the order of its adds and no further: a value is the
    sum of the n element entries t_c of the cells that share the node pair, any order of n floating-point adds
    is within g(n) * sum |t_c| of the exact sum, g(n) = (n - 1) u / (1 - (n - 1) u), u = 2^-53, so two orders
    are within 2 g(n) sum |t_c| of each other, and an entry with one contribution is bitwise equal. On
    square.msh n <= 7."""
    from femasm import fem

    m, t = C.square(dev)
    V = fem.functionspace(m, ("Lagrange", 1, (2,)))
    S = fem.functionspace(m, ("Lagrange", 1))
    g = torch.Generator().manual_seed(5)  # the small random state of the damage tests (test_gpu_damage_ad._state)
    u = (1e-3 * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).to(dev)
    E = torch.full((m.num_cells,), 1000.0, dtype=torch.float64, device=dev)
    d = fem.damage_field(S, tags=t, values=[C.TAG])
    d_ref = torch.tensor(np.asarray(C.reference("square", 8)), device=dev)
    forms = [fem.AsymDamage(V, E=E, nu=0.3, u=u, d=x) for x in (d, d_ref, torch.zeros_like(d_ref))]
    assert torch.equal(forms[0].d, forms[1].d)
    K, K_ref, K_zero = (fem.tabulate_cells(a) for a in forms)
    assert bool(torch.isfinite(K).all())
    assert torch.equal(K, K_ref)
    assert not torch.equal(K, K_zero)
    A, A_ref, A_zero = (fem.assemble_matrix(a) for a in forms)
    assert torch.equal(A.indices, A_ref.indices) and torch.equal(A.indptr, A_ref.indptr)
    # sum |t_c| and n per entry of the dense matrix, from the element matrices and the dofmap
    dofs = (V.dofmap.cpu().to(torch.int64)[:, :, None] * 2 + torch.arange(2)).reshape(m.num_cells, -1)  # [nc, 6]
    flat = (dofs[:, :, None] * V.num_dofs + dofs[:, None, :]).reshape(-1)
    mag = torch.zeros(V.num_dofs ** 2, dtype=torch.float64).index_add_(0, flat, K.cpu().abs().reshape(-1))
    cnt = torch.zeros(V.num_dofs ** 2, dtype=torch.float64).index_add_(0, flat, torch.ones(flat.numel(), dtype=torch.float64))
    assert int(cnt.max()) <= 7
    un = 2.0 ** -53 * (cnt - 1).clamp(min=0)
    bound = (2 * un / (1 - un) * mag * (1 + 2.0 ** -20)).reshape(V.num_dofs, V.num_dofs).numpy()
    D, D_ref, D_zero = A.to_dense(), A_ref.to_dense(), A_zero.to_dense()
    diff = np.abs(D - D_ref)
    print(f"assembly vs assembly with the reference d: {np.count_nonzero(diff)} of {np.count_nonzero(D)} values "
          f"differ, worst diff / bound {np.max(diff / np.where(bound > 0, bound, 1.0)):.3f}, "
          f"max |diff| / max |A| {diff.max() / np.abs(D).max():.3e}")
    assert np.isfinite(D).all()
    assert (diff <= bound).all()
    assert (np.abs(D - D_zero) > bound).any() and not torch.equal(A.data, A_zero.data)


def test_abi_argument_errors(dev):
    """Rejected on the host, before anything is launched."""
    from femasm import _lib, mesh

    L = _lib.load()
    assert L.fa_version() >= 110
    m = C.make("square", dev)
    indptr, indices, inv_deg = mesh._vertex_graph(m)
    nv = m.num_vertices
    d = torch.zeros(nv, dtype=torch.float64, device=dev)
    tmp = torch.empty_like(d)
    sh = _lib.stream_handle(dev)
    args = lambda n, dp, it: (n, indptr.data_ptr(), indices.data_ptr(), inv_deg.data_ptr(), dp, tmp.data_ptr(), it,
                              0.01, sh)
    assert L.fa_vertex_spread(*args(nv, d.data_ptr(), -1)) == _lib.FA_E_ARG
    assert b"iterations" in L.fa_last_error()
    assert L.fa_vertex_spread(*args(nv, None, 1)) == _lib.FA_E_ARG
    assert b"null" in L.fa_last_error()
    assert L.fa_vertex_spread(*args(-1, d.data_ptr(), 1)) == _lib.FA_E_ARG
    assert L.fa_vertex_spread(*args(2 ** 31, d.data_ptr(), 1)) == _lib.FA_E_CAPACITY
    assert L.fa_vertex_spread(*args(0, d.data_ptr(), 1)) == 0
    assert L.fa_vertex_spread(*args(nv, d.data_ptr(), 0)) == 0
    torch.cuda.synchronize()
    assert bool((d == 0).all())
