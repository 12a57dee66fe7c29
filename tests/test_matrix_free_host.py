"""Host-side checks of the matrix-free Jacobian action (no GPU): the C ABI's new entry points, their
argument checks (made before any device call) and fem.JacobianOperator's / nls.NonlinearProblem's
host logic on a CPU mesh."""
import ctypes
import os

import pytest
import torch


@pytest.fixture(scope="module")
def L():
    from femasm import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libfemasm.so not built (run __graft_entry__.build())")
    return _lib.load()


def test_version_and_symbols(L):
    from femasm import _lib

    assert L.fa_version() >= 102
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("fa_apply_jacobian", "fa_jacobian_block_diag", "fa_apply_plan_bytes", "fa_apply_plan"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES


def _space():
    from femasm import fem, mesh

    m = mesh.create_unit_square(2, 2)  # CPU tensors
    V = fem.functionspace(m, ("Lagrange", 1, (2,)))
    return m, V


def test_null_arguments_are_refused_before_any_device_call(L):
    from femasm import _lib, fem

    m, V = _space()
    a = fem.LinearElasticity(V, E=1.0, nu=0.3)
    fm, ff = V._fa_mesh(), fem._fa_form(a)
    adj = _lib.fa_adjacency()  # null ptr / idx
    x = torch.zeros(V.num_dofs, dtype=torch.float64)
    y = torch.zeros(V.num_dofs, dtype=torch.float64)
    calls = [
        lambda: L.fa_apply_jacobian(None, ctypes.byref(ff), ctypes.byref(adj), None, None, 1.0, x.data_ptr(), y.data_ptr(), None),
        lambda: L.fa_apply_jacobian(ctypes.byref(fm), None, ctypes.byref(adj), None, None, 1.0, x.data_ptr(), y.data_ptr(), None),
        lambda: L.fa_apply_jacobian(ctypes.byref(fm), ctypes.byref(ff), None, None, None, 1.0, x.data_ptr(), y.data_ptr(), None),
        lambda: L.fa_apply_jacobian(ctypes.byref(fm), ctypes.byref(ff), ctypes.byref(adj), None, None, 1.0, x.data_ptr(), y.data_ptr(), None),
        lambda: L.fa_jacobian_block_diag(None, ctypes.byref(ff), ctypes.byref(adj), None, 1.0, y.data_ptr(), None),
        lambda: L.fa_jacobian_block_diag(ctypes.byref(fm), None, ctypes.byref(adj), None, 1.0, y.data_ptr(), None),
        lambda: L.fa_jacobian_block_diag(ctypes.byref(fm), ctypes.byref(ff), None, None, 1.0, y.data_ptr(), None),
        lambda: L.fa_apply_plan_bytes(None, None, None, None, None),
        lambda: L.fa_apply_plan(None, None, None, 0, None),
    ]
    for call in calls:
        assert call() == _lib.FA_E_ARG
        assert L.fa_last_error() not in (None, b"")
    # null x / y and aliased x, y with an otherwise complete argument list (the pointers are never read)
    adj.ptr, adj.idx = x.data_ptr(), x.data_ptr()
    full = (ctypes.byref(fm), ctypes.byref(ff), ctypes.byref(adj), None, None, 1.0)
    assert L.fa_apply_jacobian(*full, None, y.data_ptr(), None) == _lib.FA_E_ARG
    assert L.fa_apply_jacobian(*full, x.data_ptr(), None, None) == _lib.FA_E_ARG
    assert L.fa_apply_jacobian(*full, x.data_ptr(), x.data_ptr(), None) == _lib.FA_E_ARG
    assert b"alias" in L.fa_last_error()
    assert L.fa_apply_jacobian(*full, x.data_ptr(), x.data_ptr() + 8, None) == _lib.FA_E_ARG  # overlapping
    assert L.fa_jacobian_block_diag(ctypes.byref(fm), ctypes.byref(ff), ctypes.byref(adj), None, 1.0, None, None) == _lib.FA_E_ARG


def test_operator_validates_vectors_on_the_host(L):
    from femasm import fem

    m, V = _space()
    a = fem.LinearElasticity(V, E=1.0, nu=0.3)
    op = fem.JacobianOperator(a, bcs=None, diagonal=2.5)
    assert op.bs == 2
    assert op.shape == (V.num_dofs, V.num_dofs)
    n = V.num_dofs
    good = torch.zeros(n, dtype=torch.float64)
    with pytest.raises(ValueError, match="entries"):
        op.mult(torch.zeros(n + 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        op.mult(torch.zeros(n, dtype=torch.float32))
    with pytest.raises(ValueError, match="contiguous"):
        op.mult(torch.zeros(2 * n, dtype=torch.float64)[::2])
    with pytest.raises(ValueError, match="entries"):
        op.mult(good, torch.zeros(n - 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="alias"):
        op.mult(good, good)
    with pytest.raises(ValueError, match="method"):
        fem.JacobianOperator(a, method="fast")
    with pytest.raises(TypeError):
        fem.JacobianOperator(object())


def test_nonlinear_problem_default_keeps_the_matrix_path(monkeypatch):
    from femasm import fem, nls
    from femasm.la import MatrixCSR

    m, V = _space()
    u = fem.Function(V)
    a = fem.LinearElasticity(V, E=1.0, nu=0.3, u=u)
    p = nls.NonlinearProblem(a, u, [])
    assert p.matrix_free is False
    # the pattern is built on the device: stand in a diagonal host pattern so that matrix() runs here
    pattern = (torch.arange(V.num_nodes + 1, dtype=torch.int64), torch.arange(V.num_nodes, dtype=torch.int32))
    monkeypatch.setattr(fem, "sparsity_pattern", lambda W: pattern)
    A = p.matrix()
    assert isinstance(A, MatrixCSR) and not isinstance(A, fem.JacobianOperator)
    assert A.bs == 2 and A.shape == (V.num_dofs, V.num_dofs)
    pm = nls.NonlinearProblem(a, u, [], matrix_free=True)
    assert pm.matrix_free is True
    assert isinstance(pm.matrix(), fem.JacobianOperator) and pm.matrix() is pm.matrix()
    pm.J(u.x, pm.matrix())  # nothing to assemble: no library call
