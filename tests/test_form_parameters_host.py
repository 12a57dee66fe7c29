"""The CPU oracle at the Poisson ratios and quadrature degrees of tests/form_parameters.py, so that a
failure of tests/test_gpu_form_parameters.py points at the device kernel and not at its reference.

For every element and Poisson ratio, at the default rule and at every degree of QDEG,
oracle.assemble_elasticity without bcs must be finite, symmetric to 1e-13 max|A|, and annihilate every
translation t per scalar row: |A t|_i <= 1e-12 (|A| |t|)_i (the rows of a stiffness matrix sum to zero
per component, whatever the rule integrates exactly). Also the oracle's guard: a rule with more points
than its static arrays hold (ORA_MAXQ) is an error, never an overrun."""
import numpy as np
import pytest
import torch

import form_parameters as FP

_cache = {}


def host_mesh(ct, n, perturb=0.0):
    from femasm import mesh

    m = mesh.create_unit_square(*n, cell_type=ct) if len(n) == 2 else mesh.create_unit_cube(*n, cell_type=ct)
    if perturb:  # as tests/test_gpu_parity._mesh: interior vertices moved by perturb * h
        g = torch.Generator().manual_seed(3)
        x = m.x.clone()
        interior = ((x > 1e-9) & (x < 1 - 1e-9)).all(1)
        x[interior] += perturb / max(n) * (torch.rand(x[interior].shape, generator=g, dtype=torch.float64) - 0.5)
        m.x = x
    return m


def _case(oracle, elem, perturb):
    key = (elem, perturb)
    if key not in _cache:
        from femasm import fem

        ct, p, n = FP.ELEMENTS[elem]
        m = host_mesh(ct, n, perturb)
        V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
        cells = V.dofmap.numpy()
        ip, ix = oracle.sparsity(cells, V.num_nodes)
        E = oracle.e_range()[np.arange(m.num_cells) % 200]
        _cache[key] = (ct, p, m.gdim, cells, m.cells.numpy(), m.x.numpy(), ip, ix, E, V.num_nodes)
    return _cache[key]


def _check(oracle, elem, perturb, nu, qdeg):
    ct, p, gd, cells, geom, x, ip, ix, E, nnodes = _case(oracle, elem, perturb)
    lam, mu = oracle.lame(E, nu)
    assert np.isfinite(lam).all() and np.isfinite(mu).all()
    vals = oracle.assemble_elasticity(ct, p, cells, geom, x, lam, mu, ip, ix, qdeg=qdeg)
    assert np.isfinite(vals).all()
    A = oracle.bsr_to_dense(ip, ix, vals, nnodes)
    amax = np.abs(A).max()
    assert amax > 0
    assert np.abs(A - A.T).max() <= 1e-13 * amax
    for k in range(gd):
        t = np.zeros(nnodes * gd)
        t[k::gd] = 1.0
        assert (np.abs(A @ t) <= 1e-12 * (np.abs(A) @ np.abs(t))).all(), (elem, nu, qdeg, k)


@pytest.mark.parametrize("nu", FP.NU)
@pytest.mark.parametrize("elem,perturb", FP.MESHES)
def test_oracle_default_rule(oracle, elem, perturb, nu):
    _check(oracle, elem, perturb, nu, -1)


@pytest.mark.parametrize("nu", FP.NU)
@pytest.mark.parametrize("elem,qdeg", FP.QDEG_CASES)
def test_oracle_other_rules(oracle, elem, qdeg, nu):
    _check(oracle, elem, 0.0, nu, qdeg)


def test_tables():
    """The tables' own conditions: the thresholds are in NU with an inside neighbour each, no degree
    is an element's default, and every rule fits the oracle's arrays."""
    assert FP.NU_LO in FP.NU and FP.NU_HI in FP.NU
    assert not FP.uniform_nu(FP.NU_LO) and not FP.uniform_nu(FP.NU_HI)
    assert FP.uniform_nu(-0.9899) and FP.uniform_nu(0.4899) and not FP.uniform_nu(0.4999)
    assert set(FP.NU_SHORT) <= set(FP.NU) and all(-1.0 < nu < 0.5 for nu in FP.NU)
    assert set(FP.QDEG) == set(FP.ELEMENTS)
    for e, q in FP.QDEG_CASES + FP.NEO_QDEG:
        ct, p, _ = FP.ELEMENTS[e]
        assert q != FP.default_qdeg(ct, p), (e, q)


def test_rules_fit_the_oracle(oracle):
    for e, q in FP.QDEG_CASES + FP.NEO_QDEG:
        ct, p, _ = FP.ELEMENTS[e]
        assert len(oracle.quadrature(ct, q)[1]) <= oracle.ORA_MAXQ
    for e, (ct, p, _) in FP.ELEMENTS.items():  # the load term's rule of the residual: degree 2 p
        assert len(oracle.quadrature(ct, 2 * p)[1]) <= oracle.ORA_MAXQ


def test_oracle_refuses_a_rule_past_its_arrays(oracle):
    """Hexahedra at degree 12: 7^3 = 343 points, more than ORA_MAXQ = 256. Every entry point that builds
    a rule returns an error before it writes one."""
    ct, p, gd, cells, geom, x, ip, ix, E, nnodes = _case(oracle, "hex-Q1", 0.0)
    lam, mu = oracle.lame(E, 0.3)
    assert oracle.lib().ora_quadrature_count(ct, 12) == 343 > oracle.ORA_MAXQ
    assert oracle.lib().ora_quadrature_count(ct, 10) == 216
    u = np.zeros(nnodes * gd)
    bc = np.zeros(nnodes * gd, dtype=np.int8)
    with pytest.raises(ValueError, match="ORA_MAXQ"):
        oracle.quadrature(ct, 12)
    with pytest.raises(ValueError, match="ORA_MAXQ"):
        oracle.assemble_elasticity(ct, p, cells, geom, x, lam, mu, ip, ix, qdeg=12)
    with pytest.raises(ValueError, match="ORA_MAXQ"):
        oracle.cell_matrices_elasticity(ct, p, cells, geom, x, lam, mu, qdeg=12)
    with pytest.raises(ValueError, match="ORA_MAXQ"):
        oracle.assemble_residual(ct, p, cells, geom, x, lam, mu, u=u, qdeg=12)
    with pytest.raises(ValueError, match="ORA_MAXQ"):
        oracle.apply_lifting(ct, p, cells, geom, x, lam, mu, u, bc, u, qdeg=12)
    with pytest.raises(ValueError, match="ORA_MAXQ"):
        oracle.assemble_neohookean(ct, p, cells, geom, x, lam, mu, u, ip, ix, qdeg=12)
    # the largest rule that fits still assembles
    vals = oracle.assemble_elasticity(ct, p, cells, geom, x, lam, mu, ip, ix, qdeg=10)
    ref = oracle.assemble_elasticity(ct, p, cells, geom, x, lam, mu, ip, ix)
    assert np.abs(vals - ref).max() <= 1e-12 * np.abs(ref).max()  # (affine Q1: degree 2 is already exact)
