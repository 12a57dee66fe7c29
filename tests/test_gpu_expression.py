"""GPU: per-cell expressions (fa_eval_cells through fem.evaluate / fem.Expression /
Function.interpolate) against a numpy recipe built from existing oracle calls only.

Bar: the project's parity bar, |gpu - ref| <= 1e-12 * max |ref| over the compared quantity
(tests/test_gpu_vector.py). The recipe: gg = oracle.tabulate(ct, 1, X)[1], gs = oracle.tabulate(ct, p, X)[1],
J[c,q] = sum_v x_v (x) gg[q,v], g = gs . J^-1, grad u[c,q] = sum_a u_a (x) g[q,a]; stress in closed form
(linear), oracle.damage_stress (damage law) or oracle.neo_stress (neo-Hookean). The recipes' own
error (a linear field to <= 9e-15 on perturbed meshes of all ten families; the oracle's damage stress
within 7.2e-14 of an 80-bit restatement) leaves more than 10x margin. No cell or component is masked.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-12

FAMILIES = [(3, 1, (6, 5)), (3, 2, (4, 3)), (4, 1, (4, 3)), (4, 2, (3, 3)), (4, 3, (2, 2)), (-4, 1, (2, 3, 2)),
            (-4, 2, (2, 2, 2)), (8, 1, (2, 2, 2)), (8, 2, (2, 1, 2)), (8, 3, (1, 2, 1))]
IDS = [f"ct{ct}-p{p}" for ct, p, _ in FAMILIES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _mesh(ct, n, dev, perturb=0.3, structured=True):
    """Non-affine mesh: interior vertices moved by perturb * h * (rand - 0.5), seeded."""
    from femasm import mesh

    m = mesh.create_unit_square(*n, cell_type=ct, device=dev) if len(n) == 2 else \
        mesh.create_unit_cube(*n, cell_type=ct, device=dev)
    if perturb:
        g = torch.Generator().manual_seed(3)
        x = m.x.cpu()
        interior = ((x > 1e-9) & (x < 1 - 1e-9)).all(1)
        h = 1.0 / max(n)
        x[interior] += perturb * h * (torch.rand(x[interior].shape, generator=g, dtype=torch.float64) - 0.5)
        m.x = x.to(dev)
    if not structured:
        m.structured = None
    return m


def _space(ct, p, n, dev):
    from femasm import fem

    m = _mesh(ct, n, dev, structured=p > 2)  # Q3 dofmaps need the lattice; degree <= 2: the generic numbering
    return m, fem.functionspace(m, ("Lagrange", p, (m.gdim,)))


def _points(oracle, ct):
    """The midpoint plus the degree-2 quadrature points: npts > 1."""
    from femasm import fem

    return np.concatenate([fem.interpolation_points(ct), oracle.quadrature(ct, 2)[0]], axis=0)


def _rand_u(V, dev, amp, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (amp * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).to(dev)


def _phys_grads(oracle, V, X):
    """g[c, q, a, j]: physical gradients of the space's basis at the points X of every cell."""
    m = V.mesh
    ct = int(m.cell_type)
    gg = oracle.tabulate(ct, 1, X)[1]
    gs = oracle.tabulate(ct, V.degree, X)[1]
    xv = _np(m.x)[_np(m.cells).astype(np.int64)]  # [c, v, i]
    J = np.einsum("cvi,qvk->cqik", xv, gg)
    return np.einsum("qak,cqkj->cqaj", gs, np.linalg.inv(J)), J


def _ref_grad(oracle, V, u, X):
    g, _ = _phys_grads(oracle, V, X)
    gd = V.mesh.gdim
    ua = _np(u).reshape(-1, gd)[_np(V.dofmap).astype(np.int64)]  # [c, a, i]
    return np.einsum("cai,cqaj->cqij", ua, g)


def _reduce(T):
    """[..., gd, gd] -> reduced [..., gd (gd + 1) / 2]: (xx, xy, yy) / (xx, xy, xz, yy, yz, zz)."""
    gd = T.shape[-1]
    return np.stack([T[..., i, j] for i in range(gd) for j in range(i, gd)], axis=-1)


def _shear_weights(gd):
    return np.array([1.0 if i == j else 2.0 for i in range(gd) for j in range(i, gd)])


def _sym(G):
    return 0.5 * (G + np.swapaxes(G, -1, -2))


def _lin_stress(eps, lam, mu):
    tr = np.trace(eps, axis1=-2, axis2=-1)
    return 2.0 * mu[:, None, None, None] * eps + (lam[:, None] * tr)[..., None, None] * np.eye(eps.shape[-1])


def _close(got, ref, what):
    got = _np(got).reshape(ref.shape) if isinstance(got, torch.Tensor) else got
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, rel {err / scale:.3e}")
    assert err <= RTOL * scale, f"{what}: rel err {err / scale:.3e}"


def _E_cells(oracle, nc, dev):
    return torch.tensor(oracle.e_range()[np.arange(nc) % 200], dtype=torch.float64, device=dev)


# ------------------------------------------------------------------------- 1. linear-field exactness
@pytest.mark.parametrize("ct,p,n", FAMILIES, ids=IDS)
def test_linear_field_is_exact(oracle, dev, ct, p, n):
    """u = A x + b at the geometry-mapped nodes: grad u = A and strain = sym(A) in every cell at
    every point (no oracle values in the reference)."""
    from femasm import fem

    m, V = _space(ct, p, n, dev)
    gd = m.gdim
    rng = np.random.default_rng(11)
    A = rng.uniform(-1.0, 1.0, (gd, gd))
    b = rng.uniform(-1.0, 1.0, gd)
    psi = oracle.tabulate(ct, 1, oracle.nodes(ct, p))[0]  # [a, v] geometry basis at the reference nodes
    xn = np.einsum("av,cvi->cai", psi, _np(m.x)[_np(m.cells).astype(np.int64)])
    u = np.zeros((V.num_nodes, gd))
    u[_np(V.dofmap).astype(np.int64).reshape(-1)] = (xn @ A.T + b).reshape(-1, gd)
    X = _points(oracle, ct)
    assert X.shape[0] > 1
    a = fem.LinearElasticity(V, E=1.0, nu=0.3, u=torch.tensor(u.reshape(-1), device=dev))
    r = fem.evaluate(a, ("grad", "strain"), X=X)
    npts = X.shape[0]
    assert r["grad"].shape == (m.num_cells, npts * gd * gd)
    assert r["strain"].shape == (m.num_cells, npts * gd * (gd + 1) // 2)
    _close(r["grad"], np.broadcast_to(A, (m.num_cells, npts, gd, gd)).copy(), "grad")
    _close(r["strain"], np.broadcast_to(_reduce(_sym(A)), (m.num_cells, npts, gd * (gd + 1) // 2)).copy(), "strain")


# --------------------------------------------------------------------- 2. strain, stress and energy
def _check_linear(oracle, dev, ct, p, n, lame):
    from femasm import fem

    m, V = _space(ct, p, n, dev)
    gd = m.gdim
    u = _rand_u(V, dev, 1e-3)
    E = _E_cells(oracle, m.num_cells, dev)
    lam, mu = oracle.lame(_np(E), 0.3)
    if lame:
        a = fem.LinearElasticity(V, lam=torch.tensor(lam, device=dev), mu=torch.tensor(mu, device=dev), u=u)
    else:
        a = fem.LinearElasticity(V, E=E, nu=0.3, u=u)
    w = _shear_weights(gd)
    for X in (None, _points(oracle, ct)):  # the DG0 point (staged stores) and several points (per-lane stores)
        Xr = fem.interpolation_points(ct) if X is None else X
        G = _ref_grad(oracle, V, u, Xr)
        eps = _sym(G)
        sig = _lin_stress(eps, lam, mu)
        r = fem.evaluate(a, ("grad", "strain", "stress", "energy"), X=X)
        _close(r["grad"], G, "grad")
        _close(r["strain"], _reduce(eps), "strain")
        _close(r["stress"], _reduce(sig), "stress")
        en = (eps * sig).sum((-1, -2))
        _close(r["energy"], en, "energy")
        # energy == eps : sigma of the GPU's own reduced tensors, shear terms counted twice
        rs = _np(r["strain"]).reshape(m.num_cells, -1, w.size)
        rt = _np(r["stress"]).reshape(m.num_cells, -1, w.size)
        _close(r["energy"], (rs * rt * w).sum(-1), "energy vs eps:sigma")


@pytest.mark.parametrize("ct,p,n", FAMILIES, ids=IDS)
def test_strain_stress_energy_match_the_recipe(oracle, dev, ct, p, n):
    """Random u of amplitude 1e-3, E = e_range[cell % 200], nu = 0.3."""
    _check_linear(oracle, dev, ct, p, n, lame=False)


def test_strain_stress_energy_with_lame_per_cell(oracle, dev):
    _check_linear(oracle, dev, -4, 2, (2, 2, 2), lame=True)


# ------------------------------------------------------------------------------------ 3. damage law
def _damage_state(oracle, dev, amp, n=(9, 7)):
    from femasm import fem

    m = _mesh(3, n, dev)
    V = fem.functionspace(m, ("Lagrange", 1, (2,)))
    u = _rand_u(V, dev, amp, seed=7)
    g = torch.Generator().manual_seed(8)
    d = 0.3 + 0.7 * torch.rand(V.num_nodes, generator=g, dtype=torch.float64)
    d[m.x[:, 0].cpu() < 0.4] = 0.0
    return m, V, u, d.to(dev), _E_cells(oracle, m.num_cells, dev)


def _damage_ref(oracle, V, u, d, lam, mu, X):
    G = _ref_grad(oracle, V, u, X)
    eps = _sym(G)
    phi = oracle.tabulate(3, 1, X)[0]  # [q, a]
    da = _np(d)[_np(V.dofmap).astype(np.int64)]  # [c, a]
    dq = np.zeros((da.shape[0], X.shape[0]))
    for a in range(3):
        dq += phi[None, :, a] * da[:, a, None]
    out = np.zeros(dq.shape + (3,))
    for c in range(dq.shape[0]):
        for q in range(dq.shape[1]):
            s00, s11, s01 = oracle.damage_stress([eps[c, q, 0, 0], eps[c, q, 1, 1], eps[c, q, 0, 1]], lam[c], mu[c],
                                                 dq[c, q])
            out[c, q] = (s00, s01, s11)
    return eps, dq, out


@pytest.mark.parametrize("amp", [1e-3, 1.0])
@pytest.mark.parametrize("pts", ["midpoint", "quadrature"])
@pytest.mark.parametrize("tangent", ["hand", "ad"])
def test_damage_stress_matches_the_hand_oracle(oracle, dev, tangent, pts, amp):
    from femasm import fem

    m, V, u, d, E = _damage_state(oracle, dev, amp)
    lam, mu = oracle.lame(_np(E), 0.3)
    X = None if pts == "midpoint" else oracle.quadrature(3, 2)[0]
    Xr = fem.interpolation_points(3) if X is None else X
    assert X is None or X.shape[0] == 3
    eps, dq, sig = _damage_ref(oracle, V, u, d, lam, mu, Xr)
    undamaged, damaged = (dq == 0.0).all(1).mean(), (dq > 0.0).all(1).mean()
    assert undamaged >= 0.2 and damaged >= 0.2, (undamaged, damaged)
    a = fem.AsymDamage(V, E=E, nu=0.3, u=u, d=d, tangent=tangent)
    r = fem.evaluate(a, ("strain", "stress", "energy"), X=X)
    _close(r["strain"], _reduce(eps), "strain")
    _close(r["stress"], sig, "stress")
    _close(r["energy"], (_reduce(eps) * sig * _shear_weights(2)).sum(-1), "energy")
    # d = NULL is d = 0: the linear law
    r0 = fem.evaluate(fem.AsymDamage(V, E=E, nu=0.3, u=u, tangent=tangent), ("stress",), X=X)
    _close(r0["stress"], _reduce(_lin_stress(eps, lam, mu)), "stress (d = None)")


# ----------------------------------------------------------------------------------- 4. neo-Hookean
@pytest.mark.parametrize("ct,p,n", [(-4, 2, (2, 2, 2)), (3, 2, (4, 3))], ids=["tet-p2", "tri-p2"])
def test_neo_hookean_piola_stress(oracle, dev, ct, p, n):
    from femasm import _lib, fem

    m, V = _space(ct, p, n, dev)
    gd = m.gdim
    u = _rand_u(V, dev, 1e-2)
    E = _E_cells(oracle, m.num_cells, dev)
    lam, mu = oracle.lame(_np(E), 0.3)
    a = fem.NeoHookean(V, E=E, nu=0.3, u=u)
    for X in (None, _points(oracle, ct)):
        Xr = fem.interpolation_points(ct) if X is None else X
        G = _ref_grad(oracle, V, u, Xr)
        P = np.zeros_like(G)
        for c in range(G.shape[0]):
            for q in range(G.shape[1]):
                P[c, q] = oracle.neo_stress(np.eye(gd) + G[c, q], lam[c], mu[c])
        r = fem.evaluate(a, ("grad", "strain", "stress"), X=X)
        assert r["stress"].shape == (m.num_cells, Xr.shape[0] * gd * gd)
        _close(r["grad"], G, "grad")
        _close(r["strain"], _reduce(_sym(G)), "strain")
        _close(r["stress"], P, "first Piola stress")
    with pytest.raises(_lib.FemasmError, match="FA_NEO_HOOKEAN"):
        fem.evaluate(a, ("energy",))
    with pytest.raises(_lib.FemasmError, match="-2"):
        fem.Expression(a, "energy").eval()


# ------------------------------------------------------------------- 5. tie to the assembled residual
def _residual_from_stress(oracle, V, sig_red):
    """sum_c |c| sigma_c . g_a scattered to the nodes (P1 simplices: one point, constant gradients)."""
    from femasm import fem

    m = V.mesh
    gd = m.gdim
    g, J = _phys_grads(oracle, V, fem.interpolation_points(m.cell_type))
    vol = np.abs(np.linalg.det(J[:, 0])) / (2.0 if gd == 2 else 6.0)
    idx = [(i, j) for i in range(gd) for j in range(i, gd)]
    sig = np.zeros((m.num_cells, gd, gd))
    for k, (i, j) in enumerate(idx):
        sig[:, i, j] = sig[:, j, i] = sig_red[:, k]
    r = vol[:, None, None] * np.einsum("cij,caj->cai", sig, g[:, 0])
    b = np.zeros((V.num_nodes, gd))
    np.add.at(b, _np(V.dofmap).astype(np.int64).reshape(-1), r.reshape(-1, gd))
    return b.reshape(-1)


@pytest.mark.parametrize("case", ["damage-tri", "linear-tet"])
def test_stress_is_the_residuals_stress(oracle, dev, case):
    """The expression and fa_assemble_vector use the same law and material: the residual formed in
    numpy from the GPU stress equals the assembled one."""
    from femasm import fem

    if case == "damage-tri":
        m, V, u, d, E = _damage_state(oracle, dev, 1e-3)
        a = fem.AsymDamage(V, E=E, nu=0.3, u=u, d=d)
    else:
        m, V = _space(-4, 1, (3, 4, 2), dev)
        a = fem.LinearElasticity(V, E=_E_cells(oracle, m.num_cells, dev), nu=0.3, u=_rand_u(V, dev, 1e-3))
    sig = _np(fem.evaluate(a, ("stress",))["stress"])
    b = fem.assemble_vector(a)
    _close(b, _residual_from_stress(oracle, V, sig), "residual")


# --------------------------------------------------------------------------------- 6. staged stores
@pytest.fixture(scope="module")
def big(oracle, dev):
    """(41, 39) triangles: 3,198 cells = 49 full waves + a partial one, more than one workgroup. The
    all-cells result is computed once and shared (never modified)."""
    from femasm import fem

    m = _mesh(3, (41, 39), dev)
    V = fem.functionspace(m, ("Lagrange", 1, (2,)))
    assert m.num_cells == 3198
    a = fem.LinearElasticity(V, E=_E_cells(oracle, m.num_cells, dev), nu=0.3, u=_rand_u(V, dev, 1e-3))
    full = fem.evaluate(a, ("strain", "energy"))
    perm = torch.randperm(m.num_cells, generator=torch.Generator().manual_seed(13)).to(torch.int32).to(dev)
    return m, V, a, full, perm


def test_whole_mesh_matches_the_recipe(oracle, dev, big):
    from femasm import fem

    m, V, a, full, _ = big
    assert full["strain"].shape == (3198, 3) and full["energy"].shape == (3198, 1)
    lam, mu = oracle.lame(_np(a.E), 0.3)
    eps = _sym(_ref_grad(oracle, V, a.u, fem.interpolation_points(3)))
    _close(full["strain"], _reduce(eps), "strain")
    _close(full["energy"], (eps * _lin_stress(eps, lam, mu)).sum((-1, -2)), "energy")


@pytest.mark.parametrize("offset", [1, 2], ids=["8B-aligned", "16B-aligned"])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 257, 3198])
def test_staged_store_shapes(dev, big, k, offset):
    """Subsets of 1, 63, 64, 65 and 257 cells and all of them, into outputs offset by one double (8-B
    aligned only) or two: bit-identical to the rows of the all-cells result, guard words untouched."""
    from femasm import fem

    m, V, a, full, perm = big
    cells = perm[:k]
    guard = -7.25
    bufs, out = {}, {}
    for q, vs in (("strain", 3), ("energy", 1)):
        bufs[q] = torch.full((k * vs + 4,), guard, dtype=torch.float64, device=dev)
        out[q] = bufs[q][offset:offset + k * vs]
        assert out[q].data_ptr() % 16 == (8 if offset == 1 else 0)
    r = fem.evaluate(a, ("strain", "energy"), cells=cells, out=out)
    for q in ("strain", "energy"):
        assert r[q].data_ptr() == out[q].data_ptr()
        assert torch.equal(r[q], full[q][cells.to(torch.int64)]), q
        assert bool((bufs[q][:offset] == guard).all()) and bool((bufs[q][offset + out[q].numel():] == guard).all()), q
    # freshly allocated outputs give the same bits
    r2 = fem.evaluate(a, ("strain", "energy"), cells=cells)
    assert torch.equal(r2["strain"], r["strain"]) and torch.equal(r2["energy"], r["energy"])


def test_cells_none_equals_identity_selection_and_empty_selection(dev, big):
    from femasm import fem

    m, V, a, full, _ = big
    ident = torch.arange(m.num_cells, dtype=torch.int32, device=dev)
    r = fem.evaluate(a, ("strain", "energy"), cells=ident)
    assert torch.equal(r["strain"], full["strain"]) and torch.equal(r["energy"], full["energy"])
    e = fem.evaluate(a, ("strain", "energy"), cells=torch.zeros(0, dtype=torch.int32, device=dev))
    assert e["strain"].shape == (0, 3) and e["energy"].shape == (0, 1)
    assert fem.Expression(a, "strain").eval(m, cells=[]).shape == (0, 3)
    with pytest.raises(ValueError):
        fem.evaluate(a, ("strain",), cells=[0, m.num_cells])
    with pytest.raises(ValueError):
        fem.evaluate(a, ("strain",), out={"strain": torch.empty(5, dtype=torch.float64, device=dev)})


# ---------------------------------------------------------------------- 7. Function.interpolate(expr)
def test_interpolate_expression_into_dg0(oracle, dev):
    from femasm import fem

    m, V, u, d, E = _damage_state(oracle, dev, 1e-3)
    J = fem.AsymDamage(V, E=E, nu=0.3, u=u, d=d)
    S = fem.functionspace(m, ("DG", 0, (3,)))
    stress = fem.Function(S, name="stress")
    stress.interpolate(fem.Expression(J, "stress"))
    assert stress.x.shape == (m.num_cells * 3,)
    assert torch.equal(stress.x, fem.evaluate(J, ("stress",))["stress"].reshape(-1))
    assert float(stress.x.abs().max()) > 0.0
    en = fem.Function(fem.functionspace(m, ("DG", 0)), name="energy")
    en.interpolate(fem.Expression(J, "energy"))
    assert torch.equal(en.x, fem.evaluate(J, ("energy",))["energy"].reshape(-1))
    with pytest.raises(ValueError):  # wrong block size
        fem.Function(fem.functionspace(m, ("DG", 0, (4,)))).interpolate(fem.Expression(J, "stress"))
    with pytest.raises(ValueError):  # not a DG0 space
        fem.Function(fem.functionspace(m, ("Lagrange", 1, (3,)))).interpolate(fem.Expression(J, "stress"))
    with pytest.raises(ValueError):  # npts != 1
        fem.Function(S).interpolate(fem.Expression(J, "stress", oracle.quadrature(3, 2)[0]))


# ---------------------------------------------------------------------------------- 8. repeatability
@pytest.mark.parametrize("ct,p,n", [(-4, 2, (2, 2, 2)), (8, 2, (2, 1, 2))], ids=["tet-p2", "hex-q2"])
def test_repeatable(oracle, dev, ct, p, n):
    from femasm import fem

    m, V = _space(ct, p, n, dev)
    a = fem.LinearElasticity(V, E=_E_cells(oracle, m.num_cells, dev), nu=0.3, u=_rand_u(V, dev, 1e-3))
    for X in (None, _points(oracle, ct)):
        r1 = fem.evaluate(a, fem.QUANTITIES, X=X)
        r2 = fem.evaluate(a, fem.QUANTITIES, X=X)
        for q in fem.QUANTITIES:
            assert torch.equal(r1[q], r2[q]), q
