"""The asymmetric damage law at its branch states (test infrastructure; never imported by the package).

The law (fem.AsymDamage, the reference's mechanic2d law) branches on d > 0, on the "null tensor" test
|I1|, |I2| <= 1e-12, on the double eigenvalue r < 1e-12, on zero shear |eps_xy| <= 1e-12 (hand stress),
on the signs of ev1, ev2 and I1, and on d against 1. This module holds

  STATES, PATTERNS   the table of strain states (dyadic numbers: I1, I2, delta are exact in double with
                     or without FMA contraction) and of nodal damage patterns,
  soup(order)        a P1 mesh of disjoint right triangles, one (state, pattern) pair per cell, in an
                     order that mixes the pairs inside a wave ("interleaved") or keeps every wave
                     branch-uniform ("sorted"); the same cells in both,
  generic()          the states that survive roundoff, on rotated non-right triangles,
  references(case)   per-cell long-double potential, gradient and frozen-indicator Hessian (SymPy), the
                     element vectors and matrices built from them, and the per-cell scales.

Bars: every comparison is held to BAR = 1e-12 (the project's parity bar) times the cell's scale
  stress  (lam + 2 mu) max|eps| w_cell,   tangent  (lam + 2 mu) w_cell max|grad phi|^2,
  energy  1/2 (lam + 2 mu) (sum|eps|)^2 w_cell.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
LIMIT = 1.0e-12
BAR = 1.0e-12
NU = 0.3
S = 2.0 ** -10

# name, (e11, e22, e12), spin w, class
STATES = [
    ("zero", (0.0, 0.0, 0.0), 0.0, "null"),
    ("null", (3 * 2.0 ** -43, -2 * 2.0 ** -43, 2.0 ** -43), 2.0 ** -44, "null"),
    ("just-out-of-null", (3 * 2.0 ** -40, -2.0 ** -40, 2.0 ** -38), 2.0 ** -40, "smooth"),  # I1 = 2^-39
    ("dilation+", (S, S, 0.0), 0.0, "double"),
    ("dilation-", (-S, -S, 0.0), 0.0, "double"),
    ("dilation-with-spin", (S, S, 0.0), 2.0 ** -9, "double"),
    ("uniax-x+", (S, 0.0, 0.0), 0.0, "kink"),
    ("uniax-x-", (-S, 0.0, 0.0), 0.0, "kink"),
    ("uniax-y+", (0.0, S, 0.0), 0.0, "kink"),
    ("uniax-y-", (0.0, -S, 0.0), 2.0 ** -12, "kink"),
    ("poisson-x", (S, -3 * S / 4, 0.0), 0.0, "zero-shear"),
    ("poisson-y", (-3 * S / 4, S, 0.0), 2.0 ** -11, "zero-shear"),
    ("poisson-x-compress", (-S, 3 * S / 4, 0.0), 0.0, "zero-shear"),
    ("poisson-y-compress", (3 * S / 4, -S, 0.0), 0.0, "zero-shear"),
    ("pure-shear", (0.0, 0.0, S), 0.0, "kink"),
    ("I1=0-with-shear", (S, -S, S / 4), 2.0 ** -12, "kink"),
    ("both+shear", (S, S / 2, S / 4), 2.0 ** -11, "smooth"),
    ("both-shear", (-S, -S / 2, -S / 4), 0.0, "smooth"),
    ("mixed-I1>0-shear", (S, -S / 2, S / 2), 2.0 ** -10, "smooth"),
    ("mixed-I1<0-shear", (-S, S / 2, -S / 2), 0.0, "smooth"),
    ("shear-below-limit", (S, -S / 2, 2.0 ** -41), 0.0, "zero-shear"),
    ("shear-above-limit", (S, -S / 2, 2.0 ** -39), 0.0, "smooth"),
]
STATE_NAMES = [s[0] for s in STATES]

# three nodal damage values per cell; the law sees their mean
PATTERNS = [
    (0.0, 0.0, 0.0),
    (0.4, 0.4, 0.4),
    (0.0, 0.0, 1.2),
    (1.0, 1.0, 1.0),
    (2.0 ** -60, 0.0, 0.0),
    (0.75, 1.0, 1.25),
]

# Where the reference's hand stress (asym_stress) is not the gradient of its potential, for d > 0:
#   swap        zero shear with the larger principal strain on y: the identity eigenvectors pair the
#               larger eigenvalue with x, so the hand stress is the gradient with xx and yy exchanged
#   drop-shear  0 < |e12| <= 1e-12: the same branch drops the shear stress 2 mu (..) e12
#   near-limit  |e12| just above 1e-12: the eigenvector (ev - e22, e12) of the smaller eigenvalue has
#               ev - e22 = O(e12^2 / r), lost in double next to e22, so the "eigenvector" is (0, 1) and the
#               shear stress is off by O(e12 / r) = 1e-9 of the stress scale
#   null-zero   the null-tensor branch returns zero stress; the gradient is (1 - d) sigma_linear
HAND_STRESS_NOT_GRADIENT = {
    "null": "null-zero",
    "uniax-x-": "swap",
    "uniax-y+": "swap",
    "poisson-y": "swap",
    "poisson-x-compress": "swap",
    "shear-below-limit": "drop-shear",
    "shear-above-limit": "near-limit",
}
# generic(): states whose branch survives a 1-ulp change of the strain, and whose hand stress does not
# amplify it (near-limit does, by 1 / e12)
GENERIC_STATES = [n for n, e, w, c in STATES
                  if (c in ("smooth", "null", "double") or (c == "zero-shear" and e[0] * e[1] != 0.0))
                  and n != "shear-above-limit"]

NP, NREP = len(STATES) * len(PATTERNS), 64
_OFFS = {  # vertex offsets from the cell's origin for legs (a, b); orientations 1 and 3: det J < 0
    0: lambda a, b: ((0, 0), (a, 0), (0, b)),
    1: lambda a, b: ((0, 0), (0, b), (a, 0)),
    2: lambda a, b: ((0, 0), (-a, 0), (0, -b)),
    3: lambda a, b: ((0, 0), (-a, 0), (0, b)),
}


@functools.lru_cache(maxsize=None)
def _e_range():
    from oracle import oracle

    return oracle.e_range()


def _finish(x, u, dn, si, pi, ident, order):
    nc = len(si)
    cells = np.arange(3 * nc, dtype=np.int32).reshape(nc, 3)
    E = _e_range()[ident % 200]
    mu = E / (2.0 * (1.0 + NU))
    lam = E * NU / ((1.0 + NU) * (1.0 - 2.0 * NU))
    return SimpleNamespace(order=order, x=x.reshape(-1, 2), cells=cells, u=u.reshape(-1), d=dn.reshape(-1), E=E,
                           lam=lam, mu=mu, state=si, pattern=pi, ident=ident, nc=nc,
                           strain=np.array([STATES[s][1] for s in si]))


@functools.lru_cache(maxsize=None)
def soup(order: str):
    """8448 disjoint right triangles: every (state, pattern) pair 64 times, each copy with its own legs
    (2^-j, j in 0..2), orientation and Young's modulus. Cell identity = (pair p, copy r); "interleaved"
    puts it at r * NP + p (64 different pairs per wave), "sorted" at p * 64 + r (one pair per wave). Node
    3 c + a is vertex a of cell c; the origin of the cell at position k is (2 k, 0)."""
    assert order in ("interleaved", "sorted")
    nc = NP * NREP
    k = np.arange(nc)
    p, r = (k % NP, k // NP) if order == "interleaved" else (k // NREP, k % NREP)
    si, pi = p // len(PATTERNS), p % len(PATTERNS)
    g = r + p
    j1, j2, ori = g % 3, (g // 3) % 3, (g // 9) % 4
    x = np.zeros((nc, 3, 2))
    u = np.zeros((nc, 3, 2))
    dn = np.zeros((nc, 3))
    for c in range(nc):
        (e11, e22, e12), w = STATES[si[c]][1], STATES[si[c]][2]
        G = np.array([[e11, e12 - w], [e12 + w, e22]])
        off = np.array(_OFFS[int(ori[c])](2.0 ** -int(j1[c]), 2.0 ** -int(j2[c])), dtype=np.float64)
        x[c] = off + np.array([2.0 * c, 0.0])
        u[c] = off @ G.T
        dn[c] = PATTERNS[pi[c]]
    return _finish(x, u, dn, si, pi, r * NP + p, order)


@functools.lru_cache(maxsize=None)
def generic():
    """GENERIC_STATES x PATTERNS x 4 copies on rotated, scaled scalene triangles at shifted origins: the
    strain the kernels recover from x and u carries roundoff."""
    names = GENERIC_STATES
    pairs = [(STATE_NAMES.index(n), q) for n in names for q in range(len(PATTERNS))]
    nc = len(pairs) * 4
    base = np.array([[0.0, 0.0], [1.0, 0.2], [0.3, 0.9]])
    x = np.zeros((nc, 3, 2))
    u = np.zeros((nc, 3, 2))
    dn = np.zeros((nc, 3))
    si, pi = np.zeros(nc, dtype=np.int64), np.zeros(nc, dtype=np.int64)
    for c in range(nc):
        s, q = pairs[c % len(pairs)]
        rep = c // len(pairs)
        si[c], pi[c] = s, q
        th = 0.37 + 0.61 * c
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        tri = (0.37 + 0.21 * rep) * base @ R.T
        if rep % 2:
            tri = tri[[0, 2, 1]]  # det J < 0
        (e11, e22, e12), w = STATES[s][1], STATES[s][2]
        G = np.array([[e11, e12 - w], [e12 + w, e22]])
        o = np.array([2.0 * c + 0.1, 0.1 * rep])
        x[c] = tri + o
        u[c] = (x[c] - o) @ G.T
        dn[c] = PATTERNS[q]
    return _finish(x, u, dn, si, pi, np.arange(nc), "generic")


def structured_states(n=8):
    """The reference driver's first two states on the n x n unit square: (x, cells) come from the
    caller's mesh; returns d(x) (a Gaussian) and the two displacement fields as functions of x."""
    def d(x):
        return 0.9 * np.exp(-((x[:, 0] - 0.5) ** 2 + (x[:, 1] - 0.5) ** 2) / 0.08)

    def u0(x):
        return np.zeros(2 * len(x))

    def u1(x):
        return np.stack([S * x[:, 0], np.zeros(len(x))], 1).reshape(-1)

    return d, u0, u1


# ------------------------------------------------------------------------------------ references
def cell_geometry(case):
    """Long-double physical gradients g [nc, 3, 2], weight w = |det J| / 2, and the strain (e11, e22, e12)
    recovered from x and u."""
    X = case.x[case.cells].astype(LD)
    U = case.u.reshape(-1, 2)[case.cells].astype(LD)
    J = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]], 2)  # J[c, i, k] = d x_i / d X_k
    det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
    Ji = np.empty_like(J)
    Ji[:, 0, 0], Ji[:, 0, 1] = J[:, 1, 1] / det, -J[:, 0, 1] / det
    Ji[:, 1, 0], Ji[:, 1, 1] = -J[:, 1, 0] / det, J[:, 0, 0] / det
    ref = np.array([[-1.0, -1.0], [1.0, 0.0], [0.0, 1.0]], dtype=LD)
    g = np.einsum("ak,ckj->caj", ref, Ji)
    gr = np.einsum("cai,caj->cij", U, g)  # du_i / dx_j
    eps = np.stack([gr[:, 0, 0], gr[:, 1, 1], (gr[:, 0, 1] + gr[:, 1, 0]) / 2], 1)
    return g, np.abs(det) / 2, eps


def _to_mp(v):
    import mpmath as mp

    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(LD(v) - LD(hi)))


def _from_mp(v):
    import mpmath as mp

    hi = float(v)
    return LD(hi) + LD(float(v - mp.mpf(hi)))


@functools.lru_cache(maxsize=None)
def _sympy_hessian():
    """Hessian of the reference potential in Voigt strains (e00, e11, gamma = 2 e01) with the indicator
    alphas as symbols (tests/test_oracle.py::_psi_sympy), split as lam * Hl + mu * Hm."""
    import sympy as sp

    e00, e11, gam, lam, mu, d, al, al1, al2 = sp.symbols("e00 e11 gamma lam mu d al al1 al2", real=True)
    e01 = gam / 2
    I1 = e00 + e11
    I2 = e01 * e01 - e00 * e11
    r = sp.sqrt(I1 * I1 + 4 * I2)
    ev1, ev2 = (I1 + r) / 2, (I1 - r) / 2
    psi = I1 * I1 * (1 - al * d) * lam / 2 + mu * ((1 - al1 * d) * ev1 ** 2 + (1 - al2 * d) * ev2 ** 2)
    ev = (e00, e11, gam)
    H = sp.Matrix(3, 3, lambda i, j: sp.diff(psi, ev[i], ev[j]))
    args = (e00, e11, gam, d, al, al1, al2)
    return (sp.lambdify(args, H.subs({lam: 1, mu: 0}), modules="mpmath"),
            sp.lambdify(args, H.subs({lam: 0, mu: 1}), modules="mpmath"))


_hess_cache: dict = {}


def _hessian_parts(e, d, al, a1, a2):
    import mpmath as mp

    key = (repr(e[0]), repr(e[1]), repr(e[2]), repr(d), al, a1, a2)
    if key not in _hess_cache:
        fl, fm = _sympy_hessian()
        with mp.workdps(40):
            a = (_to_mp(e[0]), _to_mp(e[1]), 2 * _to_mp(e[2]), _to_mp(d), int(al), int(a1), int(a2))
            Hl, Hm = fl(*a), fm(*a)
            _hess_cache[key] = (np.array([[_from_mp(Hl[i, j]) for j in range(3)] for i in range(3)], dtype=LD),
                                np.array([[_from_mp(Hm[i, j]) for j in range(3)] for i in range(3)], dtype=LD))
    return _hess_cache[key]


def law(eps, d, lam, mu, hessian=True):
    """The law per cell in long double. eps [n, 3] = (e11, e22, e12), d [n] the mean nodal damage.
    Returns the branch ("linear", "null", "double", "general") per cell, psi [n], the gradient
    (s11, s22, s12) [n, 3] and the Voigt Hessian [n, 3, 3] (damage limited to 1 - 1e-12 there, as both
    tangents of the reference do). Indicators are frozen at their values at eps; the double-eigenvalue
    values are (1 - alpha d) times the linear law and the null-tensor values (1 - d) times it."""
    eps, d, lam, mu = (np.asarray(a, dtype=LD) for a in (eps, d, lam, mu))
    n = eps.shape[0]
    e11, e22, e12 = eps[:, 0], eps[:, 1], eps[:, 2]
    I1 = e11 + e22
    I2 = e12 * e12 - e11 * e22
    delta = (e11 - e22) ** 2 + 4 * e12 * e12  # = I1^2 + 4 I2 without its cancellation
    r = np.sqrt(delta)
    lin = ~(d > 0)
    null = ~lin & ~((np.abs(I1) > LIMIT) | (np.abs(I2) > LIMIT))
    dbl = ~lin & ~null & (r < LIMIT)
    gen = ~lin & ~null & ~dbl
    branch = np.where(lin, "linear", np.where(null, "null", np.where(dbl, "double", "general")))
    ev1, ev2 = (I1 + r) / 2, (I1 - r) / 2
    al, a1, a2 = (I1 >= 0).astype(LD), (ev1 >= 0).astype(LD), (ev2 >= 0).astype(LD)
    dc = np.minimum(d, LD(1.0 - LIMIT))
    psi_lin = lam / 2 * I1 * I1 + mu * (e11 * e11 + e22 * e22 + 2 * e12 * e12)
    sig_lin = np.stack([lam * I1 + 2 * mu * e11, lam * I1 + 2 * mu * e22, 2 * mu * e12], 1)
    H_lin = np.zeros((n, 3, 3), dtype=LD)
    H_lin[:, 0, 0] = H_lin[:, 1, 1] = lam + 2 * mu
    H_lin[:, 0, 1] = H_lin[:, 1, 0] = lam
    H_lin[:, 2, 2] = mu
    f = np.where(lin, LD(1), np.where(null, 1 - d, 1 - al * d))  # factor on the linear law (not "general")
    fh = np.where(lin, LD(1), np.where(null, 1 - dc, 1 - al * dc))
    psi, sig, H = f * psi_lin, f[:, None] * sig_lin, fh[:, None, None] * H_lin
    # general branch: closed form with frozen indicators
    rs = np.where(gen, r, LD(1))
    c, c1, c2 = 1 - al * d, 1 - a1 * d, 1 - a2 * d
    pg = lam / 2 * c * I1 * I1 + mu * (c1 * ev1 * ev1 + c2 * ev2 * ev2)
    dr = np.stack([(e11 - e22) / rs, -(e11 - e22) / rs, 2 * e12 / rs], 1)  # d r / d (e11, e22, gamma)
    dI = np.array([1, 1, 0], dtype=LD)[None, :]
    sg = (lam * c * I1)[:, None] * dI + mu[:, None] * ((c1 * ev1)[:, None] * (dI + dr) + (c2 * ev2)[:, None] * (dI - dr))
    psi = np.where(gen, pg, psi)
    sig = np.where(gen[:, None], sg, sig)
    if hessian:
        for i in np.nonzero(gen)[0]:
            Hl, Hm = _hessian_parts(eps[i], dc[i], al[i], a1[i], a2[i])
            H[i] = lam[i] * Hl + mu[i] * Hm
    return branch, psi, sig, H


def hand_stress_model(eps, sig, kind):
    """What the reference's hand stress is at a HAND_STRESS_NOT_GRADIENT state of `kind`, from the
    gradient `sig` (None: no closed model, the oracle's own value is the record)."""
    if kind == "swap":
        return sig[:, [1, 0, 2]]
    if kind == "drop-shear":
        return sig * np.array([1, 1, 0], dtype=LD)
    if kind == "null-zero":
        return np.zeros_like(sig)
    return None


def references(case, hessian=True):
    """Everything the tests compare against, per cell, in long double."""
    g, w, eps = cell_geometry(case)
    d = case.d[case.cells].astype(LD).sum(1) / 3
    lam, mu = case.lam.astype(LD), case.mu.astype(LD)
    branch, psi, sig, H = law(eps, d, lam, mu, hessian)
    nc = case.nc
    B = np.zeros((nc, 3, 6), dtype=LD)
    for a in range(3):
        B[:, 0, 2 * a] = g[:, a, 0]
        B[:, 1, 2 * a + 1] = g[:, a, 1]
        B[:, 2, 2 * a] = g[:, a, 1]
        B[:, 2, 2 * a + 1] = g[:, a, 0]
    stiff = lam + 2 * mu
    emax = np.abs(eps).max(1)
    return SimpleNamespace(
        g=g, w=w, eps=eps, d=d, branch=branch, psi=psi, sig=sig, H=H, B=B,
        energy=psi * w, re=np.einsum("cki,ck->ci", B, sig) * w[:, None],
        Ke=np.einsum("cki,ckl,clj->cij", B, H, B) * w[:, None, None],
        s_stress=stiff * emax, s_tangent=stiff * (np.abs(g).max((1, 2)) ** 2), s_energy=stiff / 2 * np.abs(eps).sum(1) ** 2)


def element_matrices(Hook, ref):
    """w B^T H B in long double from per-cell hooks [nc, 3, 3]."""
    return np.einsum("cki,ckl,clj->cij", ref.B, np.asarray(Hook, dtype=LD), ref.B) * ref.w[:, None, None]


def element_vectors(sig, ref):
    """w B^T sigma from per-cell stresses (s11, s22, s12) [nc, 3] (not yet multiplied by w)."""
    return np.einsum("cki,ck->ci", ref.B, np.asarray(sig, dtype=LD)) * ref.w[:, None]


def oracle_cells(oracle, case):
    """The oracle's hand hook [nc, 3, 3] and hand stress [nc, 3] at the strain it recovers itself (double)."""
    _, _, eps = cell_geometry(case)
    d = oracle_damage(case)
    e = eps.astype(np.float64)
    hook = np.stack([oracle.damage_hook(e[c], case.lam[c], case.mu[c], d[c]) for c in range(case.nc)])
    sig = np.stack([oracle.damage_stress(e[c], case.lam[c], case.mu[c], d[c]) for c in range(case.nc)])
    return hook, sig


def oracle_damage(case):
    """The mean nodal damage as the oracle's assembly sums it (d0 / 3 + d1 / 3 + d2 / 3)."""
    dn = case.d[case.cells]
    return dn[:, 0] / 3.0 + dn[:, 1] / 3.0 + dn[:, 2] / 3.0


def worst(err, scale, case, what=""):
    """max over cells of err / scale with the cell's state and pattern named; cells of scale 0 must have
    err 0 (they count as ratio inf otherwise). err, scale: [nc] (reduce entries with .max first)."""
    err, scale = np.asarray(err, dtype=LD), np.asarray(scale, dtype=LD)
    ratio = np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err > 0, np.inf, 0))
    ratio = np.where(np.isfinite(np.asarray(err, dtype=np.float64)), ratio, np.inf)
    c = int(np.argmax(ratio))
    return float(ratio[c]), f"{what}: cell {c} state {STATE_NAMES[case.state[c]]!r} pattern {PATTERNS[case.pattern[c]]}"


def by_class(err, scale, case):
    """{state class: worst err / scale} for the error tables."""
    err, scale = np.asarray(err, dtype=LD), np.asarray(scale, dtype=LD)
    ratio = np.where(scale > 0, err / np.where(scale > 0, scale, 1), np.where(err > 0, np.inf, 0))
    cls = np.array([STATES[s][3] for s in case.state])
    return {k: float(ratio[cls == k].max()) for k in ("smooth", "kink", "double", "null", "zero-shear") if (cls == k).any()}


def assert_finite(a, case, what):
    a = np.asarray(a, dtype=np.float64).reshape(case.nc, -1)
    bad = ~np.isfinite(a).all(1)
    if bad.any():
        names = sorted({STATE_NAMES[s] for s in case.state[bad]})
        raise AssertionError(f"{what}: non-finite values in {int(bad.sum())} cells, states {names}")


def assert_close(got, ref, scale, case, what, bar=BAR):
    """|got - ref| <= bar * scale per cell (entries reduced by max), non-finite values named first."""
    assert_finite(got, case, what)
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD)).reshape(case.nc, -1).max(1)
    ratio, where = worst(err, scale, case, what)
    assert ratio <= bar, f"{where}: error {ratio:.3e} x scale > {bar:g}"
    return err
