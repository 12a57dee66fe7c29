"""The per-quarter LDS add order (csrc/plan_order.h) on the CPU: the stand-alone driver
csrc/plan_order_host.cpp is compiled once and fed quarters on its standard input.

A quarter is up to 16 lanes with NBG blocks each, every block with a residue (slot mod 16). An order
assigns each lane's blocks to the NBG steps; its passes are the sum over steps of the largest number of
lanes on one residue (same-slot lanes count as distinct), its bound max(NBG, largest residue total).

(a) every lane's picks are a permutation, the reported passes equal a numpy recount, and they never
    exceed the earlier descent's on the same input;
(b) where no residue total exceeds NBG the passes are exactly NBG (de Werra's theorem: hard assert);
    elsewhere passes / bound is printed;
(c) the quarters of two real plans (P2 tetrahedra on the (4,3,3) and 16^3 cubes, recorded from the
    device plan under tests/golden/plan_order/): totals against the numpy recount, ratio printed;
(d) the same driver built with -fsanitize=address,undefined runs clean on the inputs of (a)."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fem-libraries_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_order")
NBGS = (4, 5, 9)


def _cxx():
    for c in (os.environ.get("CXX"), "g++", "clang++", "c++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    pytest.fail("no C++ compiler for the host driver")


def _compile(out, flags, maybe=()):
    """maybe: flags dropped if the compiler does not know them"""
    base = [_cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags]
    tail = [os.path.join(CSRC, "plan_order_host.cpp"), "-o", out]
    r = subprocess.run(base + list(maybe) + tail, capture_output=True, text=True)
    if r.returncode != 0 and maybe:
        r = subprocess.run(base + tail, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(str(tmp_path_factory.mktemp("plan_order") / "plan_order_host"), ["-O2"])


def _run(exe, nbg, nl, res, starts=1):
    """nl [n] lanes, res [n, 16, nbg] residues -> (heads [n, 4], picks [n, 16, nbg])"""
    n = len(nl)
    rec = np.zeros((n, 1 + 16 * nbg), np.uint8)
    rec[:, 0] = nl
    rec[:, 1:] = res.reshape(n, -1)
    r = subprocess.run([exe, str(nbg), str(starts)], input=rec.tobytes(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stderr == b"", r.stderr.decode()[-2000:]
    out = np.frombuffer(r.stdout, np.uint8).reshape(n, 8 + 16 * nbg)
    heads = out[:, :8].copy().view("<u2").astype(np.int64)
    return heads, out[:, 8:].reshape(n, 16, nbg).astype(np.int64)


def _recount(nl, res, picks):
    """passes of the order `picks` and the bound, per quarter, in plain numpy"""
    n, _, nbg = res.shape
    live = np.arange(16)[None, :] < nl[:, None]                      # [n, 16]
    at = np.take_along_axis(res.astype(np.int64), picks, axis=2)      # residue of lane q at step t
    cnt = np.zeros((n, nbg, 16), np.int64)
    qi, li, ti = np.nonzero(np.broadcast_to(live[:, :, None], at.shape))
    np.add.at(cnt, (qi, ti, at[qi, li, ti]), 1)
    passes = cnt.max(axis=2).sum(axis=1)
    tot = cnt.sum(axis=1)                                             # [n, 16] residue totals
    bound = np.where(nl > 0, np.maximum(tot.max(axis=1), nbg), 0)
    return passes, bound, tot


def _quarters(nbg, seed):
    """random and adversarial quarters: (nl, res)"""
    g = np.random.default_rng(seed)
    nls, ress = [], []

    def add(nl, res):
        full = np.zeros((16, nbg), np.uint8)
        full[:nl] = res
        full[nl:] = g.integers(0, 16, (16 - nl, nbg))  # idle lanes hold anything
        nls.append(nl)
        ress.append(full)

    for nl in range(0, 17):
        add(nl, np.full((nl, nbg), 7))                              # one residue (one slot)
        add(nl, np.tile(np.arange(nbg) % 16, (nl, 1)))              # every lane the same blocks
        add(nl, (np.arange(nl)[:, None] + np.arange(nbg)[None, :]) % 16)  # a circulant
        add(nl, g.integers(0, 2, (nl, nbg)) * 8)                    # two residues
        add(nl, g.integers(0, 3, (nl, nbg)))                        # three residues
        for _ in range(40):
            add(nl, g.integers(0, 16, (nl, nbg)))                   # uniform
        for _ in range(20):                                         # a hot residue among uniform ones
            r = g.integers(0, 16, (nl, nbg))
            r[g.random((nl, nbg)) < 0.25] = 3
            add(nl, r)
    # no residue total above NBG (the theorem's case): residues dealt from a deck of NBG copies of each
    for nl in (1, 2, 5, 11, 15, 16):
        for _ in range(150):
            deck = g.permutation(np.repeat(np.arange(16), nbg))[:nl * nbg]
            add(nl, deck.reshape(nl, nbg))
    return np.array(nls, np.int64), np.stack(ress)


@pytest.mark.parametrize("starts", [1, 2])
@pytest.mark.parametrize("nbg", NBGS)
def test_order_is_valid_optimal_and_never_worse(driver, nbg, starts):
    """starts 1: the default plan's order; 2: with the second start of the opt-in search"""
    nl, res = _quarters(nbg, 100 + nbg)
    heads, picks = _run(driver, nbg, nl, res, starts)
    live = np.arange(16)[None, :] < nl[:, None]
    # (a) permutations, the recount, never worse than the descent (the earlier default plan's order; how
    # often the earlier searched order has fewer passes is printed)
    assert (np.sort(picks, axis=2)[live] == np.arange(nbg)).all()
    passes, bound, tot = _recount(nl, res, picks)
    assert (heads[:, 0] == passes).all()
    assert (heads[:, 3] == bound).all()
    assert (passes >= bound).all()
    assert (passes <= heads[:, 1]).all()
    # (b) the theorem's case is exact
    easy = (tot.max(axis=1) <= nbg) & (nl > 0)
    assert easy.sum() >= 900
    assert (passes[easy] == nbg).all()
    hard = ~easy & (nl > 0)
    print(f"NBG {nbg}, {starts} start(s): {len(nl)} quarters, {easy.sum()} with every residue total <= NBG (all at NBG passes); "
          f"the other {hard.sum()}: passes / bound = {passes[hard].sum() / bound[hard].sum():.4f} "
          f"(descent {heads[hard, 1].sum() / bound[hard].sum():.4f}, with chain search "
          f"{heads[hard, 2].sum() / bound[hard].sum():.4f}), at the bound: {(passes[hard] == bound[hard]).mean():.3f}, "
          f"worse than the searched descent on {(passes > heads[:, 2]).sum()}")


def _golden(name):
    """recorded quarters of a device plan: (nbg, nl [n], res [n, 16, nbg])"""
    with open(os.path.join(GOLDEN, name), "rb") as f:
        raw = zlib.decompress(f.read())
    nbg, n = int(raw[0]), int.from_bytes(raw[1:5], "little")
    nl = np.frombuffer(raw, np.uint8, n, 5).astype(np.int64)
    nib = np.frombuffer(raw, np.uint8, offset=5 + n)
    res = np.stack([nib & 15, nib >> 4], axis=1).reshape(-1)[:n * 16 * nbg].reshape(n, 16, nbg)
    return nbg, nl, res


@pytest.mark.parametrize("starts", [1, 2])
@pytest.mark.parametrize("name", ["p2tet_4x3x3.bin", "p2tet_16.bin"])
def test_quarters_of_real_plans(driver, name, starts):
    nbg, nl, res = _golden(name)
    heads, picks = _run(driver, nbg, nl, res, starts)
    live = np.arange(16)[None, :] < nl[:, None]
    assert (np.sort(picks, axis=2)[live] == np.arange(nbg)).all()
    passes, bound, _ = _recount(nl, res, picks)
    assert (heads[:, 0] == passes).all() and (heads[:, 3] == bound).all()
    assert (passes <= heads[:, 1]).all()
    print(f"{name}, {starts} start(s): {len(nl)} quarters, passes {passes.sum()}, bound {bound.sum()}, ratio {passes.sum() / bound.sum():.4f} "
          f"(descent {heads[:, 1].sum() / bound.sum():.4f}, with chain search {heads[:, 2].sum() / bound.sum():.4f}); "
          f"at the bound {(passes == bound).mean():.4f}; worse than the searched descent on {(passes > heads[:, 2]).sum()}")


def test_sanitizer_build_runs_clean(tmp_path):
    exe = _compile(str(tmp_path / "plan_order_host_san"),
                   ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
                   maybe=["-static-libasan", "-static-libubsan"])  # the runtimes in the program itself
    for nbg in NBGS:
        nl, res = _quarters(nbg, 100 + nbg)
        for starts in (1, 2):
            heads, picks = _run(exe, nbg, nl, res, starts)
            passes, _, _ = _recount(nl, res, picks)
            assert (heads[:, 0] == passes).all()
