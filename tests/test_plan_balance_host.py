"""Which entries share a 16-lane quarter, on the CPU: tools/plan_order/plan_balance_host.cpp holds a copy of
k_plan_perm's greedy fill and the exchange descent that DESIGN.md 3.2b "Quarter balance" measured and left
out of the plan; tools/plan_order/plan_balance_counts.py produces profiles/plan_balance/counts.txt with it.
The driver is compiled once and fed chunks on its standard input.

A chunk's entries (NN residues each, NSPLIT lanes that stay together) fill quarters of EQ = 16 / NSPLIT
entries; a quarter's order has at least max(NBG, largest residue total) passes. The driver prints, per
chunk, the entry at every position: positions 0 .. na - 1 are the quarters in order (only the last one
short), so a permutation of the entries is a placement within every quarter's capacity that keeps an
entry's lanes together.

(a) the output is a permutation; the summed bound the driver reports equals a numpy recount, before (the
    greedy fill, also redone in plain Python) and after the exchanges, and it never rises, per chunk;
(b) on the chunks of two real plans (tests/golden/plan_order/: the recorded quarters regrouped) it falls in
    total (ratio printed), and plan_order_host's passes on the re-formed quarters are no more in total;
(c) the driver's fill alone reproduces the eperm k_plan_perm wrote for chunks recorded from device plans
    (chunks_*.bin): the copy of the fill is the device's;
(d) two runs give the same bytes;
(e) adversarial chunks: one quarter, a last quarter of one entry, identical entries, one hot residue,
    NN = 4, 9, 10, NSPLIT 1 and 2, the 64-quarter chunks of the generic gather;
(f) the same driver built with -fsanitize=address,undefined runs clean on the inputs of (e).

Figures (p2tet_16.bin, 31,411 quarters): bound 216,979 -> 193,600 (-10.8 %), passes of the default order
229,582 -> 223,954 (-2.5 %)."""
import os

import numpy as np
import pytest

import plan_chunks as pc

# (NN, NSPLIT, MQ) the driver is built for
SHAPES = [(4, 1, 16), (9, 1, 16), (10, 1, 16), (10, 2, 16), (6, 2, 16), (10, 2, 64), (10, 1, 32)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return pc.compile_driver(pc.BALANCE_SRC, str(tmp_path_factory.mktemp("plan_balance") / "plan_balance_host"))


@pytest.fixture(scope="module")
def order_driver(tmp_path_factory):
    return pc.compile_driver("plan_order_host.cpp", str(tmp_path_factory.mktemp("plan_order") / "plan_order_host"))


def _adversarial(nn, ns, mq, seed):
    g = np.random.default_rng(seed)
    eq = 16 // ns
    cap = mq * eq
    out = []
    sizes = sorted({1, 2, eq - 1, eq, eq + 1, 2 * eq, 2 * eq + 1, 3 * eq + 1, 5 * eq - 1, 12 * eq, cap - eq + 1, cap - 1, cap})
    for na in (s for s in sizes if 1 <= s <= cap):  # one quarter only; a last quarter of one entry; full
        out.append(np.full((na, nn), 7))                                  # one residue
        out.append(np.tile(np.arange(nn) % 16, (na, 1)))                  # all entries identical
        out.append((np.arange(na)[:, None] + np.arange(nn)[None, :]) % 16)  # a circulant
        for _ in range(4):
            out.append(g.integers(0, 16, (na, nn)))                        # uniform
        for _ in range(4):                                                 # one hot residue
            r = g.integers(0, 16, (na, nn))
            r[g.random((na, nn)) < 0.3] = 3
            out.append(r)
        r = g.integers(0, 16, (na, nn))                                    # the hot residue in every other entry
        r[::2, : max(1, nn // 2)] = 11
        out.append(r)
        # consecutive slots from a random row start (what a P2 row's entries look like)
        out.append((g.integers(0, 16, (na, 1)) + np.sort(g.integers(0, 40, (na, nn)), axis=1)) % 16)
    return [c.astype(np.uint8) for c in out]


def _check(chunks, nn, ns, b0, b1, perms, filled):
    """(a): permutations, recounts, never worse; filled: the driver ran the greedy fill (redone here)"""
    for c, g0, g1, p in zip(chunks, b0, b1, perms):
        assert (np.sort(p) == np.arange(len(c))).all()
        assert g1 == pc.bound_of(c[p], nn, ns)
        assert g1 <= g0, "the exchanges raised a chunk's summed bound"
        if filled:
            assert g0 == pc.bound_of(c[pc.greedy_fill(c, nn, ns)], nn, ns)
        else:
            assert g0 == pc.bound_of(c, nn, ns)


@pytest.mark.parametrize("nn,ns,mq", SHAPES)
def test_adversarial_chunks(driver, nn, ns, mq):
    chunks = _adversarial(nn, ns, mq, 7 + nn + ns)
    b0, b1, mv, perms = pc.run_balance(driver, nn, ns, mq, chunks)
    _check(chunks, nn, ns, b0, b1, perms, filled=True)
    again = pc.run_balance(driver, nn, ns, mq, chunks)
    assert all((p == q).all() for p, q in zip(perms, again[3])), "two runs differ"
    # a chunk of one quarter has nothing to exchange
    eq = 16 // ns
    assert all(m == 0 for c, m in zip(chunks, mv) if len(c) <= eq)
    print(f"NN {nn} NSPLIT {ns} MQ {mq}: {len(chunks)} chunks, bound {b0.sum()} -> {b1.sum()} "
          f"({b1.sum() / b0.sum():.4f}), {mv.sum()} exchanges")


@pytest.mark.parametrize("name", ["p2tet_4x3x3.bin", "p2tet_16.bin"])
def test_recorded_plans(driver, order_driver, name):
    nn, chunks = pc.recorded_chunks(name)
    ns = 2
    b0, b1, mv, perms = pc.run_balance(driver, nn, ns, 64, chunks, mode="placed")
    _check(chunks, nn, ns, b0, b1, perms, filled=False)
    assert b1.sum() < b0.sum()
    again = pc.run_balance(driver, nn, ns, 64, chunks, mode="placed")
    assert all((p == q).all() for p, q in zip(perms, again[3])), "two runs differ"
    ident = [np.arange(len(c)) for c in chunks]
    p0, q0 = pc.run_order(order_driver, nn // ns, *pc.quarters_of(chunks, ident, nn, ns))
    p1, q1 = pc.run_order(order_driver, nn // ns, *pc.quarters_of(chunks, perms, nn, ns))
    assert q0.sum() == b0.sum() and q1.sum() == b1.sum()
    print(f"{name}: {len(chunks)} chunks, {len(p0)} quarters, bound {b0.sum()} -> {b1.sum()} ({b1.sum() / b0.sum():.4f}), "
          f"passes {p0.sum()} -> {p1.sum()} ({p1.sum() / p0.sum():.4f}), passes / bound {p0.sum() / b0.sum():.4f} -> "
          f"{p1.sum() / b1.sum():.4f}, {mv.sum()} exchanges")
    assert p1.sum() <= p0.sum()


@pytest.mark.parametrize("name", ["chunks_p2tet_4x3x3.bin", "chunks_p2tet_16.bin"])
def test_device_placement_is_reproduced(driver, name):
    """(c) chunks recorded from device plans with the eperm k_plan_perm wrote: the fill alone"""
    nn, ns, chunks, eperms = pc.load_chunks(name)
    visits = [pc.visit_order(len(c)) for c in chunks]
    b0, b1, mv, perms = pc.run_balance(driver, nn, ns, 16, [c[v] for c, v in zip(chunks, visits)], mode="fill")
    assert mv.sum() == 0 and (b0 == b1).all()
    bad = sum(int(not (v[p] == e).all()) for v, p, e in zip(visits, perms, eperms))
    print(f"{name}: {len(chunks)} chunks, bound {b0.sum()} -> {b1.sum()}, {mv.sum()} exchanges, {bad} chunks differ")
    assert bad == 0


def test_sanitizer_build_runs_clean(tmp_path):
    exe = pc.compile_driver(pc.BALANCE_SRC, str(tmp_path / "plan_balance_host_san"),
                            ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"],
                            maybe=["-static-libasan", "-static-libubsan"])  # the runtimes in the program itself
    for nn, ns, mq in SHAPES:
        chunks = _adversarial(nn, ns, mq, 7 + nn + ns)
        b0, b1, _, perms = pc.run_balance(exe, nn, ns, mq, chunks)
        assert (b1 <= b0).all()
        assert all((np.sort(p) == np.arange(len(c))).all() for c, p in zip(chunks, perms))
    nn, chunks = pc.recorded_chunks("p2tet_4x3x3.bin")
    b0, b1, _, _ = pc.run_balance(exe, nn, 2, 64, chunks, mode="placed")
    assert (b1 <= b0).all()
