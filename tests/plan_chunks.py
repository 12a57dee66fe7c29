"""Helpers of the quarter-placement tests (test_plan_balance_host.py, test_gpu_plan_balance.py): the host
drivers (tools/plan_order/plan_balance_host.cpp: k_plan_perm's greedy fill and the exchange descent that was
measured and left out of the plan; csrc/plan_order_host.cpp), the chunk fixtures, and the chunks of a device plan.

A chunk is na adjacency entries with NN residues each (slot mod 16 of every block). k_plan_perm visits
them in the order j = (jj * st) mod na (gather_perm) and places them into 16-lane quarters of
EQ = 16 / NSPLIT entries; eperm[position] = j."""
import os
import shutil
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fem-libraries_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_order")
BALANCE_SRC = os.path.join(ROOT, "tools", "plan_order", "plan_balance_host.cpp")


def cxx():
    for c in (os.environ.get("CXX"), "g++", "clang++", "c++", "/opt/rocm/llvm/bin/clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    raise RuntimeError("no C++ compiler for the host drivers")


def compile_driver(src, out, flags=("-O2",), maybe=()):
    """maybe: flags dropped if the compiler does not know them"""
    base = [cxx(), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags]
    tail = [src if os.path.isabs(src) else os.path.join(CSRC, src), "-o", out]
    r = subprocess.run(base + list(maybe) + tail, capture_output=True, text=True)
    if r.returncode != 0 and maybe:
        r = subprocess.run(base + tail, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def visit_order(na):
    """k_plan_perm's visiting order of a chunk's entries (gather_perm_stride, gather_perm)"""
    st = 97
    while na % st == 0 and st > 1:
        st -= 2
    return (np.arange(na, dtype=np.int64) * st) % na


def run_balance(exe, nn, ns, mq, chunks, mode=None):
    """mode: None (fill, then exchanges), "placed" (exchanges on the given placement), "fill" (the fill alone).
    chunks: list of [na, nn] residue arrays in the driver's input order ->
    (bound after the fill [n], bound after the descent [n], exchanges [n], list of perms)"""
    blob = bytearray()
    for c in chunks:
        assert c.ndim == 2 and c.shape[1] == nn
        blob += len(c).to_bytes(2, "little") + np.ascontiguousarray(c, np.uint8).tobytes()
    r = subprocess.run([exe, str(nn), str(ns), str(mq)] + ([mode] if mode else []), input=bytes(blob),
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stderr == b"", r.stderr.decode()[-2000:]
    out = np.frombuffer(r.stdout, "<u2").astype(np.int64)
    b0, b1, mv, perms, at = [], [], [], [], 0
    for c in chunks:
        b0.append(out[at])
        b1.append(out[at + 1])
        mv.append(out[at + 2])
        perms.append(out[at + 3:at + 3 + len(c)])
        at += 3 + len(c)
    assert at == len(out)
    return np.array(b0), np.array(b1), np.array(mv), perms


def bound_of(res, nn, ns):
    """sum over the quarters of max(NBG, largest residue total) of entries [na, nn] in position order"""
    eq, nbg = 16 // ns, nn // ns
    s = 0
    for p0 in range(0, len(res), eq):
        s += max(nbg, int(np.bincount(res[p0:p0 + eq].reshape(-1), minlength=16).max()))
    return s


def greedy_fill(res, nn, ns):
    """the fill of k_plan_perm in plain Python: entries [na, nn] in visiting order -> perm (position -> index)"""
    eq = 16 // ns
    na = len(res)
    nq = (na + eq - 1) // eq
    h = np.zeros((nq, 16), np.int64)
    fill = [0] * nq
    perm = np.zeros(na, np.int64)
    for i in range(na):
        best, bc = -1, 1 << 30
        for q in range(nq):
            if fill[q] >= (eq if q + 1 < nq else na - eq * (nq - 1)):
                continue
            cost = int(h[q][res[i]].sum())
            if cost < bc:
                bc, best = cost, q
        perm[best * eq + fill[best]] = i
        fill[best] += 1
        np.add.at(h[best], res[i], 1)
    return perm


def quarters_of(chunks, perms, nn, ns):
    """the quarters of placed chunks as plan_order_host reads them: (nl [n], res [n, 16, NBG])"""
    nbg = nn // ns
    nls, ress = [], []
    for c, p in zip(chunks, perms):
        lanes = c[p].reshape(-1, nbg)
        for l0 in range(0, len(lanes), 16):
            full = np.zeros((16, nbg), np.uint8)
            nl = min(16, len(lanes) - l0)
            full[:nl] = lanes[l0:l0 + nl]
            nls.append(nl)
            ress.append(full)
    return np.array(nls, np.int64), np.stack(ress)


def run_order(exe, nbg, nl, res):
    """plan_order_host: (passes [n], bound [n]) of the default plan's order"""
    n = len(nl)
    rec = np.zeros((n, 1 + 16 * nbg), np.uint8)
    rec[:, 0] = nl
    rec[:, 1:] = res.reshape(n, -1)
    r = subprocess.run([exe, str(nbg), "1"], input=rec.tobytes(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    heads = np.frombuffer(r.stdout, np.uint8).reshape(n, 8 + 16 * nbg)[:, :8].copy().view("<u2").astype(np.int64)
    return heads[:, 0], heads[:, 3]


def recorded_quarters(name):
    """tests/golden/plan_order/p2tet_*.bin (test_plan_order_host._golden): (nbg, nl [n], res [n, 16, nbg])"""
    with open(os.path.join(GOLDEN, name), "rb") as f:
        raw = zlib.decompress(f.read())
    nbg, n = int(raw[0]), int.from_bytes(raw[1:5], "little")
    nl = np.frombuffer(raw, np.uint8, n, 5).astype(np.int64)
    nib = np.frombuffer(raw, np.uint8, offset=5 + n)
    res = np.stack([nib & 15, nib >> 4], axis=1).reshape(-1)[:n * 16 * nbg].reshape(n, 16, nbg)
    return nbg, nl, res


def recorded_chunks(name, ns=2, mq=64):
    """the recorded quarters regrouped: a quarter of fewer than 16 lanes ends a chunk (a chunk whose last
    quarter is full runs on into the next one; at most mq quarters); lanes ns j .. ns j + ns - 1 are one
    entry. Returns nn and the chunks' entries [na, nn] in position order."""
    nbg, nl, res = recorded_quarters(name)
    nn = nbg * ns
    chunks, q0 = [], 0
    for q in range(len(nl)):
        if nl[q] < 16 or q + 1 - q0 == mq or q + 1 == len(nl):
            lanes = res[q0:q + 1].reshape(-1, nbg)[:16 * (q - q0) + nl[q]]
            chunks.append(lanes.reshape(-1, nn).astype(np.uint8))
            q0 = q + 1
    return nn, chunks


# ---- chunk fixtures recorded from a device plan: entries in adjacency order, and the device's eperm ----

def save_chunks(path, nn, ns, chunks, eperms):
    raw = bytearray(bytes([nn, ns]) + len(chunks).to_bytes(4, "little"))
    for c, p in zip(chunks, eperms):
        flat = np.append(c.reshape(-1).astype(np.uint8), np.zeros(c.size % 2, np.uint8))
        raw += len(c).to_bytes(2, "little") + (flat[0::2] | (flat[1::2] << 4)).astype(np.uint8).tobytes()
        raw += np.asarray(p, "<u2").tobytes()
    with open(path, "wb") as f:
        f.write(zlib.compress(bytes(raw), 9))


def load_chunks(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        raw = zlib.decompress(f.read())
    nn, ns, n = raw[0], raw[1], int.from_bytes(raw[2:6], "little")
    at, chunks, eperms = 6, [], []
    for _ in range(n):
        na = int.from_bytes(raw[at:at + 2], "little")
        nb = (na * nn + 1) // 2
        nib = np.frombuffer(raw, np.uint8, nb, at + 2)
        chunks.append(np.stack([nib & 15, nib >> 4], axis=1).reshape(-1)[:na * nn].reshape(na, nn))
        eperms.append(np.frombuffer(raw, "<u2", na, at + 2 + nb).astype(np.int64))
        at += 2 + nb + 2 * na
    assert at == len(raw)
    return nn, ns, chunks, eperms


def plan_chunks(V, which=0):
    """The chunks of V's cached gather plan number `which` (positional; one per row part), on the CPU: ns, and
    per chunk its entries' residues by block [na, nn] in adjacency order and the device's eperm [na]. From
    the ordered slot words ((block << 10) | chunk-relative slot, by position) and eadj (the adjacency values
    in position order: a chunk's entries are distinct (cell, node) pairs)."""
    rec = list(V._plans.values())[which]
    plan, rs, smap, eadj = rec[0], rec[1], rec[3], rec[4]
    assert eadj is not None and plan.slot_order > 0, "not a positional plan"
    nn, ns = V.nn, int(plan.slot_order)
    nch = int(plan.nchunks)
    ptr, idx = (t.cpu().numpy().astype(np.int64) for t in V.adjacency()[:2])
    rs = rs.cpu().numpy()[:nch + 1].astype(np.int64)
    words = smap.cpu().numpy().view(np.uint16).reshape(-1, nn).astype(np.int64)
    eadj = eadj.cpu().numpy().astype(np.int64)
    chunks, eperms = [], []
    for c in range(nch):
        a0, a1 = ptr[rs[c]], ptr[rs[c + 1]]
        if a1 <= a0:
            continue
        ids = idx[a0:a1]
        order = np.argsort(ids, kind="stable")
        eperm = order[np.searchsorted(ids[order], eadj[a0:a1])]
        assert (ids[eperm] == eadj[a0:a1]).all(), "eadj is not a permutation of the chunk's adjacency"
        w = words[a0:a1]                                  # by position
        bypos = np.zeros_like(w)
        np.put_along_axis(bypos, w >> 10, w & 15, axis=1)  # residue of block b
        res = np.zeros_like(bypos)
        res[eperm] = bypos
        chunks.append(res.astype(np.uint8))
        eperms.append(eperm)
    return ns, chunks, eperms
