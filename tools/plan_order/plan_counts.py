"""LDS pass counts of a positional gather plan, on the device, for a bench.py config: for every chunk,
16-lane quarter and step the largest number of the quarter's lanes whose block slot has the same residue
mod 16, summed (the passes), against the per-quarter bound max(steps, largest residue total). The same
count as tools/r4/plan_stats.py, vectorised so that config E's 63 M quarters take seconds.

usage: python tools/plan_order/plan_counts.py [--config E|Eneo|C|B] [--n N] [--search] [--root TREE]
           [--dump FILE]
--root: import femasm from another checkout (a build of the parent commit), to count its plans.
--dump: write the plan's quarters (lanes and residues, the input of csrc/plan_order_host.cpp) as a
        zlib-packed fixture for tests/test_plan_order_host.py."""
import argparse
import os
import sys
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="E")
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--dims", type=int, nargs="+", default=None, help="unit-cube cells per side instead of --n")
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)))
    ap.add_argument("--dump", default=None)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "fem-libraries_amd"))
    import torch

    import bench
    from femasm import fem, mesh

    dev = torch.device("cuda", 0)
    cfg = bench.CONFIGS[args.config]
    if args.dims:
        m = mesh.create_unit_cube(*args.dims, cell_type=mesh.CellType[cfg["cell"]], device=dev)
        V = fem.functionspace(m, ("Lagrange", cfg["degree"], (3,)))
        a = fem.form(fem.LinearElasticity(V, E=1.0, nu=0.3))
    else:
        m, V, a, _ = bench.build_problem(args.n or cfg["n"], dev, cfg=cfg)
    A = fem.create_matrix(a)
    assert len(A.parts) == 1
    torch.cuda.synchronize()
    t0 = time.time()
    fem.gather_plan(V, A, 0, a.kind, search=args.search)
    torch.cuda.synchronize()
    plan_s = time.time() - t0
    (rec,) = V._plans.values()
    plan, rs, smap, eadj = rec[0], rec[1], rec[3], rec[4]
    assert eadj is not None and plan.slot_order > 0, "not a positional plan"
    nn, ns = V.nn, int(plan.slot_order)
    nbg = nn // ns
    nch = int(plan.nchunks)
    ptr = V.adjacency()[0].to(torch.int64)
    a0 = ptr[rs[:nch]]                                   # first adjacency entry of each chunk
    na = ptr[rs[1:nch + 1]] - a0
    nqc = (na * ns + 15) // 16                           # quarters per chunk
    qoff = torch.cumsum(nqc, 0) - nqc
    words = smap.view(-1, nn)
    passes = bound = lanes = quarters = 0
    dump_nl, dump_res = [], []
    step = max(1, 4_000_000 // max(1, int(na.max())))    # chunks per slab
    for c0 in range(0, nch, step):
        c1 = min(nch, c0 + step)
        e0, e1 = int(a0[c0]), int(a0[c1 - 1] + na[c1 - 1])
        if e1 <= e0:
            continue
        ent = torch.arange(e0, e1, device=dev)
        # chunk of each entry (an empty chunk shares its a0 with the next one: right=True picks the last)
        ch = torch.searchsorted(a0[c0:c1].contiguous(), ent, right=True) - 1 + c0
        pos = ent - a0[ch]
        res = (words[e0:e1].to(torch.int32) & 15).view(-1, ns, nbg)    # [entries, parts, steps]
        lane = pos[:, None] * ns + torch.arange(ns, device=dev)[None, :]
        q0 = int(qoff[c0])
        nq = int(qoff[c1 - 1] + nqc[c1 - 1]) - q0
        qid = (qoff[ch] - q0)[:, None] + lane // 16                    # [entries, parts]
        cnt = torch.zeros(nq * nbg * 16, dtype=torch.int32, device=dev)
        idx = (qid[:, :, None] * nbg + torch.arange(nbg, device=dev)[None, None, :]) * 16 + res
        cnt.scatter_add_(0, idx.reshape(-1), torch.ones(idx.numel(), dtype=torch.int32, device=dev))
        cnt = cnt.view(nq, nbg, 16)
        passes += int(cnt.amax(dim=2).sum())
        bound += int(cnt.sum(dim=1).amax(dim=1).clamp(min=nbg).sum())
        lanes += int(lane.numel())
        quarters += nq
        if args.dump:
            nl = torch.zeros(nq, dtype=torch.int64, device=dev)
            nl.scatter_add_(0, qid.reshape(-1), torch.ones(qid.numel(), dtype=torch.int64, device=dev))
            # the order kernel's input: every lane's residues by block, not by step
            blk = (((words[e0:e1].to(torch.int32) & 0xFFFF) >> 10) % nbg).view(-1, ns, nbg).long()
            byblock = torch.zeros_like(res).scatter_(2, blk, res)
            r = torch.zeros(nq, 16, nbg, dtype=torch.uint8, device=dev)
            r[qid.reshape(-1), (lane % 16).reshape(-1)] = byblock.reshape(-1, nbg).to(torch.uint8)
            dump_nl.append(nl.to(torch.uint8).cpu())
            dump_res.append(r.cpu())
    print(f"config {args.config} n={args.dims or args.n or cfg['n']} plan={'search' if args.search else 'default'} "
          f"root={os.path.relpath(root)}: chunks {nch} quarters {quarters} lanes {lanes} NBG {nbg} "
          f"passes {passes} bound {bound} passes/bound {passes / bound:.4f} "
          f"passes/quarter-step {passes / (quarters * nbg):.4f} plan_s {plan_s:.2f}", flush=True)
    if args.dump:
        import numpy as np

        nl = torch.cat(dump_nl).numpy()
        res = torch.cat(dump_res).numpy().reshape(-1)
        res = np.append(res, np.zeros(res.size % 2, np.uint8))
        nib = (res[0::2] | (res[1::2] << 4)).astype(np.uint8)
        raw = bytes([nbg]) + len(nl).to_bytes(4, "little") + nl.tobytes() + nib.tobytes()
        with open(args.dump, "wb") as f:
            f.write(zlib.compress(raw, 9))
        print(f"wrote {args.dump}: {len(nl)} quarters, {os.path.getsize(args.dump)} bytes")


if __name__ == "__main__":
    main()
