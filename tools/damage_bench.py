#!/usr/bin/env python3
"""Timing of the damage field (fem.damage_field), in one process on one GPU.

Workload: create_rectangle triangles N x N x 2 (default N = 2000: 8 M cells, 4 M vertices, the reference's
scale), the edges on a strip |x - 1/2| <= --strip marked, --iterations spreading iterations (default 8: an
unrefined mesh's default).

Timed:
  entities       mesh.entities(m, 1), which the graph is built from (host clock around a synchronise)
  graph          mesh.vertex_graph from those edges: indptr, indices, inv_deg (the same)
  spread         fa_vertex_spread, all 2 * iterations passes in one call (device events), and per pass
  torch_*        the same passes in plain torch ops on the device, what a user would write without the
                 kernel: gather d[indices], then a segmented sum by index_add_ (atomics: the order of a
                 row's adds is not fixed) or by segment_reduce
  hbm_copy       fa_hbm_probe's copy over two 4 GiB buffers, best of 5: the stream peak bench.py --full reports

Each timing is the median of --steps runs after --warmup. Per pass the kernel has to stream 4 nnz + 40 nv
bytes (indices; indptr, inv_deg, d read and d written; the neighbour gathers of d hit cache); `of_copy` is
that count over the pass time, as a fraction of the measured copy rate. The torch results are compared with
the kernel's (bitwise for segment_reduce when it sums in order; index_add_ to rounding).

Prints one JSON line.

  python tools/damage_bench.py [--n 2000] [--out profiles/damage_field/bench.txt]

Fails when no GPU is found: a CPU run has no timing to give.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fem-libraries_amd"))

from femasm import _lib, fem, mesh  # noqa: E402


def _stats(t: list) -> dict:
    t = sorted(t)
    return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}


def timed(fn, steps: int, warmup: int, before=None) -> dict:
    """ms per call of fn (device events): median, min, max over `steps` calls after `warmup`; `before` runs
    untimed ahead of every call."""
    t = []
    for it in range(warmup + steps):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            t.append(e0.elapsed_time(e1))
    return _stats(t)


def host_timed(fn, steps: int, warmup: int, before=None) -> dict:
    """ms per call of fn on the host clock, the device synchronised before and after."""
    t = []
    for it in range(warmup + steps):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return _stats(t)


def hbm_copy(dev, gib: float = 4.0, reps: int = 5) -> float:
    """GB/s of fa_hbm_probe's copy (read + write bytes) over two `gib` GiB buffers, best of `reps`."""
    L, sh = _lib.load(), _lib.stream_handle(dev)
    n = int(gib * (1 << 30)) // 8 // 2 * 2
    a = torch.ones(n, dtype=torch.float64, device=dev)
    b = torch.empty(n, dtype=torch.float64, device=dev)
    ms = timed(lambda: _lib.check(L.fa_hbm_probe(0, b.data_ptr(), a.data_ptr(), n, sh), "fa_hbm_probe"), reps, 1)
    del a, b
    torch.cuda.empty_cache()
    return 16 * n / ms["min"] * 1e-6


def torch_passes(d, idx, row, inv_deg, lengths, iterations: int, threshold: float, how: str):
    """The definition's passes in torch ops: an nnz-long gather, then a segmented sum."""
    def sums(f):
        g = f[idx]
        if how == "segment_reduce":
            return torch.segment_reduce(g, "sum", lengths=lengths)
        return torch.zeros_like(f).index_add_(0, row, g)

    for _ in range(iterations):
        s = torch.where(d < threshold, sums(d), torch.zeros_like(d))
        d = torch.maximum(s * inv_deg, d)
        d = torch.maximum(sums(d) * inv_deg, d)
    return d


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=2000, help="squares per side (N x N x 2 triangles)")
    ap.add_argument("--strip", type=float, default=0.01, help="half width of the marked strip around x = 1/2")
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--build-steps", type=int, default=3, help="timed runs of the entity and graph builds")
    ap.add_argument("--no-hbm-probe", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("damage_bench: no GPU found (timings are taken on the device only)")
    dev = torch.device("cuda", 0)
    res = {"tool": "damage_bench", "n": args.n, "iterations": args.iterations, "threshold": args.threshold,
           "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    if not args.no_hbm_probe:
        res["hbm_copy_GBps"] = hbm_copy(dev)

    m = mesh.create_rectangle((1.0, 1.0), (args.n, args.n), mesh.CellType.triangle, device=dev)
    nv = m.num_vertices
    res["entities_ms"] = host_timed(lambda: mesh.entities(m, 1), args.build_steps, 1,
                                    before=lambda: m.__dict__.pop("_entities", None))
    res["graph_ms"] = host_timed(lambda: mesh.vertex_graph(m), args.build_steps, 1,
                                 before=lambda: m.__dict__.pop("_vgraph", None))
    indptr, indices, inv_deg = mesh._vertex_graph(m)
    nnz = int(indices.numel())
    ev = mesh.entities(m, 1)[0]
    xm = m.x[:, 0]
    on = ((xm[ev[:, 0]] - 0.5).abs() <= args.strip) & ((xm[ev[:, 1]] - 0.5).abs() <= args.strip)
    edges = torch.nonzero(on).reshape(-1)
    d0 = fem.mark_vertices(m, 1, edges)
    deg = indptr[1:] - indptr[:-1]
    res.update(cells=m.num_cells, vertices=nv, nnz=nnz, marked_edges=int(edges.numel()),
               marked_vertices=int((d0 > 0).sum()), degree_max=int(deg.max()), degree_mean=nnz / nv)

    L, sh = _lib.load(), _lib.stream_handle(dev)
    d, tmp = d0.clone(), torch.empty_like(d0)
    passes = 2 * args.iterations
    spread_ms = timed(lambda: _lib.check(L.fa_vertex_spread(nv, indptr.data_ptr(), indices.data_ptr(),
                                                            inv_deg.data_ptr(), d.data_ptr(), tmp.data_ptr(),
                                                            args.iterations, args.threshold, sh), "fa_vertex_spread"),
                      args.steps, args.warmup, before=lambda: d.copy_(d0))
    pass_bytes = 4 * nnz + 40 * nv
    per_pass = spread_ms["median"] / passes
    res["spread"] = {"ms": spread_ms, "passes": passes, "ms_per_pass": per_pass, "bytes_per_pass": pass_bytes,
                     "GBps": pass_bytes / per_pass * 1e-6}
    if "hbm_copy_GBps" in res:
        res["spread"]["of_copy"] = res["spread"]["GBps"] / res["hbm_copy_GBps"]
    public = fem.spread(m, d0, args.iterations, args.threshold)
    res["spread"]["equals_public_api"] = bool(torch.equal(public, d))
    res["positive_vertices"] = int((d > 0).sum())

    idx = indices.to(torch.int64)
    row = torch.repeat_interleave(torch.arange(nv, dtype=torch.int64, device=dev), deg)
    for how in ("index_add", "segment_reduce"):
        try:
            out = torch_passes(d0, idx, row, inv_deg, deg, args.iterations, args.threshold, how)
        except (RuntimeError, NotImplementedError, AttributeError) as e:
            res[f"torch_{how}"] = {"error": str(e).splitlines()[0][:200]}
            continue
        ms = timed(lambda: torch_passes(d0, idx, row, inv_deg, deg, args.iterations, args.threshold, how),
                   args.steps, args.warmup)
        res[f"torch_{how}"] = {"ms": ms, "ms_per_pass": ms["median"] / passes,
                               "kernel_speedup": ms["median"] / spread_ms["median"],
                               "bitwise_equal_to_kernel": bool(torch.equal(out, d)),
                               "max_abs_diff_to_kernel": float((out - d).abs().max())}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
