#!/usr/bin/env python3
"""Timing of the per-cell expression pass (fa_eval_cells) against the same result composed from
torch ops, in one process on one GPU.

Contenders, alternated repetition by repetition after a warm-up, each timed with device events:
  (a) fem.evaluate(form, ("strain", "stress")) into preallocated outputs: one fa_eval_cells launch;
  (b) what a user without it writes: gather u[dofmap], per-cell inverse Jacobians, einsum, the linear
      law in torch (the baseline). The damage law has no torch restatement: (a) only there.
(a) and (b) are compared at the parity bar (1e-12 of the largest entry) at the sizes timed. Reported per
size: ms of each contender (median, min, max), the algorithmic bytes computed from the shapes (dofmap +
geometry dofmap + material + u + vertices read once, outputs written once) and the fraction of the
copy roof, measured in the same run with fa_hbm_probe (mode 0, copy).

  python tools/eval_cells_probe.py --out profiles/eval_cells/probe.json [--reps 20] [--scale 1.0]

--scale shrinks every mesh edge count (a rehearsal at toy size measures overheads only).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fem-libraries_amd"))

from femasm import _lib, fem, mesh  # noqa: E402

RTOL = 1e-12
# edges of the reference triangle / tetrahedron in basix order (the P2 edge nodes)
TRI_E = ((1, 2), (0, 2), (0, 1))
TET_E = ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))


def ref_gradients(td, p):
    """dphi [nn, td] of the P1 / P2 simplex basis at the midpoint (basix ordering)."""
    lam = np.full(td + 1, 1.0 / (td + 1))
    gl = np.concatenate([-np.ones((1, td)), np.eye(td)], 0)
    if p == 1:
        return gl
    rows = [(4.0 * lam[a] - 1.0) * gl[a] for a in range(td + 1)]
    rows += [4.0 * (lam[i] * gl[j] + lam[j] * gl[i]) for i, j in (TRI_E if td == 2 else TET_E)]
    return np.stack(rows)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def torch_strain_stress(V, u, lam, mu, dphi):
    """(b): strain and stress [nc, vs] at the midpoint of affine simplices, in torch."""
    m = V.mesh
    gd = m.gdim
    xv = m.x[m.cells.to(torch.int64)]  # [nc, nv, gd]
    J = (xv[:, 1:, :] - xv[:, :1, :]).transpose(1, 2)  # J[i][k] = x_{k+1}[i] - x_0[i]
    g = torch.matmul(dphi, torch.linalg.inv(J))  # [nc, nn, gd]
    ua = u.view(-1, gd)[V.dofmap.to(torch.int64)]  # [nc, nn, gd]
    G = torch.einsum("cai,caj->cij", ua, g)
    eps = 0.5 * (G + G.transpose(1, 2))
    tr = torch.diagonal(eps, dim1=1, dim2=2).sum(1)
    sig = 2.0 * mu[:, None, None] * eps + (lam * tr)[:, None, None] * torch.eye(gd, dtype=eps.dtype, device=eps.device)
    iu = torch.triu_indices(gd, gd, device=eps.device)
    return eps[:, iu[0], iu[1]].contiguous(), sig[:, iu[0], iu[1]].contiguous()


def copy_roof(dev, reps):
    """Measured copy rate (read + written bytes per second) of fa_hbm_probe mode 0 over 2 x 2 GiB."""
    L = _lib.load()
    n = 1 << 28
    src = torch.ones(n, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    sh = _lib.stream_handle(dev)

    def run():
        _lib.check(L.fa_hbm_probe(0, dst.data_ptr(), src.data_ptr(), n, sh), "fa_hbm_probe")

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = [timed(run) for _ in range(reps)]
    return 2.0 * n * 8 / (np.median(ms) * 1e-3), ms


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "reps": len(ms)}


def run_size(name, dev, reps, roof):
    kind, p, n = SIZES[name]
    if len(n) == 2:
        m = mesh.create_unit_square(*n, cell_type=mesh.CellType.triangle, device=dev)
    else:
        m = mesh.create_unit_cube(*n, cell_type=mesh.CellType.tetrahedron, device=dev)
    V = fem.functionspace(m, ("Lagrange", p, (m.gdim,)))
    nc, gd = m.num_cells, m.gdim
    g = torch.Generator().manual_seed(1)
    u = (1e-3 * (torch.rand(V.num_dofs, generator=g, dtype=torch.float64) - 0.5)).to(dev)
    E = (1e3 + 1e5 * torch.rand(nc, generator=g, dtype=torch.float64)).to(dev)
    if kind == "damage":
        d = torch.rand(V.num_nodes, generator=g, dtype=torch.float64)
        band = (m.x[:, 0].cpu() > 0.4) & (m.x[:, 0].cpu() < 0.6)
        d[~band] = 0.0  # a damage band
        a = fem.AsymDamage(V, E=E, nu=0.3, u=u, d=d.to(dev))
    else:
        a = fem.LinearElasticity(V, E=E, nu=0.3, u=u)
    vs = gd * (gd + 1) // 2
    out = {q: torch.empty((nc, vs), dtype=torch.float64, device=dev) for q in ("strain", "stress")}
    run_a = lambda: fem.evaluate(a, ("strain", "stress"), out=out)  # noqa: E731
    res = {"cells": nc, "nodes": V.num_nodes, "degree": p, "cell": m.cell_type.name, "law": kind}
    nbytes = nc * V.nn * 4 + nc * (gd + 1) * 4 + nc * 8 + V.num_nodes * gd * 8 + m.num_vertices * gd * 8 + 2 * nc * vs * 8
    if kind == "damage":
        nbytes += V.num_nodes * 8
    res["algorithmic_bytes"] = int(nbytes)
    run_b = None
    if kind == "linear":
        nu = 0.3
        mu = E / (2.0 * (1.0 + nu))
        lam = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
        dphi = torch.tensor(ref_gradients(gd, p), dtype=torch.float64, device=dev)
        keep = {}

        def run_b():
            keep["strain"], keep["stress"] = torch_strain_stress(V, u, lam, mu, dphi)

    for _ in range(3):
        run_a()
        if run_b:
            run_b()
    torch.cuda.synchronize()
    if run_b:
        for q in ("strain", "stress"):
            scale = float(keep[q].abs().max())
            err = float((out[q] - keep[q]).abs().max())
            res[f"{q}_rel_diff"] = err / scale
            if not err <= RTOL * scale:
                raise SystemExit(f"{name}: {q} of fa_eval_cells and the torch composition differ: rel {err / scale:.3e}")
    ta, tb = [], []
    for _ in range(reps):  # alternating
        ta.append(timed(run_a))
        if run_b:
            tb.append(timed(run_b))
    res["eval_cells"] = stats(ta)
    res["eval_cells"]["bytes_per_s"] = nbytes / (res["eval_cells"]["median_ms"] * 1e-3)
    res["eval_cells"]["fraction_of_copy_roof"] = res["eval_cells"]["bytes_per_s"] / roof
    if run_b:
        res["torch_composition"] = stats(tb)
        res["speedup_median"] = res["torch_composition"]["median_ms"] / res["eval_cells"]["median_ms"]
    print(name, json.dumps(res), flush=True)
    return res


SIZES = {
    "p1_tet_119": ("linear", 1, (119, 119, 119)),   # config C's mesh
    "p2_tet_100": ("linear", 2, (100, 100, 100)),
    "p1_tri_damage_2000": ("damage", 1, (2000, 2000)),  # the reference's own scale
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sizes", default=",".join(SIZES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this probe measures on the device only")
    if args.reps < 20 and args.scale == 1.0:
        raise SystemExit("--reps: at least 20 at full size")
    if args.scale != 1.0:
        for k, (kind, p, n) in list(SIZES.items()):
            SIZES[k] = (kind, p, tuple(max(2, int(round(v * args.scale))) for v in n))
    dev = torch.device("cuda", 0)
    roof, roof_ms = copy_roof(dev, max(args.reps, 5))
    rec = {"device": torch.cuda.get_device_name(0), "fa_version": _lib.load().fa_version(), "scale": args.scale,
           "copy_roof_bytes_per_s": roof, "copy_roof": stats(roof_ms), "sizes": {}}
    print("copy roof", json.dumps(rec["copy_roof"]), f"{roof / 1e12:.2f} TB/s", flush=True)
    for name in args.sizes.split(","):
        rec["sizes"][name] = run_size(name, dev, args.reps, roof)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
