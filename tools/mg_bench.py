#!/usr/bin/env python3
"""Timing of the geometric multigrid (femasm.mg), in one process on one GPU.

  --mode transfer   fa_prolong / fa_restrict / fa_cheb_step at the P2 <-> P1 level of an N^3 tetrahedron
                    mesh (bs 3: coarse lattice (N+1)^3, fine lattice (2N+1)^3), each call timed with
                    device events after a warm-up, as achieved GB/s of the bytes the call has to move
                    (every array once), beside fa_hbm_probe's copy over a vector of the fine size in the
                    same run.
  --mode solve      linear elasticity on P2 tetrahedra N^3 x 6 with bench.py's materials (E =
                    E_range[cell % 200], nu = 0.3) and bcs (x = 0 clamped, x = 1 prescribed), solved to
                    rtol by nls.KrylovSolver on the matrix-free operator, once with block-Jacobi and
                    once with mg.GeometricMultigrid: iterations, seconds to solution, the multigrid
                    set-up (update()), ms per V-cycle and the share of it spent in the fine action.

  --refine R        the same two modes on meshes without a lattice, made by mesh.refine. transfer: the
                    tetrahedron box N^3 with its lattice record dropped, refined R times; the last
                    refinement's fa_prolong_edges / fa_restrict_edges (bs 3) with the bytes they have to
                    move (vectors, markers and index tables once each). solve: tests/golden/square.msh
                    refined R times (or, with --box, the N^3 tetrahedron box without its lattice record),
                    Lagrange --degree, E per physical tag, same bcs.

  --amg             solve mode with mg.SmoothedAggregation: the mesh of the solve mode (lattice box, or with
                    --refine the refined square.msh / box) is rebuilt without its lattice record and without
                    its parents, so the package can only coarsen it algebraically. Reports levels, operator
                    complexity, set-up (the first update()), update() and per-apply times, the product-list
                    lengths of every algebraic transfer, and PCG iterations and solve time against
                    block-Jacobi; and, on the original mesh with its chain or lattice, against
                    mg.GeometricMultigrid.

Prints one JSON line.

  python tools/mg_bench.py --mode transfer --n 96 [--out profiles/multigrid/transfer_n96.json]
  python tools/mg_bench.py --mode solve --n 48 --rtol 1e-8 [--out profiles/multigrid/solve_n48.json]
  python tools/mg_bench.py --mode transfer --n 48 --refine 1 [--out profiles/multigrid/edge_transfer_n48_r1.json]
  python tools/mg_bench.py --mode solve --refine 3 --degree 1 --rtol 1e-10
  python tools/mg_bench.py --mode solve --amg --refine 6 --degree 1 [--out profiles/amg/square_r6_p1.json]
  python tools/mg_bench.py --mode solve --amg --n 32 [--out profiles/amg/box32_p2.json]

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

from femasm import _lib, fem, mesh, mg, nls  # noqa: E402
from femasm.materials import e_range  # noqa: E402


def timed(fn, steps: int, warmup: int) -> dict:
    """ms per call of fn (device events): median, min, max over `steps` calls after `warmup`."""
    t = []
    for it in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            t.append(e0.elapsed_time(e1))
    t.sort()
    return {"median": t[len(t) // 2], "min": t[0], "max": t[-1]}


def transfer_mode(args, dev) -> dict:
    n, bs = args.n, 3
    t = mg.Transfer(3, True, bs, (n, n, n))
    nf, nc = t.num_fine_dofs, t.num_coarse_dofs
    g = torch.Generator().manual_seed(1)
    rnd = lambda k: (torch.rand(k, generator=g, dtype=torch.float64) - 0.5).to(dev)
    xc, xf, rc, rf = rnd(nc), rnd(nf), rnd(nc), rnd(nf)
    mf = (torch.rand(nf, generator=g) < 0.05).to(torch.int8).to(dev)
    mc = (torch.rand(nc, generator=g) < 0.05).to(torch.int8).to(dev)
    Dinv = rnd(nf * bs).reshape(-1, bs, bs).contiguous()
    b, Ax, d = rnd(nf), rnd(nf), rnd(nf)
    even = nf - (nf & 1)
    L, sh = _lib.load(), _lib.stream_handle(dev)
    src, dst = rnd(even), torch.empty(even, dtype=torch.float64, device=dev)
    calls = {
        # name: (callable, bytes moved: every array once)
        "hbm_copy": (lambda: _lib.check(L.fa_hbm_probe(0, dst.data_ptr(), src.data_ptr(), even, sh)), 16 * even),
        "prolong": (lambda: mg.prolong(t, xc, xf), 8 * (nc + nf)),
        "prolong_add": (lambda: mg.prolong(t, xc, xf, add=True), 8 * (nc + 2 * nf)),
        "prolong_add_masked": (lambda: mg.prolong(t, xc, xf, bc_c=mc, bc_f=mf, add=True), 8 * (nc + 2 * nf) + nc + nf),
        "restrict": (lambda: mg.restrict(t, rf, rc), 8 * (nc + nf)),
        "restrict_masked": (lambda: mg.restrict(t, rf, rc, bc_f=mf, bc_c=mc), 8 * (nc + nf) + nc + nf),
        "cheb_step": (lambda: mg.cheb_step(Dinv, b, Ax, 0.3, 0.7, d, xf), 8 * nf * (bs + 6)),
    }
    res = {"fine_dofs": nf, "coarse_dofs": nc}
    for name, (fn, nbytes) in calls.items():
        ms = timed(fn, args.steps, args.warmup)
        res[name] = {"ms": ms, "bytes": int(nbytes), "GBps": nbytes / ms["median"] * 1e-6}
    for name in calls:
        if name != "hbm_copy":
            res[name]["of_copy"] = res[name]["GBps"] / res["hbm_copy"]["GBps"]
    return res


def unstructured_box(n, dev) -> mesh.Mesh:
    """The N^3 tetrahedron box without its lattice record: an unstructured mesh to the package."""
    b = mesh.create_box((1.0, 1.0, 1.0), (n, n, n), mesh.CellType.tetrahedron, device=dev)
    return mesh.Mesh(b.cell_type, b.x, b.cells, None, None)


def edge_transfer_mode(args, dev) -> dict:
    bs = 3
    m = unstructured_box(args.n, dev)
    for _ in range(args.refine - 1):
        m = mesh.refine(m)
    ev = mesh.entities(m, 1)[0]
    t = mg.EdgeTransfer(ev, m.num_vertices, bs)
    del ev
    nf, nc, ne, nv = t.num_fine_dofs, t.num_coarse_dofs, t.nedges, t.ncoarse
    g = torch.Generator().manual_seed(1)
    rnd = lambda k: (torch.rand(k, generator=g, dtype=torch.float64) - 0.5).to(dev)
    xc, xf, rc, rf = rnd(nc), rnd(nf), rnd(nc), rnd(nf)
    mf = (torch.rand(nf, generator=g) < 0.05).to(torch.int8).to(dev)
    mc = (torch.rand(nc, generator=g) < 0.05).to(torch.int8).to(dev)
    even = nf - (nf & 1)
    L, sh = _lib.load(), _lib.stream_handle(dev)
    src, dst = rnd(even), torch.empty(even, dtype=torch.float64, device=dev)
    pro_idx, res_idx = 8 * ne, 8 * (nv + 1) + 8 * ne  # edge_verts; vptr and vedges
    calls = {
        "hbm_copy": (lambda: _lib.check(L.fa_hbm_probe(0, dst.data_ptr(), src.data_ptr(), even, sh)), 16 * even),
        "prolong": (lambda: mg.prolong(t, xc, xf), 8 * (nc + nf) + pro_idx),
        "prolong_add": (lambda: mg.prolong(t, xc, xf, add=True), 8 * (nc + 2 * nf) + pro_idx),
        "prolong_add_masked": (lambda: mg.prolong(t, xc, xf, bc_c=mc, bc_f=mf, add=True),
                               8 * (nc + 2 * nf) + nc + nf + pro_idx),
        "restrict": (lambda: mg.restrict(t, rf, rc), 8 * (nc + nf) + res_idx),
        "restrict_masked": (lambda: mg.restrict(t, rf, rc, bc_f=mf, bc_c=mc), 8 * (nc + nf) + nc + nf + res_idx),
    }
    valence = t.vptr[1:] - t.vptr[:-1]
    res = {"refine": args.refine, "fine_nodes": nv + ne, "coarse_nodes": nv, "edges": ne, "fine_dofs": nf,
           "coarse_dofs": nc, "valence_max": int(valence.max()), "valence_mean": 2.0 * ne / nv}
    for name, (fn, nbytes) in calls.items():
        ms = timed(fn, args.steps, args.warmup)
        res[name] = {"ms": ms, "bytes": int(nbytes), "GBps": nbytes / ms["median"] * 1e-6}
    for name in calls:
        if name != "hbm_copy":
            res[name]["of_copy"] = res[name]["GBps"] / res["hbm_copy"]["GBps"]
    return res


def _krylov_run(args, A, b, M):
    """(result record, solution) of one PCG solve with preconditioner M (None: block-Jacobi)."""
    ks = nls.KrylovSolver(rtol=args.rtol, max_it=args.max_it)
    if M is not None:
        ks.set_preconditioner(M)
    x = torch.zeros_like(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ks.set_operator(A)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ks.solve(x, b)  # untimed: the first use of a kernel or a BLAS routine loads it
    torch.cuda.synchronize()
    t1w = time.perf_counter()
    its = ks.solve(x, b)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    r = b - A.mult(x)
    rec = {"iterations": its, "first_solve_s": t1w - t1, "setup_s": t1 - t0, "solve_s": t2 - t1w, "true_residual_rel": float(r.norm() / b.norm())}
    if M is not None:
        z = torch.empty_like(b)
        rec.update(levels=M.levels, operator_complexity=M.operator_complexity,
                   vcycle_ms=timed(lambda: M.apply(b, z), args.steps, args.warmup))
    return rec, x


def _linear_problem(args, m, dev):
    V = fem.functionspace(m, ("Lagrange", args.degree if args.refine else 2, (m.gdim,)))
    cid = m.cell_tags.to(torch.int64) if m.cell_tags is not None else \
        torch.arange(m.num_cells, device=dev, dtype=torch.int64)
    E = torch.tensor(e_range(), dtype=torch.float64, device=dev)[cid % 200]
    u = fem.Function(V)
    a = fem.LinearElasticity(V, E=E, nu=0.3, u=u)
    left = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.zeros_like(x[0])))
    right = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.ones_like(x[0])))
    bcs = [fem.dirichletbc(0.0, left, V), fem.dirichletbc([0.01] + [0.0] * (m.gdim - 1), right, V)]
    problem = nls.NonlinearProblem(a, u, bcs, matrix_free=True)
    b = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
    problem.F(u.x, b)
    return V, a, bcs, problem.matrix(), b


def amg_mode(args, dev) -> dict:
    n = args.n
    if args.refine:
        full = unstructured_box(n, dev) if args.box else \
            mesh.read_gmsh(os.path.join(ROOT, "tests", "golden", "square.msh"), gdim=2, device=dev)
        for _ in range(args.refine):
            full = mesh.refine(full)
    else:
        full = mesh.create_box((1.0, 1.0, 1.0), (n, n, n), mesh.CellType.tetrahedron, device=dev)
    m = mesh.Mesh(full.cell_type, full.x, full.cells, full.cell_tags, None)  # no lattice, no parents
    V, a, bcs, A, b = _linear_problem(args, m, dev)
    res = {"cells": m.num_cells, "dofs": V.num_dofs, "degree": V.degree, "rtol": args.rtol}
    res["jacobi"], xj = _krylov_run(args, A, b, None)
    M = mg.SmoothedAggregation(a, bcs, fine_operator=A, smoother_degree=args.smoother_degree,
                               coarse_dofs=args.coarse_dofs)
    res["amg"], xa = _krylov_run(args, A, b, M)  # setup_s: the first update() (aggregates, lists, prolongators)
    upd = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M.update()
        torch.cuda.synchronize()
        upd.append(time.perf_counter() - t0)
    res["amg"].update(update_s=sorted(upd)[1], rebuilds=M.rebuilds, updates=M.updates,
                      lmax=[getattr(L, "lmax", None) for L in M._levels])
    res["amg"]["transfers"] = [
        {"fine_nodes": tr.n, "aggregates": tr.nagg, "dead": int(tr.dead.sum()), "list_bytes": tr.list_bytes(),
         "lists": {k: dict(zip(("products", "blocks", "median", "max"), (p.nprod, p.nout) + p.list_stats()))
                   for k, p in (("A.T", tr.AT), ("A.P", tr.AP), ("Pt.Y", tr.PtY))}} for tr in M.transfers]
    res["amg"]["solutions_rel_diff"] = float((xa - xj).norm() / xj.norm())
    if full.structured is not None or full.parent is not None:
        Vg, ag, bcg, Ag, bg = _linear_problem(args, full, dev)
        G = mg.GeometricMultigrid(ag, bcg, fine_operator=Ag, smoother_degree=args.smoother_degree,
                                  coarse_dofs=args.coarse_dofs)
        res["gmg"], xg = _krylov_run(args, Ag, bg, G)
        # (a lattice mesh numbers its degree-2 nodes differently: compare the norms there)
        res["gmg"]["solutions_rel_diff"] = float((xg - xj).norm() / xj.norm()) if full.structured is None else \
            abs(float(xg.norm() / xj.norm()) - 1.0)
    return res


def solve_mode(args, dev) -> dict:
    n = args.n
    if args.refine:
        m = unstructured_box(n, dev) if args.box else \
            mesh.read_gmsh(os.path.join(ROOT, "tests", "golden", "square.msh"), gdim=2, device=dev)
        for _ in range(args.refine):
            m = mesh.refine(m)
        V = fem.functionspace(m, ("Lagrange", args.degree, (m.gdim,)))
    else:
        m = mesh.create_box((1.0, 1.0, 1.0), (n, n, n), mesh.CellType.tetrahedron, device=dev)
        V = fem.functionspace(m, ("Lagrange", 2, (3,)))
    cid = m.cell_tags.to(torch.int64) if m.cell_tags is not None else \
        torch.arange(m.num_cells, device=dev, dtype=torch.int64)
    E = torch.tensor(e_range(), dtype=torch.float64, device=dev)[cid % 200]
    u = fem.Function(V)
    a = fem.LinearElasticity(V, E=E, nu=0.3, u=u)
    left = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.zeros_like(x[0])))
    right = fem.locate_dofs_geometrical(V, lambda x: torch.isclose(x[0], torch.ones_like(x[0])))
    bcs = [fem.dirichletbc(0.0, left, V), fem.dirichletbc([0.01] + [0.0] * (m.gdim - 1), right, V)]
    problem = nls.NonlinearProblem(a, u, bcs, matrix_free=True)
    b = torch.zeros(V.num_dofs, dtype=torch.float64, device=dev)
    problem.F(u.x, b)
    A = problem.matrix()
    res = {"cells": m.num_cells, "dofs": V.num_dofs, "rtol": args.rtol}
    sols = {}
    for name in ("jacobi", "mg"):
        ks = nls.KrylovSolver(rtol=args.rtol, max_it=args.max_it)
        M = None
        if name == "mg":
            M = mg.GeometricMultigrid(a, bcs, fine_operator=A, smoother_degree=args.smoother_degree,
                                      coarse_dofs=args.coarse_dofs)
            ks.set_preconditioner(M)
        x = torch.zeros_like(b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ks.set_operator(A)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        its = ks.solve(x, b)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        r = b - A.mult(x)
        res[name] = {"iterations": its, "setup_s": t1 - t0, "solve_s": t2 - t1,
                     "true_residual_rel": float(r.norm() / b.norm())}
        sols[name] = x
        if M is not None:
            z = torch.empty_like(b)
            cyc = timed(lambda: M.apply(b, z), args.steps, args.warmup)
            y = torch.empty_like(b)
            act = timed(lambda: A.mult(x, y), args.steps, args.warmup)
            fine_actions = 2 * M.smoother_degree  # pre: degree - 1, residual: 1, post: degree
            res[name].update(levels=M.levels, operator_complexity=M.operator_complexity, vcycle_ms=cyc,
                             fine_action_ms=act, fine_actions_per_cycle=fine_actions,
                             fine_action_share=fine_actions * act["median"] / cyc["median"],
                             lmax=[getattr(L, "lmax", None) for L in M._levels])
    res["solutions_rel_diff"] = float((sols["mg"] - sols["jacobi"]).norm() / sols["jacobi"].norm())
    res["speedup_solve"] = res["jacobi"]["solve_s"] / res["mg"]["solve_s"]
    res["speedup_with_setup"] = (res["jacobi"]["solve_s"] + res["jacobi"]["setup_s"]) / \
        (res["mg"]["solve_s"] + res["mg"]["setup_s"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mode", choices=("transfer", "solve"), default="transfer")
    ap.add_argument("--n", type=int, default=96)
    ap.add_argument("--refine", type=int, default=0, help="refine an unstructured mesh this many times")
    ap.add_argument("--box", action="store_true", help="solve --refine: the N^3 tetrahedron box, not square.msh")
    ap.add_argument("--degree", type=int, default=2, help="solve --refine: Lagrange degree")
    ap.add_argument("--amg", action="store_true", help="solve: smoothed aggregation on the mesh without lattice or parents")
    ap.add_argument("--coarse-dofs", type=int, default=6000)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--max-it", type=int, default=20000)
    ap.add_argument("--smoother-degree", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mg_bench: no GPU found (timings are taken on the device only)")
    dev = torch.device("cuda", 0)
    res = {"tool": "mg_bench", "mode": args.mode, "n": args.n, "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    if args.refine < 0:
        sys.exit("mg_bench: --refine must not be negative")
    if args.mode == "solve":
        res.update(amg_mode(args, dev) if args.amg else solve_mode(args, dev))
    else:
        res.update(edge_transfer_mode(args, dev) if args.refine else transfer_mode(args, dev))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
