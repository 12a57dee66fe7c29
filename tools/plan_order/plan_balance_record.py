"""Record the chunks of device plans with the eperm k_plan_perm wrote, as fixtures for
tests/test_plan_balance_host.py (tests/golden/plan_order/chunks_*.bin; format: tests/plan_chunks.py).
P2 tetrahedra on the (4,3,3) box (every chunk) and the 16^3 cube (every 8th chunk, to stay small).

usage: python tools/plan_order/plan_balance_record.py OUTDIR"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "fem-libraries_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    import torch

    import plan_chunks as pc
    from femasm import fem, mesh

    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    dev = torch.device("cuda", 0)
    for name, dims, every in (("chunks_p2tet_4x3x3.bin", (4, 3, 3), 1), ("chunks_p2tet_16.bin", (16, 16, 16), 8)):
        m = mesh.create_unit_cube(*dims, cell_type=mesh.CellType.tetrahedron, device=dev)
        V = fem.functionspace(m, ("Lagrange", 2, (3,)))
        a = fem.form(fem.LinearElasticity(V, E=1.0, nu=0.3))
        A = fem.create_matrix(a)
        fem.gather_plan(V, A, 0, a.kind)
        torch.cuda.synchronize()
        ns, chunks, eperms = pc.plan_chunks(V)
        path = os.path.join(out, name)
        pc.save_chunks(path, V.nn, ns, chunks[::every], eperms[::every])
        print(f"{name}: {len(chunks[::every])} of {len(chunks)} chunks, {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
