"""bench.py --dump-outputs / --full: the dump holds the matrix values a caller of the timed path
receives (every block, or the same seeded sample in every run), and a plain run carries the headline
figure without the secondary measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _matrix(nrows=40, bs=3, max_part_bytes=8 * 9 * 64):
    """A BSR matrix on the host with 1..5 blocks per row, split into several row parts."""
    from femasm.la import MatrixCSR

    rng = np.random.default_rng(3)
    per_row = rng.integers(1, 6, nrows)
    indptr = torch.tensor(np.concatenate([[0], np.cumsum(per_row)]), dtype=torch.int64)
    indices = torch.tensor(np.concatenate([np.sort(rng.choice(nrows, k, replace=False)) for k in per_row]),
                           dtype=torch.int32)
    A = MatrixCSR(indptr, indices, bs, max_part_bytes=max_part_bytes)
    for _, _, d in A.parts:
        d.copy_(torch.tensor(rng.standard_normal(tuple(d.shape))))
    return A


def _load(d):
    return [np.load(os.path.join(d, f"{n}.npy")) for n in ("values", "block_positions", "block_columns")]


def test_dump_whole_matrix(tmp_path):
    import bench

    A = _matrix()
    assert len(A.parts) > 1
    info = bench.dump_outputs(A, str(tmp_path / "d"))
    vals, pos, cols = _load(tmp_path / "d")
    assert info == {"blocks": A.num_blocks, "of": A.num_blocks, "sampled": False}
    assert vals.dtype == pos.dtype == cols.dtype == np.float64
    assert np.array_equal(pos, np.arange(A.num_blocks))
    assert np.array_equal(vals, A.data.numpy())
    assert np.array_equal(cols, A.indices.numpy())


def test_dump_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    import bench

    A = _matrix()
    cap = 17
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", cap * 8 * (A.bs * A.bs + 2))
    info = bench.dump_outputs(A, str(tmp_path / "a"))
    assert info == {"blocks": cap, "of": A.num_blocks, "sampled": True}
    vals, pos, cols = _load(tmp_path / "a")
    assert vals.nbytes + pos.nbytes + cols.nbytes <= bench.DUMP_MAX_BYTES
    p = pos.astype(np.int64)
    assert np.all(np.diff(p) > 0) and p[0] >= 0 and p[-1] < A.num_blocks
    assert np.array_equal(vals, A.data.numpy()[p])
    assert np.array_equal(cols, A.indices.numpy()[p])
    # another run, other values: the same positions
    for _, _, d in A.parts:
        d.mul_(2.0)
    bench.dump_outputs(A, str(tmp_path / "b"))
    vals2, pos2, _ = _load(tmp_path / "b")
    assert np.array_equal(pos2, pos)
    assert np.array_equal(vals2, 2.0 * vals)


def test_dump_limit_is_below_64_MB():
    import bench

    assert bench.DUMP_MAX_BYTES + 3 * 4096 <= 64_000_000


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """One plain run of the benchmark on a 6^3 x 6 P2 mesh: the line's headline fields, no secondary
    measurement, and a dump equal to an assembly of the same problem in this process."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--side", "6", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["unit"] == "Melements/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    ncells = 6 ** 3 * 6
    assert line["value"] == pytest.approx(ncells / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    assert line["cpu_baseline"] is None and line["eneo"] is None and line["roofline"]["peak_measured"] is None

    import bench
    from femasm import fem

    dev = torch.device("cuda", 0)
    m, V, a, bcs = bench.build_problem(6, dev, cfg=bench.CONFIGS["E"])
    A = fem.assemble_matrix(a, bcs=bcs)
    torch.cuda.synchronize()
    vals, pos, cols = _load(out)
    assert np.array_equal(pos, np.arange(A.num_blocks))
    assert np.array_equal(cols, A.indices.cpu().numpy())
    ref = A.data.cpu().numpy()
    # two runs of the (non-deterministic-order) gather differ by summation order only: a few ulps of the
    # largest entry of a block row; 1e-12 is the project's parity bar (tests/rowparity.py)
    assert np.abs(vals - ref).max() <= 1e-12 * np.abs(ref).max()
