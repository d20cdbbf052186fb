"""bench.py's plain line and its output dump (--dump-outputs): what the timed path returned in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_keeps_a_fixed_sample_of_a_large_output(tmp_path):
    """An output above the limit is cut to the same rows at every run (their indices beside it), and the directory
    stays within the limit; a small one is written whole, in float64."""
    import bench
    big = np.arange(1100 * 9000, dtype=np.float64).reshape(1100, 9000)  # 79.2 MB
    small = np.linspace(0.0, 1.0, 7, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": big, "y": small})
        total = sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d))
        assert total <= bench.DUMP_LIMIT_BYTES
    rows = np.load(tmp_path / "a" / "x_rows.npy")
    assert np.array_equal(rows, np.load(tmp_path / "b" / "x_rows.npy"))
    assert rows.dtype == np.float64 and 0 < rows.size < big.shape[0] and np.all(np.diff(rows) > 0)
    x = np.load(tmp_path / "a" / "x.npy")
    assert x.dtype == np.float64 and np.array_equal(x, big[rows.astype(np.int64)])
    y = np.load(tmp_path / "a" / "y.npy")
    assert y.dtype == np.float64 and np.array_equal(y, small.astype(np.float64))
    assert not os.path.exists(tmp_path / "a" / "y_rows.npy")


@pytest.mark.gpu
def test_plain_bench_line_and_its_dump_match_the_oracle(tmp_path):
    """A plain run prints the headline fields only, times exactly --steps steps, and dumps the x of its last circuit:
    config 2's grid(100), against the oracle's SuperLU solve."""
    from nodal_amd import generators as gen
    from oracle import nodal_oracle as oracle
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg2", "--steps", "2",
                        "--warmup", "1", "--per-step", "1", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    for key in ("roofline", "cpu_baseline", "reuse_symbolic", "concurrent", "also"):
        assert key not in line, key
    x = np.load(out / "x.npy")
    G, A = oracle.assemble_fast(gen.grid_table(100))
    xo, _ = oracle.solve(G.tocsr(), A, True)
    assert x.dtype == np.float64 and x.shape == xo.shape
    assert np.abs(x - xo).max() <= 1e-9 * np.abs(xo).max()
