"""Child process of tests/test_gpu_tail_dense.py (NODAL_SA_TAIL_DENSE is read once per process).

Solves the shapes named on the command line through the smoothed-aggregation hierarchy and leaves, per shape, a line
`RESULT <shape> <info> <iterations, comma separated>` on stdout and the solution in <out dir>/<shape>.npy.  A line
`SHAPE <shape>` goes to stderr in front of each, so that the parent can tell whose `[sagg]` trace lines follow."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from nodal_amd import _ffi, generators as gen  # noqa: E402


def single(table):
    h = _ffi.Handle(0)
    h.upload(table)
    info = h.run(False)
    x = h.download_x()
    its = [h.solve_info()[0]]
    h.close()
    return info, its, x


def batch(N, members):
    table = gen.grid_table(N)
    vals = np.ones((members, table.ncomp))
    for b in range(members):
        vals[b, :-1] = gen.cfg4_values(b, N)
    h = _ffi.Handle(0)
    h.upload(table)
    h.upload_values(vals)
    x, info = h.run_batch(0, members)
    its = [h.solve_info()[0]]
    h.close()
    return int(np.abs(info).max()), its, x


def pairs32():
    table = gen.grid_table(300)
    rng = np.random.default_rng(17)
    ia = rng.integers(0, table.K, size=32).astype(np.int32)
    ib = rng.integers(0, table.K, size=32).astype(np.int32)
    ib[ib == ia] = -1
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    res, info = h.solve_pairs(ia, ib, dense=False)
    h.close()
    return info, None, np.asarray(res)  # (the blocks' iteration counts: the parent reads them from the trace)


SHAPES = {
    "grid400": lambda: single(gen.grid_table(400)),
    "grid300": lambda: single(gen.grid_table(300)),
    "cfg5_300": lambda: single(gen.cfg5_table(300)),
    "batch16x60": lambda: batch(60, 16),
    "batch100x24": lambda: batch(24, 100),
    "pairs32_grid300": pairs32,
}


def main():
    out = sys.argv[1]
    for name in sys.argv[2:]:
        assert re.fullmatch(r"\w+", name)
        print("SHAPE", name, file=sys.stderr, flush=True)
        info, its, x = SHAPES[name]()
        np.save(os.path.join(out, name + ".npy"), x)
        print("RESULT", name, info, ",".join(str(i) for i in its) if its is not None else "-", flush=True)
    print("tail dense child ok")


if __name__ == "__main__":
    main()
