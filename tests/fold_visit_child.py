"""Child process of tests/test_gpu_fold_visit.py (NODAL_SA_FOLD_VISIT, NODAL_SA_VISIT_CAP, NODAL_SA_VISIT_CHECK and
NODAL_POISON are read once per process; NODAL_SA_NU per call, so the child sets it per shape).

Per shape named on the command line: sets the network up on a fresh handle, solves it through the multigrid, and leaves
`RESULT <shape> <info> <iterations, one per solve>` on stdout, the last solution in <out dir>/<shape>.npy, per solve the
exported arrays of the level that visits in three launches in <out dir>/<shape>.<solve>.npz (`level` = -1 and nothing
else when no level does), and `SHAPE <shape>` on stderr in front of the shape's `[sagg]` trace lines."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import hierarchy_child as hc  # noqa: E402
from nodal_amd import _ffi, generators as gen  # noqa: E402

KEEP = ("acol", "aval", "alen", "dinv", "wcol", "wval", "wlen", "p2col", "p2val", "p2len", "d2")
WORDS = ("n", "ld", "nc", "maxlen", "wslots", "fold", "refreshed", "omega")


def grid400():
    """The smallest shape that reaches the path with the production sweep counts: 160 k -> 23 k -> 1.4 k -> tail."""
    return gen.grid_table(400, hc.grid_values(400, seed=400))


def cfg5_100():
    return hc.cfg5(100)


def refresh_members():
    table = hc.grid100()
    v0 = table.value.copy()
    v1 = v0.copy()
    v1[:-1] *= np.random.default_rng(101).uniform(0.5, 2.0, size=len(v0) - 1)
    return table, np.stack([v0, v1, v0])


# shape: (table, NODAL_SA_NU or None, method, members)
SHAPES = {
    "grid400": lambda: (grid400(), None, _ffi.SPARSE_PCG, None),
    "grid100_222": lambda: (hc.grid100(), "222", _ffi.SPARSE_PCG, None),
    "refresh100_222": lambda: (*refresh_members()[:1], "222", _ffi.SPARSE_PCG, refresh_members()[1]),
    "cfg5_100_222": lambda: (cfg5_100(), "222", _ffi.SPARSE_LU, None),
}


def main():
    out = sys.argv[1]
    for name in sys.argv[2:]:
        assert re.fullmatch(r"\w+", name)
        table, nu, method, members = SHAPES[name]()
        if nu is None:
            os.environ.pop("NODAL_SA_NU", None)
        else:
            os.environ["NODAL_SA_NU"] = nu
        print("SHAPE", name, file=sys.stderr, flush=True)
        h = _ffi.Handle(0)
        h.upload(table)
        if members is not None:
            h.upload_values(members)
        h.assemble_symbolic()
        its, info = [], 0
        for member in range(1 if members is None else len(members)):
            assert h.assemble_numeric(member)[0] == _ffi.OK
            x, info_m, _, _ = h.solve_sparse(method=method)
            info = max(info, abs(info_m))
            its.append(h.solve_info()[0])
            levels = h.debug_hierarchy()
            at = [l for l, lv in enumerate(levels) if len(lv["p2col"])]
            assert len(at) <= 1, at
            keep = {"level": np.int64(at[0] if at else -1), "sizes": np.array([lv["n"] for lv in levels])}
            if at:
                lv = levels[at[0]]
                keep.update({k: lv[k] for k in KEEP})
                keep.update({k: np.float64(lv[k]) for k in WORDS})
            np.savez(os.path.join(out, f"{name}.{member}.npz"), **keep)
        h.close()
        np.save(os.path.join(out, name + ".npy"), x)
        print("RESULT", name, info, ",".join(str(i) for i in its), flush=True)
    print("fold visit child ok")


if __name__ == "__main__":
    main()
