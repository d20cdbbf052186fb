"""Child process of tests/test_gpu_restrict_from_b.py (NODAL_SA_RESTRICT_B, NODAL_SA_RESTRICT_CHECK and NODAL_POISON are
read once per process; NODAL_SA_NU per call, so the child sets it per shape).

Per shape named on the command line: sets the network up on a fresh handle, solves it through the multigrid, and leaves
`RESULT <shape> <info> <iterations, one per solve>` on stdout, every solve's solution in <out dir>/<shape>.<solve>.npy,
the exported arrays of the levels that restrict from b in <out dir>/<shape>.<solve>.npz (`levels` empty when none does),
and `SHAPE <shape>` on stderr in front of the shape's `[sagg]` trace lines.  Shapes marked `twice` are solved once more
on a second fresh handle: <out dir>/<shape>.again.npy."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import fold_visit_child as fv  # noqa: E402
import hierarchy_child as hc  # noqa: E402
from nodal_amd import _ffi  # noqa: E402

KEEP = ("wcol", "wval", "wlen", "wtstart", "wtcol", "wtval", "wtsrc")
WORDS = ("n", "ld", "nc", "wslots", "fold", "refreshed")

# shape: (table, NODAL_SA_NU or None, method, members, twice)
SHAPES = {
    "grid100": lambda: (hc.grid100(), None, _ffi.SPARSE_PCG, None, True),
    "grid400": lambda: (fv.grid400(), None, _ffi.SPARSE_PCG, None, True),
    "cfg5_100": lambda: (hc.cfg5(100), None, _ffi.SPARSE_LU, None, False),
    "grid100_222": lambda: (hc.grid100(), "222", _ffi.SPARSE_PCG, None, False),
    "refresh100": lambda: (fv.refresh_members()[0], None, _ffi.SPARSE_PCG, fv.refresh_members()[1], False),
}


def solve_all(out, name, table, method, members, keep):
    h = _ffi.Handle(0)
    h.upload(table)
    if members is not None:
        h.upload_values(members)
    h.assemble_symbolic()
    its, info, xs = [], 0, []
    for member in range(1 if members is None else len(members)):
        assert h.assemble_numeric(member)[0] == _ffi.OK
        x, info_m, _, _ = h.solve_sparse(method=method)
        info = max(info, abs(info_m))
        its.append(h.solve_info()[0])
        xs.append(x)
        if keep:
            levels = h.debug_hierarchy()
            at = [l for l, lv in enumerate(levels) if len(lv["wtstart"])]
            arrays = {"levels": np.array(at, dtype=np.int64), "sizes": np.array([lv["n"] for lv in levels])}
            for l in at:
                arrays.update({f"{k}{l}": levels[l][k] for k in KEEP})
                arrays.update({f"{k}{l}": np.int64(levels[l][k]) for k in WORDS})
            np.savez(os.path.join(out, f"{name}.{member}.npz"), **arrays)
    h.close()
    return info, its, xs


def main():
    out = sys.argv[1]
    for name in sys.argv[2:]:
        assert re.fullmatch(r"\w+", name)
        table, nu, method, members, twice = SHAPES[name]()
        if nu is None:
            os.environ.pop("NODAL_SA_NU", None)
        else:
            os.environ["NODAL_SA_NU"] = nu
        print("SHAPE", name, file=sys.stderr, flush=True)
        info, its, xs = solve_all(out, name, table, method, members, True)
        for k, x in enumerate(xs):
            np.save(os.path.join(out, f"{name}.{k}.npy"), x)
        if twice:
            print("SHAPE", name + "_again", file=sys.stderr, flush=True)
            info2, _, xs2 = solve_all(out, name, table, method, members, False)
            info = max(info, info2)
            np.save(os.path.join(out, f"{name}.again.npy"), xs2[0])
        print("RESULT", name, info, ",".join(str(i) for i in its), flush=True)
    print("restrict from b child ok")


if __name__ == "__main__":
    main()
