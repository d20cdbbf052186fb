"""Source sweeps (nodal_solve_sources) against the same members solved one by one with nodal_run.

Config 3's network, grid(1000) (a1 plus seven more current sources spread over the grid: eight A sources, random
values), takes the multigrid route: member 0 builds the hierarchy, the rest go sixteen at a time through the block
iteration.  Config 5's network (cfg5_table(1000), every E source swept) takes the sparse-LU route.  For each sweep
length m: ms per member, the block iterations (the last block's), the largest scaled residual.  The one-by-one
baseline is nodal_run with the symbolic phase kept, member by member from an uploaded value table (its cost per
member does not depend on m: timed over 16 members).

Timing: the library's own HIP events around the sweep (nodal_last_timings [2]) and, for both routes, the host's
clock between two synchronisations of the handle's stream (every call returns after that stream has drained).

    python tools/sweep_probe.py [--out profiles/sweep_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nodal_amd import _ffi  # noqa: E402
from nodal_amd import constants as c  # noqa: E402
from nodal_amd import generators as gen  # noqa: E402
from nodal_amd.lowering import ComponentTable  # noqa: E402


def with_loads(table, nodes):
    """table plus one current source from each node to ground"""
    t = ComponentTable(table.ncomp + len(nodes), table.K, table.B)
    for name in ("type", "value", "a", "b", "c", "d", "drv", "k"):
        getattr(t, name)[:table.ncomp] = getattr(table, name)
    t.type[table.ncomp:] = c.T_A
    t.value[table.ncomp:] = 1.0
    t.a[table.ncomp:] = nodes
    t.b[table.ncomp:] = -1
    return t


def sweep_case(h, table, rows, ms, rng, baseline_members=16):
    out = {"n": int(h.n), "swept_rows": int(len(rows)), "sweeps": []}
    # warm-up: one sweep of 17 members (hierarchy / analysis, buffers)
    h.solve_sources(rows, rng.uniform(-5, 5, (17, len(rows))), dense=False)
    for m in ms:
        values = rng.uniform(-5, 5, (m, len(rows)))
        h.synchronize()
        t0 = time.perf_counter()
        x, info, resid = h.solve_sources(rows, values, dense=False)
        h.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        ev = h.timings()[2]
        it, _, _ = h.solve_info()
        out["sweeps"].append({"members": m, "wall_ms": wall, "event_ms": ev, "ms_per_member_wall": wall / m,
                              "ms_per_member_event": ev / m, "last_block_iterations": int(it),
                              "max_scaled_residual": float(np.max(resid)), "singular": int((info > 0).sum())})
        print(json.dumps(out["sweeps"][-1]), flush=True)
    # one by one: nodal_run, symbolic kept, members from an uploaded value table
    vals = np.tile(table.value, (baseline_members, 1))
    vals[:, rows] = rng.uniform(-5, 5, (baseline_members, len(rows)))
    h.upload_values(vals)
    h.run(False, member=0, reuse_symbolic=False)
    h.synchronize()
    t0 = time.perf_counter()
    ev = 0.0
    for k in range(baseline_members):
        h.run(False, member=k, reuse_symbolic=True)
        ev += sum(h.timings())
    h.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    out["one_by_one"] = {"members": baseline_members, "ms_per_member_wall": wall / baseline_members,
                         "ms_per_member_event": ev / baseline_members}
    print(json.dumps(out["one_by_one"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sweep_probe.json")
    ap.add_argument("--members", default="16,64,256")
    args = ap.parse_args()
    ms = [int(v) for v in args.members.split(",")]
    rng = np.random.default_rng(2026)
    record = {"tool": "tools/sweep_probe.py", "members": ms}

    grid = gen.grid_table(1000)
    loads = rng.choice(np.arange(1, grid.K), 7, replace=False).astype(np.int32)
    grid = with_loads(grid, loads)
    h = _ffi.Handle(0)
    h.upload(grid)
    h.assemble_symbolic()
    h.assemble_numeric(0)
    rows = np.flatnonzero(grid.type == c.T_A)
    record["cfg3_grid1000_8A"] = sweep_case(h, grid, rows, ms, rng)
    h.close()

    cfg5 = gen.cfg5_table(1000)
    h = _ffi.Handle(0)
    h.upload(cfg5)
    h.assemble_symbolic()
    h.assemble_numeric(0)
    rows = np.flatnonzero(cfg5.type == c.T_E)
    record["cfg5_all_E"] = sweep_case(h, cfg5, rows, ms, rng)
    h.close()

    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
