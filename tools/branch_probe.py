"""What the branch quantities and the sweep envelope cost (nodal_branches, nodal_solve_sources_branches).

The two sweep workloads of tools/sweep_probe.py -- grid(1000) with eight A sources (multigrid route), cfg5's network
with every E source swept (sparse-LU route) -- at 16 / 64 / 256 members, three ways in ONE process, alternating
A / B / C / A / B / C after a warm-up sweep:

    A  x downloaded, no envelope          (nodal_solve_sources: the call as it was)
    B  x downloaded, envelope
    C  x_out = NULL, envelope             (no [M][n] array on the host at all)

and, next to C, what the envelope costs on the host instead: the numpy formula on the members A downloaded (gather
two potentials per component, divide, running maximum; per-node minimum and maximum).  Then nodal_branches after one
nodal_run of each network against nodal_download_x + the numpy formula.

Timing: the host's clock between two synchronisations of the handle's stream (every call returns after that stream
has drained).  Next to the times: the algorithmic bytes of one block of sixteen members, from the shapes alone --
per table row 17 B of table (type, value, a, b) + 4 B slot + 4 B k, 2 x 8 B gathered per member, 12 B read and 12 B
written of envelope; per node 8 B per member and 24 B read + 24 B written -- so that a rate can be stated once the
kernels' own times are known (`rocprofv3 --kernel-trace --stats -- python tools/branch_probe.py --members 16`
lists k_branch_envelope, k_node_envelope, k_power_totals, k_branch_single by name; that run is separate from this
one's timings).

    python tools/branch_probe.py [--out profiles/branch_probe.json] [--members 16,64,256] [--repeats 2]
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
from tools.sweep_probe import with_loads  # noqa: E402


def numpy_branches(table, x, value=None):
    value = table.value if value is None else value
    xe = np.append(x, 0.0)
    v = xe[table.a] - xe[table.b]
    branch = xe[np.where(table.k >= 0, table.K + table.k, -1)]
    with np.errstate(all="ignore"):
        cur = np.where(table.type == c.T_R, v / value, np.where(table.type == c.T_A, value, branch))
    return v, cur


def numpy_envelope(table, rows, values, x):
    """the host's way to the same envelope from the downloaded members"""
    best = np.full(table.ncomp, -np.inf)
    who = np.full(table.ncomp, -1, dtype=np.int32)
    value = np.array(table.value)
    for m in range(x.shape[0]):
        value[rows] = values[m]
        mag = np.abs(numpy_branches(table, x[m], value)[1])
        better = mag > best
        best[better] = mag[better]
        who[better] = m
    K = table.K
    return best, who, x[:, :K].min(0), x[:, :K].max(0)


def block_bytes(table, members=16):
    per_row = 17 + 4 + 4 + 2 * 8 * members + 12 + 12
    per_node = 8 * members + 24 + 24
    return {"per_table_row": per_row, "per_node": per_node,
            "per_block_of_%d" % members: int(table.ncomp) * per_row + int(table.K) * per_node}


def timed(h, fn):
    h.synchronize()
    t0 = time.perf_counter()
    out = fn()
    h.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def sweep_case(h, table, rows, ms, rng, repeats):
    out = {"n": int(h.n), "ncomp": int(table.ncomp), "swept_rows": int(len(rows)), "algorithmic_bytes": block_bytes(table),
           "sweeps": []}
    warm = rng.uniform(-5, 5, (17, len(rows)))
    h.solve_sources(rows, warm, dense=False)
    h.solve_sources_branches(rows, warm, dense=False, keep_solutions=False)
    for m in ms:
        values = rng.uniform(-5, 5, (m, len(rows)))
        legs = {"x_no_envelope": [], "x_and_envelope": [], "envelope_only": []}
        x = env = None
        for _ in range(repeats):
            t, (x, _, _) = timed(h, lambda: h.solve_sources(rows, values, dense=False))
            legs["x_no_envelope"].append(t / m)
            t, (_, _, _, env) = timed(h, lambda: h.solve_sources_branches(rows, values, dense=False))
            legs["x_and_envelope"].append(t / m)
            t, (_, info, _, env) = timed(h, lambda: h.solve_sources_branches(rows, values, dense=False,
                                                                            keep_solutions=False))
            legs["envelope_only"].append(t / m)
        t0 = time.perf_counter()
        best, _who, lo, hi = numpy_envelope(table, rows, values, x[:min(m, 16)])
        host_ms = (time.perf_counter() - t0) * 1e3 / min(m, 16)
        agree = None
        if m <= 16:
            agree = bool(np.allclose(best, env["current_absmax"], rtol=1e-9, atol=1e-12)
                         and np.allclose(lo, env["potential_min"], rtol=1e-9, atol=1e-12)
                         and np.allclose(hi, env["potential_max"], rtol=1e-9, atol=1e-12))
        rec = {"members": m, "ms_per_member": {k: v for k, v in legs.items()},
               "ms_per_member_best": {k: min(v) for k, v in legs.items()},
               "numpy_envelope_ms_per_member_on_this_host": host_ms, "numpy_envelope_agrees": agree,
               "singular": int((info > 0).sum())}
        out["sweeps"].append(rec)
        print(json.dumps(rec), flush=True)
    # one solution: nodal_branches against download + numpy
    h.run(False, member=0, reuse_symbolic=False)
    h.branches()
    dev, host = [], []
    for _ in range(max(repeats, 3)):
        t, _ = timed(h, h.branches)
        dev.append(t)
        t, _ = timed(h, lambda: numpy_branches(table, np.array(h.download_x())))
        host.append(t)
    t, _ = timed(h, lambda: h.branches(voltage=False, current=False, power=False))
    out["single"] = {"nodal_branches_ms": dev, "download_x_plus_numpy_ms": host, "nodal_branches_totals_only_ms": t}
    print(json.dumps(out["single"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/branch_probe.json")
    ap.add_argument("--members", default="16,64,256")
    ap.add_argument("--repeats", type=int, default=2)
    args = ap.parse_args()
    ms = [int(v) for v in args.members.split(",")]
    rng = np.random.default_rng(2026)
    record = {"tool": "tools/branch_probe.py", "members": ms, "repeats": args.repeats,
              "legs": "alternating in one process after a warm-up sweep; host clock between stream synchronisations"}

    grid = gen.grid_table(1000)
    loads = rng.choice(np.arange(1, grid.K), 7, replace=False).astype(np.int32)
    grid = with_loads(grid, loads)
    for name, table, kind in (("cfg3_grid1000_8A", grid, c.T_A), ("cfg5_all_E", gen.cfg5_table(1000), c.T_E)):
        h = _ffi.Handle(0)
        h.upload(table)
        h.assemble_symbolic()
        h.assemble_numeric(0)
        record[name] = sweep_case(h, table, np.flatnonzero(table.type == kind), ms, rng, args.repeats)
        h.close()

    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
