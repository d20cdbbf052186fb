"""What a transient step costs (nodal_transient) against a repeated single solve and a source sweep of as many members.

The two sweep workloads of tools/sweep_probe.py -- grid(1000) with eight A sources (passive: the multigrid route), cfg5's
network (branch unknowns and controlled sources: the sparse LU route) -- each with a capacitor from every node to ground
(backward Euler; the companion resistors are appended to the table, Circuit.transient's child), at 64 and 256 steps, in
ONE process:

    first   the first nodal_transient call on the child handle: hierarchy setup or sparse analysis + factorisation
    A       nodal_transient again with the matrix work kept (waveforms of 8 probes down, no solutions kept)
    B       nodal_solve_sources on the PARENT table for as many members, solutions down (the yardstick), alternating
            with A

and per run: ms per step, iterations per step (first, median, last), the largest scaled residual.

The claim to check: a step on the multigrid route costs no more than a repeated nodal_run with the symbolic phases kept
(plus the spread the box shows between two runs of it) -- the companion conductances make the matrix more diagonally
dominant.  That yardstick is measured in a process of its own, `--nodal-run-only`, and with `--parent-lib PATH` on the
library built from the parent commit (two runs of sixteen solves: their spread is recorded).

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their
own, `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/transient_probe.py --networks grid
--steps 64 --repeats 1 --envelope --skip-yardstick --out DIR/probe.json`; `--networks grid --kernel-stats DIR/.../kernel_stats.csv` then adds the
k_transient_* kernels to that network's record.

    python tools/transient_probe.py [--out profiles/transient_probe.json] [--steps 64,256] [--repeats 2]
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nodal_amd import _ffi  # noqa: E402
from nodal_amd import constants as c  # noqa: E402
from nodal_amd import generators as gen  # noqa: E402
from tools.sweep_probe import with_loads  # noqa: E402

KERNELS = ("k_transient_history", "k_signed_list_add", "k_transient_probe", "k_transient_envelope")
DT = 1.0  # (of the order of a node's own RC: unit resistors, capacitors of 0.5 .. 2)


def timed(h, fn):
    h.synchronize()
    t0 = time.perf_counter()
    out = fn()
    h.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def network(name, rng):
    if name == "grid":
        grid = gen.grid_table(1000)
        loads = rng.choice(np.arange(1, grid.K), 7, replace=False).astype(np.int32)
        table = with_loads(grid, loads)
        return table, np.flatnonzero(table.type == c.T_A)
    table = gen.cfg5_table(1000)
    return table, np.flatnonzero(table.type == c.T_E)


def assembled(table):
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    h.assemble_numeric(0)
    return h


def case(table, rows, steps_list, rng, repeats, envelope=False):
    K = table.K
    farads = rng.uniform(0.5, 2.0, K)
    nodes = np.arange(K, dtype=np.int32)
    child_table = table.with_rows_appended(np.full(K, c.T_R, dtype=np.uint8), DT / farads, nodes, np.full(K, -1, np.int32))
    cap_rows = np.arange(table.ncomp, table.ncomp + K, dtype=np.int64)
    parent, child = assembled(table), assembled(child_table)
    assert parent.run(False) == 0
    x0 = parent.download_x()
    pa = rng.choice(K, 8, replace=False).astype(np.int32)
    pb = np.full(8, -1, dtype=np.int32)
    out = {"n": int(parent.n), "capacitors": int(K), "swept_rows": int(len(rows)), "dt": DT, "runs": []}

    def transient(values):
        return child.transient(cap_rows, rows, values, x0, pa, pb, dense=False, method=0, envelope=envelope)

    warm = rng.uniform(-5, 5, (17, len(rows)))
    out["first_transient_call_ms"], _ = timed(child, lambda: transient(warm))
    out["first_transient_matrix_ms"] = child.timings()[0]
    out["first_sweep_call_ms"] = timed(parent, lambda: parent.solve_sources(rows, warm, dense=False))[0]
    for steps in steps_list:
        values = rng.uniform(-5, 5, (steps, len(rows)))
        tr_ms, sw_ms = [], []
        for _ in range(repeats):
            ms, (wave, _, _, resid, info, iters) = timed(child, lambda: transient(values))
            tr_ms.append(ms)
            matrix_ms = child.timings()[0]
            ms, (x, sinfo, sresid) = timed(parent, lambda: parent.solve_sources(rows, values, dense=False))
            sw_ms.append(ms)
            del x
        rec = {"steps": steps, "transient_ms": tr_ms, "solve_sources_ms": sw_ms, "ms_per_step": min(tr_ms) / steps,
               "ms_per_sweep_member": min(sw_ms) / steps, "kept_call_matrix_ms": matrix_ms,
               "iterations_first_median_last": [int(iters[0]), float(np.median(iters)), int(iters[-1])],
               "largest_scaled_residual": float(resid.max()), "sweep_largest_scaled_residual": float(sresid.max()),
               "singular": int((info > 0).sum() + (sinfo > 0).sum())}
        out["runs"].append(rec)
        print(json.dumps(rec), flush=True)
    parent.close()
    child.close()
    return out


def nodal_run_only(lib, networks, solves=16):
    """repeated nodal_run with the symbolic phases kept, two runs of `solves` each: ms per solve (host clock)"""
    if lib:  # (an older build: the binding is cut down to the entry points it exports)
        import ctypes
        _ffi.LIB_PATH = os.path.abspath(lib)
        older = ctypes.CDLL(_ffi.LIB_PATH)
        for name in [name for name in _ffi.SIGNATURES if not hasattr(older, name)]:
            del _ffi.SIGNATURES[name]
    rng = np.random.default_rng(2026)
    out = {"library": lib or "this build", "solves_per_run": solves}
    for name in networks:
        table, _ = network(name, rng)
        h = assembled(table)
        assert h.run(False) == 0
        runs = []
        for _ in range(2):
            ms, _ = timed(h, lambda: [h.run(False, member=0, reuse_symbolic=True) for _ in range(solves)])
            runs.append(ms / solves)
        out[name] = {"ms_per_solve": runs, "spread_ms": abs(runs[0] - runs[1]), "iterations": h.solve_info()[0]}
        h.close()
    return out


def kernel_stats(path, record, network_key):
    found = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for key in KERNELS:
                if key in name:
                    found[key] = {"calls": int(row["Calls"]), "total_ns": float(row["TotalDurationNs"]),
                                  "average_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"]),
                                  "max_ns": float(row["MaxNs"])}
    record[network_key]["kernels"] = found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/transient_probe.json")
    ap.add_argument("--steps", default="64,256")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--networks", default="grid,cfg5")
    ap.add_argument("--parent-lib", default=None, help="libnodal_hip.so built from the parent commit: the repeated "
                    "nodal_run is measured on it as well")
    ap.add_argument("--nodal-run-only", action="store_true", help="print the repeated-solve record of --lib and exit")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--envelope", action="store_true", help="keep the per-node envelope too (the profiled run: all four "
                    "kernels are launched)")
    ap.add_argument("--skip-yardstick", action="store_true", help="no repeated-nodal_run processes (the profiled run)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a run of this tool: merged "
                    "into the record at --out instead of measuring")
    args = ap.parse_args()
    networks = args.networks.split(",")
    keys = {"grid": "cfg3_grid1000_8A", "cfg5": "cfg5"}
    if args.nodal_run_only:
        print(json.dumps(nodal_run_only(args.lib, networks)))
        return
    if args.kernel_stats:
        with open(args.out) as f:
            record = json.load(f)
        kernel_stats(args.kernel_stats, record, keys[networks[0]])
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print(json.dumps(record[keys[networks[0]]]["kernels"]))
        return
    steps_list = [int(v) for v in args.steps.split(",")]
    record = {"tool": "tools/transient_probe.py", "steps": steps_list, "repeats": args.repeats,
              "legs": "alternating in one process after a first call of each; host clock between stream synchronisations; "
                      "ms_per_* from the faster repeat"}
    # the yardstick first, each library in a fresh process of its own (this one has not touched the device yet)
    me = [sys.executable, os.path.abspath(__file__), "--nodal-run-only", "--networks", args.networks]
    record["repeated_nodal_run"] = []
    for lib in [] if args.skip_yardstick else ([args.parent_lib] if args.parent_lib else []) + [None]:
        done = subprocess.run(me + (["--lib", lib] if lib else []), stdout=subprocess.PIPE, text=True)
        if done.returncode != 0:
            sys.exit(f"the repeated-solve process failed ({lib or 'this build'})")
        record["repeated_nodal_run"].append(json.loads(done.stdout.splitlines()[-1]))
    print(json.dumps(record["repeated_nodal_run"]), flush=True)
    rng = np.random.default_rng(2026)
    for name in networks:
        table, rows = network(name, rng)
        record[keys[name]] = case(table, rows, steps_list, rng, args.repeats, envelope=args.envelope)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
