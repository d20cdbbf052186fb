"""What inductors add to a transient step (nodal_transient_rlc) -- and that the capacitors-only call is what it was.

tools/transient_probe.py's grid workload -- grid(1000) with eight A sources, a capacitor from every node to ground,
backward Euler, dt = 1, 8 probes, no solutions kept, the multigrid route -- and on top 64 seeded inductors of 0.5-3 H from
seeded nodes to ground, all of them probed.  In ONE process, after a first call of each, alternating, faster of
`--repeats`:

    P    the PARENT commit's library (--parent-lib), nodal_transient, capacitors only
    N0   this build, nodal_transient, capacitors only: every output compared bit for bit with P's
    N1   this build, nodal_transient_rlc with the 64 inductors (started from x_0 of the parent table and zero currents:
         the step's cost does not depend on the start)

and once: the first call of the DC clone -- the parent table with one zero-volt E row and one branch unknown per
inductor, uploaded, assembled and solved (nodal_solve_sparse) -- which is what Circuit.transient pays for its DC start.

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their own,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/transient_rl_probe.py --repeats 1 --out
DIR/probe.json`; `--kernel-stats DIR/.../kernel_stats.csv` then adds the k_transient_* kernels to the record at --out.

    python tools/transient_rl_probe.py [--parent-lib PATH] [--out profiles/transient_rl_probe.json] [--steps 64]
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nodal_amd import _ffi  # noqa: E402
from nodal_amd import constants as c  # noqa: E402
from nodal_amd.transient import dc_table  # noqa: E402
from tools.transient_probe import DT, assembled, network, timed  # noqa: E402

KERNELS = ("k_transient_history", "k_signed_list_add", "k_transient_probe", "k_transient_inductor_start",
           "k_transient_inductor", "k_transient_current_probe")
INDUCTORS = 64


def handle_on(lib):
    """a Handle bound to another build of the library (the parent commit's: only the entry points it exports)"""
    mine = _ffi.load()
    for name, (res, args) in _ffi.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    _ffi._lib = lib
    try:
        return _ffi.Handle(0)
    finally:
        _ffi._lib = mine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/transient_rl_probe.json")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libnodal_hip.so built from the parent commit (leg P)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a run of this tool: merged "
                    "into the record at --out instead of measuring")
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as f:
            record = json.load(f)
        found = {}
        with open(args.kernel_stats, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                for key in KERNELS:
                    if key + "(" in name or name.endswith(key) or key + "E" in name:
                        found[key] = {"calls": int(row["Calls"]), "average_ns": float(row["AverageNs"]),
                                      "min_ns": float(row["MinNs"]), "max_ns": float(row["MaxNs"])}
        record["kernels"] = found
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print(json.dumps(found))
        return

    steps = args.steps
    rng = np.random.default_rng(2026)
    table, rows = network("grid", rng)
    K = table.K
    farads = rng.uniform(0.5, 2.0, K)
    nodes = np.arange(K, dtype=np.int32)
    ground = np.full(K, -1, np.int32)
    at = rng.choice(K, INDUCTORS, replace=False).astype(np.int32)
    henries = rng.uniform(0.5, 3.0, INDUCTORS)
    r_code = np.full(K + INDUCTORS, c.T_R, dtype=np.uint8)
    cap_table = table.with_rows_appended(r_code[:K], DT / farads, nodes, ground)
    rlc_table = table.with_rows_appended(r_code, np.concatenate([DT / farads, henries / DT]), np.concatenate([nodes, at]),
                                         np.full(K + INDUCTORS, -1, np.int32))
    cap_rows = np.arange(table.ncomp, table.ncomp + K, dtype=np.int64)
    ind_rows = np.arange(table.ncomp + K, table.ncomp + K + INDUCTORS, dtype=np.int64)
    pa, pb = rng.choice(K, 8, replace=False).astype(np.int32), np.full(8, -1, dtype=np.int32)
    cur_index = np.arange(INDUCTORS, dtype=np.int32)

    parent = assembled(table)
    assert parent.run(False) == 0
    x0 = parent.download_x()
    parent.close()
    record = {"tool": "tools/transient_rl_probe.py", "n": int(table.K + table.B), "capacitors": int(K),
              "inductors": INDUCTORS, "steps": steps, "repeats": args.repeats, "dt": DT,
              "legs": "alternating in one process after a first call of each; host clock between stream "
                      "synchronisations; ms_per_step from the faster repeat"}

    # the DC clone's first call: upload, assembly and one sparse solve of the system with B = 64
    t0 = time.perf_counter()
    dc = assembled(dc_table(table, at, np.full(INDUCTORS, -1, np.int32)))
    try:
        e, info, iters, resid = dc.solve_sparse()
        dc.synchronize()
        record["dc_clone_first_call_ms"] = (time.perf_counter() - t0) * 1e3
        record["dc_clone"] = {"n": int(dc.n), "info": int(info), "iterations": int(iters), "relative_residual": float(resid)}
        record["dc_clone_second_solve_ms"] = timed(dc, dc.solve_sparse)[0]
    except _ffi.NodalHipError as exc:  # (recorded, not fatal: the step times do not depend on it)
        record["dc_clone"] = {"n": int(dc.n), "error": str(exc)}
    dc.close()
    print(json.dumps({k: v for k, v in record.items() if k.startswith("dc_clone")}), flush=True)

    legs = {}
    if args.parent_lib:
        h = handle_on(ctypes.CDLL(os.path.abspath(args.parent_lib)))
        h.upload(cap_table)
        h.assemble_symbolic()
        h.assemble_numeric(0)
        legs["P"] = (h, lambda h, v: h.transient(cap_rows, rows, v, x0, pa, pb, dense=False, method=0))
    legs["N0"] = (assembled(cap_table), lambda h, v: h.transient(cap_rows, rows, v, x0, pa, pb, dense=False, method=0))
    legs["N1"] = (assembled(rlc_table), lambda h, v: h.transient_rlc(cap_rows, ind_rows, rows, v, x0, np.zeros(INDUCTORS),
                                                                     pa, pb, cur_index, dense=False, method=0))
    warm = rng.uniform(-5, 5, (17, len(rows)))
    record["first_call_ms"] = {name: timed(h, lambda: fn(h, warm))[0] for name, (h, fn) in legs.items()}
    values = rng.uniform(-5, 5, (steps, len(rows)))
    times, outs = {name: [] for name in legs}, {}
    for _ in range(args.repeats):
        for name, (h, fn) in legs.items():
            ms, out = timed(h, lambda: fn(h, values))
            times[name].append(ms)
            outs[name] = out
            assert h.timings()[0] == 0.0, name  # (the matrix work was kept)
    record["call_ms"] = times
    record["ms_per_step"] = {name: min(ms) / steps for name, ms in times.items()}
    for name, out in outs.items():
        record.setdefault("largest_scaled_residual", {})[name] = float(out[3].max())
        record.setdefault("iterations_first_median_last", {})[name] = [int(out[5][0]), float(np.median(out[5])), int(out[5][-1])]
        assert (out[4] == 0).all(), name
    if "P" in outs:
        same = all(np.array_equal(outs["P"][q], outs["N0"][q]) for q in (0, 3, 4, 5))
        record["capacitors_only_bits_equal_to_parent"] = bool(same)
        record["N0_over_P"] = record["ms_per_step"]["N0"] / record["ms_per_step"]["P"]
    record["N1_over_N0"] = record["ms_per_step"]["N1"] / record["ms_per_step"]["N0"]
    record["largest_inductor_current"] = float(np.abs(outs["N1"][6]).max())
    for h, _ in legs.values():
        h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
