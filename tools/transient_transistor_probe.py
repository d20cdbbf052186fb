"""What bipolar transistors add to a time step of the nonlinear transient analysis (nodal_transient_nl_bjt).

The network is tools/transient_diodes_probe.py's: grid(1000) with eight A sources that switch between their table values
and 1.5 times them in blocks of eight steps (n = 999 999), a capacitor from every node to ground (backward Euler, dt = 1),
tools/operating_point_probe.py's 1024 seeded diodes, and tools/transistor_probe.py's 256 seeded NPNs (collector on a
seeded node, base on its neighbour, emitter on ground), over `--steps` steps.  GM rows make the network non-passive, so
every Newton iteration takes the sparse LU route, factored anew on its kept analysis.

In ONE process, after a first call of each, alternating, faster of `--repeats`:

    T   nodal_transient_nl_bjt from the network's nonlinear DC point (nodal_newton_dc_bjt) at SPICE's tolerances, every
        transistor probed: ms per step, ms per Newton iteration, iterations per step, the largest scaled residual of a
        linear solve
    D   nodal_transient_nl of the SAME network with the diodes only, sent through the sparse LU route by ONE further GM
        row of value 0.0 on a resistor's two nodes, from its own DC point: what a step of that route costs without
        transistors.  The expectation to confirm or refute: the transport lanes and the probe kernel do not show beside
        the factorisation, so the difference per Newton iteration stays inside the run-to-run spreads.

and, with `--parent-lib PATH` (a libnodal_hip.so built from the parent commit), the diodes-only nodal_transient_nl of
tools/transient_diodes_probe.py's conducting case (the multigrid route) on this build and on the parent's, alternating,
`--repeats` (at least four) times each: every output bit for bit, the time difference against the spreads.

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their own,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/transient_transistor_probe.py --repeats 1
--out DIR/probe.json`; `--kernel-stats DIR/.../kernel_stats.csv` then adds k_tnl_transport_probe and the k_transport_*
kernels and their summed time to the record at --out.

    python tools/transient_transistor_probe.py [--out profiles/transient_transistor_probe.json] [--parent-lib PATH]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nodal_amd import constants as c  # noqa: E402
from nodal_amd.operating_point import _with_transport_rows  # noqa: E402
from tools.operating_point_probe import DIODES, GMIN, SPICE, seeded_diodes  # noqa: E402
from tools.transient_diodes_probe import MAX_ITER, parent_handle, switching, with_rows  # noqa: E402
from tools.transient_probe import DT, assembled, network, timed  # noqa: E402
from tools.transistor_probe import BETA_F, BETA_R, TRANSISTORS, seeded_transistors  # noqa: E402

KERNELS = ("k_tnl_transport_probe", "k_transport_linearise", "k_transport_update", "k_transport_check", "k_transport_fill")
KERNEL_TRACE = "the summed time of k_tnl_transport_probe and the k_transport_* kernels (a kernel trace of its own, --kernel-stats)"
NOT_MEASURED = ["the dense route's time (n <= 64)", "cfg5's network", "more than 256 transistors",
                "step parity and the nonlinear residual against the host reference at this size (a sparse factorisation of "
                "n = 999 999 per Newton iteration on the host; tests/test_gpu_transient_transistors.py holds both at "
                "n <= 151)", KERNEL_TRACE]


def case(rng, steps, repeats):
    table, rows = network("grid", rng)
    K = table.K
    farads = rng.uniform(0.5, 2.0, K)
    i_sat, n_vt, ia, ib = seeded_diodes(table, rng)
    col, base, i_s, t_nvt = seeded_transistors(table, rng)
    T = TRANSISTORS
    ground = np.full(T, -1, dtype=np.int32)
    # the junctions behind the diodes: base -> emitter (ground) and base -> collector, forward then reverse
    all_sat = np.concatenate([i_sat, np.stack([i_s / BETA_F, i_s / BETA_R], axis=1).reshape(-1)])
    all_nvt = np.concatenate([n_vt, np.repeat(t_nvt, 2)])
    all_a = np.concatenate([ia, np.repeat(base, 2)]).astype(np.int32)
    all_b = np.concatenate([ib, np.stack([ground, col], axis=1).reshape(-1)]).astype(np.int32)
    junction = (DIODES + np.arange(2 * T, dtype=np.int32)).reshape(T, 2)
    nodes, to_ground = np.arange(K, dtype=np.int32), np.full(K, -1, np.int32)
    values = switching(table, rows, steps)
    none = np.zeros(0, dtype=np.int64)

    def tables(base_table):
        """(with transistors: table, diode rows, GM rows), (diodes only + one GM row of 0.0: table, diode rows)"""
        t_table, t_rows = with_rows(base_table, 1.0 / (all_sat / all_nvt + GMIN), all_a, all_b)
        t_table, gm_rows = _with_transport_rows(t_table, all_a, all_b, col, ground, junction, i_s / t_nvt, -i_s / t_nvt)
        d_table, d_rows = with_rows(base_table, 1.0 / (i_sat / n_vt + GMIN), ia, ib)
        first = int(np.flatnonzero((np.asarray(table.type) == c.T_R) & (np.asarray(table.a) >= 0) & (np.asarray(table.b) >= 0))[0])
        a0, b0 = int(table.a[first]), int(table.b[first])
        d_table = d_table.with_controlled_rows_appended(np.array([c.T_GM], dtype=np.uint8), [0.0], [a0], [b0], [a0], [b0])
        return (t_table, t_rows, gm_rows), (d_table, d_rows)

    # ---- the starts: the nonlinear DC points, capacitors open ----
    (dc_t, dc_t_rows, dc_gm), (dc_d, dc_d_rows) = tables(table)
    h = assembled(dc_t)
    start_t = h.newton_dc_bjt(dc_t_rows, all_sat, all_nvt, GMIN, dc_gm, junction, i_s, none, np.zeros(0), None, dense=False,
                              max_iter=100, **SPICE)
    h.close()
    h = assembled(dc_d)
    start_d = h.newton_dc(dc_d_rows, i_sat, n_vt, GMIN, none, np.zeros(0), None, dense=False, max_iter=100, **SPICE)
    h.close()
    assert start_t["converged"] and start_d["converged"]
    # ---- the two legs ----
    cap_table, cap_rows = with_rows(table, DT / farads, nodes, to_ground)
    (t_table, t_rows, gm_rows), (d_table, d_rows) = tables(cap_table)
    with_t, without = assembled(t_table), assembled(d_table)
    pa, pb = np.arange(8, dtype=np.int32) * (K // 8), np.full(8, -1, dtype=np.int32)
    no_cur = np.zeros(0, dtype=np.int32)
    dprobe, tprobe = np.arange(DIODES, dtype=np.int32), np.arange(T, dtype=np.int32)

    def run_t():
        return with_t.transient_nl_bjt(cap_rows, none, t_rows, all_sat, all_nvt, GMIN, gm_rows, junction, i_s, rows, values,
                                       start_t["x"], np.zeros(0), pa, pb, no_cur, dprobe, tprobe, dense=False,
                                       max_iter=MAX_ITER, **SPICE)

    def run_d():
        return without.transient_nl(cap_rows, none, d_rows, i_sat, n_vt, GMIN, rows, values, start_d["x"], np.zeros(0), pa, pb,
                                    no_cur, dprobe, dense=False, max_iter=MAX_ITER, **SPICE)

    out = {"n": int(with_t.n), "diodes": DIODES, "transistors": T, "steps": steps, "tolerances": dict(SPICE, gmin=GMIN),
           "dc_start_newton_iterations": {"transistors": int(start_t["iterations"]), "diodes_only": int(start_d["iterations"])}}
    out["first_call_ms"] = {}
    out["first_call_ms"]["transistors"], first = timed(with_t, run_t)
    out["first_call_timings_transistors"] = with_t.timings()
    out["first_call_ms"]["diodes_only"], _ = timed(without, run_d)
    t_ms, d_ms = [], []
    for _ in range(repeats):
        ms, rt = timed(with_t, run_t)
        t_ms.append(ms)
        kept_t = with_t.timings()
        ms, rd = timed(without, run_d)
        d_ms.append(ms)
        kept_d = without.timings()
    et, ed = rt[8], rd[8]
    same = all(np.array_equal(first[q], rt[q], equal_nan=True) for q in (0, 3, 4, 5)) and \
        all(np.array_equal(first[8][k], et[k], equal_nan=True) for k in et)
    nt, ndi = int(et["newton"].sum()), int(ed["newton"].sum())
    out.update({
        "info": sorted(set(int(q) for q in rt[4])), "newton_iterations": [int(q) for q in et["newton"]],
        "matrix_updates_equal_newton_iterations": bool(np.array_equal(et["newton"], et["updates"])),
        "newton_iterations_per_step": nt / steps, "solver_iterations": sorted(set(int(q) for q in rt[5])),
        "largest_scaled_residual": float(np.nanmax(rt[3])), "repeated_call_same_bits": bool(same),
        "highest_junction_voltage": float(np.nanmax(et["tv"])), "largest_collector_current": float(np.nanmax(et["ti"][:, :, 2])),
        "call_ms": t_ms, "ms_per_step": min(t_ms) / steps, "ms_per_newton_iteration": min(t_ms) / max(nt, 1),
        "kept_call_timings": kept_t, "matrix_work_ms_per_iteration": kept_t[0] / max(nt, 1),
        "diodes_only": {"info": sorted(set(int(q) for q in rd[4])), "newton_iterations": [int(q) for q in ed["newton"]],
                        "matrix_updates": [int(q) for q in ed["updates"]], "newton_iterations_per_step": ndi / steps,
                        "largest_scaled_residual": float(np.nanmax(rd[3])), "call_ms": d_ms, "ms_per_step": min(d_ms) / steps,
                        "ms_per_newton_iteration": min(d_ms) / max(ndi, 1), "kept_call_timings": kept_d,
                        "matrix_work_ms_per_iteration": kept_d[0] / max(ndi, 1)},
        "spread_ms_per_iteration": {"transistors": (max(t_ms) - min(t_ms)) / max(nt, 1),
                                    "diodes_only": (max(d_ms) - min(d_ms)) / max(ndi, 1)}})
    diff = out["ms_per_newton_iteration"] - out["diodes_only"]["ms_per_newton_iteration"]
    out["difference_ms_per_iteration"] = diff
    out["inside_the_spread"] = bool(abs(diff) <= max(out["spread_ms_per_iteration"].values()))
    print(json.dumps(out), flush=True)
    with_t.close()
    without.close()
    return out


def no_regression(path, rng, repeats, steps):
    """diodes-only nodal_transient_nl (the multigrid route) on this build and on the parent's, alternating"""
    from nodal_amd import _ffi
    table, rows = network("grid", rng)
    K = table.K
    farads = rng.uniform(0.5, 2.0, K)
    i_sat, n_vt, ia, ib = seeded_diodes(table, rng)
    cap_table, cap_rows = with_rows(table, DT / farads, np.arange(K, dtype=np.int32), np.full(K, -1, np.int32))
    nl_table, diode_rows = with_rows(cap_table, 1.0 / (i_sat / n_vt + GMIN), ia, ib)
    handles = {"this": _ffi.Handle(0), "parent": parent_handle(path)}
    for h in handles.values():
        h.upload(nl_table)
        h.assemble_symbolic()
        h.assemble_numeric(0)
    x0 = np.zeros(handles["this"].n)
    pa, pb = np.arange(8, dtype=np.int32) * (K // 8), np.full(8, -1, dtype=np.int32)
    values = switching(table, rows, steps)
    none, index = np.zeros(0, dtype=np.int64), np.arange(DIODES, dtype=np.int32)
    run = lambda h: h.transient_nl(cap_rows, none, diode_rows, i_sat, n_vt, GMIN, rows, values, x0, np.zeros(0), pa, pb,  # noqa: E731
                                   np.zeros(0, dtype=np.int32), index, dense=False, max_iter=MAX_ITER, envelope=True, **SPICE)
    ms, last = {k: [] for k in handles}, {}
    for h in handles.values():
        timed(h, lambda: run(h))
    for _ in range(repeats):
        for key, h in handles.items():
            t, last[key] = timed(h, lambda: run(h))
            ms[key].append(t)
    a, b = last["this"], last["parent"]
    same = all(np.array_equal(a[q], b[q], equal_nan=True) for q in (0, 3, 4, 5)) and \
        all(np.array_equal(a[2][k], b[2][k]) for k in a[2]) and all(np.array_equal(a[8][k], b[8][k], equal_nan=True) for k in a[8])
    out = {"steps": steps, "newton_iterations": int(a[8]["newton"].sum()), "this_ms": ms["this"], "parent_ms": ms["parent"],
           "difference_ms_per_step": (min(ms["this"]) - min(ms["parent"])) / steps,
           "spread_ms_per_step": {k: (max(v) - min(v)) / steps for k, v in ms.items()}, "bit_equal": bool(same)}
    out["inside_the_spread"] = bool(abs(out["difference_ms_per_step"]) <= max(out["spread_ms_per_step"].values()))
    for h in handles.values():
        h.close()
    print("no regression", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/transient_transistor_probe.json")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parent-lib", default=None)
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
                    if key in name:
                        found[key] = {"calls": int(row["Calls"]), "average_ns": float(row["AverageNs"]),
                                      "total_ns": float(row.get("TotalDurationNs", 0.0))}
        record["kernels"] = found
        record["transport_kernels_total_ns"] = sum(v["total_ns"] for v in found.values())
        record["not_measured"] = [what for what in record.get("not_measured", []) if what != KERNEL_TRACE]
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print(json.dumps(found))
        return
    record = {"tool": "tools/transient_transistor_probe.py", "repeats": args.repeats,
              "legs": "alternating in one process after a first call of each; host clock between stream "
                      "synchronisations; ms_per_* from the faster repeat",
              "not_measured": list(NOT_MEASURED)}
    record["grid_8A"] = case(np.random.default_rng(2026), args.steps, args.repeats)
    if args.parent_lib:
        record["diodes_only_against_the_parent"] = no_regression(args.parent_lib, np.random.default_rng(2026),
                                                                 max(args.repeats, 4), args.steps)
    else:
        record["not_measured"].append("the diodes-only transient against the parent commit's library")
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
