"""What bipolar transistors add to a Newton iteration of the operating-point analysis (nodal_newton_dc_bjt).

The network is tools/operating_point_probe.py's grid: grid(N) (N = 1000: n = 999 999) with eight A sources and the same
1024 seeded diodes, plus 256 seeded NPNs (i_s 1e-14 .. 1e-12 A, beta_f 100, beta_r 1, n_vt 25.85 .. 39 mV), each with
its collector on a seeded node, its base on that node's neighbour and its emitter on ground.  GM rows make the network
non-passive, so every iteration takes the sparse LU route, factored anew on its kept analysis.

In ONE process, after a first call of each, alternating, faster of `--repeats`:

    T   nodal_newton_dc_bjt from zeros at SPICE's tolerances on the handle that holds the diodes' and junctions' R rows
        and the transports' GM rows: ms per Newton iteration = the call / its iterations, and the part of it that is
        the matrix work (assembly and numeric factorisation: nodal_last_timings [0] / iterations)
    D   nodal_newton_dc of the SAME network with the diodes only, sent through the sparse LU route by ONE further GM row
        of value 0.0 that lies on a resistor's two nodes (it adds no entry to the pattern and nothing to any value, but
        the network no longer counts as passive): what an iteration of that route costs without transistors

and, with `--parent-lib PATH` (a libnodal_hip.so built from the parent commit), the diodes-only operating point
(nodal_newton_dc, the multigrid route) on this build and on the parent's, alternating, bit for bit
(tools/operating_point_gradient_probe.py's no_regression).

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their own,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/transistor_probe.py --repeats 1 --out
DIR/probe.json`; `--kernel-stats DIR/.../kernel_stats.csv` then adds the k_transport_* kernels and their summed time to
the record at --out.

    python tools/transistor_probe.py [--out profiles/transistor_probe.json] [--grid 1000] [--parent-lib PATH]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nodal_amd import constants as c  # noqa: E402
from nodal_amd import generators as gen  # noqa: E402
from nodal_amd.operating_point import transistor_companion_table  # noqa: E402
from tools.operating_point_probe import DIODES, GMIN, SPICE, seeded_diodes  # noqa: E402
from tools.transient_probe import assembled, timed, with_loads  # noqa: E402

KERNELS = ("k_transport_linearise", "k_transport_update", "k_transport_outputs", "k_transport_check", "k_transport_fill")
TRANSISTORS = 256
BETA_F, BETA_R = 100.0, 1.0
KERNEL_TRACE = "the summed time of the k_transport_* kernels (a kernel trace of its own, merged with --kernel-stats)"
NOT_MEASURED = ["the dense route (n <= 64)", "more than 256 transistors", "cfg5's network", KERNEL_TRACE]


def grid_network(N, rng):
    """tools/transient_probe.py's grid at side N: grid(N) with seven further loads"""
    grid = gen.grid_table(N)
    loads = rng.choice(np.arange(1, grid.K), 7, replace=False).astype(np.int32)
    return with_loads(grid, loads)


def seeded_transistors(table, rng):
    """(collector, base int32 [T], i_s, n_vt [T]): the collector on a seeded node, the base on the next node (its
    neighbour in the grid's row, or one node further along for a node that ends a row), the emitter on ground"""
    col = rng.choice(np.arange(0, table.K - 1), TRANSISTORS, replace=False).astype(np.int32)
    return col, col + 1, 1e-14 * 10 ** rng.uniform(0, 2, TRANSISTORS), 0.02585 * rng.uniform(1.0, 1.5, TRANSISTORS)


def case(N, rng, repeats):
    table = grid_network(N, rng)
    i_sat, n_vt, ia, ib = seeded_diodes(table, rng)
    col, base, i_s, t_nvt = seeded_transistors(table, rng)
    T = TRANSISTORS
    # the junctions behind the diodes: base -> emitter (ground) and base -> collector, forward then reverse
    j_sat = np.stack([i_s / BETA_F, i_s / BETA_R], axis=1).reshape(-1)
    j_nvt = np.repeat(t_nvt, 2)
    ja = np.repeat(base, 2)
    jb = np.stack([np.full(T, -1, dtype=np.int32), col], axis=1).reshape(-1)
    all_sat, all_nvt = np.concatenate([i_sat, j_sat]), np.concatenate([n_vt, j_nvt])
    all_a, all_b = np.concatenate([ia, ja]).astype(np.int32), np.concatenate([ib, jb]).astype(np.int32)
    junction = (DIODES + np.arange(2 * T, dtype=np.int32)).reshape(T, 2)
    bjt_table, bjt_rows, gm_rows = transistor_companion_table(table, all_sat, all_nvt, all_a, all_b, col,
                                                              np.full(T, -1, dtype=np.int32), junction, i_s, GMIN)
    # the diodes alone, and one GM row of value 0.0 on the two nodes of the grid's first resistor
    first = int(np.flatnonzero((np.asarray(table.type) == c.T_R) & (np.asarray(table.a) >= 0) & (np.asarray(table.b) >= 0))[0])
    a0, b0 = int(table.a[first]), int(table.b[first])
    plain = table.with_rows_appended(np.full(DIODES, c.T_R, dtype=np.uint8), 1.0 / (i_sat / n_vt + GMIN), ia, ib)
    plain = plain.with_controlled_rows_appended(np.array([c.T_GM], dtype=np.uint8), [0.0], [a0], [b0], [a0], [b0])
    plain_rows = np.arange(table.ncomp, table.ncomp + DIODES, dtype=np.int64)
    none = np.zeros(0, dtype=np.int64)
    with_t, without = assembled(bjt_table), assembled(plain)

    def run_t():
        return with_t.newton_dc_bjt(bjt_rows, all_sat, all_nvt, GMIN, gm_rows, junction, i_s, none, np.zeros(0), None,
                                    dense=False, max_iter=100, **SPICE)

    def run_d():
        return without.newton_dc(plain_rows, i_sat, n_vt, GMIN, none, np.zeros(0), None, dense=False, max_iter=100, **SPICE)

    out = {"grid": N, "n": int(with_t.n), "diodes": DIODES, "transistors": T, "tolerances": dict(SPICE, gmin=GMIN)}
    out["first_call_ms"] = {}
    out["first_call_ms"]["transistors"], rt = timed(with_t, run_t)
    out["first_call_timings_transistors"] = with_t.timings()
    out["first_call_ms"]["diodes_only"], rd = timed(without, run_d)
    t_ms, d_ms = [], []
    for _ in range(repeats):
        ms, rt2 = timed(with_t, run_t)
        t_ms.append(ms)
        kept_t = with_t.timings()
        ms, rd = timed(without, run_d)
        d_ms.append(ms)
        kept_d = without.timings()
    its_t, its_d = int(rt2["iterations"]), int(rd["iterations"])
    same = all(np.array_equal(rt[k], rt2[k]) for k in ("x", "v", "i", "g", "it", "gmf", "gmr", "record", "route"))
    out.update({
        "converged": bool(rt2["converged"]), "newton_iterations": its_t,
        "routes": sorted(set(int(q) for q in rt2["route"])),
        "not_converged": [int(q) for q in rt2["record"][:, 0]], "limited": [int(q) for q in rt2["record"][:, 1]],
        "transports_not_converged": [int(q) for q in rt2["record"][:, 4]],
        "largest_scaled_residual": float(rt2["record"][:, 3].max()), "repeated_call_same_bits": bool(same),
        "call_ms": t_ms, "ms_per_newton_iteration": min(t_ms) / its_t, "kept_call_timings": kept_t,
        "matrix_work_ms_per_iteration": kept_t[0] / its_t,
        "diodes_only": {"converged": bool(rd["converged"]), "newton_iterations": its_d,
                        "routes": sorted(set(int(q) for q in rd["route"])), "call_ms": d_ms,
                        "ms_per_newton_iteration": min(d_ms) / its_d, "kept_call_timings": kept_d,
                        "matrix_work_ms_per_iteration": kept_d[0] / its_d},
        "spread_ms_per_iteration": {"transistors": (max(t_ms) - min(t_ms)) / its_t,
                                    "diodes_only": (max(d_ms) - min(d_ms)) / its_d}})
    out["transistors_over_diodes_only_per_iteration"] = out["ms_per_newton_iteration"] / out["diodes_only"]["ms_per_newton_iteration"]
    print(json.dumps(out), flush=True)
    with_t.close()
    without.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/transistor_probe.json")
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
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
                                      "min_ns": float(row["MinNs"]), "max_ns": float(row["MaxNs"]),
                                      "total_ns": float(row.get("TotalDurationNs", 0.0))}
        record["kernels"] = found
        record["transport_kernels_total_ns"] = sum(v["total_ns"] for v in found.values())
        record["not_measured"] = [what for what in record.get("not_measured", []) if what != KERNEL_TRACE]
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print(json.dumps(found))
        return
    record = {"tool": "tools/transistor_probe.py", "repeats": args.repeats,
              "legs": "alternating in one process after a first call of each; host clock between stream "
                      "synchronisations; ms_per_* from the faster repeat",
              "not_measured": NOT_MEASURED}
    record["grid_8A"] = case(args.grid, np.random.default_rng(2026), args.repeats)
    if args.parent_lib:
        from tools.operating_point_gradient_probe import no_regression
        record["operating_point_against_the_parent"] = no_regression(args.parent_lib, np.random.default_rng(2026),
                                                                     max(args.repeats, 4))
    else:
        record["not_measured"] = NOT_MEASURED + ["the diodes-only operating point against the parent commit's library"]
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
