"""What a frequency of the AC gradient costs (nodal_ac_gradient) against a frequency of an AC sweep and of an AC port
analysis with two ports on the same build.

The AC probe's network: grid(N) (N = 1000: 2n ~ 2e6) with eight A sources, a capacitor of 0.5-2 F from every node to
ground and 64 seeded inductors of 0.5-3 H from seeded nodes to ground, the sparse LU route, frequencies log-spaced from
1e-3 to 1e1 Hz, 8 probes with seeded cotangents.  G is symmetric here: the forward and the adjoint right-hand side are two
columns of one factorisation per frequency.  In ONE process:

    first   the first gradient call on the handle: the child's pattern, the symbolic analysis, then the frequencies --
            nodal_last_timings [0] is the pattern + analysis, [1] the numeric factorisations
    kept    alternating, `--repeats` times, faster of each: the gradient, the AC sweep (the same 8 probes) and the port
            call with 2 ground-referenced ports: ms per frequency, the factorisations' share, the largest scaled residual

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their own,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ac_gradient_probe.py --repeats 1 --out
DIR/probe.json`; `--kernel-stats DIR/.../kernel_stats.csv` then adds the k_acgrad_* kernels (calls, total and mean time,
share of all kernel time) and the ten kernels with the most time to the record at --out.

    python tools/ac_gradient_probe.py [--grid 1000] [--out profiles/ac_gradient_probe.json] [--frequencies 16] [--repeats 2]
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
from tools.sweep_probe import with_loads  # noqa: E402
from tools.transient_probe import assembled, timed  # noqa: E402

KERNELS = ("k_acgrad_load", "k_acgrad_rhs", "k_acgrad_take", "k_acgrad_probe", "k_acgrad_rows", "k_acgrad_cross",
           "k_acgrad_react", "k_acgrad_sources", "k_ac_values")
INDUCTORS = 64
PROBES = 8


def merge_kernel_stats(args):
    with open(args.out) as f:
        record = json.load(f)
    rows = []
    with open(args.kernel_stats, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            total = float(row.get("TotalDurationNs") or float(row["AverageNs"]) * int(row["Calls"]))
            rows.append((name, int(row["Calls"]), total))
    whole = sum(t for _, _, t in rows)
    found = {}
    for key in KERNELS:
        for name, calls, total in rows:
            if key + "(" in name or name.endswith(key) or key + "E" in name:
                found[key] = {"calls": calls, "total_ms": total * 1e-6, "mean_us": total * 1e-3 / calls,
                              "share_of_kernel_time": total / whole if whole else None}
    top = sorted(rows, key=lambda r: -r[2])[:10]
    own = sum(v["total_ms"] for k, v in found.items() if k.startswith("k_acgrad"))
    record["kernels"] = {"all_kernels_total_ms": whole * 1e-6, "k_acgrad": found, "k_acgrad_total_ms": own,
                         "k_acgrad_share_of_kernel_time": own / (whole * 1e-6) if whole else None,
                         "top10": [{"name": n[:120], "calls": k, "total_ms": t * 1e-6, "share": t / whole} for n, k, t in top]}
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record["kernels"]["k_acgrad"]), record["kernels"]["k_acgrad_share_of_kernel_time"])


def case(table, args, rng):
    count = args.frequencies
    K = table.K
    rows = np.flatnonzero((table.type == c.T_A) | (table.type == c.T_E))
    farads = rng.uniform(0.5, 2.0, K)
    at = rng.choice(K, INDUCTORS, replace=False).astype(np.int32)
    henries = rng.uniform(0.5, 3.0, INDUCTORS)
    kind = np.concatenate([np.zeros(K, np.uint8), np.ones(INDUCTORS, np.uint8)])
    value = np.concatenate([farads, henries])
    lead_a = np.concatenate([np.arange(K, dtype=np.int32), at])
    lead_b = np.full(K + INDUCTORS, -1, np.int32)
    amplitudes = rng.uniform(-2, 2, len(rows)) + 1j * rng.uniform(-2, 2, len(rows))
    pa, pb = rng.choice(K, PROBES, replace=False).astype(np.int32), np.full(PROBES, -1, dtype=np.int32)
    cot = rng.uniform(-1, 1, (count, PROBES)) + 1j * rng.uniform(-1, 1, (count, PROBES))
    none = np.zeros(0, dtype=np.int32)
    omega = 2.0 * np.pi * np.logspace(-3, 1, count)
    h = assembled(table)

    def gradient():
        out = h.ac_gradient(omega, kind, value, lead_a, lead_b, rows, amplitudes, pa, pb, cot, dense=False)
        return out, h.timings()

    def sweep():
        out = h.ac_sweep(omega, kind, value, lead_a, lead_b, rows, amplitudes, pa, pb, none, dense=False)
        return out, h.timings()

    def ports():
        out = h.ac_ports(omega, kind, value, lead_a, lead_b, pa[:2], pb[:2], dense=False)
        return out, h.timings()

    record = {"network": {"n": int(h.n), "nodes": int(K), "unknowns_of_the_real_system": 2 * int(h.n), "ncomp": int(table.ncomp),
                          "capacitors": int(K), "inductors": INDUCTORS, "frequencies": count, "probes": PROBES,
                          "driven_sources": int(len(rows)), "symmetric": True}}
    ms, (out, timings) = timed(h, gradient)
    record["first_call"] = {"ms": ms, "pattern_and_analysis_ms": timings[0], "numeric_factorisations_ms": timings[1],
                            "device_ms": timings[2], "largest_scaled_residual": float(np.nanmax(out[5])),
                            "singular": int((out[6] > 0).sum()), "work": out[7].tolist()}
    print(json.dumps(record["first_call"]), flush=True)
    legs = {"ac_gradient": (gradient, 5, 6), "ac_sweep": (sweep, 4, 5), "ac_ports_2": (ports, 2, 3)}
    best = {}
    for r in range(args.repeats + 1):  # (the first round also pays the other analyses' own first calls: not kept)
        for leg, (fn, at_resid, at_info) in legs.items():
            ms, (out, timings) = timed(h, fn)
            extra = {"work": out[7].tolist()} if leg == "ac_gradient" else {"work": out[4].tolist()} if leg == "ac_ports_2" else {}
            if r > 0 and (leg not in best or ms < best[leg]["ms"]):
                best[leg] = {"ms": ms, "ms_per_frequency": ms / count, "pattern_and_analysis_ms": timings[0],
                             "numeric_factorisations_ms_per_frequency": timings[1] / count,
                             "factorisations_share": timings[1] / ms, "largest_scaled_residual": float(np.nanmax(out[at_resid])),
                             "singular": int((out[at_info] > 0).sum()), **extra}
    record["kept"] = best
    per = {leg: best[leg]["ms_per_frequency"] for leg in best}
    record["comparisons"] = {"gradient_over_ac_sweep": per["ac_gradient"] / per["ac_sweep"],
                             "gradient_over_ac_ports_2": per["ac_gradient"] / per["ac_ports_2"],
                             "ms_per_frequency_beyond_the_factorisation": per["ac_gradient"]
                             - best["ac_gradient"]["numeric_factorisations_ms_per_frequency"]}
    record["not_measured"] = ["a network whose G is not symmetric: two factorisations per frequency, the known cost",
                              "the dense routes"]
    print(json.dumps(record["kept"]), json.dumps(record["comparisons"]), flush=True)
    h.close()
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ac_gradient_probe.json")
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--frequencies", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a run of this tool: merged "
                    "into the record at --out instead of measuring")
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args)
    rng = np.random.default_rng(2026)
    grid = gen.grid_table(args.grid)
    table = with_loads(grid, rng.choice(np.arange(1, grid.K), 7, replace=False).astype(np.int32))
    record = {"tool": "tools/ac_gradient_probe.py", "grid": args.grid, "frequencies_hz": [1e-3, 1e1], "repeats": args.repeats,
              "timing": "host clock between stream synchronisations; kept calls: the faster repeat, legs alternating",
              "kernels": "not measured in this run (see --kernel-stats)"}
    record.update(case(table, args, rng))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out, flush=True)


if __name__ == "__main__":
    main()
