"""What a frequency of a noise sweep costs (nodal_ac_noise) against a frequency of an AC sweep on the same build.

The AC probe's network: grid(N) (N = 1000: 2n ~ 2e6) with eight A sources, a capacitor of 0.5-2 F from every node to
ground and 64 seeded inductors of 0.5-3 H from seeded nodes to ground, the sparse LU route, frequencies log-spaced from
1e-3 to 1e1 Hz.  Two networks:

    a_sources     the grid as it is: G symmetric, the noise analysis runs on the child it shares with the AC sweep
    one_e_source  the same with one E source from a seeded node to ground: a branch row, G not symmetric, the noise
                  analysis builds the transposed child of its own

Per network, in ONE process:

    first   the first noise call on the handle (16 frequencies, 1 output): the child's pattern, the symbolic analysis,
            then the frequencies -- nodal_last_timings [0] is the pattern + analysis, [1] the numeric factorisations
    kept    alternating, `--repeats` times, faster of each: the noise call with 1 output, the AC sweep of tools/ac_probe.py
            (8 probes, 64 inductor currents, peaks), the noise call with 16 outputs, and the noise call with 1 output, the
            gain from an input source and the integrated contributions [1][ncomp]: ms per frequency, the factorisations'
            share, the largest scaled residual, and noise over AC per frequency

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their own,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/noise_probe.py --repeats 1
--out DIR/probe.json`; `--kernel-stats DIR/.../kernel_stats.csv` then adds the k_noise_* kernels (calls, total and mean
time), the ten kernels with the most time and the sum over all kernels to the record at --out.

    python tools/noise_probe.py [--grid 1000] [--out profiles/noise_probe.json] [--frequencies 16] [--repeats 2]
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
from nodal_amd.noise import trapezoid_weights  # noqa: E402
from tools.sweep_probe import with_loads  # noqa: E402
from tools.transient_probe import assembled, timed  # noqa: E402

KERNELS = ("k_noise_rows", "k_noise_fold", "k_noise_gain", "k_noise_rhs", "k_ac_values")
INDUCTORS = 64


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
    record["kernels"] = {"all_kernels_total_ms": whole * 1e-6, "k_noise": found,
                         "top10": [{"name": n[:120], "calls": k, "total_ms": t * 1e-6, "share": t / whole} for n, k, t in top]}
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record["kernels"]["k_noise"]))


def case(name, table, args, rng):
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
    pa, pb = rng.choice(K, 8, replace=False).astype(np.int32), np.full(8, -1, dtype=np.int32)
    cur_index = np.arange(K, K + INDUCTORS, dtype=np.int32)
    outs = rng.choice(K, 16, replace=False).astype(np.int32)
    hz = np.logspace(-3, 1, count)
    omega = 2.0 * np.pi * hz
    weight = trapezoid_weights(hz)
    h = assembled(table)

    def noise(nout, full=False):
        out = h.ac_noise(omega, kind, value, lead_a, lead_b, 300.0, outs[:nout], np.full(nout, -1, np.int32), dense=False,
                         input_row=int(rows[-1]) if full else -1, weight=weight if full else None)
        return out, h.timings()

    def sweep():
        out = h.ac_sweep(omega, kind, value, lead_a, lead_b, rows, amplitudes, pa, pb, cur_index, dense=False, peaks=True)
        return out, h.timings()

    record = {"n": int(h.n), "unknowns_of_the_real_system": 2 * int(h.n), "ncomp": int(table.ncomp), "branch_rows": int(table.B),
              "capacitors": int(K), "inductors": INDUCTORS, "frequencies": count}
    ms, ((_, _, _, resid, info), timings) = timed(h, lambda: noise(1))
    record["first_call"] = {"outputs": 1, "ms": ms, "pattern_and_analysis_ms": timings[0], "numeric_factorisations_ms": timings[1],
                            "device_ms": timings[2], "largest_scaled_residual": float(np.nanmax(resid)),
                            "singular": int((info > 0).sum())}
    print(name, json.dumps(record["first_call"]), flush=True)
    legs = {"noise_1_output": lambda: noise(1), "ac_sweep": sweep, "noise_16_outputs": lambda: noise(16),
            "noise_1_output_gain_contributions": lambda: noise(1, full=True)}
    best = {}
    for r in range(args.repeats + 1):  # (the first round also pays the AC child's own first call: not kept)
        for leg, fn in legs.items():
            ms, (out, timings) = timed(h, fn)
            resid, info = (out[3], out[4]) if leg != "ac_sweep" else (out[4], out[5])
            if r > 0 and (leg not in best or ms < best[leg]["ms"]):
                best[leg] = {"ms": ms, "ms_per_frequency": ms / count, "pattern_and_analysis_ms": timings[0],
                             "numeric_factorisations_ms_per_frequency": timings[1] / count,
                             "largest_scaled_residual": float(np.nanmax(resid)), "singular": int((info > 0).sum())}
    record["kept"] = best
    ac = best["ac_sweep"]["ms_per_frequency"]
    record["noise_over_ac_per_frequency"] = {leg: best[leg]["ms_per_frequency"] / ac for leg in legs if leg != "ac_sweep"}
    print(name, json.dumps(record["kept"]), json.dumps(record["noise_over_ac_per_frequency"]), flush=True)
    h.close()
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/noise_probe.json")
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
    pinned = int(rng.integers(1, grid.K))
    with_e = table.with_branch_rows_appended(np.array([c.T_E], dtype=np.uint8), np.array([1.0]), np.array([pinned], dtype=np.int32),
                                             np.array([-1], dtype=np.int32))
    record = {"tool": "tools/noise_probe.py", "grid": args.grid, "frequencies_hz": [1e-3, 1e1], "repeats": args.repeats,
              "timing": "host clock between stream synchronisations; kept calls: the faster repeat, legs alternating",
              "kernels": "not measured in this run (see --kernel-stats)"}
    for name, t in (("a_sources", table), ("one_e_source", with_e)):
        record[name] = case(name, t, args, rng)
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print("wrote", args.out, flush=True)


if __name__ == "__main__":
    main()
