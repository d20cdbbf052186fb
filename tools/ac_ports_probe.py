"""What a frequency of an AC port analysis costs (nodal_ac_ports) against a frequency of an AC sweep and of a noise sweep
on the same build.

The AC probe's network: grid(N) (N = 1000: 2n ~ 2e6) with eight A sources, a capacitor of 0.5-2 F from every node to
ground and 64 seeded inductors of 0.5-3 H from seeded nodes to ground, the sparse LU route, frequencies log-spaced from
1e-3 to 1e1 Hz.  In ONE process:

    first   the first port call on the handle (16 frequencies, 1 port): the child's pattern, the symbolic analysis, then the
            frequencies -- nodal_last_timings [0] is the pattern + analysis, [1] the numeric factorisations
    kept    alternating, `--repeats` times, faster of each: the port call with 1 / 16 / 64 ground-referenced seeded ports,
            each without and with the node peaks, the AC sweep of tools/ac_probe.py (8 probes, 64 inductor currents,
            peaks) and the noise call with 16 outputs: ms per frequency, the factorisations' share, the largest scaled
            residual, the largest reciprocity(); then ms per further port from 16 -> 64 against the noise analysis's ms
            per further output, and one port against one ac() frequency

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their own,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ac_ports_probe.py --repeats 1 --ports 16,64
--out DIR/probe.json` (full blocks only, so that every call of the peak kernel reads sixteen columns);
`--kernel-stats DIR/.../kernel_stats.csv --kernel-record DIR/probe.json` then adds the k_acport_* kernels (calls, total
and mean time), the peak kernel's achieved bandwidth (the node rows of 2 x nodes x 16 doubles it reads once per call,
over its mean time), the ten kernels with the most time and the sum over all kernels to the record at --out.

    python tools/ac_ports_probe.py [--grid 1000] [--out profiles/ac_ports_probe.json] [--frequencies 16] [--repeats 2]
                                   [--ports 1,16,64]
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

KERNELS = ("k_acport_rhs", "k_acport_residual", "k_acport_correct", "k_acport_gather", "k_acport_peak", "k_acport_merge",
           "k_ac_peak_root", "k_acport_rows", "k_ac_values")
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
    record["kernels"] = {"all_kernels_total_ms": whole * 1e-6, "k_acport": found,
                         "top10": [{"name": n[:120], "calls": k, "total_ms": t * 1e-6, "share": t / whole} for n, k, t in top]}
    peak = found.get("k_acport_peak")
    if peak and args.kernel_record:
        with open(args.kernel_record) as f:
            run = json.load(f)
        # the peak legs of that run: per frequency and round of repeats one call per block of its port counts
        rounds, count, nodes = run["repeats"] + 1, run["network"]["frequencies"], run["network"]["nodes"]
        columns = rounds * count * sum(run["ports"])
        calls = rounds * count * sum(-(-p // 16) for p in run["ports"])
        read = columns * 2 * nodes * 8
        record["kernels"]["k_acport_peak_bandwidth"] = {
            "ports_of_the_run": run["ports"], "calls_expected": calls, "bytes_read": read,
            "GB_per_s": read / (peak["total_ms"] * 1e-3) * 1e-9,
            "note": "2 x nodes x columns doubles read once per call, all calls of the run over their total time"}
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record["kernels"]["k_acport"]), json.dumps(record["kernels"].get("k_acport_peak_bandwidth")))


def reciprocity(z):
    worst = 0.0
    for zf in z:
        top = np.abs(zf).max()
        if top > 0:
            worst = max(worst, float(np.abs(zf - zf.T).max() / top))
    return worst


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
    pa, pb = rng.choice(K, 8, replace=False).astype(np.int32), np.full(8, -1, dtype=np.int32)
    cur_index = np.arange(K, K + INDUCTORS, dtype=np.int32)
    outs = rng.choice(K, 16, replace=False).astype(np.int32)
    PORTS = args.ports
    sites = rng.choice(K, max(PORTS), replace=False).astype(np.int32)
    omega = 2.0 * np.pi * np.logspace(-3, 1, count)
    h = assembled(table)

    def ports(nports, peaks):
        out = h.ac_ports(omega, kind, value, lead_a, lead_b, sites[:nports], np.full(nports, -1, np.int32), dense=False, peaks=peaks)
        return out, h.timings()

    def sweep():
        out = h.ac_sweep(omega, kind, value, lead_a, lead_b, rows, amplitudes, pa, pb, cur_index, dense=False, peaks=True)
        return out, h.timings()

    def noise():
        out = h.ac_noise(omega, kind, value, lead_a, lead_b, 300.0, outs, np.full(16, -1, np.int32), dense=False)
        return out, h.timings()

    n2 = 2 * int(h.n)
    record = {"network": {"n": int(h.n), "nodes": int(K), "unknowns_of_the_real_system": n2, "ncomp": int(table.ncomp),
                          "capacitors": int(K), "inductors": INDUCTORS, "frequencies": count},
              "interleaved_block_vectors": {"count": 4, "bytes_each": n2 * 16 * 8, "MiB_all": 4 * n2 * 16 * 8 / 2 ** 20}}
    ms, ((z, _, resid, info, work), timings) = timed(h, lambda: ports(PORTS[0], False))
    record["first_call"] = {"ports": PORTS[0], "ms": ms, "pattern_and_analysis_ms": timings[0], "numeric_factorisations_ms": timings[1],
                            "device_ms": timings[2], "largest_scaled_residual": float(np.nanmax(resid)),
                            "singular": int((info > 0).sum()), "work": work.tolist()}
    print(json.dumps(record["first_call"]), flush=True)
    legs = {}
    for nports in PORTS:
        legs[f"ports_{nports}"] = lambda nports=nports: ports(nports, False)
        legs[f"ports_{nports}_peaks"] = lambda nports=nports: ports(nports, True)
    legs["ac_sweep"] = sweep
    legs["noise_16_outputs"] = noise
    best = {}
    for r in range(args.repeats + 1):  # (the first round also pays the other analyses' own first calls: not kept)
        for leg, fn in legs.items():
            ms, (out, timings) = timed(h, fn)
            if leg.startswith("ports"):
                resid, info, extra = out[2], out[3], {"work": out[4].tolist(), "largest_reciprocity": reciprocity(out[0])}
            elif leg == "ac_sweep":
                resid, info, extra = out[4], out[5], {}
            else:
                resid, info, extra = out[3], out[4], {}
            if r > 0 and (leg not in best or ms < best[leg]["ms"]):
                best[leg] = {"ms": ms, "ms_per_frequency": ms / count, "pattern_and_analysis_ms": timings[0],
                             "numeric_factorisations_ms_per_frequency": timings[1] / count,
                             "factorisations_share": timings[1] / ms, "largest_scaled_residual": float(np.nanmax(resid)),
                             "singular": int((info > 0).sum()), **extra}
    record["kept"] = best
    per = {leg: best[leg]["ms_per_frequency"] for leg in best}
    record["comparisons"] = {
        "ms_per_further_noise_output_from_16": (per["noise_16_outputs"] - per["ac_sweep"]) / 15.0,
        "peaks_ms_per_frequency": {str(p): per[f"ports_{p}_peaks"] - per[f"ports_{p}"] for p in PORTS},
        "note": "the noise figure takes an AC sweep's frequency for the cost of the noise call's first output"}
    if "ports_1" in per:
        record["comparisons"]["one_port_over_one_ac_frequency"] = per["ports_1"] / per["ac_sweep"]
    for lo, hi in zip(PORTS, PORTS[1:]):
        record["comparisons"][f"ms_per_further_port_{lo}_to_{hi}"] = (per[f"ports_{hi}"] - per[f"ports_{lo}"]) / (hi - lo)
    print(json.dumps(record["kept"]), json.dumps(record["comparisons"]), flush=True)
    h.close()
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ac_ports_probe.json")
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--frequencies", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--ports", type=lambda text: [int(p) for p in text.split(",")], default=[1, 16, 64])
    ap.add_argument("--kernel-record", default=None, help="the record the profiled run wrote (its repeats and ports)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a run of this tool: merged "
                    "into the record at --out instead of measuring")
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args)
    rng = np.random.default_rng(2026)
    grid = gen.grid_table(args.grid)
    table = with_loads(grid, rng.choice(np.arange(1, grid.K), 7, replace=False).astype(np.int32))
    record = {"tool": "tools/ac_ports_probe.py", "grid": args.grid, "frequencies_hz": [1e-3, 1e1], "repeats": args.repeats,
              "ports": args.ports, "timing": "host clock between stream synchronisations; kept calls: the faster repeat, legs alternating",
              "kernels": "not measured in this run (see --kernel-stats)"}
    record.update(case(table, args, rng))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out, flush=True)


if __name__ == "__main__":
    main()
