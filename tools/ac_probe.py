"""What a frequency of an AC sweep costs (nodal_ac_sweep) against what a user does on the host today.

The transient probes' grid workload turned to the frequency domain: grid(N) (N = 1000: 2n ~ 2e6) with eight A sources,
all of them driven with seeded complex amplitudes, a capacitor of 0.5-2 F from every node to ground and 64 seeded
inductors of 0.5-3 H from seeded nodes to ground; 8 probes, the 64 inductor currents, peaks on, no solutions kept; the
sparse LU route.  Frequencies log-spaced from 1e-3 to 1e1 Hz.  In ONE process:

    first   the first call on the handle (16 frequencies): the doubled system's pattern, the symbolic analysis, then the
            frequencies -- nodal_last_timings [0] is the pattern + analysis, [1] the numeric factorisations
    kept    the call again with pattern and analysis kept, 16 and 64 frequencies, faster of `--repeats`: ms per frequency,
            the factorisations' share, the largest scaled residual, the singular frequencies
    host    what a user does today, on this box's host: G exported once (nodal_export_csr), G + j B formed with scipy and
            scipy.sparse.linalg.spsolve per frequency -- `--host-frequencies` of them (default 2, not 64), and the largest
            difference from the device's phasors at those frequencies over the largest phasor

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their own,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ac_probe.py --repeats 1 --host-frequencies 0
--out DIR/probe.json`; `--kernel-stats DIR/.../kernel_stats.csv --traced-run DIR/probe.json` then adds the k_ac_* kernels,
the ten kernels with the most time, the sum over all kernels and its share of the traced calls to the record at --out.

    python tools/ac_probe.py [--grid 1000] [--out profiles/ac_probe.json] [--frequencies 16,64] [--repeats 2]
"""
import argparse
import csv
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
from tools.transient_probe import assembled, timed  # noqa: E402

KERNELS = ("k_ac_values", "k_ac_sources_off", "k_ac_probe", "k_ac_current", "k_ac_peak", "k_ac_peak_root")
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
                found[key] = {"calls": calls, "total_ms": total * 1e-6, "share_of_kernel_time": total / whole if whole else None}
    top = sorted(rows, key=lambda r: -r[2])[:10]
    record["kernels"] = {"all_kernels_total_ms": whole * 1e-6, "k_ac": found,
                         "k_ac_share_of_kernel_time": sum(v["total_ms"] for v in found.values()) / (whole * 1e-6) if whole else None,
                         "top10": [{"name": n[:120], "calls": k, "total_ms": t * 1e-6, "share": t / whole} for n, k, t in top]}
    if args.traced_run:  # the traced run's own record: what its calls took on the host's clock, tracer attached
        with open(args.traced_run) as f:
            traced = json.load(f)
        wall = traced["first_call"]["ms"] + sum(k["ms"] * traced["repeats"] for k in traced["kept"])
        record["kernels"]["traced_calls"] = {"first_call_ms": traced["first_call"]["ms"],
                                             "kept_calls_ms": [k["ms"] for k in traced["kept"]], "all_calls_ms": wall,
                                             "kernels_share_of_the_calls": whole * 1e-6 / wall}
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print(json.dumps(record["kernels"]["k_ac"]), record["kernels"]["k_ac_share_of_kernel_time"])


def host_system(h, table, rows, amplitudes):
    """what the host route starts from: G exported from the device as a complex scipy matrix, the right-hand side from
    the table; (G, s, ms)"""
    import scipy.sparse as sp
    t0 = time.perf_counter()
    indptr, indices, data, _ = h.export_csr()
    n = h.n
    G = sp.csr_matrix((data, indices, indptr), shape=(n, n)).astype(np.complex128)
    s = np.zeros(n, dtype=np.complex128)
    for row, amp in zip(rows, amplitudes):  # (A rows: +v on lead a, -v on lead b)
        if table.a[row] >= 0:
            s[table.a[row]] += amp
        if table.b[row] >= 0:
            s[table.b[row]] -= amp
    return G, s, (time.perf_counter() - t0) * 1e3


def host_solve(G, s, K, omega, farads, at, henries):
    """G + j B with scipy and spsolve per frequency: (ms per frequency, X [F, n])"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    n = G.shape[0]
    per, X = [], []
    for w in omega:
        t0 = time.perf_counter()
        b = np.zeros(n)
        b[:K] = w * farads
        np.add.at(b, at, -1.0 / (w * henries))
        M = (G + 1j * sp.diags(b)).tocsc()
        X.append(spla.spsolve(M, s))
        per.append((time.perf_counter() - t0) * 1e3)
    return per, np.array(X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ac_probe.json")
    ap.add_argument("--grid", type=int, default=1000)
    ap.add_argument("--frequencies", default="16,64")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--host-frequencies", type=int, default=2)
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a run of this tool: merged "
                    "into the record at --out instead of measuring")
    ap.add_argument("--traced-run", default=None, help="with --kernel-stats: the record that traced run wrote (its --out)")
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args)
    counts = [int(v) for v in args.frequencies.split(",")]
    rng = np.random.default_rng(2026)
    grid = gen.grid_table(args.grid)
    table = with_loads(grid, rng.choice(np.arange(1, grid.K), 7, replace=False).astype(np.int32))
    rows = np.flatnonzero(table.type == c.T_A)
    K = table.K
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

    def omegas(count):
        return 2.0 * np.pi * np.logspace(-3, 1, count)

    h = assembled(table)

    def sweep(omega):
        out = h.ac_sweep(omega, kind, value, lead_a, lead_b, rows, amplitudes, pa, pb, cur_index, dense=False, peaks=True)
        return out, h.timings()

    record = {"tool": "tools/ac_probe.py", "grid": args.grid, "n": int(h.n), "unknowns_of_the_real_system": 2 * int(h.n),
              "capacitors": int(K), "inductors": INDUCTORS, "driven_sources": int(len(rows)), "probes": 8,
              "frequencies_hz": [1e-3, 1e1], "repeats": args.repeats,
              "timing": "host clock between stream synchronisations; kept calls: the faster repeat"}
    ms, ((wave, cur, _, peak, resid, info), timings) = timed(h, lambda: sweep(omegas(counts[0])))
    record["first_call"] = {"frequencies": counts[0], "ms": ms, "pattern_and_analysis_ms": timings[0],
                            "numeric_factorisations_ms": timings[1], "device_ms": timings[2],
                            "largest_scaled_residual": float(np.nanmax(resid)), "singular": int((info > 0).sum())}
    print(json.dumps(record["first_call"]), flush=True)
    record["kept"] = []
    waves = {}
    for count in counts:
        best = None
        for _ in range(args.repeats):
            ms, ((wave, cur, _, peak, resid, info), timings) = timed(h, lambda: sweep(omegas(count)))
            if best is None or ms < best["ms"]:
                best = {"frequencies": count, "ms": ms, "ms_per_frequency": ms / count, "pattern_and_analysis_ms": timings[0],
                        "numeric_factorisations_ms_per_frequency": timings[1] / count,
                        "largest_scaled_residual": float(np.nanmax(resid)), "singular": int((info > 0).sum()),
                        "largest_peak": float(np.nanmax(peak[0]))}
        waves[count] = wave
        record["kept"].append(best)
        print(json.dumps(best), flush=True)
    record["host"] = "not measured in this run"
    record["kernels"] = "not measured in this run (see --kernel-stats)"
    if args.host_frequencies > 0:
        G, s, export_ms = host_system(h, table, rows, amplitudes)
    h.close()

    def write():
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print("wrote", args.out, flush=True)

    write()  # (the device's part is on file before the host's solves begin: they take the longest)
    if args.host_frequencies > 0:
        count = counts[0]
        pick = np.linspace(0, count - 1, args.host_frequencies).round().astype(int)
        per, X = host_solve(G, s, K, omegas(count)[pick], farads, at, henries)
        got = waves[count][pick]
        want = X[:, pa]
        record["host"] = {"what": "nodal_export_csr once, G + j B with scipy, scipy.sparse.linalg.spsolve per frequency",
                          "frequencies_timed": int(args.host_frequencies), "export_and_form_G_ms": export_ms,
                          "ms_per_frequency": per, "cpus": os.cpu_count(),
                          "largest_difference_from_device_phasors_over_largest_phasor":
                              float(np.abs(got - want).max() / np.abs(want).max())}
        print(json.dumps(record["host"]), flush=True)
        write()


if __name__ == "__main__":
    main()
