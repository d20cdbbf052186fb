"""What a gradient through the operating point (nodal_newton_gradient) costs beside one Newton iteration.

tools/operating_point_probe.py's two workloads, 1024 seeded diodes each:

    grid   grid(1000) with eight A sources (n = 999 999, the multigrid route)
    cfg5   cfg5's network (E sources and dependent sources, the sparse LU route on the transposed child)

In ONE process, after a first call of each, alternating, faster of `--repeats`:

    N   nodal_newton_dc from zeros at SPICE's tolerances on the handle that holds the table with the companion rows:
        ms per Newton iteration = the call / its iterations
    G   nodal_newton_gradient at N's x with a seeded cotangent, on the same handle: ms per call; the first call apart
        (on cfg5 it makes the transposed child and analyses it)
    H   the host loop the call replaces, on the same box: export the assembled matrix (the handle's G holds the
        companion rows at the last linearisation), scipy's splu of its transpose and one solve, the numpy formulas of
        the resistor rows and of the diodes (the other rows' formulas and the cross terms of cfg5's driving resistors
        are left out, in the host loop's favour: `host_loop_agrees` compares what it does compute)

and, with `--parent-lib PATH` (a libnodal_hip.so built from the parent commit), nodal_newton_dc itself on this build and
on that one, alternating, every output compared bit for bit.

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their own,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/operating_point_gradient_probe.py --networks
grid --repeats 1 --no-host --out DIR/probe.json`; `--kernel-stats DIR/.../kernel_stats.csv` then adds the lane kernels
to the record at --out.

    python tools/operating_point_gradient_probe.py [--out profiles/operating_point_gradient_probe.json] [--parent-lib PATH]
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
from tools.operating_point_probe import DIODES, GMIN, SPICE, seeded_diodes  # noqa: E402
from tools.transient_diodes_probe import parent_handle  # noqa: E402
from tools.transient_probe import assembled, network, timed  # noqa: E402

KERNELS = ("k_opgrad_diodes", "k_opgrad_total", "k_newton_linearise", "k_newton_start", "k_newton_check", "k_newton_fill",
           "k_signed_list_add", "k_gradient_block", "k_gradient_cross", "k_gradient_sources")


def host_gradient(handle, table, x, cot, i_sat, n_vt, ia, ib, diode_rows):
    """the loop the call replaces: the assembled matrix down, scipy's transposed solve, numpy formulas"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    indptr, indices, data, _ = handle.export_csr()
    n = len(x)
    J = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    lam = spla.splu(J.T.tocsc()).solve(cot)
    L, X = np.append(lam, 0.0), np.append(x, 0.0)
    rows = np.flatnonzero(np.asarray(table.type) == c.T_R)
    a, b, v = np.asarray(table.a)[rows], np.asarray(table.b)[rows], np.asarray(table.value)[rows]
    grad = np.zeros(table.ncomp)
    grad[rows] = (L[a] - L[b]) * (X[a] - X[b]) / (v * v)
    grad[diode_rows] = 0.0
    D, vd = L[ia] - L[ib], X[ia] - X[ib]
    e = np.exp(vd / n_vt)
    return grad, -D * (e - 1.0), D * i_sat * e * vd / n_vt ** 2, float(np.sum(-D * vd))


def case(name, rng, repeats, host):
    table, _ = network(name, rng)
    i_sat, n_vt, ia, ib = seeded_diodes(table, rng)
    value0 = 1.0 / (i_sat / n_vt + GMIN)
    child_table = table.with_rows_appended(np.full(DIODES, c.T_R, dtype=np.uint8), value0, ia, ib)
    diode_rows = np.arange(table.ncomp, table.ncomp + DIODES, dtype=np.int64)
    none = np.zeros(0, dtype=np.int64)
    handle = assembled(child_table)
    cot = rng.standard_normal(handle.n)

    def run_newton():
        return handle.newton_dc(diode_rows, i_sat, n_vt, GMIN, none, np.zeros(0), None, dense=False, max_iter=100, **SPICE)

    def run_gradient(x):
        return handle.newton_gradient(diode_rows, i_sat, n_vt, GMIN, none, np.zeros(0), x, cot, dense=False)

    out = {"n": int(handle.n), "diodes": DIODES, "tolerances": dict(SPICE, gmin=GMIN)}
    out["first_newton_call_ms"], r = timed(handle, run_newton)
    x = r["x"]
    out["first_gradient_call_ms"], g = timed(handle, lambda: run_gradient(x))
    out["first_gradient_call_timings"] = handle.timings()
    n_ms, g_ms, resid = [], [], [g["resid"]]
    for _ in range(repeats):
        ms, r = timed(handle, run_newton)
        n_ms.append(ms)
        ms, g2 = timed(handle, lambda: run_gradient(r["x"]))
        g_ms.append(ms)
        kept = handle.timings()
        resid.append(g2["resid"])
    its = int(r["iterations"])
    same = all(np.array_equal(g[k], g2[k]) for k in ("grad", "i_sat", "n_vt", "sources")) and g["gmin"] == g2["gmin"]
    out.update({"converged": bool(r["converged"]), "newton_iterations": its,
                "routes": sorted(set(int(q) for q in r["route"])), "newton_call_ms": n_ms,
                "ms_per_newton_iteration": min(n_ms) / its, "gradient_call_ms": g_ms, "ms_per_gradient_call": min(g_ms),
                "gradient_over_newton_iteration": min(g_ms) / (min(n_ms) / its), "kept_gradient_call_timings": kept,
                "largest_scaled_residual": float(max(resid)), "operating_point_residual": float(g2["op_resid"]),
                "info": int(g2["info"]), "repeated_call_same_bits": bool(same)})
    print(json.dumps(out), flush=True)
    if host:
        t0 = time.perf_counter()
        hg = host_gradient(handle, child_table, r["x"], cot, i_sat, n_vt, ia, ib, diode_rows)
        out["host_loop_ms"] = (time.perf_counter() - t0) * 1e3
        resistors = np.flatnonzero(np.asarray(child_table.type) == c.T_R)
        scale = np.abs(hg[0][resistors]).max()
        out["host_loop_agrees"] = {"resistor_rows": float(np.abs(hg[0][resistors] - g2["grad"][resistors]).max() / scale),
                                   "i_sat": float(np.abs(hg[1] - g2["i_sat"]).max() / np.abs(hg[1]).max()),
                                   "n_vt": float(np.abs(hg[2] - g2["n_vt"]).max() / np.abs(hg[2]).max()),
                                   "gmin": float(abs(hg[3] - g2["gmin"]) / abs(hg[3]))}
        print(json.dumps({"host_loop_ms": out["host_loop_ms"], "host_loop_agrees": out["host_loop_agrees"]}), flush=True)
    handle.close()
    return out


def no_regression(path, rng, repeats):
    """nodal_newton_dc on this build and on the parent's, alternating, bit for bit"""
    table, _ = network("grid", rng)
    i_sat, n_vt, ia, ib = seeded_diodes(table, rng)
    child_table = table.with_rows_appended(np.full(DIODES, c.T_R, dtype=np.uint8), 1.0 / (i_sat / n_vt + GMIN), ia, ib)
    diode_rows = np.arange(table.ncomp, table.ncomp + DIODES, dtype=np.int64)
    none = np.zeros(0, dtype=np.int64)
    handles = {"this": _ffi.Handle(0), "parent": parent_handle(path)}
    for h in handles.values():
        h.upload(child_table)
        h.assemble_symbolic()
        h.assemble_numeric(0)
    run = lambda h: h.newton_dc(diode_rows, i_sat, n_vt, GMIN, none, np.zeros(0), None, dense=False, max_iter=100,  # noqa: E731
                                keep_iterates=False, **SPICE)
    ms, last = {k: [] for k in handles}, {}
    for h in handles.values():
        timed(h, lambda: run(h))
    for _ in range(repeats):
        for key, h in handles.items():
            t, last[key] = timed(h, lambda: run(h))
            ms[key].append(t)
    a, b = last["this"], last["parent"]
    same = all(np.array_equal(a[k], b[k]) for k in ("x", "v", "i", "g", "record", "info", "iters", "route")) and \
        a["iterations"] == b["iterations"] and a["converged"] == b["converged"]
    its = int(a["iterations"])
    out = {"newton_iterations": its, "this_ms": ms["this"], "parent_ms": ms["parent"],
           "difference_ms_per_iteration": (min(ms["this"]) - min(ms["parent"])) / its,
           "spread_ms_per_iteration": {k: (max(v) - min(v)) / its for k, v in ms.items()}, "bit_equal": bool(same)}
    out["inside_the_spread"] = bool(out["difference_ms_per_iteration"] <= max(out["spread_ms_per_iteration"].values()))
    for h in handles.values():
        h.close()
    print("no regression", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/operating_point_gradient_probe.json")
    ap.add_argument("--networks", default="grid,cfg5")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a run of this tool: merged "
                    "into the record at --out instead of measuring")
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as f:
            record = json.load(f)
        found, total = {}, 0.0
        with open(args.kernel_stats, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name") or row.get("KernelName") or ""
                total += float(row["TotalDurationNs"]) if "TotalDurationNs" in row else 0.0
                for key in KERNELS:
                    if key in name:
                        found[key] = {"calls": int(row["Calls"]), "average_ns": float(row["AverageNs"]),
                                      "min_ns": float(row["MinNs"]), "max_ns": float(row["MaxNs"]),
                                      "total_ns": float(row.get("TotalDurationNs", 0.0))}
        lanes = sum(v["total_ns"] for v in found.values())
        record["kernels"] = found
        record["lane_kernels_share_of_kernel_time"] = lanes / total if total > 0 else None
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print(json.dumps({"kernels": found, "share": record["lane_kernels_share_of_kernel_time"]}))
        return
    keys = {"grid": "cfg3_grid1000_8A", "cfg5": "cfg5"}
    record = {"tool": "tools/operating_point_gradient_probe.py", "repeats": args.repeats,
              "legs": "alternating in one process after a first call of each; host clock between stream "
                      "synchronisations; ms_per_* from the faster repeat"}
    rng = np.random.default_rng(2026)
    for name in args.networks.split(","):
        record[keys[name]] = case(name, rng, args.repeats, not args.no_host)
    if args.parent_lib:
        record["operating_point_against_the_parent"] = no_regression(args.parent_lib, np.random.default_rng(2026),
                                                                     max(args.repeats, 4))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
