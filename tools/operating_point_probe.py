"""What a Newton iteration of the operating-point analysis (nodal_newton_dc) costs beside a fresh numeric solve.

Two workloads, tools/transient_probe.py's networks with 1024 seeded diodes (i_sat 1e-14 .. 1e-12 A, n_vt 25.85 .. 39 mV):

    grid   grid(1000) with eight A sources (n = 999 999, the multigrid route): a diode on every source node, forward for
           its source, the rest on seeded nodes, half of them to ground in either direction, half between neighbours
    cfg5   cfg5's network (E sources and dependent sources, the sparse LU route), diodes placed the same way

In ONE process, after a first call of each, alternating, faster of `--repeats`:

    N   nodal_newton_dc from zeros at SPICE's tolerances (reltol 1e-3, vntol 1e-6, abstol 1e-12, gmin 1e-12) on the handle
        that holds the table with the companion rows: ms per Newton iteration = the call / its iterations
    R   a repeated nodal_run(reuse_symbolic=1) of the same matrix (the companion rows at their v = 0 values) on a second
        handle: the fresh numeric solve an iteration is compared with
    H   the host loop the call replaces, `--host-iterations` of it on a third handle: download x, the diode pass in
        numpy, nodal_upload_values of the whole column, nodal_assemble_numeric, nodal_solve_sparse (the right-hand
        side's history currents would need a further upload: left out, in the host loop's favour)

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their own,
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/operating_point_probe.py --networks grid
--repeats 1 --host-iterations 0 --out DIR/probe.json`; `--kernel-stats DIR/.../kernel_stats.csv` then adds the k_newton_*
kernels to the record at --out.

    python tools/operating_point_probe.py [--out profiles/operating_point_probe.json] [--networks grid,cfg5]
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nodal_amd import _ffi  # noqa: E402
from nodal_amd import constants as c  # noqa: E402
from tools.transient_probe import assembled, network, timed  # noqa: E402

KERNELS = ("k_newton_linearise", "k_newton_update", "k_newton_outputs", "k_newton_start", "k_newton_check",
           "k_signed_list_add")
DIODES = 1024
SPICE = dict(reltol=1e-3, vntol=1e-6, abstol=1e-12)
GMIN = 1e-12


def seeded_diodes(table, rng):
    """(i_sat, n_vt, ia, ib): one diode on the first lead of every A row, forward for a positive source, the rest seeded"""
    K = table.K
    ia, ib = [], []
    for row in np.flatnonzero(table.type == c.T_A):
        node = int(table.a[row]) if table.a[row] >= 0 else int(table.b[row])
        push = (table.value[row] > 0) == (table.a[row] >= 0)  # the source raises this node
        ia.append(node if push else -1)
        ib.append(-1 if push else node)
    while len(ia) < DIODES:
        k = int(rng.integers(0, K - 1))
        u = rng.random()
        if u < 0.25:
            ia.append(k), ib.append(-1)
        elif u < 0.5:
            ia.append(-1), ib.append(k)
        else:
            ia.append(k), ib.append(k + 1)
    ia, ib = np.asarray(ia[:DIODES], dtype=np.int32), np.asarray(ib[:DIODES], dtype=np.int32)
    return 1e-14 * 10 ** rng.uniform(0, 2, DIODES), 0.02585 * rng.uniform(1.0, 1.5, DIODES), ia, ib


def case(name, rng, repeats, host_iterations):
    table, _ = network(name, rng)
    i_sat, n_vt, ia, ib = seeded_diodes(table, rng)
    value0 = 1.0 / (i_sat / n_vt + GMIN)
    child_table = table.with_rows_appended(np.full(DIODES, c.T_R, dtype=np.uint8), value0, ia, ib)
    diode_rows = np.arange(table.ncomp, table.ncomp + DIODES, dtype=np.int64)
    none = np.zeros(0, dtype=np.int64)
    newton, fresh = assembled(child_table), assembled(child_table)

    def run_newton():
        return newton.newton_dc(diode_rows, i_sat, n_vt, GMIN, none, np.zeros(0), None, dense=False, max_iter=100, **SPICE)

    out = {"n": int(newton.n), "diodes": DIODES, "tolerances": dict(SPICE, gmin=GMIN)}
    out["first_newton_call_ms"], r = timed(newton, run_newton)
    out["first_newton_call_timings"] = newton.timings()
    assert fresh.run(False) == 0
    n_ms, r_ms = [], []
    for _ in range(repeats):
        ms, r = timed(newton, run_newton)
        n_ms.append(ms)
        kept = newton.timings()
        ms, _ = timed(fresh, lambda: [fresh.run(False, member=0, reuse_symbolic=True) for _ in range(8)])
        r_ms.append(ms / 8)
    its = int(r["iterations"])
    out.update({"converged": bool(r["converged"]), "newton_iterations": its, "routes": sorted(set(int(q) for q in r["route"])),
                "solver_iterations": [int(q) for q in r["iters"]], "not_converged": [int(q) for q in r["record"][:, 0]],
                "limited": [int(q) for q in r["record"][:, 1]], "largest_scaled_residual": float(r["record"][:, 3].max()),
                "newton_call_ms": n_ms, "ms_per_newton_iteration": min(n_ms) / its, "kept_call_timings": kept,
                "matrix_work_ms_per_iteration": kept[0] / its, "repeated_nodal_run_ms": r_ms,
                "ms_per_fresh_solve": min(r_ms), "fresh_solve_iterations": int(fresh.solve_info()[0]),
                "iteration_over_fresh_solve": min(n_ms) / its / min(r_ms)})
    print(json.dumps(out), flush=True)
    newton.close()
    fresh.close()
    if host_iterations > 0:  # the loop the call replaces
        host = assembled(child_table)
        host.solve_sparse()
        values = np.array(child_table.value, dtype=np.float64)
        lead = lambda x, idx: np.where(idx >= 0, x[np.maximum(idx, 0)], 0.0)  # noqa: E731
        vh = np.zeros(DIODES)

        def host_loop():
            nonlocal vh
            for _ in range(host_iterations):
                x = host.download_x()
                v = lead(x, ia) - lead(x, ib)
                vh = np.minimum(v, vh + 2 * n_vt)  # (a stand-in for the limiter: the cost is the same numpy pass)
                values[diode_rows] = 1.0 / (i_sat * np.exp(vh / n_vt) / n_vt + GMIN)
                host.upload_values(values[None, :])
                host.assemble_numeric(0)
                host.solve_sparse()

        timed(host, host_loop)
        ms, _ = timed(host, host_loop)
        out["host_loop_ms_per_iteration"] = ms / host_iterations
        out["host_loop_iterations_timed"] = host_iterations
        host.close()
        print(json.dumps({"host_loop_ms_per_iteration": out["host_loop_ms_per_iteration"]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/operating_point_probe.json")
    ap.add_argument("--networks", default="grid,cfg5")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--host-iterations", type=int, default=3)
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
                                      "min_ns": float(row["MinNs"]), "max_ns": float(row["MaxNs"])}
        record["kernels"] = found
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print(json.dumps(found))
        return
    keys = {"grid": "cfg3_grid1000_8A", "cfg5": "cfg5"}
    record = {"tool": "tools/operating_point_probe.py", "repeats": args.repeats,
              "legs": "alternating in one process after a first call of each; host clock between stream "
                      "synchronisations; ms_per_* from the faster repeat"}
    rng = np.random.default_rng(2026)
    for name in args.networks.split(","):
        record[keys[name]] = case(name, rng, args.repeats, args.host_iterations)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
