"""What adjoint sensitivities cost (nodal_sensitivities) against a source sweep of as many members.

The two sweep workloads of tools/sweep_probe.py -- grid(1000) with eight A sources (passive: block multigrid route),
cfg5's network (branch unknowns and controlled sources: sparse LU of the transposed child) -- at 1 / 16 / 64 outputs,
in ONE process, alternating A / B after a warm-up of each:

    A  nodal_sensitivities for M outputs (potentials, voltages and component currents mixed), [M][ncomp] downloaded
    B  nodal_solve_sources for M members, [M][n] downloaded: the same block solves without the table kernel

and the numpy formula pass over downloaded lambda and x on this host (what the table kernel replaces).  The very first
call on each network is reported on its own: on cfg5 it pays the transposition of the pattern and the sparse analysis
of G^T, which later calls keep.

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their
own, `rocprofv3 --kernel-trace --stats -d DIR -- python tools/sensitivity_probe.py --networks cfg5 --members 64
--repeats 1 --out DIR/probe.json`; `--networks cfg5 --kernel-stats DIR/.../kernel_stats.csv` then adds
k_sensitivity_block, k_sensitivity_cross and k_sens_rhs to that network's record, with the table kernel's bytes/s from
`block_bytes` below.

    python tools/sensitivity_probe.py [--out profiles/sensitivity_probe.json] [--members 1,16,64] [--repeats 2]
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

ACHIEVABLE_BYTES_PER_S = 6.3e12  # HBM bandwidth an MI355X kernel can reach


def block_bytes(ncomp, plain, cols):
    """Algorithmic bytes of one launch of k_sensitivity_block over `cols` columns: the table record (17 B per row of
    a plain table, 33 B with the four columns of the dependent rows), the gathered x (<= 5 doubles per row), the
    gathered lambda (cols x <= 3 doubles per row) and cols x ncomp doubles written.  An upper bound per row."""
    return int(ncomp) * ((17 if plain else 33) + 5 * 8 + cols * 3 * 8 + cols * 8)


def numpy_formulas(table, lam, x):
    """the host's way from downloaded lambda [M][n] and x [n] to the same [M][ncomp]"""
    L = np.concatenate([lam, np.zeros((lam.shape[0], 1))], axis=1)
    X = np.append(x, 0.0)
    v = table.value
    m = np.where(table.k >= 0, table.K + table.k, -1)
    dL, Lm = L[:, table.a] - L[:, table.b], L[:, m]
    dX, dXc = X[table.a] - X[table.b], X[table.c] - X[table.d]
    Rd = np.where(table.drv >= 0, v[np.where(table.drv >= 0, table.drv, 0)], 1.0)
    t = table.type
    with np.errstate(all="ignore"):
        w = np.where(t == c.T_R, dX / (v * v), np.where((t == c.T_A) | (t == c.T_E), 1.0,
                     np.where(t == c.T_VCVS, dXc, -dXc / Rd)))
        s = np.where((t == c.T_R) | (t == c.T_A), dL, Lm) * w
        for j in np.flatnonzero(((t == c.T_CCVS) | (t == c.T_CCCS)) & (table.drv >= 0)):
            i = table.drv[j]
            s[:, i] += Lm[:, j] * v[j] * dXc[j] / (v[i] * v[i])
    return s


def outputs_of(table, count, rng):
    """a mix of potentials, voltages and resistor currents"""
    res = np.flatnonzero(table.type == c.T_R)
    kind = (np.arange(count) % 3 == 2).astype(np.int32)
    p = np.where(kind == 1, rng.choice(res, count), rng.integers(table.K, size=count)).astype(np.int32)
    q2 = np.where((kind == 0) & (np.arange(count) % 3 == 1), rng.integers(table.K, size=count), -1).astype(np.int32)
    return kind, p, q2


def timed(h, fn):
    h.synchronize()
    t0 = time.perf_counter()
    out = fn()
    h.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def case(h, table, rows, ms, rng, repeats):
    plain = table.B == 0
    out = {"n": int(h.n), "ncomp": int(table.ncomp), "swept_rows": int(len(rows)), "runs": [],
           "algorithmic_bytes_per_block_of_16": block_bytes(table.ncomp, plain, 16)}

    def solve():
        assert h.run(False, member=0, reuse_symbolic=True) == 0

    solve()
    t, _ = timed(h, lambda: h.sensitivities(*outputs_of(table, 17, rng), dense=False))
    out["first_call_ms_17_outputs"] = t
    t, _ = timed(h, lambda: h.solve_sources(rows, rng.uniform(-5, 5, (17, len(rows))), dense=False))
    out["first_sweep_ms_17_members"] = t
    for m in ms:
        kind, p, q2 = outputs_of(table, m, rng)
        values = rng.uniform(-5, 5, (m, len(rows)))
        legs = {"sensitivities": [], "sensitivities_fresh_array": [], "sweep": []}
        # (one page-locked result array for the repeated calls; the leg beside it lets the binding lock a new one
        # every time, as Circuit.sensitivities does for a result its caller keeps)
        kept = _ffi.host_empty(m * table.ncomp, np.float64).reshape(m, table.ncomp)
        for _ in range(repeats):
            solve()
            t, _ = timed(h, lambda: h.sensitivities(kind, p, q2, dense=False, out=kept))
            legs["sensitivities"].append(t)
            solve()
            t, _ = timed(h, lambda: h.sensitivities(kind, p, q2, dense=False))
            legs["sensitivities_fresh_array"].append(t)
            t, (_, info, _) = timed(h, lambda: h.solve_sources(rows, values, dense=False))
            legs["sweep"].append(t)
        solve()
        few = min(m, 4)
        S, _, lam, resid, sinfo = h.sensitivities(kind[:few], p[:few], q2[:few], dense=False, adjoints=True)
        x = np.array(h.download_x())
        t0 = time.perf_counter()
        host = numpy_formulas(table, np.asarray(lam), x)
        host_ms = (time.perf_counter() - t0) * 1e3 / few
        for q in np.flatnonzero(kind[:few] == 1):  # (the explicit term of a resistor's own current)
            i = p[q]
            xe = np.append(x, 0.0)
            host[q, i] -= (xe[table.a[i]] - xe[table.b[i]]) / table.value[i] ** 2
        scale = np.abs(host).max(axis=1, keepdims=True)
        rec = {"outputs": m, "ms": legs, "ms_best": {k: min(v) for k, v in legs.items()},
               "ms_per_output_best": {k: min(v) / m for k, v in legs.items()},
               "downloaded_bytes": {"sensitivities": m * int(table.ncomp) * 8, "sweep": m * int(h.n) * 8},
               "numpy_formula_pass_ms_per_output_on_this_host": host_ms,
               "numpy_agrees_to": float((np.abs(np.asarray(S) - host) / np.where(scale > 0, scale, 1.0)).max()),
               "worst_scaled_residual": float(resid.max()), "singular": int((sinfo > 0).sum() + (info > 0).sum())}
        out["runs"].append(rec)
        print(json.dumps(rec), flush=True)
    return out


def kernel_stats(path, record, network):
    """the kernels' rows of a rocprofv3 --stats file of a run on `network` alone, and the table kernel's rate"""
    found = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for key in ("k_sensitivity_block", "k_sensitivity_cross", "k_sens_rhs", "k_sens_values", "k_gather_values"):
                if key in name:
                    label = key + ("<interleaved>" if "ILb1" in name or "<true>" in name else
                                   "<strided>" if "ILb0" in name or "<false>" in name else "")
                    found[label] = {"calls": int(row["Calls"]), "total_ns": float(row["TotalDurationNs"]),
                                    "average_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"]),
                                    "max_ns": float(row["MaxNs"])}
    record[network]["kernels"] = found
    il = found.get("k_sensitivity_block<interleaved>")
    if il:
        b = record[network]["algorithmic_bytes_per_block_of_16"]
        rate = b / (il["max_ns"] * 1e-9)  # (the longest launch is a full block of sixteen)
        record[network]["table_kernel"] = {"bytes": b, "ns": il["max_ns"], "bytes_per_s": rate,
                                           "share_of_achievable": rate / ACHIEVABLE_BYTES_PER_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/sensitivity_probe.json")
    ap.add_argument("--members", default="1,16,64")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--networks", default="grid,cfg5")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a run of this tool: merged "
                    "into the record at --out instead of measuring")
    args = ap.parse_args()
    if args.kernel_stats:
        with open(args.out) as f:
            record = json.load(f)
        name = {"grid": "cfg3_grid1000_8A", "cfg5": "cfg5"}[args.networks]
        kernel_stats(args.kernel_stats, record, name)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
        print(json.dumps(record[name].get("table_kernel")))
        return
    ms = [int(v) for v in args.members.split(",")]
    rng = np.random.default_rng(2026)
    record = {"tool": "tools/sensitivity_probe.py", "outputs": ms, "repeats": args.repeats,
              "legs": "alternating in one process after a first call of each; host clock between stream synchronisations; "
                      "a single solve (not timed) precedes every sensitivities call"}
    wanted = args.networks.split(",")
    if "grid" in wanted:
        grid = gen.grid_table(1000)
        loads = rng.choice(np.arange(1, grid.K), 7, replace=False).astype(np.int32)
        nets = [("cfg3_grid1000_8A", with_loads(grid, loads), c.T_A)]
    else:
        nets = []
    if "cfg5" in wanted:
        nets.append(("cfg5", gen.cfg5_table(1000), c.T_E))
    for name, table, kind in nets:
        h = _ffi.Handle(0)
        h.upload(table)
        h.assemble_symbolic()
        h.assemble_numeric(0)
        record[name] = case(h, table, np.flatnonzero(table.type == kind), ms, rng, args.repeats)
        h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
