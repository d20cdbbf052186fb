"""What a loss gradient costs (nodal_gradient) against the source sweep of as many members.

The two sweep workloads of tools/sweep_probe.py -- grid(1000) with eight A sources (passive: block multigrid route),
cfg5's network (branch unknowns and controlled sources: sparse LU of the transposed child) -- at 1 / 16 / 64 / 256
members, in ONE process, alternating A / B after a warm-up of each:

    A  nodal_gradient for M members: cotangents [M][n] and solutions [M][n] go up, [ncomp] + [M][nsrc] come down
    B  nodal_solve_sources for M members, [M][n] downloaded: the same block solves (the yardstick)

The call should cost about one sweep plus the two uploads.  The host-to-device share is reported on its own, two ways:
leg A again with both arrays in page-locked memory (what is left is DMA at link rate), and the bare copy of as many
bytes from pageable memory (nodal_upload_values of [M][ncomp] doubles on a second handle; ncomp is about 2 n, so that is
the size of the two uploads together).

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their
own, `rocprofv3 --kernel-trace --stats -d DIR -- python tools/gradient_probe.py --networks cfg5 --members 64
--repeats 1 --out DIR/probe.json`; `--networks cfg5 --kernel-stats DIR/.../kernel_stats.csv` then adds the k_gradient_*
kernels to that network's record, with the table kernel's bytes/s from `block_bytes` below.

    python tools/gradient_probe.py [--out profiles/gradient_probe.json] [--members 1,16,64,256] [--repeats 2]
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
KERNELS = ("k_gradient_block", "k_gradient_cross", "k_gradient_sources", "k_gradient_interleave", "k_gradient_spread")


def block_bytes(ncomp, plain, cols):
    """Algorithmic bytes of one launch of k_gradient_block over `cols` members: the table record (17 B per row of a
    plain table, 33 B with the four columns of the dependent rows), per member at most 2 gathered doubles of lambda and
    2 of x, and the row's sum read and written once.  An upper bound per row: A and E rows read no x."""
    return int(ncomp) * ((17 if plain else 33) + cols * 4 * 8 + 16)


def timed(h, fn):
    h.synchronize()
    t0 = time.perf_counter()
    out = fn()
    h.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def pinned(shape):
    return _ffi.host_empty(int(np.prod(shape)), np.float64).reshape(shape)


def case(h, h_copy, table, rows, ms, rng, repeats):
    n, ncomp = int(h.n), int(table.ncomp)
    out = {"n": n, "ncomp": ncomp, "swept_rows": int(len(rows)), "runs": [],
           "algorithmic_bytes_per_block_of_16": block_bytes(ncomp, table.B == 0, 16)}
    values = rng.uniform(-5, 5, (17, len(rows)))
    t, (x, _, _) = timed(h, lambda: h.solve_sources(rows, values, dense=False))
    out["first_sweep_ms_17_members"] = t
    t, _ = timed(h, lambda: h.gradient(rng.standard_normal((17, n)), dense=False, rows=rows, solutions=x))
    out["first_call_ms_17_members"] = t
    for m in ms:
        values = rng.uniform(-5, 5, (m, len(rows)))
        x, info, _ = h.solve_sources(rows, values, dense=False)
        cot = rng.standard_normal((m, n))
        x_pin, cot_pin = pinned((m, n)), pinned((m, n))
        x_pin[:], cot_pin[:] = x, cot
        bare = np.ones((m, ncomp))
        legs = {"gradient": [], "gradient_page_locked_inputs": [], "sweep": [], "bare_upload_of_as_many_bytes": []}
        for _ in range(repeats):
            t, res = timed(h, lambda: h.gradient(cot, dense=False, rows=rows, solutions=x))
            legs["gradient"].append(t)
            t, (_, sinfo, _) = timed(h, lambda: h.solve_sources(rows, values, dense=False))
            legs["sweep"].append(t)
            t, res_pin = timed(h, lambda: h.gradient(cot_pin, dense=False, rows=rows, solutions=x_pin))
            legs["gradient_page_locked_inputs"].append(t)
            t, _ = timed(h_copy, lambda: h_copy.upload_values(bare))
            legs["bare_upload_of_as_many_bytes"].append(t)
        grad, gsrc, _, resid, ginfo = res
        best = {k: min(v) for k, v in legs.items()}
        rec = {"members": m, "ms": legs, "ms_best": best,
               "gradient_over_sweep": best["gradient"] / best["sweep"],
               "gradient_minus_sweep_ms": best["gradient"] - best["sweep"],
               "host_to_device": {"bytes": 2 * m * n * 8, "bare_copy_ms": best["bare_upload_of_as_many_bytes"],
                                  "saved_by_page_locked_inputs_ms": best["gradient"] - best["gradient_page_locked_inputs"]},
               "downloaded_bytes": {"gradient": (ncomp + m * len(rows)) * 8, "sweep": m * n * 8},
               "same_bits_from_page_locked_inputs": bool(np.array_equal(grad, res_pin[0])),
               # the gradient at a swept row is the sum of the members' own derivatives
               "swept_rows_sum_defect": float(np.abs(grad[rows] - gsrc.sum(axis=0)).max() /
                                              max(np.abs(gsrc).sum(axis=0).max(), 1e-300)),
               "worst_scaled_residual": float(resid.max()),
               "singular": int((ginfo > 0).sum() + (sinfo > 0).sum() + (info > 0).sum())}
        out["runs"].append(rec)
        print(json.dumps(rec), flush=True)
    return out


def kernel_stats(path, record, network):
    """the kernels' rows of a rocprofv3 --stats file of a run on `network` alone, and the table kernel's rate"""
    found = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for key in KERNELS:
                if key in name:
                    label = key + ("<interleaved>" if "ILb1" in name or "<true>" in name else
                                   "<strided>" if "ILb0" in name or "<false>" in name else "")
                    found[label] = {"calls": int(row["Calls"]), "total_ns": float(row["TotalDurationNs"]),
                                    "average_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"]),
                                    "max_ns": float(row["MaxNs"])}
    record[network]["kernels"] = found
    il = found.get("k_gradient_block<interleaved>")
    if il:
        b = record[network]["algorithmic_bytes_per_block_of_16"]
        rate = b / (il["max_ns"] * 1e-9)  # (the longest launch is a full block of sixteen)
        record[network]["table_kernel"] = {"bytes": b, "ns": il["max_ns"], "bytes_per_s": rate,
                                           "share_of_achievable": rate / ACHIEVABLE_BYTES_PER_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/gradient_probe.json")
    ap.add_argument("--members", default="1,16,64,256")
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
    record = {"tool": "tools/gradient_probe.py", "members": ms, "repeats": args.repeats,
              "legs": "alternating in one process after a first call of each; host clock between stream synchronisations"}
    wanted = args.networks.split(",")
    nets = []
    if "grid" in wanted:
        grid = gen.grid_table(1000)
        loads = rng.choice(np.arange(1, grid.K), 7, replace=False).astype(np.int32)
        nets.append(("cfg3_grid1000_8A", with_loads(grid, loads), c.T_A))
    if "cfg5" in wanted:
        nets.append(("cfg5", gen.cfg5_table(1000), c.T_E))
    for name, table, kind in nets:
        h, h_copy = _ffi.Handle(0), _ffi.Handle(0)
        for handle in (h, h_copy):
            handle.upload(table)
        h.assemble_symbolic()
        h.assemble_numeric(0)
        record[name] = case(h, h_copy, table, np.flatnonzero(table.type == kind), ms, rng, args.repeats)
        h.close()
        h_copy.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
