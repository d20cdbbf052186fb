"""What a multiport equivalent costs (nodal_port_matrix) against a source sweep of as many members.

The two sweep workloads of tools/sweep_probe.py -- grid(1000) with eight A sources (passive: block multigrid route),
cfg5's network (branch unknowns and controlled sources: one sparse LU) -- at P = 16 / 64 / 256 ground-referenced ports
drawn with a fixed seed, in ONE process, alternating A / B after a warm-up of each:

    A  nodal_port_matrix for P ports (V_oc included): P x P numbers downloaded
    B  nodal_solve_sources for P members, [P][n] downloaded: the same block solves, the solutions brought to the host

For the grid also, at 16 terminals: nodal_solve_pairs over all 120 pairs (what equivalent_resistance_sweep calls)
against nodal_port_matrix on the 15 ports (t_i, t_0) (what resistance_matrix calls), and how far the two disagree.

Timing: the host's clock between two synchronisations of the handle's stream.  Kernel times come from a run of their
own, `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ports_probe.py --networks grid
--ports 64 --repeats 1 --out DIR/probe.json`; `--networks grid --kernel-stats DIR/.../kernel_stats.csv` then adds
k_port_rhs and k_port_gather to that network's record.

    python tools/ports_probe.py [--out profiles/ports_probe.json] [--ports 16,64,256] [--repeats 2]
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


def timed(h, fn):
    h.synchronize()
    t0 = time.perf_counter()
    out = fn()
    h.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def reciprocity(z):
    scale = np.abs(z).max(initial=0.0)
    return float(np.abs(z - z.T).max() / scale) if scale > 0 else 0.0


def case(h, table, rows, ps, rng, repeats):
    def solve():  # the single solve whose solution V_oc reads (not timed; the symbolic phase, and with it the kept
        assert h.run(False, member=0, reuse_symbolic=True) == 0  # sparse analysis of the pattern, stays)

    assert h.run(False) == 0
    out = {"n": int(h.n), "swept_rows": int(len(rows)), "runs": []}
    # the first call of each leg on its own: hierarchy or sparse analysis and factorisation, buffers
    ia = rng.choice(table.K, 17, replace=False).astype(np.int32)
    out["first_port_call_ms"] = timed(h, lambda: h.port_matrix(ia, np.full(17, -1, np.int32), dense=False))[0]
    out["first_sweep_call_ms"] = timed(h, lambda: h.solve_sources(rows, rng.uniform(-5, 5, (17, len(rows))), dense=False))[0]
    for P in ps:
        ia = rng.choice(table.K, P, replace=False).astype(np.int32)
        ib = np.full(P, -1, dtype=np.int32)
        values = rng.uniform(-5, 5, (P, len(rows)))
        port_ms, sweep_ms = [], []
        for _ in range(repeats):
            solve()
            ms, (z, v_oc, info, resid) = timed(h, lambda: h.port_matrix(ia, ib, dense=False))
            port_ms.append(ms)
            ms, (x, sinfo, sresid) = timed(h, lambda: h.solve_sources(rows, values, dense=False))
            sweep_ms.append(ms)
            del x
        rec = {"ports": P, "port_matrix_ms": port_ms, "solve_sources_ms": sweep_ms,
               "ms_per_port": min(port_ms) / P, "ms_per_sweep_member": min(sweep_ms) / P,
               "port_over_sweep": min(port_ms) / min(sweep_ms),
               "largest_scaled_residual": float(resid.max()), "sweep_largest_scaled_residual": float(sresid.max()),
               "reciprocity": reciprocity(z), "singular": int((info > 0).sum() + (sinfo > 0).sum())}
        out["runs"].append(rec)
        print(json.dumps(rec), flush=True)
    return out


def pairs_case(h, table, rng, repeats):
    """all pairs among 16 terminals: the pair sweep against the port matrix of 15 ports"""
    t = rng.choice(table.K, 16, replace=False).astype(np.int32)
    pi, pj = np.triu_indices(16, 1)
    sweep_ms, matrix_ms = [], []
    for _ in range(repeats + 1):  # (the first round is the warm-up of both)
        ms, (res, pinfo) = timed(h, lambda: h.solve_pairs(t[pi], t[pj], dense=False))
        sweep_ms.append(ms)
        ms, (z, _, info, resid) = timed(h, lambda: h.port_matrix(t[1:], np.full(15, t[0], np.int32), dense=False, voc=False))
        matrix_ms.append(ms)
    zp = np.zeros((16, 16))
    zp[1:, 1:] = z
    d = np.diag(zp)
    R = d[:, None] + d[None, :] - zp - zp.T
    rec = {"terminals": 16, "pairs": int(len(pi)), "pair_sweep_ms": sweep_ms[1:], "port_matrix_ms": matrix_ms[1:],
           "sweep_over_matrix": min(sweep_ms[1:]) / min(matrix_ms[1:]),
           "largest_relative_difference": float((np.abs(R[pi, pj] - res) / res).max()),
           "singular": int(pinfo > 0) + int((info > 0).sum())}
    print(json.dumps(rec), flush=True)
    return rec


def kernel_stats(path, record, network):
    """the two port kernels' rows of a rocprofv3 --stats file of a run on `network` alone"""
    found = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for key in ("k_port_rhs", "k_port_gather"):
                if key in name:
                    found[key] = {"calls": int(row["Calls"]), "total_ns": float(row["TotalDurationNs"]),
                                  "average_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"]),
                                  "max_ns": float(row["MaxNs"])}
    record[network]["kernels"] = found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ports_probe.json")
    ap.add_argument("--ports", default="16,64,256")
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
        print(json.dumps(record[name]["kernels"]))
        return
    ps = [int(v) for v in args.ports.split(",")]
    rng = np.random.default_rng(2026)
    record = {"tool": "tools/ports_probe.py", "ports": ps, "repeats": args.repeats,
              "legs": "alternating in one process after a first call of each; host clock between stream synchronisations; "
                      "ms_per_* from the faster repeat; a single solve (not timed) precedes every port call"}
    wanted = args.networks.split(",")
    nets = []
    if "grid" in wanted:
        grid = gen.grid_table(1000)
        loads = rng.choice(np.arange(1, grid.K), 7, replace=False).astype(np.int32)
        nets.append(("cfg3_grid1000_8A", with_loads(grid, loads), c.T_A))
    if "cfg5" in wanted:
        nets.append(("cfg5", gen.cfg5_table(1000), c.T_E))
    for name, table, kind in nets:
        h = _ffi.Handle(0)
        h.upload(table)
        record[name] = case(h, table, np.flatnonzero(table.type == kind), ps, rng, args.repeats)
        if name == "cfg3_grid1000_8A":
            record[name]["all_pairs_of_16_terminals"] = pairs_case(h, table, rng, args.repeats)
        h.close()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
