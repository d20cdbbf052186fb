"""What the gradient through time costs (nodal_transient_gradient) against the forward run it differentiates.

The two workloads of tools/transient_probe.py -- grid(1000) with eight A sources (passive: the multigrid route, the
backward sweep on the forward run's own hierarchy) and cfg5's network (branch unknowns and controlled sources: the sparse
LU route, the backward sweep on the transposed child) -- each with a capacitor from every node to ground, backward
Euler, 8 probes, at 64 and 256 steps, in ONE process on the child handle, after a first call of each, alternating, the
faster of `--repeats`:

    recorded   nodal_transient with NODAL_OPT_TRANSIENT_TAPE set (x_k written into the tape)
    backward   nodal_transient_gradient with seeded cotangents of the 8 waveforms (grad, grad_sources, grad_x0 down)
    plain      nodal_transient with the option off, on the same build

and per run: ms per step, the backward sweep's matrix work (the first call's, then 0.0), the largest scaled residual of
both sweeps.  Timing: the host's clock between two synchronisations of the handle's stream.

    python tools/transient_gradient_probe.py [--out profiles/transient_gradient_probe.json] [--steps 64,256] [--repeats 2]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nodal_amd import _ffi  # noqa: E402
from nodal_amd import constants as c  # noqa: E402
from tools.transient_probe import DT, assembled, network, timed  # noqa: E402


def case(table, rows, steps_list, rng, repeats):
    K = table.K
    farads = rng.uniform(0.5, 2.0, K)
    nodes = np.arange(K, dtype=np.int32)
    child_table = table.with_rows_appended(np.full(K, c.T_R, dtype=np.uint8), DT / farads, nodes, np.full(K, -1, np.int32))
    cap_rows = np.arange(table.ncomp, table.ncomp + K, dtype=np.int64)
    parent, child = assembled(table), assembled(child_table)
    assert parent.run(False) == 0
    x0 = parent.download_x()
    parent.close()
    pa = rng.choice(K, 8, replace=False).astype(np.int32)
    pb = np.full(8, -1, dtype=np.int32)
    out = {"n": int(child.n), "capacitors": int(K), "swept_rows": int(len(rows)), "dt": DT, "runs": []}

    def forward(values, record):
        child.set_option(_ffi.OPT_TRANSIENT_TAPE, int(record))
        try:
            return child.transient(cap_rows, rows, values, x0, pa, pb, dense=False, method=0)
        finally:
            child.set_option(_ffi.OPT_TRANSIENT_TAPE, 0)

    def backward(steps, cot):
        return child.transient_gradient(steps, len(rows), pa, pb, cot, dense=False)

    warm = rng.uniform(-5, 5, (17, len(rows)))
    out["first_recorded_call_ms"], _ = timed(child, lambda: forward(warm, True))
    out["first_backward_call_ms"], _ = timed(child, lambda: backward(17, rng.uniform(-1, 1, (18, 8))))
    out["first_backward_matrix_ms"] = child.timings()[0]
    for steps in steps_list:
        values = rng.uniform(-5, 5, (steps, len(rows)))
        cot = rng.uniform(-1, 1, (steps + 1, 8))
        rec_ms, back_ms, plain_ms = [], [], []
        for _ in range(repeats):
            ms, (_, _, _, resid, info, _) = timed(child, lambda: forward(values, True))
            rec_ms.append(ms)
            ms, (grad, _, _, _, bresid, binfo) = timed(child, lambda: backward(steps, cot))
            back_ms.append(ms)
            matrix_ms = child.timings()[0]
            ms, _ = timed(child, lambda: forward(values, False))
            plain_ms.append(ms)
        rec = {"steps": steps, "recorded_ms": rec_ms, "backward_ms": back_ms, "plain_ms": plain_ms,
               "recorded_ms_per_step": min(rec_ms) / steps, "backward_ms_per_step": min(back_ms) / steps,
               "plain_ms_per_step": min(plain_ms) / steps, "kept_backward_matrix_ms": matrix_ms,
               "largest_scaled_residual_forward": float(resid.max()), "largest_scaled_residual_backward": float(bresid.max()),
               "singular": int((info > 0).sum() + (binfo > 0).sum()), "grad_finite": bool(np.isfinite(grad).all())}
        out["runs"].append(rec)
        print(json.dumps(rec), flush=True)
    child.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/transient_gradient_probe.json")
    ap.add_argument("--steps", default="64,256")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--networks", default="grid,cfg5")
    args = ap.parse_args()
    steps_list = [int(v) for v in args.steps.split(",")]
    keys = {"grid": "cfg3_grid1000_8A", "cfg5": "cfg5"}
    record = {"tool": "tools/transient_gradient_probe.py", "steps": steps_list, "repeats": args.repeats,
              "legs": "alternating in one process after a first call of each; host clock between stream synchronisations; "
                      "ms_per_step from the faster repeat"}
    rng = np.random.default_rng(2026)
    for name in args.networks.split(","):
        table, rows = network(name, rng)
        record[keys[name]] = case(table, rows, steps_list, rng, args.repeats)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
