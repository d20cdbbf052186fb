"""What a time step with diodes (nodal_transient_nl) costs beside a linear step and beside the host loop it replaces.

The network is tools/transient_probe.py's grid: grid(1000) with eight A sources (n = 999 999, the multigrid route), a
capacitor from every node to ground (backward Euler, dt = 1), and 1024 diodes, over `--steps` steps whose sources switch
between their table values and 1.5 times them in blocks of eight steps.  In ONE process, after a first call of each leg,
alternating, faster of `--repeats`:

  conducting  tools/operating_point_probe.py's 1024 seeded diodes, the start their nonlinear DC point (nodal_newton_dc)
      N   nodal_transient_nl: ms per step, Newton iterations per step, matrix updates, and this file's count of what one
          iteration launches besides the assembly and the solver
      L   nodal_transient on the same network without the diodes, the same sources: the linear step
      H   the host loop N replaces, `--host-iterations` Newton iterations of it: download x, the diode pass and the
          capacitors' history currents in numpy, nodal_upload_values of the whole column, nodal_assemble_numeric,
          nodal_solve_sparse (the upload of the history currents left out, in the host loop's favour); its ms per step is
          its ms per iteration times N's iterations per step
  at rest     1024 diodes on the nodes the DC solution moves furthest from ground, every one reverse-biased, the sources
              scaled so that the least of them sits at -3 V: N against L on the same sources (the expectation to confirm or
              refute: about the same ms per step), with the least reverse bias seen and the matrix updates

and `--parent-lib PATH`, a libnodal_hip.so built from the parent commit: nodal_transient on tools/transient_probe.py's case
(64 steps) alternating between the two libraries in this process, `--repeats` times each: the difference of the faster
runs beside the run-to-run spread of each library's own runs, and whether every output has the same bits.

Timing: the host's clock between two synchronisations of the handle's stream.

    python tools/transient_diodes_probe.py [--out profiles/transient_diodes_probe.json] [--parent-lib PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nodal_amd import _ffi  # noqa: E402
from nodal_amd import constants as c  # noqa: E402
from tools.operating_point_probe import DIODES, GMIN, SPICE, seeded_diodes  # noqa: E402
from tools.transient_probe import DT, assembled, network, timed  # noqa: E402

LAUNCHES_PER_ITERATION = {"k_newton_linearise": 1, "copy rhs = base (device to device)": 1, "k_signed_list_add": 1,
                          "k_newton_update<true>": 1, "besides": "stamp_numeric (when the matrix moved) and the solver's own"}
MAX_ITER = 50


def with_rows(table, values, ia, ib):
    rows = np.arange(table.ncomp, table.ncomp + len(values), dtype=np.int64)
    return table.with_rows_appended(np.full(len(values), c.T_R, dtype=np.uint8), values, ia, ib), rows


def switching(table, rows, steps, scale=1.0):
    base = scale * np.asarray(table.value, dtype=np.float64)[rows]
    return np.array([base * (1.0 if (k // 8) % 2 == 0 else 1.5) for k in range(steps)])


def legs(table, rows, values, farads, diodes, x0, steps, repeats, label):
    """N against L on one network: the record of both"""
    K = table.K
    i_sat, n_vt, ia, ib = diodes
    nodes, ground = np.arange(K, dtype=np.int32), np.full(K, -1, np.int32)
    lin_table, cap_rows = with_rows(table, DT / farads, nodes, ground)
    nl_table, diode_rows = with_rows(lin_table, 1.0 / (i_sat / n_vt + GMIN), ia, ib)
    lin, nl = assembled(lin_table), assembled(nl_table)
    pa, pb = np.arange(8, dtype=np.int32) * (K // 8), np.full(8, -1, dtype=np.int32)
    none, index = np.zeros(0, dtype=np.int64), np.arange(DIODES, dtype=np.int32)

    def run_nl():
        return nl.transient_nl(cap_rows, none, diode_rows, i_sat, n_vt, GMIN, rows, values, x0, np.zeros(0), pa, pb,
                               np.zeros(0, dtype=np.int32), index, dense=False, max_iter=MAX_ITER, **SPICE)

    def run_lin():
        return lin.transient(cap_rows, rows, values, x0, pa, pb, dense=False, method=0)

    out = {"n": int(nl.n), "diodes": DIODES, "steps": steps, "tolerances": dict(SPICE, gmin=GMIN)}
    out["first_nl_call_ms"], _ = timed(nl, run_nl)
    out["first_nl_call_timings"] = nl.timings()
    out["first_linear_call_ms"], _ = timed(lin, run_lin)
    n_ms, l_ms = [], []
    for _ in range(repeats):
        ms, r = timed(nl, run_nl)
        n_ms.append(ms)
        kept = nl.timings()
        ms, rl = timed(lin, run_lin)
        l_ms.append(ms)
    wave, _, _, resid, info, iters, _, _, extra = r
    newton, updates = extra["newton"], extra["updates"]
    out.update({"nl_call_ms": n_ms, "linear_call_ms": l_ms, "ms_per_step": min(n_ms) / steps,
                "linear_ms_per_step": min(l_ms) / steps, "nl_over_linear": min(n_ms) / min(l_ms),
                "newton_iterations": [int(q) for q in newton], "newton_iterations_per_step": float(newton.mean()),
                "matrix_updates": [int(q) for q in updates], "ms_per_newton_iteration": min(n_ms) / max(int(newton.sum()), 1),
                "solver_iterations": [int(q) for q in iters], "info": sorted(set(int(q) for q in info)),
                "largest_scaled_residual": float(np.nanmax(resid)), "linear_largest_scaled_residual": float(rl[3].max()),
                "kept_call_timings": kept, "highest_junction_voltage": float(np.nanmax(extra["v"])),
                "launches_per_iteration": LAUNCHES_PER_ITERATION})
    print(label, json.dumps(out), flush=True)
    nl.close()
    lin.close()
    return out, nl_table, diode_rows, cap_rows


def host_loop(nl_table, diode_rows, cap_rows, farads, diodes, iterations):
    i_sat, n_vt, ia, ib = diodes
    host = assembled(nl_table)
    host.solve_sparse()
    values = np.array(nl_table.value, dtype=np.float64)
    lead = lambda x, idx: np.where(idx >= 0, x[np.maximum(idx, 0)], 0.0)  # noqa: E731
    state = {"vh": np.zeros(DIODES)}

    def loop():
        for _ in range(iterations):
            x = host.download_x()
            v = lead(x, ia) - lead(x, ib)
            state["vh"] = np.minimum(v, state["vh"] + 2 * n_vt)  # (a stand-in for the limiter: the same numpy pass)
            values[diode_rows] = 1.0 / (i_sat * np.exp(np.minimum(state["vh"], 1.0) / n_vt) / n_vt + GMIN)
            state["J"] = (farads / DT) * x[:len(farads)]  # the capacitors' history currents (their upload left out)
            host.upload_values(values[None, :])
            host.assemble_numeric(0)
            host.solve_sparse()

    timed(host, loop)
    ms, _ = timed(host, loop)
    host.close()
    return ms / iterations


def parent_handle(path):
    """a Handle on another build of the library (the binding cut down to what it exports)"""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _ffi.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    mine, _ffi._lib = _ffi.load(), lib
    try:
        return _ffi.Handle(0)
    finally:
        _ffi._lib = mine


def no_regression(path, rng, repeats, steps=64):
    table, rows = network("grid", rng)
    K = table.K
    farads = rng.uniform(0.5, 2.0, K)
    child_table, cap_rows = with_rows(table, DT / farads, np.arange(K, dtype=np.int32), np.full(K, -1, np.int32))
    handles = {"this": _ffi.Handle(0), "parent": parent_handle(path)}
    for h in handles.values():
        h.upload(child_table)
        h.assemble_symbolic()
        h.assemble_numeric(0)
    x0 = np.zeros(handles["this"].n)
    pa, pb = rng.choice(K, 8, replace=False).astype(np.int32), np.full(8, -1, dtype=np.int32)
    values = rng.uniform(-5, 5, (steps, len(rows)))
    run = lambda h: h.transient(cap_rows, rows, values, x0, pa, pb, dense=False, method=0, envelope=True)  # noqa: E731
    ms, last = {k: [] for k in handles}, {}
    for h in handles.values():
        timed(h, lambda: run(h))
    for _ in range(repeats):
        for key, h in handles.items():
            t, last[key] = timed(h, lambda: run(h))
            ms[key].append(t)
    a, b = last["this"], last["parent"]
    same = all(np.array_equal(a[q], b[q]) for q in (0, 3, 4, 5)) and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
    out = {"steps": steps, "this_ms": ms["this"], "parent_ms": ms["parent"],
           "difference_ms_per_step": (min(ms["this"]) - min(ms["parent"])) / steps,
           "spread_ms_per_step": {k: (max(v) - min(v)) / steps for k, v in ms.items()}, "bit_equal": bool(same)}
    out["inside_the_spread"] = bool(out["difference_ms_per_step"] <= max(out["spread_ms_per_step"].values()))
    for h in handles.values():
        h.close()
    print("no regression", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/transient_diodes_probe.json")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--host-iterations", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    record = {"tool": "tools/transient_diodes_probe.py", "repeats": args.repeats,
              "legs": "alternating in one process after a first call of each; host clock between stream "
                      "synchronisations; ms_per_* from the faster repeat",
              "not_measured": ["the dense route's time", "the sparse LU route on cfg5's network", "more than 1024 diodes"]}
    rng = np.random.default_rng(2026)
    table, rows = network("grid", rng)
    K = table.K
    farads = rng.uniform(0.5, 2.0, K)
    none = np.zeros(0, dtype=np.int64)
    # ---- conducting ----
    diodes = seeded_diodes(table, rng)
    dc_table, dc_rows = with_rows(table, 1.0 / (diodes[0] / diodes[1] + GMIN), diodes[2], diodes[3])
    dc = assembled(dc_table)
    start = dc.newton_dc(dc_rows, diodes[0], diodes[1], GMIN, none, np.zeros(0), None, dense=False, max_iter=100, **SPICE)
    dc.close()
    assert start["converged"]
    values = switching(table, rows, args.steps)
    rec, nl_table, diode_rows, cap_rows = legs(table, rows, values, farads, diodes, start["x"], args.steps, args.repeats,
                                               "conducting")
    rec["dc_start_newton_iterations"] = int(start["iterations"])
    if args.host_iterations > 0:
        per = host_loop(nl_table, diode_rows, cap_rows, farads, diodes, args.host_iterations)
        rec["host_loop_ms_per_iteration"] = per
        rec["host_loop_ms_per_step"] = per * rec["newton_iterations_per_step"]
        rec["host_loop_over_device"] = rec["host_loop_ms_per_step"] / rec["ms_per_step"]
        print(json.dumps({"host_loop_ms_per_iteration": per}), flush=True)
    record["conducting"] = rec
    # ---- at rest: every junction reverse-biased, the least of them at -3 V ----
    lin = assembled(table)
    assert lin.run(False) == 0
    x = lin.download_x()[:K]
    lin.close()
    far = np.argsort(-np.abs(x))[:DIODES].astype(np.int32)
    scale = 3.0 / float(np.abs(x[far]).min())
    up = x[far] > 0  # a node above ground: the cathode there, the anode on ground
    ground = np.full(DIODES, -1, dtype=np.int32)
    rest = (diodes[0], diodes[1], np.where(up, ground, far).astype(np.int32), np.where(up, far, ground).astype(np.int32))
    rec, _, _, _ = legs(table, rows, switching(table, rows, args.steps, scale), farads, rest, np.append(scale * x, np.zeros(
        assembled_n(table) - K)), args.steps, args.repeats, "at rest")
    rec["source_scale"] = scale
    record["at_rest"] = rec
    if args.parent_lib:
        record["no_regression_without_diodes"] = no_regression(args.parent_lib, np.random.default_rng(2026), max(args.repeats, 4))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out)


def assembled_n(table):
    return table.K + table.B


if __name__ == "__main__":
    main()
