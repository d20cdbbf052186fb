"""The bits of the three nonlinear analyses (nodal_newton_dc, nodal_transient_nl, nodal_newton_gradient) as SHA-256
digests per output array, for comparing two builds of the library on one machine: a restructuring of csrc/newton.hip,
transient_nl.hip and newton_gradient.hip must leave every digest as it was.

Every call is made twice on one circuit and asks for every optional output; the second call's arrays are digested, its
integer outputs, `timings[1] == 0.0` (no symbolic work) and an error status are recorded as values.  The networks are
those of tests/newton_reference.py and tests/transient_nl_reference.py.

    newton_dc         a diode behind a resistor (dense and sparse), the sparse LU network from a cold and a hard start,
                      the multigrid network, no diodes, no unknowns, max_iter too small, the underflowed diode (singular:
                      NaN on the sparse path, the error status on the dense one), the start that overflows and the
                      ordinary solve after it
    transient_nl      the rectifier (both methods, both paths; the sparse Euler run wraps the ring of 64 records), the LU
                      network with inductors, the multigrid network, clamps at rest with and without NODAL_TNL_REUSE=0,
                      no steps, max_iter 1 (info 2), the floating island (info 1), the step that overflows and a linear
                      solve after it
    newton_gradient   the closed-form case, the transposed child, the LU network, the multigrid network, no diodes, the
                      singular Jacobian on both paths, the conductance that overflows and an ordinary call after it

    python tools/newton_family_digest.py --out A.json [--root TREE]   the library and package of TREE (default: this tree)
    python tools/newton_family_digest.py --compare A.json B.json      exit status 1 unless every digest and value is equal
"""
import argparse
import hashlib
import json
import os
import sys
import warnings

import numpy as np


def circuit_of(rows, sparse):
    import nodal_amd as n
    return n.Circuit(n.Netlist.from_rows([list(r) for r in rows]), sparse=sparse, device=0)


def twice(call):
    """what the second of two identical calls returned"""
    call()
    return call()


def newton_dc(circ, diodes, gmin=1e-12, initial=None, max_iter=100):
    from nodal_amd import _ffi
    from nodal_amd.operating_point import resolve_diodes
    from tests.newton_reference import TIGHT
    _, i_sat, n_vt, ia, ib = resolve_diodes(circ.netlist, diodes)
    child, rows = circ._newton_companion(i_sat, n_vt, ia, ib, gmin)
    h = child._handle
    x0 = None if initial is None else np.asarray(initial, dtype=np.float64)
    try:
        r = twice(lambda: h.newton_dc(rows, i_sat, n_vt, gmin, np.zeros(0, dtype=np.int64), np.zeros(0), x0,
                                      dense=not circ.sparse, max_iter=max_iter, keep_iterates=True, **TIGHT))
    except _ffi.NodalHipError as exc:
        return [], {"status": int(exc.status)}
    arrays = [r[k] for k in ("x", "v", "i", "g", "record", "iterates", "vh")]
    values = {"iterations": r["iterations"], "converged": r["converged"], "timings1_is_zero": float(h.timings()[1]) == 0.0,
              **{k: [int(v) for v in r[k]] for k in ("info", "iters", "route")}}
    return arrays, values


def transient_nl(circ, case, method="euler", initial=None, max_iter=50, steps=None, envelope=True):
    """envelope=False where no step may finish: the envelope is then nobody's to define"""
    from tests.newton_reference import TIGHT
    rows, caps, inds, diodes, dt, nsteps, sources = case
    if steps is not None:
        nsteps, sources = steps, {name: np.asarray(wave)[:steps] for name, wave in sources.items()} if steps else None
    nodes = sorted(circ.netlist.nodenum, key=circ.netlist.nodenum.get)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr = twice(lambda: circ.transient(caps, dt, nsteps, sources=sources, probes=nodes, method=method, initial=initial,
                                          inductors=inds, current_probes=[i[0] for i in inds], diodes=diodes,
                                          diode_probes=[d[0] for d in diodes], keep_every=1, envelope=envelope,
                                          max_iter=max_iter, **TIGHT))
    env = tr.envelope
    arrays = [tr.waveforms, tr.solutions, tr.scaled_residual, tr.currents, tr.final_currents, tr.diode_voltages,
              tr.diode_currents, tr.final_junctions] + ([env.potential_min, env.potential_max] if envelope else [])
    integers = [("info", tr.info), ("iterations", tr.iterations), ("newton", tr.newton_iterations), ("updates", tr.matrix_updates)]
    if envelope:
        integers += [("min_step", env.potential_min_step), ("max_step", env.potential_max_step)]
    values = {"timings1_is_zero": float(tr.timings[1]) == 0.0, **{k: [int(v) for v in a] for k, a in integers}}
    return arrays, values


def newton_gradient(circ, diodes, x=None, gmin=1e-12, seed=7):
    """at the operating point the device finds (x None) or at the caller's x, through the companion child's handle"""
    from nodal_amd import _ffi
    from nodal_amd.operating_point import resolve_diodes
    from tests.newton_reference import TIGHT
    _, i_sat, n_vt, ia, ib = resolve_diodes(circ.netlist, diodes)
    child, rows = circ._newton_companion(i_sat, n_vt, ia, ib, gmin)
    h = child._handle
    none = np.zeros(0, dtype=np.int64), np.zeros(0)
    if x is None:
        x = h.newton_dc(rows, i_sat, n_vt, gmin, *none, None, dense=not circ.sparse, max_iter=100, **TIGHT)["x"]
    cot = np.random.default_rng(seed).uniform(-1.0, 1.0, h.n)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            r = twice(lambda: h.newton_gradient(rows, i_sat, n_vt, gmin, *none, x, cot, dense=not circ.sparse, adjoints=True))
    except _ffi.NodalHipError as exc:
        return [], {"status": int(exc.status)}
    arrays = [r["grad"], r["i_sat"], r["n_vt"], r["sources"], r["adjoint"], np.array([r["gmin"], r["resid"], r["op_resid"]])]
    return arrays, {"info": r["info"], "timings1_is_zero": float(h.timings()[1]) == 0.0}


def solve_on(child):
    x, info = child._handle.solve_sparse()[:2]
    return [x], {"info": int(info)}


def measure():
    from tests import newton_reference as nr
    from tests import transient_nl_reference as tn
    I_SAT, N_VT = nr.I_SAT, nr.N_VT
    lu_rows, lu_diodes, lu_hard = nr.lu_case()
    mg_rows, mg_diodes = nr.mg_case()
    series, d_series = nr.series_rows(5.0, 1000.0), [("d1", I_SAT, N_VT, "2", "g")]
    hanging = [["a1", "A", "1", "1", "g"], ["r1", "R", "1", "1", "g"], ["a2", "A", "0", "2", "g"]]
    d_hanging = [("d1", I_SAT, N_VT, "2", "1")]
    one = [["a1", "A", "1", "1", "g"], ["r1", "R", "1", "1", "g"]]
    d_one = [("d1", I_SAT, N_VT, "1", "g")]
    hot = np.zeros(145)
    cases = {}

    def case(name, result):
        cases[name] = result
        print(name, "done", flush=True)

    # ---- nodal_newton_dc ----
    for sparse in (False, True):
        case(f"dc/series/sparse_{sparse}", newton_dc(circuit_of(series, sparse), d_series))
        circ = circuit_of(hanging, sparse)
        reverse = np.zeros(2)
        reverse[circ.netlist.nodenum["2"]] = -30.0  # exp(-30 / n_vt) underflows: g is exactly 0 and node 2 floats
        case(f"dc/underflowed/sparse_{sparse}", newton_dc(circ, d_hanging, gmin=0.0, initial=reverse))
        circ = circuit_of(one, sparse)
        case(f"dc/overflow/sparse_{sparse}", newton_dc(circ, d_one, initial=[100.0]))
        case(f"dc/overflow/sparse_{sparse}/then", newton_dc(circ, d_one))
    circ = circuit_of(lu_rows, True)
    hot[circ.netlist.nodenum["30"]] = 100.0
    case("dc/lu/cold", newton_dc(circ, lu_diodes))
    case("dc/lu/hard", newton_dc(circ, lu_diodes, initial=lu_hard))
    case("dc/lu/max_iter_2", newton_dc(circ, lu_diodes, initial=lu_hard, max_iter=2))
    case("dc/lu/no_diodes", newton_dc(circ, []))
    case("dc/multigrid", newton_dc(circuit_of(mg_rows, True), mg_diodes))
    case("dc/no_unknowns", newton_dc(circuit_of([["r1", "R", "2", "g", "g"], ["a1", "A", "1", "g", "g"]], True), []))

    # ---- nodal_transient_nl ----
    for method in ("euler", "trapezoidal"):
        for sparse in (False, True):
            case(f"tnl/rectifier/{method}/sparse_{sparse}",
                 transient_nl(circuit_of(tn.rectifier_case()[0], sparse), tn.rectifier_case(), method))
    wrapped = sum(cases["tnl/rectifier/euler/sparse_True"][1]["newton"])
    assert wrapped > 64, wrapped  # (the ring of 64 records wraps)
    case("tnl/lu_inductors", transient_nl(circuit_of(lu_rows, True), tn.lu_transient_case(True), "trapezoidal"))
    case("tnl/multigrid", transient_nl(circuit_of(mg_rows, True), tn.mg_transient_case()))
    for size in (4, 12):
        for reuse in ("1", "0"):
            os.environ["NODAL_TNL_REUSE"] = reuse
            case(f"tnl/clamps/{size}/reuse_{reuse}", transient_nl(circuit_of(tn.reuse_case(size)[0], True), tn.reuse_case(size)))
            os.environ.pop("NODAL_TNL_REUSE")
            updates, newton = (cases[f"tnl/clamps/{size}/reuse_{reuse}"][1][k] for k in ("updates", "newton"))
            assert updates == (newton if reuse == "0" else [1] + [0] * (len(newton) - 1)), (updates, newton)
    lu_case = tn.lu_transient_case(False)
    circ = circuit_of(lu_rows, True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x0 = circ.operating_point(lu_diodes, **nr.TIGHT).x
    case("tnl/no_steps", transient_nl(circ, lu_case, initial=x0, steps=0, envelope=False))
    case("tnl/max_iter_1", transient_nl(circ, lu_case, initial=x0, max_iter=1, envelope=False))
    island = nr.grid_rows(9, [("a1", 0.5, 1)], extra=[["ri", "R", "1", "isl1", "isl2"], ["ai", "A", "0", "isl1", "isl2"]])
    circ = circuit_of(island, True)
    case("tnl/island", transient_nl(circ, (island, [("c1", 1.0, "1", "g")], [], [("d1", I_SAT, N_VT, "1", "g")], 0.05, 3, {}),
                                    initial=np.zeros(circ.table.n), envelope=False))
    circ = circuit_of(lu_rows, True)
    case("tnl/overflow", transient_nl(circ, lu_case, initial=hot, steps=2, envelope=False))
    case("tnl/overflow/then", solve_on(circ._transient_child[1]))

    # ---- nodal_newton_gradient ----
    for sparse in (False, True):
        case(f"grad/closed_form/sparse_{sparse}", newton_gradient(circuit_of(nr.source_diode_rows(1.0), sparse), d_one, gmin=0.0))
        case(f"grad/transposed/sparse_{sparse}", newton_gradient(circuit_of(series, sparse), d_series))
        circ = circuit_of(hanging, sparse)
        x = np.zeros(2)
        x[circ.netlist.nodenum["1"]], x[circ.netlist.nodenum["2"]] = 1.0, -29.0
        case(f"grad/singular/sparse_{sparse}", newton_gradient(circ, d_hanging, x=x, gmin=0.0))
        circ = circuit_of(one, sparse)
        case(f"grad/overflow/sparse_{sparse}", newton_gradient(circ, d_one, x=np.array([100.0])))
        case(f"grad/overflow/sparse_{sparse}/then", newton_gradient(circ, d_one))
    circ = circuit_of(lu_rows, True)
    case("grad/lu", newton_gradient(circ, lu_diodes))
    case("grad/lu/no_diodes", newton_gradient(circ, []))
    case("grad/multigrid", newton_gradient(circuit_of(mg_rows, True), mg_diodes))

    digests, values = {}, {}
    for name, (arrays, vals) in cases.items():
        for k, a in enumerate(arrays):
            a = np.ascontiguousarray(np.zeros(0) if a is None else a)
            digests[f"{name}/{k}:{a.dtype}{list(a.shape)}"] = hashlib.sha256(a.tobytes()).hexdigest()
        values[name] = vals
    return {"digests": digests, "values": values}


def compare(a_path, b_path):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    differ = [key for part in ("digests", "values") for key in sorted(set(a[part]) | set(b[part]))
              if a[part].get(key) != b[part].get(key)]
    print(f"{len(a['digests'])} digests, {len(a['values'])} value records:", "all equal" if not differ else f"{len(differ)} differ")
    for key in differ:
        print("  differs:", key)
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="newton_family_digest.json")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the tree whose nodal_amd package, library and tests/ networks are measured")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path.insert(0, os.path.abspath(args.root))
    import nodal_amd
    print("measuring", os.path.dirname(os.path.abspath(nodal_amd.__file__)), flush=True)
    record = {"tool": "tools/newton_family_digest.py", **measure()}
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out, len(record["digests"]), "digests")


if __name__ == "__main__":
    main()
