"""The operating-point reference (tests/newton_reference.py) against closed forms and against itself, the parity check
of tests/test_gpu_operating_point.py against planted defects, and the parts of Circuit.operating_point that need no
device: argument errors and the companion table.  No GPU."""
import numpy as np
import pytest

import nodal_amd as n
from nodal_amd.lowering import lower
from tests import newton_reference as nr
from tests.newton_reference import I_SAT, N_VT, TIGHT, TOL, NewtonReference

MAX_ITER = 100  # Circuit.operating_point's default, which the GPU tests run with


def parity_errors(ref, X, VH, x0):
    """The one-step parity of the GPU tests: the reference advances somebody's (x_k, vh_k) by one step and is compared
    with that somebody's x_{k+1}, vh_{k+1}.  Returns (worst x error / |x_{k+1}|_inf, worst vh error / max(|x_{k+1}|_inf,
    |vh_{k+1}|_inf), comparisons left out, comparisons, per iterate (not converged, limited, left out) of the reference): a diode whose raw v lies within 4 TOL |x|_inf
    of a limiter threshold is left out of the vh comparison and of the counts."""
    ex = ev = 0.0
    left = total = 0
    counts = []
    x_k = x0
    for k in range(len(X)):
        x, vh, flags = ref.one_step(x_k, VH[k])
        xs = np.abs(X[k]).max()
        ex = max(ex, np.abs(x - X[k]).max() / xs)
        decidable = flags["margin"] > 4 * TOL * xs
        left += int((~decidable).sum())
        total += len(decidable)
        if decidable.any():
            scale = max(xs, np.abs(VH[k + 1]).max())
            ev = max(ev, np.abs(vh - VH[k + 1])[decidable].max() / scale)
        counts.append((int(flags["not_converged"].sum()), int(flags["limited"].sum()), int((~decidable).sum())))
        x_k = X[k]
    return ex, ev, left, total, counts


CASES = {"lu": nr.lu_case, "mg": nr.mg_case}


@pytest.fixture(scope="module")
def runs():
    """every input of the GPU tests, run once with both solves"""
    out = {}
    for name, case in CASES.items():
        made = case()
        rows, diodes = made[0], made[1]
        starts = {"cold": None}
        if len(made) > 2:
            starts["hard"] = made[2]
        for label, x0 in starts.items():
            ref = NewtonReference(rows, diodes, max_iter=MAX_ITER, **TIGHT)
            out[name, label] = (ref, x0, ref.run(x0, both=True))
    return out


@pytest.mark.parametrize("amps", [1e-9, 1e-6, 1e-3, 1.0])
def test_the_reference_meets_the_closed_form_of_a_source_into_a_diode(amps):
    ref = NewtonReference(nr.source_diode_rows(amps), [("d1", I_SAT, N_VT, "1", "g")], gmin=0.0, **TIGHT)
    r = ref.run(both=True)
    v = nr.source_diode_closed_form(amps, I_SAT, N_VT)
    print(f"I = {amps:g}: {r['iterations']} iterations, v = {r['x'][0]!r}, closed form {v!r}")
    assert r["converged"] and abs(r["x"][0] - v) <= 1e-13 * abs(v)
    assert ref.worst_disagreement <= TOL / 1000


def test_the_reference_meets_the_series_circuit():
    ref = NewtonReference(nr.series_rows(5.0, 1000.0), [("d1", I_SAT, N_VT, "2", "g")], gmin=0.0, **TIGHT)
    r = ref.run(both=True)
    v = nr.series_closed_form(5.0, 1000.0, I_SAT, N_VT)
    assert r["converged"] and abs(r["x"][1] - v) <= 1e-13 * abs(v)
    assert abs(r["x"][2] - (5.0 - v) / 1000.0) <= 1e-13 * 5e-3  # (the branch unknown: the current the source delivers)


@pytest.mark.parametrize("key", [("lu", "cold"), ("lu", "hard"), ("mg", "cold")])
def test_the_reference_converges_on_the_inputs_of_the_gpu_tests(runs, key):
    ref, x0, r = runs[key]
    print(f"{key}: {r['iterations']} iterations, limited {r['limited']}, not converged {r['not_converged']}, "
          f"two solves disagree by {ref.worst_disagreement:.2e}, nearest threshold {r['margins'].min():.2e}")
    assert r["converged"] and r["iterations"] <= MAX_ITER // 2
    assert ref.worst_disagreement <= TOL / 1000
    # no raw voltage of any iterate lies in the band where the limiter's branch is undecidable
    assert (r["margins"] > 4 * TOL * np.abs(r["iterates"]).max(axis=1)[:, None]).all()
    res, scale = ref.residual(r["x"])
    assert np.abs(res).max() / scale.max() <= nr.RESID_BAR + TIGHT["reltol"] + TIGHT["abstol"] / scale.max()
    if key[1] == "hard":
        assert sum(r["limited"]) > 0  # (limiting acts on the start above v_crit)


def test_a_diode_between_a_node_and_itself_carries_nothing(runs):
    ref, _, r = runs["lu", "cold"]
    d = ref.names.index("d_same")
    assert (r["vh"][:, d] == 0.0).all() and ref.current(ref.voltages(r["x"]))[d] == 0.0


@pytest.mark.parametrize("key", [("lu", "cold"), ("lu", "hard"), ("mg", "cold")])
def test_the_parity_check_passes_on_the_reference_itself(runs, key):
    ref, x0, r = runs[key]
    start = np.zeros(ref.n) if x0 is None else x0
    ex, ev, left, total, counts = parity_errors(ref, r["iterates"], r["vh"], start)
    assert ex <= 2 * TOL and ev <= 2 * TOL and left == 0
    assert [c[0] for c in counts] == r["not_converged"] and [c[1] for c in counts] == r["limited"]


@pytest.mark.parametrize("defect", ["J_sign", "no_limiting", "g_without_gmin"])
def test_the_parity_check_bites_on_planted_defects(runs, defect):
    """a copy of the reference's own output with one step redone wrongly: the check must see it"""
    ref, x0, r = runs["lu", "hard"]
    if defect == "g_without_gmin":  # (gmin = 1e-12 S is below TOL beside the grid's 1 S: a case where it carries the current)
        ref = NewtonReference(nr.source_diode_rows(1e-12), [("d1", 1e-16, N_VT, "g", "1")], gmin=1e-9, **TIGHT)
        x0, r = None, ref.run()
    X, VH = r["iterates"].copy(), r["vh"].copy()
    k = 0
    x, vh, _ = ref.one_step(None, VH[k], defect=defect)
    X[k], VH[k + 1] = x, vh
    start = np.zeros(ref.n) if x0 is None else x0
    ex, ev, left, total, counts = parity_errors(ref, X[:k + 1], VH[:k + 2], start)
    print(f"{defect}: x error {ex:.2e}, vh error {ev:.2e}")
    assert ex > 2 * TOL or ev > 2 * TOL


# ---- the front end, without a device --------------------------------------------------------------------------------
def _netlist():
    return n.Netlist.from_rows([["a1", "A", "1", "1", "g"], ["r1", "R", "2", "1", "2"], ["r2", "R", "3", "2", "g"]])


def test_resolve_diodes_and_its_errors():
    from nodal_amd.operating_point import resolve_diodes
    nl = _netlist()
    names, i_sat, n_vt, ia, ib = resolve_diodes(nl, [("d1", 1e-14, 0.026, "1", "g"), ("d2", 2e-14, 0.03, "2", "1")])
    assert names == ["d1", "d2"] and i_sat.tolist() == [1e-14, 2e-14] and n_vt.tolist() == [0.026, 0.03]
    assert ia.tolist() == [nl.nodenum["1"], nl.nodenum["2"]] and ib.tolist() == [-1, nl.nodenum["1"]]
    assert ia.dtype == np.int32 and resolve_diodes(nl, [])[1].shape == (0,)
    for bad in ([("d1", 1e-14, 0.026, "9", "g")], [("d1", 1e-14, 0.026, "1", "nowhere")],
                [("d1", 1e-14, 0.026, "1", "g"), ("d1", 1e-14, 0.026, "2", "g")], [("r1", 1e-14, 0.026, "1", "g")],
                [("d1", 0.0, 0.026, "1", "g")], [("d1", -1e-14, 0.026, "1", "g")], [("d1", 1e-14, 0.0, "1", "g")],
                [("d1", 1e-14, float("inf"), "1", "g")], [("d1", float("nan"), 0.026, "1", "g")], [("d1", 1e-14, "1", "g")]):
        with pytest.raises(ValueError):
            resolve_diodes(nl, bad)


def test_check_operating_point_arguments():
    from nodal_amd.operating_point import check_operating_point_arguments as check
    assert check(100, 1e-3, 1e-6, 1e-12, 1e-12, None, 3) == (100, 1e-3, 1e-6, 1e-12, 1e-12, None)
    x0 = check(1, 0.0, 0.0, 0.0, 0.0, [1, 2, 3], 3)[-1]
    assert x0.dtype == np.float64 and x0.tolist() == [1.0, 2.0, 3.0]
    for kwargs in (dict(max_iter=0), dict(max_iter=1.5), dict(reltol=-1e-3), dict(vntol=-1.0), dict(abstol=-1e-12),
                   dict(gmin=-1e-12), dict(gmin=float("nan")), dict(reltol=float("inf")), dict(initial=[1.0, 2.0]),
                   dict(initial=[1.0, float("nan"), 0.0]), dict(initial=[[1.0, 2.0, 3.0]]),
                   dict(initial=[1.0, float("inf"), 0.0])):
        args = dict(max_iter=100, reltol=1e-3, vntol=1e-6, abstol=1e-12, gmin=1e-12, initial=None)
        args.update(kwargs)
        with pytest.raises(ValueError):
            check(n=3, **args)


def test_companion_table_rows_and_values():
    from nodal_amd.operating_point import companion_table, resolve_diodes
    nl = _netlist()
    table = lower(nl)
    _, i_sat, n_vt, ia, ib = resolve_diodes(nl, [("d1", 1e-14, 0.026, "1", "g"), ("d2", 2e-14, 0.03, "2", "1"),
                                                 ("d3", 1e-14, 0.026, "2", "2")])
    out, rows = companion_table(table, i_sat, n_vt, ia, ib, gmin=1e-12)
    assert rows.tolist() == [3, 4, 5] and rows.dtype == np.int64
    assert out.ncomp == 6 and out.K == table.K and out.B == table.B
    for name in ("type", "value", "a", "b"):  # the netlist's rows keep their places
        assert np.array_equal(getattr(out, name)[:3], getattr(table, name))
    assert out.type[3:].tolist() == [0, 0, 0]  # R
    assert np.array_equal(out.value[3:], 1.0 / (i_sat / n_vt + 1e-12))  # the linearisation at v = 0
    assert out.a[3:].tolist() == [nl.nodenum["1"], nl.nodenum["2"], -1]  # both leads on a node: ground to ground
    assert out.b[3:].tolist() == [-1, nl.nodenum["1"], -1]
    assert ia.tolist()[2] == ib.tolist()[2] == nl.nodenum["2"]  # (the caller's arrays are not written to)


def test_operating_point_is_a_plain_container():
    from nodal_amd.operating_point import NewtonHistory, OperatingPoint
    hist = NewtonHistory([[2, 1, 0.5, 1e-16], [0, 0, 1e-14, 2e-16]], [0, 0], [1, 1], [1, 3])
    assert hist.not_converged.tolist() == [2, 0] and hist.limited.tolist() == [1, 0] and hist.route == ["lu", "direct"]
    op = OperatingPoint(np.zeros(2), ["d1"], np.zeros(1), np.zeros(1), np.ones(1), True, 2, hist)
    assert op.scaled_residual == 2e-16 and op.converged and len(op.history) == 2
    with pytest.raises(ValueError):
        op.linearised()
