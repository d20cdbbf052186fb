"""tests/transient_bjt_reference.py held to a closed form, to itself (two linear solves per Newton step), to convergence on
every input of tests/test_gpu_transient_transistors.py within the max_iter that file passes, and to planted defects that
its checks must catch; and what Circuit.transient(transistors=...) does before any device call: the companion table's row
order, the GM rows' control leads, the probe check.  No device."""
import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import constants as c
from nodal_amd import operating_point as op
from nodal_amd import transient as tm
from nodal_amd.lowering import lower
from tests import transient_bjt_reference as tb
from tests.transient_bjt_reference import I_SAT, N_VT, TIGHT, TOL, TransientTransistorReference, npn, pnp

MAX_ITER = 50  # what the GPU tests pass
MOST = 18      # Newton iterations per step that the cases were found to need at most


def test_the_reference_meets_the_closed_form_of_a_diode_connected_transistor():
    C, h, steps = 1e-3, 1e-4, 5
    ref = TransientTransistorReference(tb.tn.rc_diode_rows(), [("c1", C, "1", "g")], [], [], [npn("q1", 1, 1, "g")], h,
                                       "euler", gmin=0.0, max_iter=MAX_ITER, **TIGHT)
    A = ref.rhs_steps({}, steps)
    X, _, its = ref.run(np.array([0.7]), np.zeros(0), A, both=True)
    v = tb.diode_connected_closed_form(0.7, C, h, steps)
    print("closed form", v, "reference", X[:, 0], "iterations", its, "worst error", np.abs(X[:, 0] - v).max())
    assert ref.unconverged == 0 and (np.abs(X[:, 0] - v) <= 2 * TOL / 1000 * np.abs(v)).all()
    assert ref.newton.worst_disagreement <= TOL / 1000
    assert ref.parity(X, np.zeros(0), A)[0] <= 0.0 and ref.residual_excess(X, np.zeros(0), A)[0] <= 0.0
    assert (ref.junction_voltages(X[-1])[:, 1] == 0.0).all()  # (collector and base on one node)


def reference_of(name, method):
    rows, caps, inds, diodes, transistors, dt, steps, sources = tb.CASES[name]()
    ref = TransientTransistorReference(rows, caps, inds, diodes, transistors, dt, method, max_iter=MAX_ITER, **TIGHT)
    x0, i0, dc_its = ref.dc_start()
    return ref, x0, i0, dc_its, ref.rhs_steps(sources, steps)


@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
@pytest.mark.parametrize("name", list(tb.CASES))
def test_every_case_converges_and_passes_the_reference_s_own_checks(name, method):
    ref, x0, i0, dc_its, A = reference_of(name, method)
    both = ref.n <= 64
    X, I, its = ref.run(x0, i0, A, both=both)
    print(f"{name} {method}: n {ref.n}, DC start {dc_its} iterations, steps {its.tolist()}, highest junction "
          f"{ref.highest_junction:.3f} V, two solves disagree by {ref.newton.worst_disagreement:.2e}")
    assert ref.n == tb.SIZES[name]
    assert dc_its <= MAX_ITER and ref.unconverged == 0 and (its <= MOST).all()
    if both:
        assert ref.newton.worst_disagreement <= TOL / 1000
    excess, rel, _, _ = ref.parity(X, i0, A)
    rexcess, worst = ref.residual_excess(X, i0, A)
    print(f"{name} {method}: the reference against its own checks: parity {rel:.2e}, residual {worst:.2e}")
    assert excess <= 0.0 and rexcess <= 0.0
    # Kirchhoff at every transistor, at every step
    for x in X:
        ic, ib, ie = ref.terminal_currents(x)
        assert (np.abs(ic + ib + ie) <= 4 * np.finfo(float).eps * (np.abs(ic) + np.abs(ib) + np.abs(ie))).all()
    if name.endswith("inverter") or name.endswith("inverter_l"):
        out = X[:, tb.nr._index(ref.newton.nl, "3" if name == "inverter" else "qc")]
        vr = np.array([ref.junction_voltages(x)[-1, 1] for x in X])
        print(f"{name} {method}: output from {out[0]:.3f} down to {out.min():.3f} and back to {out[-1]:.3f} V, the reverse "
              f"junction up to {vr.max():.3f} V")
        assert out[0] > 4.5 and out.min() < 0.2 and out[-1] > 4.5 and vr.max() > 0.5  # (it saturates and recovers)


@pytest.fixture(scope="module", params=["inverter", "lu_inverter"])
def planted(request):
    ref, x0, i0, _, A = reference_of(request.param, "euler")
    return request.param, ref, x0, i0, A


@pytest.mark.parametrize("defect", tb.DEFECTS)
def test_a_planted_defect_loses_the_run_or_exceeds_the_parity_bar(planted, defect):
    name, ref, x0, i0, A = planted
    ref.unconverged = 0
    try:
        with np.errstate(all="ignore"):
            X, _, its = ref.run(x0, i0, A, defect=defect)
    except RuntimeError as exc:  # (SuperLU: the factor is exactly singular)
        print(f"{name} {defect}: lost, {exc}")
        return
    lost, ref.unconverged = ref.unconverged, 0
    if not np.isfinite(X).all():
        print(f"{name} {defect}: lost, the states are not finite")
        return
    # a step that does not converge in max_iter is info 2 on the device, and the GPU tests hold every step to info 0; the
    # states it leaves are held to the parity bar all the same, unless the clean step from one of them cannot be solved
    try:
        with np.errstate(all="ignore"):
            excess, rel, _, _ = ref.parity(X, i0, A)
    except RuntimeError as exc:
        print(f"{name} {defect}: iterations {its.tolist()}, {lost} steps did not converge; the clean step from its states: {exc}")
        assert lost > 0
        return
    finally:
        ref.unconverged = 0
    print(f"{name} {defect}: iterations {its.tolist()}, {lost} steps did not converge, parity error {rel:.2e}")
    assert excess > 0.0


# ---- what Circuit.transient(transistors=...) does before any device call -------------------------------------------------
def small_netlist():
    return n.Netlist.from_rows([["e1", "E", "5", "1", "g"], ["r1", "R", "1000", "1", "2"], ["r2", "R", "1000", "2", "3"]])


def test_the_companion_table_holds_capacitors_inductors_diodes_junctions_then_the_gm_rows():
    nl = small_netlist()
    table = lower(nl)
    first = table.ncomp
    diodes = [("d1", I_SAT, N_VT, "3", "g")]
    transistors = [npn("q1", 3, 2, "g"), pnp("q2", "g", 2, 3), npn("q3", 1, 1, 1)]
    tnames, sign, junctions, ta, tbb, junction, i_s = op.resolve_transistors(nl, transistors, first=len(diodes))
    names, i_sat, n_vt, da, db = op.resolve_diodes(nl, diodes + junctions)
    _, farads, ca, cb = tm.resolve_capacitors(nl, [("c1", 1e-6, "2", "g"), ("c2", 2e-6, "2", "3")])
    _, henries, la, lb = tm.resolve_inductors(nl, [("l1", 1e-3, "3", "g")])
    out, cap_rows, ind_rows, diode_rows, gm_rows = tm.bjt_companion_table(
        table, farads, ca, cb, 1e-6, tm.METHODS["euler"], henries, la, lb, i_sat, n_vt, da, db, ta, tbb, junction, i_s, 1e-12)
    D, T = len(names), len(transistors)
    assert D == 1 + 2 * T and junction.tolist() == [[1, 2], [3, 4], [5, 6]]
    assert cap_rows.tolist() == [first, first + 1] and ind_rows.tolist() == [first + 2]
    assert diode_rows.tolist() == list(range(first + 3, first + 3 + D))
    assert gm_rows.tolist() == [[first + 3 + D + 2 * t, first + 3 + D + 2 * t + 1] for t in range(T)]
    assert out.ncomp == first + 3 + D + 2 * T
    kind, value = np.array(out.type), np.array(out.value)
    a, b, cc, dd = (np.array(getattr(out, k)) for k in "abcd")
    assert (kind[first:first + 3 + D] == c.TYPE_CODE["R"]).all() and (kind[gm_rows.ravel()] == c.T_GM).all()
    assert np.array_equal(value[cap_rows], 1e-6 / farads) and np.array_equal(value[ind_rows], henries / 1e-6)
    # the original rows keep their places and values
    for k in ("type", "value", "a", "b"):
        assert np.array_equal(np.array(getattr(out, k))[:first], np.array(getattr(table, k)))
    # a GM row: the transport's leads as a, b; the (grounded-where-same) leads of its junction's row as c, d
    for t in range(T):
        for q in range(2):
            r, rj = gm_rows[t, q], diode_rows[junction[t, q]]
            same = ta[t] == tbb[t]
            assert (a[r], b[r]) == ((-1, -1) if same else (ta[t], tbb[t]))
            assert (cc[r], dd[r]) == (a[rj], b[rj])
            assert value[r] == (i_s[t] / N_VT if q == 0 else -i_s[t] / N_VT)
    # q3, every lead on one node: rows between ground and ground, control leads ground and ground
    assert (a[gm_rows[2]] == -1).all() and (b[gm_rows[2]] == -1).all() and (cc[gm_rows[2]] == -1).all()
    assert sign.tolist() == [1.0, -1.0, 1.0]
    # the PNP: i_T enters at the emitter
    assert (ta[1], tbb[1]) == (nl.nodenum["3"], -1)


def test_the_transistor_probes_are_checked():
    assert tm.check_transistor_probes(["q1", "q2"], ["q2", "q1"]).tolist() == [1, 0]
    assert tm.check_transistor_probes(["q1"], ()).shape == (0,) and tm.check_transistor_probes((), ()).dtype == np.int32
    with pytest.raises(ValueError, match="not the name of a transistor"):
        tm.check_transistor_probes(["q1"], ["q9"])
    with pytest.raises(ValueError, match="given twice"):
        tm.check_transistor_probes(["q1", "q2"], ["q1", "q1"])
    with pytest.raises(ValueError, match="not the name of a transistor"):
        tm.check_transistor_probes((), ["q1"])


def test_a_transient_without_transistors_carries_empty_transistor_fields():
    tr = tm.Transient(np.arange(4.0), np.zeros((4, 1)), ["1"], np.zeros(3, dtype=np.int32), np.zeros(3), np.zeros(3))
    assert tr.transistor_probes == [] and tr.junction_voltages.shape == (4, 0, 2)
    for field in (tr.collector_currents, tr.base_currents, tr.emitter_currents):
        assert field.shape == (4, 0)
