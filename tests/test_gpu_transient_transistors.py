"""Circuit.transient(transistors=...) (nodal_transient_nl_bjt) on the device against the fp64 reference of
tests/transient_bjt_reference.py: a closed form, an inverter that saturates and a push-pull stage with a PNP, a diode and
an inductor on the dense-panel route; a grid with an E source, thirteen diodes and five or six transistors (and
inductors) on the sparse LU route; both methods.  Step parity from the device's own DC start, the nonlinear residual of
every step, the transistors' probes at every step, the rule that a run with transistors assembles in every iteration, what
stays bit for bit without transistors, repeat calls, the failure paths and what the entry refuses.

The bars are test_gpu_transient_diodes.py's: (2 TOL + reltol) max |x_k| + vntol = 2.1e-9 max |x_k| for step parity,
RESID_BAR + reltol + abstol / scale = 1.0e-10 for the nonlinear residual, RESID_BAR = 1e-12 for a linear solve, 2 TOL |v|
for the closed form, 2 TOL max |x_k| for a junction voltage and 2 TOL (|reference| + i_s) for a terminal current.
Measured on an MI355X (parity: the worst |x_k - reference| over max |x_k|; residual: the worst nonlinear defect over its
scale; currents: the worst terminal-current error over |reference| + i_s), both values of `sparse` alike:
    closed form    error 3.3e-16 V against 2 TOL |v| = 1.4e-9 V, three Newton iterations a step
    inverter       parity 2.3e-16 (trapezoidal 5.3e-16), residual 4.0e-18, currents 3.4e-16, up to 18 iterations a step
    pushpull       parity 4.7e-15 (trapezoidal 3.1e-15), residual 1.8e-16, currents 2.2e-16
    lu_bjt         parity 2.5e-15 (trapezoidal 4.9e-15), residual 2.9e-16, currents 3.5e-16; with inductors 2.4e-15
                   (4.8e-15), 1.0e-16, 2.7e-16
    lu_inverter    parity 1.5e-15 (trapezoidal 2.9e-15), residual 2.9e-16, currents 3.5e-16; with inductors 1.5e-15
                   (2.9e-15), 1.0e-16, 2.7e-16
    junction voltages: the bits of the reference's S^T x_k; I_C + I_B + I_E at most 2.2e-16 of the largest of the three
    reuse_case(12): matrix updates [1, 0, 0, 0, 0, 0] without transistors, [1, 2, 2, 2, 2, 2] = the iterations with one
Each test prints its own figures before it asserts."""
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd import operating_point as opm
from tests import transient_bjt_reference as tb
from tests import transient_nl_reference as tn
from tests.transient_bjt_reference import I_SAT, N_VT, RESID_BAR, TIGHT, TOL, TransientTransistorReference, npn

pytestmark = pytest.mark.gpu
MAX_ITER = 50
SPICE = dict(reltol=1e-3, vntol=1e-6, abstol=1e-12)  # for the entry's own tests, which start from an arbitrary state


def circuit_of(rows, sparse):
    return n.Circuit(n.Netlist.from_rows([list(r) for r in rows]), sparse=sparse, device=0)


def node_labels(circ):
    return sorted(circ.netlist.nodenum, key=circ.netlist.nodenum.get)


@pytest.fixture(scope="module")
def references():
    """reference(name, method): the reference of a case with its DC start, made once"""
    made = {}

    def reference(name, method):
        if (name, method) not in made:
            rows, caps, inds, diodes, transistors, dt, steps, sources = tb.CASES[name]()
            ref = TransientTransistorReference(rows, caps, inds, diodes, transistors, dt, method, max_iter=MAX_ITER, **TIGHT)
            made[name, method] = (ref, ref.dc_start(), ref.rhs_steps(sources, steps))
        return made[name, method]
    return reference


def transient_of(circ, case, method, **more):
    rows, caps, inds, diodes, transistors, dt, steps, sources = case
    kw = dict(sources=sources, probes=node_labels(circ), method=method, inductors=inds, current_probes=[i[0] for i in inds],
              diodes=diodes, diode_probes=[d[0] for d in diodes], transistors=transistors,
              transistor_probes=[t[0] for t in transistors], keep_every=1, max_iter=MAX_ITER, **TIGHT)
    kw.update(more)
    return circ.transient(caps, dt, steps, **kw)


def check_transistor_outputs(ref, tr, X, label):
    """the probes at every step against the reference's formulas at the device's own x_k"""
    nw = ref.newton
    T, D0 = nw.T, nw.D0
    assert tr.transistor_probes == nw.transistor_names and tr.junction_voltages.shape == (len(X), T, 2)
    worst_v = worst_i = worst_sum = 0.0
    for k in range(len(X)):
        xs = np.abs(X[k]).max()
        vj = ref.junction_voltages(X[k])
        worst_v = max(worst_v, np.abs(tr.junction_voltages[k] - vj).max() / xs)
        assert np.abs(tr.junction_voltages[k] - vj).max() <= 2 * TOL * xs
        theirs = ref.terminal_currents(X[k])
        mine = (tr.collector_currents[k], tr.base_currents[k], tr.emitter_currents[k])
        for a, b in zip(mine, theirs):
            assert a.shape == (T,)
            worst_i = max(worst_i, (np.abs(a - b) / (np.abs(b) + nw.i_s)).max())
            assert (np.abs(a - b) <= 2 * TOL * (np.abs(b) + nw.i_s)).all()
        largest = np.max(np.abs(theirs), axis=0)
        worst_sum = max(worst_sum, (np.abs(mine[0] + mine[1] + mine[2]) / (largest + nw.i_s)).max())
        assert (np.abs(mine[0] + mine[1] + mine[2]) <= 2 * TOL * (largest + nw.i_s)).all()
    print(f"{label}: junction voltages off by {worst_v:.2e} of max |x_k|, terminal currents by {worst_i:.2e} of |reference| + "
          f"i_s, I_C + I_B + I_E by {worst_sum:.2e}")
    # the caller's diodes stay the caller's; the junctions stand behind them in final_junctions
    assert tr.diode_voltages.shape == (len(X), D0) and tr.final_junctions.shape == (D0 + 2 * T,)
    assert np.abs(tr.final_junctions - nw.voltages(X[-1])).max() <= (2 * TOL + ref.reltol) * np.abs(X[-1]).max() + ref.vntol


def run_and_check(references, name, method, sparse):
    """one run from the device's own nonlinear DC start with every check of the file; returns (circuit, Transient, ref, X)"""
    case = tb.CASES[name]()
    rows, caps, inds, diodes, transistors, dt, steps, sources = case
    label = f"{name} {method}, sparse {sparse}"
    ref, (x0_ref, i0_ref, _), A = references(name, method)
    circ = circuit_of(rows, sparse)
    assert circ._handle.n == tb.SIZES[name]
    table = {col: np.array(getattr(circ.table, col)) for col in ("type", "value", "a", "b")}
    tr = transient_of(circ, case, method)
    print(f"{label}: Newton iterations {tr.newton_iterations.tolist()}, matrix updates {tr.matrix_updates.tolist()}, solver "
          f"iterations {tr.iterations.tolist()}, worst scaled residual {tr.scaled_residual.max():.2e}, timings {tr.timings}")
    assert (tr.info == 0).all() and (tr.scaled_residual <= RESID_BAR).all()
    assert (tr.newton_iterations >= 1).all() and np.array_equal(tr.matrix_updates, tr.newton_iterations)
    # the start against the reference's DC start
    K = circ.table.K
    x0 = np.zeros(ref.n)
    x0[:K] = tr.waveforms[0]
    top = np.abs(x0_ref).max()
    assert np.abs(x0[:K] - x0_ref[:K]).max() <= (2 * TOL + ref.reltol) * top + ref.vntol
    i0 = tr.currents[0]
    assert np.abs(i0 - i0_ref).max(initial=0.0) <= (2 * TOL + ref.reltol) * max(top, np.abs(i0_ref).max(initial=0.0)) + ref.vntol
    # (the branch unknowns of x_0 enter nothing: the histories read potentials, the probes too)
    X = np.vstack([x0[None, :], tr.solutions])
    assert np.array_equal(tr.waveforms[1:], tr.solutions[:, :K])
    excess, rel, its, I = ref.parity(X, i0, A)
    rexcess, worst = ref.residual_excess(X, i0, A)
    print(f"{label}: parity {rel:.2e} of max |x_k| (the reference's iterations {its}), nonlinear residual {worst:.2e} of its scale")
    assert excess <= 0.0
    assert rexcess <= 0.0
    if len(inds):  # the inductor currents against those rebuilt from the device's solutions
        assert np.abs(tr.currents - I).max() <= 2 * TOL * max(np.abs(I).max(), np.abs(X).max())
        assert np.array_equal(tr.final_currents, tr.currents[-1])
    nw = ref.newton
    for k in range(steps + 1):  # the caller's diodes, as test_gpu_transient_diodes.py holds them
        v = nw.voltages(X[k])[:nw.D0]
        i = nw.current(nw.voltages(X[k]))[:nw.D0]
        assert np.abs(tr.diode_voltages[k] - v).max(initial=0.0) <= 2 * TOL * np.abs(X[k]).max()
        assert (np.abs(tr.diode_currents[k] - i) <= 2 * TOL * (np.abs(i) + nw.i_sat[:nw.D0] + nw.gmin * np.abs(v))).all()
    check_transistor_outputs(ref, tr, X, label)
    for col, column in table.items():  # the circuit itself is left as it was
        assert np.array_equal(np.array(getattr(circ.table, col)), column)
    return circ, tr, ref, X


# ---- 1. closed form: a capacitor discharging into a diode-connected transistor ------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_a_capacitor_discharging_into_a_diode_connected_transistor_meets_the_closed_form(sparse):
    C, h, steps = 1e-3, 1e-4, 5
    circ = circuit_of(tn.rc_diode_rows(), sparse)
    tr = circ.transient([("c1", C, "1", "g")], h, steps, probes=["1"], initial=np.array([0.7]),
                        transistors=[npn("q1", 1, 1, "g")], transistor_probes=["q1"], gmin=0.0, max_iter=MAX_ITER, **TIGHT)
    v = tb.diode_connected_closed_form(0.7, C, h, steps)
    print(f"sparse {sparse}: v {tr.waveforms[:, 0].tolist()}, closed form {v.tolist()}, Newton iterations "
          f"{tr.newton_iterations.tolist()}, worst error {np.abs(tr.waveforms[:, 0] - v).max():.2e}")
    assert (tr.info == 0).all() and (tr.iterations == 0).all()  # (the dense panel)
    assert (np.abs(tr.waveforms[:, 0] - v) <= 2 * TOL * np.abs(v)).all()
    assert (tr.scaled_residual <= RESID_BAR).all() and np.array_equal(tr.matrix_updates, tr.newton_iterations)
    assert np.array_equal(tr.junction_voltages[:, 0, 0], tr.waveforms[:, 0])
    assert (tr.junction_voltages[:, 0, 1] == 0.0).all()  # (collector and base on one node: exactly nothing)
    assert tr.final_junctions.shape == (2,) and tr.final_junctions[1] == 0.0 and tr.diode_voltages.shape == (steps + 1, 0)
    # the emitter carries the whole discharge: i_s (1 + 1 / beta_f) (exp(v / n_vt) - 1), out of the terminal
    i = I_SAT * (1.0 + 1.0 / tb.BETA_F) * np.expm1(v / N_VT)
    assert (np.abs(tr.emitter_currents[:, 0] + i) <= 2 * TOL * np.abs(v) / N_VT * (np.abs(i) + I_SAT)).all()


# ---- 2. the dense panel: an inverter that saturates, a push-pull stage with a PNP, a diode and an inductor -----------------
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
def test_the_inverter_saturates_and_recovers(references, method, sparse):
    circ, tr, ref, X = run_and_check(references, "inverter", method, sparse)
    assert (tr.iterations == 0).all()
    out = tr.waveforms[:, circ.netlist.nodenum["3"]]
    print(f"inverter {method}: output {out[0]:.3f} -> {out.min():.3f} -> {out[-1]:.3f} V, reverse junction up to "
          f"{tr.junction_voltages[:, :, 1].max():.3f} V")
    assert out[0] > 4.5 and out.min() < 0.2 and out[-1] > 4.5
    assert tr.junction_voltages[:, :, 1].max() > 0.5  # (saturation: the reverse GM row carries current)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
def test_the_push_pull_stage(references, method, sparse):
    circ, tr, ref, X = run_and_check(references, "pushpull", method, sparse)
    assert (tr.iterations == 0).all() and circ.table.B == 3
    # both halves conduct in turn: the NPN sources its emitter current, the PNP sinks it
    qn, qp = tr.transistor_probes.index("qn"), tr.transistor_probes.index("qp")
    assert tr.emitter_currents[:, qn].min() < -1e-3 and tr.emitter_currents[:, qp].max() > 1e-3


# ---- 3. the sparse LU route ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
@pytest.mark.parametrize("name", ["lu_bjt", "lu_bjt_l", "lu_inverter", "lu_inverter_l"])
def test_the_sparse_lu_route(references, name, method, sparse):
    circ, tr, ref, X = run_and_check(references, name, method, sparse)
    assert (tr.iterations >= 1).all() and circ.table.B == (1 if name.startswith("lu_bjt") else 3)
    q5 = tr.transistor_probes.index("q5")  # every lead on one node: exactly nothing, throughout
    assert (tr.junction_voltages[:, q5] == 0.0).all()
    for field in (tr.collector_currents, tr.base_currents, tr.emitter_currents):
        assert (field[:, q5] == 0.0).all()
    if name.startswith("lu_inverter"):
        out = tr.waveforms[:, circ.netlist.nodenum["qc"]]
        q6 = tr.transistor_probes.index("q6")
        assert out[0] > 4.5 and out.min() < 0.2 and out[-1] > 4.5 and tr.junction_voltages[:, q6, 1].max() > 0.5


# ---- 4. the re-use rule: none with transistors, untouched without ------------------------------------------------------------
def test_clamps_at_rest_without_transistors_still_reuse_the_matrix():
    rows, caps, inds, diodes, dt, steps, sources = tn.reuse_case(12)
    circ = circuit_of(rows, True)
    kw = dict(sources=sources, probes=["1"], diodes=diodes, max_iter=MAX_ITER, **TIGHT)
    tr = circ.transient(caps, dt, steps, transistors=(), **kw)
    print(f"reuse(12) without transistors: Newton iterations {tr.newton_iterations.tolist()}, updates {tr.matrix_updates.tolist()}")
    assert (tr.info == 0).all() and tr.matrix_updates[0] == 1 and (tr.matrix_updates[1:] == 0).all()
    # one transistor at rest on the same network: every iteration assembles
    with_q = circ.transient(caps, dt, steps, transistors=[npn("q1", "vdd", 1, 2)], **kw)
    print(f"reuse(12) with one transistor: Newton iterations {with_q.newton_iterations.tolist()}, updates "
          f"{with_q.matrix_updates.tolist()}")
    assert (with_q.info == 0).all() and np.array_equal(with_q.matrix_updates, with_q.newton_iterations)


# ---- 5. nothing changes without transistors ------------------------------------------------------------------------------------
def fields(tr):
    env = tr.envelope
    return [tr.waveforms, tr.solutions, tr.info, tr.scaled_residual, tr.iterations, tr.currents, tr.final_currents,
            tr.newton_iterations, tr.matrix_updates, tr.diode_voltages, tr.diode_currents, tr.final_junctions,
            tr.junction_voltages, tr.collector_currents, tr.base_currents, tr.emitter_currents] + \
        ([env.potential_min, env.potential_min_step, env.potential_max, env.potential_max_step] if env else [])


def same_bits(one, two):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(fields(one), fields(two)))


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("with_diodes", [False, True])
def test_without_transistors_nothing_changes(with_diodes, sparse):
    rows, caps, inds, diodes, dt, steps, sources = tn.lu_transient_case(True)
    kw = dict(sources=sources, probes=["1", "30"], inductors=inds, current_probes=["l1"], keep_every=2, envelope=True)
    if with_diodes:
        kw.update(diodes=diodes, diode_probes=["d_fwd"], max_iter=MAX_ITER, **TIGHT)
    plain = circuit_of(rows, sparse).transient(caps, dt, steps, **kw)
    empty = circuit_of(rows, sparse).transient(caps, dt, steps, transistors=(), transistor_probes=(), **kw)
    assert (plain.info == 0).all() and same_bits(plain, empty)
    assert empty.junction_voltages.shape == (steps + 1, 0, 2) and empty.transistor_probes == []
    assert len(empty.final_junctions) == (len(diodes) if with_diodes else 0)


def child_of(circ):
    entry = circ._transient_child
    assert len(entry) == 6  # (key, child, capacitor rows, inductor rows, diode rows, GM rows)
    return entry[1:]


def test_the_entry_without_transports_is_nodal_transient_nl():
    case = tb.CASES["lu_bjt_l"]()
    rows, caps, inds, diodes, transistors, dt, steps, sources = case
    circ = circuit_of(rows, True)
    transient_of(circ, case, "euler")
    child, cap_rows, ind_rows, diode_rows, gm_rows = child_of(circ)
    h = child._handle
    D = len(diodes)  # the caller's diodes alone: the junctions' rows keep their last linearisation, the GM rows too
    _, i_sat, n_vt, _, _ = opm.resolve_diodes(circ.netlist, diodes)
    src = np.array([circ.netlist.component_keys.index("a1")], dtype=np.int64)
    values = np.asarray(sources["a1"], dtype=np.float64)[:, None]
    x0, i0 = np.linspace(-0.2, 0.3, h.n), np.array([0.1, -0.2])
    pa, pb, cur = np.array([0, 5], dtype=np.int32), np.array([-1, 3], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    probe = np.array([0, 3], dtype=np.int32)
    common = dict(dense=False, max_iter=MAX_ITER, method=1, keep_every=1, envelope=True, **SPICE)
    a = h.transient_nl(cap_rows, ind_rows, diode_rows[:D], i_sat, n_vt, 1e-12, src, values, x0, i0, pa, pb, cur, probe, **common)
    b = h.transient_nl_bjt(cap_rows, ind_rows, diode_rows[:D], i_sat, n_vt, 1e-12, np.zeros((0, 2), dtype=np.int64),
                           np.zeros((0, 2), dtype=np.int32), np.zeros(0), src, values, x0, i0, pa, pb, cur, probe,
                           np.zeros(0, dtype=np.int32), **common)
    assert (a[4] == 0).all() and a[8]["newton"].max() >= 2
    for q in (0, 1, 3, 4, 5, 6, 7):
        assert np.array_equal(a[q], b[q]), q
    assert all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
    assert all(np.array_equal(a[8][k], b[8][k]) for k in a[8])
    assert b[8]["tv"].shape == (steps + 1, 0, 2) and b[8]["ti"].shape == (steps + 1, 0, 3)


# ---- 6. repeat calls, the children ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_a_second_identical_call_gives_the_same_bits_and_keeps_the_children(sparse):
    case = tb.CASES["lu_inverter_l"]()
    rows, caps = case[0], case[1]
    circ = circuit_of(rows, sparse)
    one = transient_of(circ, case, "trapezoidal", envelope=True)
    kept = circ._transient_child[1], circ._transient_nl_dc[1]
    two = transient_of(circ, case, "trapezoidal", envelope=True)
    assert (one.info == 0).all() and same_bits(one, two)
    assert (circ._transient_child[1], circ._transient_nl_dc[1]) == kept and two.timings[1] == 0.0, two.timings
    # other leads of one transistor: both children are keyed by the transports too
    moved = list(case)
    moved[4] = case[4][:-1] + [npn("q6", "qc", "qb", "1")]
    transient_of(circ, tuple(moved), "trapezoidal")
    assert circ._transient_child[1] is not kept[0] and circ._transient_nl_dc[1] is not kept[1]
    circ.set_values(circ.values)
    assert circ._transient_child is None and circ._transient_nl_dc is None


# ---- 7. the failure paths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_too_few_iterations_give_info_2_and_leave_the_circuit_usable(sparse):
    case = tb.CASES["lu_inverter"]()
    rows, caps, inds, diodes, transistors, dt, steps, sources = case
    circ = circuit_of(rows, sparse)
    x0 = circ.operating_point(diodes, transistors=transistors, max_iter=MAX_ITER, **TIGHT).x  # (a start of its own)
    with pytest.warns(RuntimeWarning, match="did not converge") as caught:
        tr = transient_of(circ, case, "euler", initial=x0, max_iter=1, envelope=True)
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == 1
    first = int(np.argmax(tr.info == 2))
    print(f"sparse {sparse}: max_iter=1: info {tr.info.tolist()}, Newton iterations {tr.newton_iterations.tolist()}")
    assert (tr.info[:first] == 0).all() and (tr.info[first:] == 2).all() and tr.newton_iterations[first] == 1
    assert (tr.newton_iterations[first + 1:] == 0).all() and np.array_equal(tr.matrix_updates, tr.newton_iterations)
    assert np.isfinite(tr.waveforms[:first + 1]).all() and np.isnan(tr.waveforms[first + 1:]).all()
    assert np.isnan(tr.solutions[first:]).all() and np.isnan(tr.final_junctions).all()
    for field in (tr.junction_voltages, tr.collector_currents, tr.base_currents, tr.emitter_currents, tr.diode_voltages):
        assert np.isfinite(field[:first + 1]).all() and np.isnan(field[first + 1:]).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        after = transient_of(circ, case, "euler", initial=x0, envelope=True)
        fresh = transient_of(circuit_of(rows, sparse), case, "euler", initial=x0, envelope=True)
    assert (after.info == 0).all() and same_bits(after, fresh)


def test_a_dc_start_that_does_not_converge_warns_once_and_gives_nan_everywhere():
    case = tb.CASES["lu_inverter_l"]()
    circ = circuit_of(case[0], True)
    with pytest.warns(RuntimeWarning, match="DC start did not converge") as caught:
        tr = transient_of(circ, case, "euler", max_iter=1, envelope=True)
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == 1
    assert (tr.info == 2).all() and (tr.newton_iterations == 0).all() and (tr.matrix_updates == 0).all()
    T, D = len(case[4]), len(case[3])
    assert tr.junction_voltages.shape == (case[6] + 1, T, 2) and tr.final_junctions.shape == (D + 2 * T,)
    for field in (tr.waveforms, tr.solutions, tr.scaled_residual, tr.currents, tr.final_currents, tr.diode_voltages,
                  tr.diode_currents, tr.final_junctions, tr.junction_voltages, tr.collector_currents, tr.base_currents,
                  tr.emitter_currents, tr.envelope.potential_min):
        assert np.isnan(field).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert (transient_of(circ, case, "euler").info == 0).all()


@pytest.mark.parametrize("sparse", [False, True])
def test_a_transconductance_that_overflows_ends_the_step_like_a_diode_s(sparse):
    """i_s = 1e300 with betas of 1e295: the junctions' i_sat is 1e5 A and their g stays finite at 0.7 V, where
    gmf = i_s exp(0.7 / n_vt) / n_vt is not"""
    hot = [("q1", "npn", 1e300, 1e295, 1e295, N_VT, "1", "1", "g")]
    circ = circuit_of(tn.rc_diode_rows(), sparse)
    caps = [("c1", 1e-3, "1", "g")]
    with pytest.warns(RuntimeWarning, match="step 1 did not converge"):
        tr = circ.transient(caps, 1e-4, 2, probes=["1"], initial=np.array([0.7]), transistors=hot, transistor_probes=["q1"],
                            keep_every=1, max_iter=MAX_ITER, **TIGHT)
    assert tr.info.tolist() == [2, 2] and tr.newton_iterations.tolist() == [1, 0] and tr.matrix_updates.tolist() == [1, 0]
    assert np.isnan(tr.waveforms[1:]).all() and np.isnan(tr.solutions).all() and np.isnan(tr.final_junctions).all()
    assert tr.junction_voltages[0, 0].tolist() == [0.7, 0.0] and np.isnan(tr.junction_voltages[1:]).all()
    assert np.isnan(tr.collector_currents[1:]).all()
    # the handle holds a legal matrix again: 1.0 in the junctions' rows, 0.0 in the GM rows
    child, cap_rows, ind_rows, diode_rows, gm_rows = child_of(circ)
    values = np.array(child.table.value)
    values[diode_rows] = 1.0
    values[gm_rows.ravel()] = 0.0
    fresh = n.Circuit._clone_of(circ, child.table.with_values(values))
    x, info = child._handle.solve_sparse()[:2]
    want, info_fresh = fresh._handle.solve_sparse()[:2]
    assert info == 0 and info_fresh == 0 and np.isfinite(want).all() and np.array_equal(x, want)


@pytest.mark.parametrize("sparse", [False, True])
def test_the_circuit_itself_is_untouched_and_the_arguments_are_checked(sparse):
    case = tb.CASES["inverter"]()
    rows, caps, inds, diodes, transistors, dt, steps, sources = case
    circ = circuit_of(rows, sparse)
    before = circ.solve().result.copy()
    values = np.array(circ.table.value)
    kw = dict(sources=sources, transistors=transistors)
    with pytest.raises(ValueError, match="adjoint of a run with transistors"):
        circ.transient(caps, dt, steps, record=True, **kw)
    with pytest.raises(ValueError, match="name of a diode"):
        circ.transient(caps, dt, steps, sources=sources, diodes=[("q1", I_SAT, N_VT, "2", "g")], transistors=transistors)
    with pytest.raises(ValueError, match="not the name of a transistor"):
        circ.transient(caps, dt, steps, transistor_probes=["q9"], **kw)
    with pytest.raises(ValueError, match="given twice"):
        circ.transient(caps, dt, steps, transistor_probes=["q1", "q1"], **kw)
    with pytest.raises(ValueError, match="not the name of a transistor"):
        circ.transient(caps, dt, steps, sources=sources, transistor_probes=["q1"])  # (no transistors at all)
    for bad, match in ((("q1", "npn", 0.0, 100.0, 1.0, N_VT, "3", "2", "g"), "i_s"),
                       (("q1", "fet", I_SAT, 100.0, 1.0, N_VT, "3", "2", "g"), "kind"),
                       (("q1", "npn", I_SAT, 100.0, 1.0, N_VT, "3", "2", "nowhere"), "q1"),
                       (("rb", "npn", I_SAT, 100.0, 1.0, N_VT, "3", "2", "g"), "name of a component"),
                       (("q1", "npn", I_SAT, 100.0, 1.0, N_VT, "3", "2"), "collector, base")):
        with pytest.raises(ValueError, match=match):
            circ.transient(caps, dt, steps, sources=sources, transistors=[bad])
    with pytest.raises(ValueError, match="twice"):
        circ.transient(caps, dt, steps, sources=sources, transistors=transistors + transistors)
    tr = circ.transient(caps, dt, steps, max_iter=MAX_ITER, **kw, **TIGHT)  # (no probes: empty fields)
    assert (tr.info == 0).all() and tr.junction_voltages.shape == (steps + 1, 0, 2) and tr.final_junctions.shape == (2,)
    assert np.array_equal(circ._handle.download_x(), before) and np.array_equal(np.array(circ.table.value), values)
    assert circ.table.ncomp == len(values)


# ---- the entry itself (nodal_transient_nl_bjt) ---------------------------------------------------------------------------------
def test_what_the_entry_refuses():
    case = tb.CASES["lu_inverter_l"]()
    rows, caps, inds, diodes, transistors, dt, steps, sources = case
    circ = circuit_of(rows, True)
    transient_of(circ, case, "euler")
    child, cap_rows, ind_rows, diode_rows, gm_rows = child_of(circ)
    h = child._handle
    D, T = len(diodes), len(transistors)
    _, _, junctions, ta, tbb, junction, i_s = opm.resolve_transistors(circ.netlist, transistors, first=D)
    _, i_sat, n_vt, _, _ = opm.resolve_diodes(circ.netlist, list(diodes) + junctions)
    src = np.array([circ.netlist.component_keys.index("a1")], dtype=np.int64)
    values = np.asarray(sources["a1"], dtype=np.float64)[:, None]
    x0, i0 = np.zeros(h.n), np.zeros(len(inds))
    pa, pb, cur = np.array([0], dtype=np.int32), np.array([-1], dtype=np.int32), np.array([0], dtype=np.int32)

    def call(rows_=diode_rows, sat=i_sat, gm=gm_rows, jn=junction, i_s_=i_s, dprobe=(0,), tprobe=(0,), max_iter=MAX_ITER):
        return h.transient_nl_bjt(cap_rows, ind_rows, rows_, sat, n_vt, 1e-12, gm, jn, i_s_, src, values, x0, i0, pa, pb, cur,
                                  np.asarray(dprobe, dtype=np.int32), np.asarray(tprobe, dtype=np.int32), dense=False,
                                  max_iter=max_iter, method=0, keep_every=1, envelope=False, **SPICE)

    assert (call()[4] == 0).all()
    far_rows = diode_rows.copy()
    far_rows[0] = child.table.ncomp
    not_gm, far_gm, split = gm_rows.copy(), gm_rows.copy(), gm_rows.copy()
    not_gm[0, 0] = diode_rows[0]          # an R row
    far_gm[1, 1] = child.table.ncomp      # out of range
    split[0, 1] = gm_rows[1, 1]           # the two rows of transport 0 do not share their leads a, b
    swapped = junction.copy()
    swapped[0] = junction[0, ::-1]        # each GM row's c, d are then the OTHER junction's leads
    outside, negative = junction.copy(), junction.copy()
    outside[T - 1, 1] = D + 2 * T
    negative[0, 0] = -1
    for kw in (dict(rows_=far_rows), dict(sat=np.where(np.arange(D + 2 * T) == D, 0.0, i_sat)), dict(dprobe=(D + 2 * T,)),
               dict(max_iter=0), dict(gm=not_gm), dict(gm=far_gm), dict(gm=split), dict(jn=swapped), dict(jn=outside),
               dict(jn=negative), dict(i_s_=np.where(np.arange(T) == 1, 0.0, i_s)),
               dict(i_s_=np.where(np.arange(T) == 2, np.inf, i_s)), dict(tprobe=(T,)), dict(tprobe=(-1,))):
        with pytest.raises(_ffi.NodalHipError) as exc:
            call(**kw)
        assert exc.value.status == _ffi.E_INVALID, kw
    assert (call()[4] == 0).all()  # (and the handle is usable afterwards)
