"""Circuit.operating_point (nodal_newton_dc) on the device against the fp64 reference of tests/newton_reference.py:
closed forms on the dense-panel route, a grid with an E source on the sparse LU route, a 66 x 66 grid on the multigrid
route; one-step parity of every iterate, the nonlinear residual at the answer, repeatability, warm starts, the
small-signal circuit and the failure paths."""
import warnings

import numpy as np
import pytest

import nodal_amd as n
from tests import newton_reference as nr
from tests.newton_reference import I_SAT, N_VT, RESID_BAR, TIGHT, TOL, NewtonReference
from tests.test_newton_reference import parity_errors

pytestmark = pytest.mark.gpu


def circuit_of(rows, sparse):
    return n.Circuit(n.Netlist.from_rows([list(r) for r in rows]), sparse=sparse, device=0)


def check_answer(ref, op, label=""):
    """the checks at the answer: nonlinear residual, one further reference step, the diodes' outputs"""
    x = op.x
    xs = np.abs(x).max()
    res, scale = ref.residual(x)
    worst = np.abs(res).max() / scale.max()
    x1, _, _ = ref.one_step(x, ref.voltages(x))
    moved = np.abs(x1 - x).max()
    print(f"{label}: nonlinear residual {worst:.2e} of its scale, one more reference step moves x by {moved:.2e}")
    assert worst <= RESID_BAR + ref.reltol + ref.abstol / scale.max()
    assert moved <= (2 * TOL + ref.reltol) * xs + ref.vntol
    v = ref.voltages(x)
    assert np.abs(op.voltages - v).max(initial=0.0) <= 2 * TOL * xs
    i, g = ref.current(v), ref.conductance(v)
    assert (np.abs(op.currents - i) <= 2 * TOL * (np.abs(i) + ref.i_sat + ref.gmin * np.abs(v))).all()
    assert (np.abs(op.conductances - g) <= 2 * TOL * g).all()


def run_and_check(circ, ref, diodes, initial=None, sources=None, label="", solvable=True, again=True):
    """one operating point with every check of the file; returns it"""
    before = circ.solve().result.copy() if solvable else None
    table = {name: np.array(getattr(circ.table, name)) for name in ("type", "value", "a", "b")}
    op = circ.operating_point(diodes, sources=sources, initial=initial, keep_iterates=True, **TIGHT)
    hist = op.history
    print(f"{label}: {op.iterations} Newton iterations, routes {hist.route}, solver iterations {hist.iterations.tolist()}, "
          f"not converged {hist.not_converged.tolist()}, limited {hist.limited.tolist()}, "
          f"worst scaled residual {hist.scaled_residual.max():.2e}, timings {op.timings}")
    assert op.converged and op.iterations == len(hist) == len(op.iterates) == len(op.limited_voltages) - 1
    assert (hist.info == 0).all() and (hist.scaled_residual <= RESID_BAR).all()
    # one-step parity: the reference advances the DEVICE's (x_k, vh_k)
    start = np.zeros(ref.n) if initial is None else np.asarray(initial, dtype=np.float64)
    assert np.array_equal(op.limited_voltages[0], ref.voltages(start))
    ex, ev, left, total, counts = parity_errors(ref, op.iterates, op.limited_voltages, start)
    print(f"{label}: parity x {ex:.2e}, vh {ev:.2e}, {left} of {total} comparisons undecidable")
    assert ex <= 2 * TOL and ev <= 2 * TOL and left <= 0.01 * total
    for k, (bad, limited, undecided) in enumerate(counts):
        if undecided == 0:
            assert (hist.not_converged[k], hist.limited[k]) == (bad, limited), k
    assert np.array_equal(op.iterates[-1], op.x)
    check_answer(ref, op, label)
    if again:  # a second identical call: the same bits, and no symbolic work
        op2 = circ.operating_point(diodes, sources=sources, initial=initial, keep_iterates=True, **TIGHT)
        assert np.array_equal(op2.x, op.x) and np.array_equal(op2.history.record, hist.record)
        assert np.array_equal(op2.iterates, op.iterates) and np.array_equal(op2.limited_voltages, op.limited_voltages)
        assert op2.history.route == hist.route and op2.timings[1] == 0.0, op2.timings
    # the circuit itself is left as it was
    if solvable:
        assert np.array_equal(circ._handle.download_x(), before)
    for name, column in table.items():
        assert np.array_equal(np.array(getattr(circ.table, name)), column)
    return op


# ---- closed forms: the dense-panel route --------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("amps", [1e-9, 1e-6, 1e-3, 1.0])
def test_a_source_into_a_diode_meets_the_closed_form(amps, sparse):
    rows, diodes = nr.source_diode_rows(amps), [("d1", I_SAT, N_VT, "1", "g")]
    ref = NewtonReference(rows, diodes, gmin=0.0, **TIGHT)
    circ = circuit_of(rows, sparse)
    before = np.array(circ.table.value)
    op = circ.operating_point(diodes, gmin=0.0, keep_iterates=True, **TIGHT)
    v = nr.source_diode_closed_form(amps, I_SAT, N_VT)
    print(f"I = {amps:g}, sparse {sparse}: routes {op.history.route}, {op.iterations} iterations, v = {op.x[0]!r}, "
          f"closed form {v!r}")
    assert op.converged and set(op.history.route) == {"dense"}
    assert abs(op.x[0] - v) <= 2 * TOL * abs(v)
    assert (op.history.info == 0).all() and (op.history.scaled_residual <= RESID_BAR).all()
    ex, ev, left, total, _ = parity_errors(ref, op.iterates, op.limited_voltages, np.zeros(1))
    assert ex <= 2 * TOL and ev <= 2 * TOL and left <= 0.01 * total
    check_answer(ref, op, f"I = {amps:g}")
    assert np.array_equal(np.array(circ.table.value), before)


@pytest.mark.parametrize("sparse", [False, True])
def test_a_source_behind_a_resistor_meets_the_closed_form(sparse):
    rows, diodes = nr.series_rows(5.0, 1000.0), [("d1", I_SAT, N_VT, "2", "g")]
    circ = circuit_of(rows, sparse)
    assert circ.table.B == 1
    # every check of the file at the default gmin, which the closed form does not know ...
    run_and_check(circ, NewtonReference(rows, diodes, **TIGHT), diodes, label=f"E-R-diode, sparse {sparse}")
    # ... and the closed form at gmin = 0
    op = circ.operating_point(diodes, gmin=0.0, keep_iterates=True, **TIGHT)
    v = nr.series_closed_form(5.0, 1000.0, I_SAT, N_VT)
    assert set(op.history.route) == {"dense"} and op.converged
    assert abs(op.x[1] - v) <= 2 * TOL * abs(v)
    ref = NewtonReference(rows, diodes, gmin=0.0, **TIGHT)
    ex, ev, left, total, _ = parity_errors(ref, op.iterates, op.limited_voltages, np.zeros(3))
    assert ex <= 2 * TOL and ev <= 2 * TOL and left <= 0.01 * total
    check_answer(ref, op, "E-R-diode, gmin 0")


# ---- the sparse LU route -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lu_inputs():
    rows, diodes, initial = nr.lu_case()
    return rows, diodes, initial, NewtonReference(rows, diodes, **TIGHT)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("start", ["cold", "hard"])
def test_the_sparse_lu_route(lu_inputs, start, sparse):
    rows, diodes, initial, ref = lu_inputs
    circ = circuit_of(rows, sparse)
    assert circ.table.B == 1 and circ.table.K == 144
    op = run_and_check(circ, ref, diodes, initial=initial if start == "hard" else None,
                       label=f"grid(12) + E, {start} start, sparse {sparse}")
    assert set(op.history.route) <= {"lu", "direct"}
    d = op.diodes.index("d_same")  # both leads on one node: exactly nothing
    assert (op.limited_voltages[:, d] == 0.0).all() and op.currents[d] == 0.0 and op.voltages[d] == 0.0
    if start == "hard":
        assert op.history.limited.sum() > 0  # (limiting acts on the start above v_crit)


# ---- the multigrid route ---------------------------------------------------------------------------------------------------
def test_the_multigrid_route():
    rows, diodes = nr.mg_case()
    ref = NewtonReference(rows, diodes, **TIGHT)
    circ = circuit_of(rows, True)
    assert circ.table.B == 0 and circ.table.K == 4355
    op = run_and_check(circ, ref, diodes, label="grid(66)")
    handed_over = [k for k, route in enumerate(op.history.route) if route == "direct"]
    print(f"grid(66): steps handed to the direct solve: {handed_over}")
    assert set(op.history.route) <= {"multigrid", "direct"} and "multigrid" in op.history.route


# ---- sources= and warm starts ----------------------------------------------------------------------------------------------
def test_a_source_sweep_with_warm_starts(lu_inputs):
    rows, diodes, _, _ = lu_inputs
    circ = circuit_of(rows, True)
    previous = None
    for volts in (3.0, 3.5, 4.0, 4.5):
        sources = {"e1": volts, "a1": volts / 6.0}
        ref = NewtonReference(rows, diodes, sources=sources, **TIGHT)
        cold = circ.operating_point(diodes, sources=sources, **TIGHT)
        op = run_and_check(circ, ref, diodes, initial=previous, sources=sources, label=f"e1 = {volts}", again=False)
        print(f"e1 = {volts}: {op.iterations} iterations from the previous point, {cold.iterations} from zeros")
        assert cold.converged and np.abs(cold.x - op.x).max() <= (4 * TOL + 2 * TIGHT["reltol"]) * np.abs(op.x).max()
        assert op.timings[1] == 0.0  # (the child and everything symbolic on it were kept)
        if previous is not None:
            assert op.iterations <= cold.iterations
        previous = op.x


# ---- the small-signal circuit ----------------------------------------------------------------------------------------------
def test_thevenin_on_the_linearised_circuit(lu_inputs):
    rows, diodes, _, ref = lu_inputs
    circ = circuit_of(rows, True)
    op = circ.operating_point(diodes, **TIGHT)
    assert op.converged
    port = ("1", "g")
    small = op.linearised()
    assert small.table.ncomp == circ.table.ncomp + len(diodes)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        z = small.thevenin([port], sources=False).z[0, 0]
    # the slope of the port voltage against a small current injected into the port, from the reference's own Jacobian
    e = np.zeros(ref.n)
    e[nr._index(ref.nl, port[0])] = 1.0
    slope = ref.solve(ref.jacobian(op.x), e)[nr._index(ref.nl, port[0])]
    print(f"port resistance at the operating point {z!r}, the reference's Jacobian gives {slope!r}")
    assert abs(z - slope) <= 2 * TOL * abs(slope)
    # ... and it IS the finite-difference slope of the nonlinear circuit (fp64 reference, central difference)
    dI = 1e-6
    up = NewtonReference(rows, diodes, sources={"a1": 0.5 + dI}, **TIGHT).run(op.x)["x"]
    down = NewtonReference(rows, diodes, sources={"a1": 0.5 - dI}, **TIGHT).run(op.x)["x"]
    at = nr._index(ref.nl, port[0])
    assert abs((up[at] - down[at]) / (2 * dI) - slope) <= 1e-5 * abs(slope)


# ---- failure paths that fault nothing ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_too_few_iterations_warn_and_return(lu_inputs, sparse):
    rows, diodes, initial, _ = lu_inputs
    circ = circuit_of(rows, sparse)
    with pytest.warns(RuntimeWarning, match="did not converge") as caught:
        op = circ.operating_point(diodes, initial=initial, max_iter=2, keep_iterates=True, **TIGHT)
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == 1
    assert not op.converged and op.iterations == 2 and len(op.history) == 2
    assert np.isfinite(op.x).all() and np.isfinite(op.voltages).all() and np.isfinite(op.currents).all()
    assert np.isfinite(op.conductances).all() and np.isfinite(op.history.record).all()
    assert op.iterates.shape == (2, len(op.x)) and op.limited_voltages.shape == (3, len(diodes))


@pytest.mark.parametrize("sparse", [False, True])
def test_a_node_held_by_an_underflowed_diode_is_singular(sparse):
    """node 2 hangs on a diode alone; gmin = 0 and 30 V of reverse bias: exp(-30 / n_vt) underflows, g is exactly 0"""
    from scipy.sparse.linalg import MatrixRankWarning
    rows = [["a1", "A", "1", "1", "g"], ["r1", "R", "1", "1", "g"], ["a2", "A", "0", "2", "g"]]
    diodes = [("d1", I_SAT, N_VT, "2", "1")]
    circ = circuit_of(rows, sparse)
    initial = np.zeros(2)
    initial[circ.netlist.nodenum["2"]] = -30.0
    if sparse:
        with pytest.warns(MatrixRankWarning):
            op = circ.operating_point(diodes, gmin=0.0, initial=initial, **TIGHT)
        assert not op.converged and op.iterations == 1 and op.history.info.tolist() == [1]
        assert np.isnan(op.x).all() and np.isnan(op.voltages).all() and np.isnan(op.history.record).all()
    else:
        with pytest.raises((np.linalg.LinAlgError, n.UnconnectedCircuitError)):
            circ.operating_point(diodes, gmin=0.0, initial=initial, **TIGHT)
    # the circuit and its child stay usable: with gmin the same start is an ordinary operating point
    op = circ.operating_point(diodes, gmin=1e-12, initial=initial, **TIGHT)
    assert op.converged and np.isfinite(op.x).all()
    check_answer(NewtonReference(rows, diodes, gmin=1e-12, **TIGHT), op, "after the singular call")


@pytest.mark.parametrize("sparse", [False, True])
def test_a_start_whose_exponential_overflows_ends_the_loop(sparse):
    """100 V across a junction: exp(100 / n_vt) is inf, g is inf and 1 / g is 0 -- the first assembly reports it, the
    loop ends there without a state, and the circuit and its child stay usable"""
    rows, diodes = [["a1", "A", "1", "1", "g"], ["r1", "R", "1", "1", "g"]], [("d1", I_SAT, N_VT, "1", "g")]
    circ = circuit_of(rows, sparse)
    with pytest.warns(RuntimeWarning, match="did not converge"):
        op = circ.operating_point(diodes, initial=[100.0], keep_iterates=True, **TIGHT)
    assert not op.converged and op.iterations == 1 and op.history.info.tolist() == [0]
    assert np.isnan(op.x).all() and np.isnan(op.currents).all() and np.isnan(op.history.record).all()
    assert op.limited_voltages[0].tolist() == [100.0]
    ref = NewtonReference(rows, diodes, **TIGHT)
    op = run_and_check(circ, ref, diodes, label=f"after the overflow, sparse {sparse}")
    assert abs(op.x[0] - ref.run()["x"][0]) <= 2 * TOL * abs(op.x[0])


@pytest.mark.parametrize("sparse", [False, True])
def test_without_diodes_it_is_one_linear_solve(lu_inputs, sparse):
    rows = lu_inputs[0]
    circ = circuit_of(rows, sparse)
    x = circ.solve().result
    op = circ.operating_point([], **TIGHT)
    assert op.converged and op.iterations == 1 and len(op.voltages) == 0
    assert np.abs(op.x - x).max() <= 2 * TOL * np.abs(x).max()
    assert op.history.scaled_residual[0] <= RESID_BAR
