"""What nodal_newton_dc, nodal_transient_nl and nodal_newton_gradient share (csrc/newton.hip: DiodeSet and
newton_iteration), stated through the three entry points so that it holds whether the library has one copy of the
iteration or two:

(a) One time step of a network without capacitors or inductors has an empty history, so it IS the DC Newton loop from
    the same start with the same sources and tolerances: the same iteration count, the same verdict, and -- the two
    run the same statements in the same order -- the same bits in the limited voltages and in x.  Measured on an
    MI355X before the two loops were merged: every bit equal, on both networks and both routes; so equal bits are asserted.
    A step that does not converge reports NaN (nodal_transient_nl's contract), so there the counts and verdicts are
    compared and the NaNs are asserted.
(b) After a linearisation that overflowed (100 V across a junction: exp is inf, 1 / g is 0) each entry point returns what
    its contract says, and the handle holds a legal matrix again: 1.0 in every companion row.  A sparse solve on it
    has the bits of the same solve on a fresh handle with that table.
(c) The count of diodes whose next 1 / g moved decides whether an iteration assembles: 1 matrix update in the first step
    and 0 afterwards for clamps at rest, as many updates as iterations with NODAL_TNL_REUSE=0.  That is exactly
    tests/test_gpu_transient_diodes.py::test_clamps_at_rest_reuse_the_matrix, and is not repeated here."""
import warnings

import numpy as np
import pytest

import nodal_amd as n
from tests import newton_reference as nr
from tests.newton_reference import I_SAT, N_VT, TIGHT

pytestmark = pytest.mark.gpu


def circuit_of(rows, sparse):
    return n.Circuit(n.Netlist.from_rows([list(r) for r in rows]), sparse=sparse, device=0)


def panel_case():
    """E behind 1 kOhm into a diode to ground, a second diode across r2: 3 nodes, n = 4, the dense panel"""
    rows = nr.series_rows(5.0, 1000.0) + [["r2", "R", "500", "2", "3"], ["r3", "R", "2000", "3", "g"]]
    return rows, [("d1", I_SAT, N_VT, "2", "g"), ("d2", 2e-14, 0.03, "3", "2")]


@pytest.fixture(scope="module")
def lu_inputs():
    rows, diodes, _ = nr.lu_case()  # n = 145: the sparse LU route
    return rows, diodes


def network(name, lu_inputs):
    return panel_case() if name == "panel" else lu_inputs


# ---- (a) one transient step is the DC loop ----------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("max_iter", [50, 2])
@pytest.mark.parametrize("name", ["panel", "lu"])
def test_one_step_without_history_is_the_dc_loop(lu_inputs, name, max_iter, sparse):
    rows, diodes = network(name, lu_inputs)
    circ = circuit_of(rows, sparse)
    x0 = np.zeros(circ.table.n)  # a cold start: the first solve puts volts across junctions, the limiter acts
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        op = circ.operating_point(diodes, initial=x0, max_iter=max_iter, keep_iterates=True, **TIGHT)
        tr = circ.transient([], 1.0, 1, initial=x0, diodes=diodes, keep_every=1, max_iter=max_iter, **TIGHT)
    print(f"{name}, sparse {sparse}, max_iter {max_iter}: DC {op.iterations} iterations, converged {op.converged}, limited "
          f"{op.history.limited.tolist()}; the step {tr.newton_iterations.tolist()} iterations, info {tr.info.tolist()}, "
          f"largest difference in x {np.abs(tr.solutions[0] - op.x).max():.2e}, "
          f"in vh {np.abs(tr.final_junctions - op.limited_voltages[op.iterations]).max():.2e}")
    assert op.history.limited.sum() > 0 and (op.history.info == 0).all()
    assert op.converged == (max_iter == 50)
    assert tr.newton_iterations[0] == op.iterations
    assert (tr.info[0] == 0) == op.converged and tr.info[0] in (0, 2)
    if op.converged:
        assert np.array_equal(tr.final_junctions, op.limited_voltages[op.iterations])
        assert np.array_equal(tr.solutions[0], op.x)
    else:
        assert np.isnan(tr.final_junctions).all() and np.isnan(tr.solutions[0]).all() and np.isfinite(op.x).all()


# ---- (b) after an overflowed linearisation the handle is usable ---------------------------------------------------------
def hot_start(circ):
    x = np.zeros(circ.table.n)
    x[circ.netlist.nodenum["30"]] = 100.0  # across d_hard, node 30 to ground
    return x


def check_handle_after_overflow(circ, child, diode_rows):
    """the child's sparse solve against the same solve on a fresh handle whose table holds 1.0 in the companion rows"""
    values = np.array(child.table.value)
    values[diode_rows] = 1.0
    fresh = n.Circuit._clone_of(circ, child.table.with_values(values))
    x, info = child._handle.solve_sparse()[:2]
    want, info_fresh = fresh._handle.solve_sparse()[:2]
    assert info == 0 and info_fresh == 0 and np.isfinite(want).all()
    assert np.array_equal(x, want)


def test_after_an_overflow_in_newton_dc(lu_inputs):
    rows, diodes = lu_inputs
    circ = circuit_of(rows, True)
    with pytest.warns(RuntimeWarning, match="did not converge"):
        op = circ.operating_point(diodes, initial=hot_start(circ), keep_iterates=True, **TIGHT)
    assert not op.converged and op.iterations == 1 and op.history.info.tolist() == [0]
    assert np.isnan(op.x).all() and np.isnan(op.voltages).all() and np.isnan(op.history.record).all()
    _, child, diode_rows = circ._newton_child
    check_handle_after_overflow(circ, child, diode_rows)


def test_after_an_overflow_in_transient_nl(lu_inputs):
    rows, diodes = lu_inputs
    circ = circuit_of(rows, True)
    caps = [("c1", 1.0, "1", "g"), ("c2", 0.5, "30", "g")]
    with pytest.warns(RuntimeWarning, match="step 1 did not converge"):
        tr = circ.transient(caps, 0.05, 2, probes=["1"], initial=hot_start(circ), diodes=diodes, diode_probes=["d_hard"],
                            keep_every=1, max_iter=50, **TIGHT)
    assert tr.info.tolist() == [2, 2] and tr.newton_iterations.tolist() == [1, 0] and tr.matrix_updates.tolist() == [0, 0]
    assert np.isnan(tr.waveforms[1:]).all() and np.isnan(tr.solutions).all() and np.isnan(tr.final_junctions).all()
    assert tr.diode_voltages[0].tolist() == [100.0]
    _, child, _, _, diode_rows = circ._transient_child
    check_handle_after_overflow(circ, child, diode_rows)


def test_after_an_overflow_in_newton_gradient(lu_inputs):
    rows, diodes = lu_inputs
    circ = circuit_of(rows, True)
    op = circ.operating_point(diodes, **TIGHT)
    assert op.converged
    _, child, diode_rows = circ._newton_child
    r = child._handle.newton_gradient(diode_rows, op.i_sat, op.n_vt, op.gmin, op.source_rows, op.source_values,
                                      hot_start(circ), np.ones(circ.table.n), dense=False, adjoints=True)
    assert r["info"] == 0 and np.isnan(r["grad"]).all() and np.isnan(r["i_sat"]).all() and np.isnan(r["n_vt"]).all()
    assert np.isnan(r["gmin"]) and np.isnan(r["adjoint"]).all() and np.isnan(r["resid"]) and np.isnan(r["op_resid"])
    check_handle_after_overflow(circ, child, diode_rows)
