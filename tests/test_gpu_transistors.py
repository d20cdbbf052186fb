"""Circuit.operating_point(transistors=...) (nodal_newton_dc_bjt) on the device against the fp64 reference of
tests/transistor_reference.py: every region of the Ebers-Moll model on the dense-panel route, a grid with an E source on
the sparse LU route; one-step parity of every iterate, the answer, the terminal currents, repeatability, the hybrid-pi
circuit, the entry without transports, what the ABI refuses and an overflow."""
import numpy as np
import pytest
import scipy.sparse as sp

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd._ffi import NodalHipError
from tests import newton_reference as nr
from tests import transistor_reference as tr
from tests.newton_reference import I_SAT, N_VT, RESID_BAR, TIGHT, TOL
from tests.transistor_reference import TransistorReference, parity_errors

pytestmark = pytest.mark.gpu


def circuit_of(rows, sparse):
    return n.Circuit(n.Netlist.from_rows([list(r) for r in rows]), sparse=sparse, device=0)


@pytest.fixture(scope="module")
def references():
    """the reference of every case, made once and left unchanged"""
    out = {}
    for name, case in tr.CASES.items():
        rows, diodes, transistors = case()
        out[name] = (rows, diodes, transistors, TransistorReference(rows, diodes, transistors, **TIGHT))
    return out


def check_answer(ref, op, label=""):
    """the checks at the answer: nonlinear residual, one further reference step, the diodes' and transistors' outputs"""
    x = op.x
    xs = np.abs(x).max()
    res, scale = ref.residual(x)
    worst = np.abs(res).max() / scale.max()
    x1, _, _ = ref.one_step(x, ref.voltages(x))
    moved = np.abs(x1 - x).max()
    print(f"{label}: nonlinear residual {worst:.2e} of its scale, one more reference step moves x by {moved:.2e}")
    assert worst <= RESID_BAR + ref.reltol + ref.abstol / scale.max()
    assert moved <= (2 * TOL + ref.reltol) * xs + ref.vntol
    D, T = ref.D0, ref.T
    v = ref.voltages(x)
    i, g = ref.current(v), ref.conductance(v)
    assert np.abs(op.voltages - v[:D]).max(initial=0.0) <= 2 * TOL * xs
    assert (np.abs(op.currents - i[:D]) <= 2 * TOL * (np.abs(i[:D]) + ref.i_sat[:D] + ref.gmin * np.abs(v[:D]))).all()
    assert (np.abs(op.conductances - g[:D]) <= 2 * TOL * g[:D]).all()
    assert op.transistors == ref.transistor_names and op.junction_voltages.shape == (T, 2)
    assert np.abs(op.junction_voltages - v[D:].reshape(T, 2)).max(initial=0.0) <= 2 * TOL * xs
    _, gmf, gmr = ref.transport(v)
    assert (np.abs(op.transconductances - np.stack([gmf, gmr], axis=1)) <= 2 * TOL * np.stack([gmf, gmr], axis=1)).all()
    currents = (op.collector_currents, op.base_currents, op.emitter_currents)
    for mine, theirs in zip(currents, ref.terminal_currents(x)):
        assert mine.shape == (T,) and (np.abs(mine - theirs) <= 2 * TOL * (np.abs(theirs) + ref.i_s)).all()
    i_c, i_b, i_e = currents
    assert (np.abs(i_c + i_b + i_e) <= 4 * TOL * (np.abs(i_c) + np.abs(i_b) + np.abs(i_e))).all()


def run_and_check(circ, ref, diodes, transistors, label="", gmin=1e-12):
    """one operating point with every check of the file; returns it"""
    before = circ.solve().result.copy()
    table = {name: np.array(getattr(circ.table, name)) for name in ("type", "value", "a", "b", "c", "d")}
    args = dict(transistors=transistors, gmin=gmin, keep_iterates=True, **TIGHT)
    op = circ.operating_point(diodes, **args)
    hist = op.history
    print(f"{label}: {op.iterations} Newton iterations, routes {hist.route}, not converged {hist.not_converged.tolist()}, "
          f"limited {hist.limited.tolist()}, transports {hist.transistors_not_converged.tolist()}, "
          f"worst scaled residual {hist.scaled_residual.max():.2e}, timings {op.timings}")
    assert op.converged and op.iterations == len(hist) == len(op.iterates) == len(op.limited_voltages) - 1
    assert op.limited_voltages.shape[1] == ref.D0 + 2 * ref.T and op.diodes == ref.names[:ref.D0]
    assert hist.record.shape == (op.iterations, 5)
    assert (hist.info == 0).all() and (hist.scaled_residual <= RESID_BAR).all()
    # one-step parity: the reference advances the DEVICE's (x_k, vh_k)
    start = np.zeros(ref.n)
    assert np.array_equal(op.limited_voltages[0], ref.voltages(start))
    ex, ev, left, total, counts = parity_errors(ref, op.iterates, op.limited_voltages, start)
    print(f"{label}: parity x {ex:.2e}, vh {ev:.2e}, {left} of {total} comparisons undecidable")
    assert ex <= 2 * TOL and ev <= 2 * TOL and left <= 0.01 * total
    for k, (bad, limited, undecided, tbad) in enumerate(counts):
        if undecided == 0:
            assert (hist.not_converged[k], hist.limited[k], hist.transistors_not_converged[k]) == (bad, limited, tbad), k
    assert np.array_equal(op.iterates[-1], op.x)
    check_answer(ref, op, label)
    # a second identical call: the same bits, and no symbolic work
    op2 = circ.operating_point(diodes, **args)
    assert np.array_equal(op2.x, op.x) and np.array_equal(op2.history.record, hist.record)
    assert np.array_equal(op2.iterates, op.iterates) and np.array_equal(op2.limited_voltages, op.limited_voltages)
    assert np.array_equal(op2.transconductances, op.transconductances)
    assert op2.history.route == hist.route and op2.timings[1] == 0.0, op2.timings
    # the circuit itself is left as it was
    assert np.array_equal(circ._handle.download_x(), before)
    for name, column in table.items():
        assert np.array_equal(np.array(getattr(circ.table, name)), column)
    return op


def assembled(circ):
    """the circuit's assembled matrix through the handle's CSR export"""
    indptr, indices, data, _ = circ._handle.export_csr()
    return sp.csr_matrix((data, indices, indptr), shape=(circ._handle.n, circ._handle.n))


def check_linearised(ref, op, label=""):
    """the hybrid-pi circuit's matrix IS the reference's Jacobian at the answer"""
    small = op.linearised()
    assert small.table.ncomp == op._circuit.table.ncomp + ref.D0 + 4 * ref.T
    J = ref.jacobian(op.x).toarray()
    worst = np.abs(assembled(small).toarray() - J).max() / np.abs(J).max()
    print(f"{label}: the linearised circuit's matrix differs from the reference's Jacobian by {worst:.2e} of its largest entry")
    assert worst <= 2 * TOL


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("name", ["ce_amp", "switch_sat", "reverse_active", "mirror", "pnp_follower", "diff_pair"])
def test_the_dense_panel_route(references, name, sparse):
    rows, diodes, transistors, ref = references[name]
    circ = circuit_of(rows, sparse)
    assert circ._handle.n == tr.SIZES[name] <= 64
    op = run_and_check(circ, ref, diodes, transistors, label=f"{name}, sparse {sparse}")
    assert set(op.history.route) == {"dense"}
    check_linearised(ref, op, name)
    with pytest.raises(ValueError, match="adjoint with transistors is not implemented"):
        op.gradient(np.ones(len(op.x)))


@pytest.mark.parametrize("sparse", [False, True])
def test_the_sparse_lu_route(references, sparse):
    rows, diodes, transistors, ref = references["lu_grid"]
    circ = circuit_of(rows, sparse)
    assert circ._handle.n == 145 and circ.table.B == 1
    op = run_and_check(circ, ref, diodes, transistors, label=f"lu_grid, sparse {sparse}")
    assert set(op.history.route) <= {"lu", "direct"}
    check_linearised(ref, op, "lu_grid")
    t = op.transistors.index("q5")  # every lead on one node: exactly nothing
    assert op.collector_currents[t] == 0.0 and op.base_currents[t] == 0.0 and op.emitter_currents[t] == 0.0
    assert (op.junction_voltages[t] == 0.0).all()
    d = op.diodes.index("d_same")
    assert (op.limited_voltages[:, d] == 0.0).all() and op.currents[d] == 0.0


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("amps", [1e-9, 1e-6, 1e-3, 1.0])
def test_a_diode_connected_transistor_meets_the_closed_form(amps, sparse):
    rows, diodes, transistors = tr.diode_connected(amps)
    ref = TransistorReference(rows, diodes, transistors, gmin=0.0, **TIGHT)
    circ = circuit_of(rows, sparse)
    op = circ.operating_point(diodes, transistors=transistors, gmin=0.0, keep_iterates=True, **TIGHT)
    v = tr.diode_connected_closed_form(amps)
    print(f"I = {amps:g}, sparse {sparse}: routes {op.history.route}, {op.iterations} iterations, v = {op.x[0]!r}, "
          f"closed form {v!r}")
    assert op.converged and set(op.history.route) == {"dense"}
    assert abs(op.x[0] - v) <= 2 * TOL * abs(v)
    assert (op.history.info == 0).all() and (op.history.scaled_residual <= RESID_BAR).all()
    # (no bar on the comparisons left out here: the first iterate from zeros is I n_vt / i_s, up to 1e12 V, and beside
    # it the band 4 TOL |x| swallows the thresholds of the base-collector junction, whose voltage is exactly 0)
    ex, ev, left, total, _ = parity_errors(ref, op.iterates, op.limited_voltages, np.zeros(1))
    print(f"I = {amps:g}: parity x {ex:.2e}, vh {ev:.2e}, {left} of {total} comparisons undecidable")
    assert ex <= 2 * TOL and ev <= 2 * TOL
    j = ref.jr[0]
    assert (op.limited_voltages[:, j] == 0.0).all() and op.junction_voltages[0, 1] == 0.0
    check_answer(ref, op, f"I = {amps:g}")


# ---- the entry itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_without_transports_the_entry_is_nodal_newton_dc(sparse):
    rows, diodes, initial = nr.lu_case()
    circ = circuit_of(rows, sparse)
    op = circ.operating_point(diodes, initial=initial, keep_iterates=True, **TIGHT)
    _, child, diode_rows = circ._newton_child
    args = (np.zeros(0, dtype=np.int64), np.zeros(0), initial)
    kwargs = dict(dense=not sparse, max_iter=100, keep_iterates=True, **TIGHT)
    plain = child._handle.newton_dc(diode_rows, op.i_sat, op.n_vt, 1e-12, *args, **kwargs)
    none = child._handle.newton_dc_bjt(diode_rows, op.i_sat, op.n_vt, 1e-12, np.zeros((0, 2), dtype=np.int64),
                                       np.zeros((0, 2), dtype=np.int32), np.zeros(0), *args, **kwargs)
    assert plain["converged"] and none["converged"] and plain["iterations"] == none["iterations"]
    for key in ("x", "v", "i", "g", "iterates", "vh", "info", "iters", "route"):
        assert np.array_equal(plain[key], none[key]), key
    assert np.array_equal(none["record"][:, :4], plain["record"]) and (none["record"][:, 4] == 0.0).all()
    assert np.array_equal(plain["x"], op.x)


def test_what_the_entry_refuses(references):
    from nodal_amd.operating_point import resolve_diodes, resolve_transistors, transistor_companion_table
    rows, diodes, transistors, _ = references["ce_amp"]
    circ = circuit_of(rows, True)
    _, _, junctions, ta, tb, junction, i_s = resolve_transistors(circ.netlist, transistors)
    _, i_sat, n_vt, ia, ib = resolve_diodes(circ.netlist, junctions)
    table, diode_rows, gm_rows = transistor_companion_table(circ.table, i_sat, n_vt, ia, ib, ta, tb, junction, i_s, 1e-12)
    child = n.Circuit._clone_of(circ, table)
    none = (np.zeros(0, dtype=np.int64), np.zeros(0), None)
    kwargs = dict(dense=False, max_iter=100, **TIGHT)

    def call(gm=gm_rows, jn=junction, sat=i_s):
        return child._handle.newton_dc_bjt(diode_rows, i_sat, n_vt, 1e-12, gm, jn, sat, *none, **kwargs)

    assert call()["converged"]
    swapped_junctions = junction[:, ::-1].copy()  # (each GM row's c, d are then the OTHER junction's leads)
    for bad in (dict(gm=np.array([[diode_rows[0], gm_rows[0, 1]]])), dict(jn=swapped_junctions),
                dict(jn=np.array([[0, 2]], dtype=np.int32)), dict(jn=np.array([[-1, 1]], dtype=np.int32)),
                dict(sat=np.array([0.0])), dict(sat=np.array([-1e-14])), dict(sat=np.array([np.inf])),
                dict(gm=np.array([[gm_rows[0, 0], table.ncomp]]))):
        with pytest.raises(NodalHipError) as caught:
            call(**bad)
        assert caught.value.status == _ffi.E_INVALID, bad
    assert call()["converged"]  # (the handle stays usable)


@pytest.mark.parametrize("sparse", [False, True])
def test_an_exponential_that_overflows_ends_the_loop(sparse):
    """a transistor between a 1000 V source and ground without any resistance: the first solve puts 1000 V on both
    junctions, and the loop must end -- on the overflow or on an iterate that is not finite -- without converging"""
    rows = [["e1", "E", "1000", "1", "g"]]
    transistors = [tr.npn("q1", "g", 1, "g")]
    circ = circuit_of(rows, sparse)
    with pytest.warns(RuntimeWarning, match="did not converge"):
        op = circ.operating_point([], transistors=transistors, max_iter=2000, **TIGHT)
    print(f"overflow, sparse {sparse}: {op.iterations} iterations, x {op.x}, record {op.history.record[-1]}")
    assert not op.converged and op.iterations < 2000
    assert not np.isfinite(op.x).all() or not np.isfinite(op.history.record[-1]).all()
    # the circuit and its child stay usable: a gentler source is an ordinary operating point
    ref = TransistorReference(rows, [], transistors, sources={"e1": 0.7}, **TIGHT)
    op = circ.operating_point([], transistors=transistors, sources={"e1": 0.7}, **TIGHT)
    assert op.converged and np.abs(op.x - ref.run()["x"]).max() <= 2 * TOL * np.abs(op.x).max()
