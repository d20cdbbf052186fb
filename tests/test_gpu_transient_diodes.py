"""Circuit.transient(diodes=...) (nodal_transient_nl) on the device against the fp64 reference of
tests/transient_nl_reference.py: a closed form and a rectifier on the dense-panel route, a grid with an E source (and
inductors) on the sparse LU route, a 66 x 66 grid on the multigrid route, both methods; step parity, the nonlinear
residual of every step, the diodes' outputs, the matrix re-use of clamps at rest against NODAL_TNL_REUSE=0 in a fresh
process, and the failure paths.

Measured on an MI355X (parity: the worst |x_k - reference| over max |x_k|; residual: the worst defect over its scale;
solves: the worst scaled residual of a linear solve), against the bars (2 TOL + reltol) max |x_k| + vntol = 2.1e-9 max |x_k|,
RESID_BAR + reltol + abstol / scale = 1.0e-10 and RESID_BAR = 1e-12:
    closed form   error 1.1e-16 V against 2 TOL |v| = 1.4e-9 V
    rectifier     parity 8.0e-16, residual 2.5e-16, solves 1.1e-16
    sparse LU     parity 4.8e-15, residual 2.1e-16, solves 3.8e-17 (with inductors: 4.8e-15, 1.2e-16, 2.9e-17)
    multigrid     parity 2.9e-13, residual 1.3e-13, solves 1.2e-13
Each test prints its own figures before it asserts."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd.operating_point import resolve_diodes
from tests import transient_diodes_child as child
from tests import transient_nl_reference as tn
from tests.transient_nl_reference import I_SAT, N_VT, RESID_BAR, TIGHT, TOL, TransientDiodeReference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_ITER = 50


def circuit_of(rows, sparse):
    return n.Circuit(n.Netlist.from_rows([list(r) for r in rows]), sparse=sparse, device=0)


def node_labels(circ):
    return sorted(circ.netlist.nodenum, key=circ.netlist.nodenum.get)


def run_and_check(case, method, sparse, label):
    """one run from the device's own nonlinear DC start with every check of the file; returns (circuit, Transient, ref)"""
    rows, caps, inds, diodes, dt, steps, sources = case
    ref = TransientDiodeReference(rows, caps, inds, diodes, dt, method, max_iter=MAX_ITER, **TIGHT)
    circ = circuit_of(rows, sparse)
    table = {name: np.array(getattr(circ.table, name)) for name in ("type", "value", "a", "b")}
    tr = circ.transient(caps, dt, steps, sources=sources, probes=node_labels(circ), method=method, inductors=inds,
                        current_probes=[i[0] for i in inds], diodes=diodes, diode_probes=[d[0] for d in diodes],
                        keep_every=1, max_iter=MAX_ITER, **TIGHT)
    print(f"{label}: Newton iterations {tr.newton_iterations.tolist()}, matrix updates {tr.matrix_updates.tolist()}, solver "
          f"iterations {tr.iterations.tolist()}, worst scaled residual {tr.scaled_residual.max():.2e}, timings {tr.timings}")
    assert (tr.info == 0).all() and (tr.scaled_residual <= RESID_BAR).all()
    assert (tr.newton_iterations >= 1).all() and (tr.matrix_updates <= tr.newton_iterations).all()
    # the start: the potentials of x_0 are row 0 of the waveforms (every node is probed), i_0 row 0 of the currents; the
    # histories read nothing else of x_0
    K = circ.table.K
    x0_ref, i0_ref, _ = ref.dc_start()
    x0 = np.zeros(ref.n)
    x0[:K] = tr.waveforms[0]
    top = np.abs(x0_ref).max()
    assert np.abs(x0[:K] - x0_ref[:K]).max() <= (2 * TOL + ref.reltol) * top + ref.vntol
    i0 = tr.currents[0]
    assert np.abs(i0 - i0_ref).max(initial=0.0) <= (2 * TOL + ref.reltol) * max(top, np.abs(i0_ref).max(initial=0.0)) + ref.vntol
    X = np.vstack([x0[None, :], tr.solutions])
    assert np.array_equal(tr.waveforms[1:], tr.solutions[:, :K])
    A = ref.rhs_steps(sources, steps)
    excess, rel, its, I = ref.parity(X, i0, A)
    rexcess, worst = ref.residual_excess(X, i0, A)
    print(f"{label}: parity {rel:.2e} of max |x_k| (the reference's iterations {its}), nonlinear residual {worst:.2e} of its scale")
    assert excess <= 0.0
    assert rexcess <= 0.0
    # the inductor currents against those rebuilt from the device's solutions
    if len(inds):
        assert np.abs(tr.currents - I).max() <= 2 * TOL * max(np.abs(I).max(), np.abs(X).max())
        assert np.array_equal(tr.final_currents, tr.currents[-1])
    # the diodes' outputs, as test_gpu_operating_point.check_answer holds them
    nw = ref.newton
    for k in range(steps + 1):
        v = nw.voltages(X[k])
        xs = np.abs(X[k]).max()
        assert np.abs(tr.diode_voltages[k] - v).max(initial=0.0) <= 2 * TOL * xs
        i = nw.current(v)
        assert (np.abs(tr.diode_currents[k] - i) <= 2 * TOL * (np.abs(i) + nw.i_sat + nw.gmin * np.abs(v))).all()
    assert np.abs(tr.final_junctions - nw.voltages(X[-1])).max() <= (2 * TOL + ref.reltol) * np.abs(X[-1]).max() + ref.vntol
    # the circuit itself is left as it was
    for name, column in table.items():
        assert np.array_equal(np.array(getattr(circ.table, name)), column)
    return circ, tr, ref


# ---- 1. closed form on the dense panel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
def test_a_capacitor_discharging_into_a_diode_meets_the_closed_form(sparse):
    C, h, steps = 1e-3, 1e-4, 5
    circ = circuit_of(tn.rc_diode_rows(), sparse)
    tr = circ.transient([("c1", C, "1", "g")], h, steps, probes=["1"], initial=np.array([0.7]),
                        diodes=[("d1", I_SAT, N_VT, "1", "g")], diode_probes=["d1"], gmin=0.0, max_iter=MAX_ITER, **TIGHT)
    v = tn.rc_diode_closed_form(0.7, C, I_SAT, N_VT, h, steps)
    print(f"sparse {sparse}: v {tr.waveforms[:, 0].tolist()}, closed form {v.tolist()}, Newton iterations "
          f"{tr.newton_iterations.tolist()}, worst error {np.abs(tr.waveforms[:, 0] - v).max():.2e}")
    assert (tr.info == 0).all() and (tr.iterations == 0).all()  # (the dense panel)
    assert (np.abs(tr.waveforms[:, 0] - v) <= 2 * TOL * np.abs(v)).all()
    assert (tr.scaled_residual <= RESID_BAR).all()
    assert np.array_equal(tr.diode_voltages[:, 0], tr.waveforms[:, 0])
    i = I_SAT * np.expm1(v / N_VT)
    # (an error of 2 TOL |v| in v is one of (2 TOL |v| / n_vt) (|i| + i_sat) in i: the slope of the exponential)
    assert (np.abs(tr.diode_currents[:, 0] - i) <= 2 * TOL * np.abs(v) / N_VT * (np.abs(i) + I_SAT)).all()


# ---- 2. the half-wave rectifier on the dense panel, B = 1 ----------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
def test_the_half_wave_rectifier(method, sparse):
    circ, tr, ref = run_and_check(tn.rectifier_case(), method, sparse, f"rectifier {method}, sparse {sparse}")
    assert circ.table.B == 1 and ref.n <= 64 and (tr.iterations == 0).all()
    out = tr.waveforms[:, circ.netlist.nodenum["3"]]
    assert out.max() > 3.0 and out.min() > -1e-3  # (it rectifies: the load never goes negative)


# ---- 3. the sparse LU route --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
@pytest.mark.parametrize("with_inductors", [False, True])
def test_the_sparse_lu_route(with_inductors, method, sparse):
    circ, tr, ref = run_and_check(tn.lu_transient_case(with_inductors), method, sparse,
                                  f"grid(12) + E, inductors {with_inductors}, {method}, sparse {sparse}")
    assert circ.table.B == 1 and circ.table.K == 144 and (tr.iterations >= 1).all()
    assert tr.newton_iterations.max() >= 3  # (the sources switch: the junctions move)


# ---- 4. the multigrid route ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
def test_the_multigrid_route(method):
    circ, tr, ref = run_and_check(tn.mg_transient_case(), method, True, f"grid(66), {method}")
    assert circ.table.B == 0 and circ.table.K == 4355
    levels = circ._transient_child[1]._handle.solve_info()[1]
    print(f"grid(66), {method}: multigrid levels {levels}")
    assert levels >= 2 and tr.iterations.max() > 1  # (the sparse LU reports 1 per step, the dense panel 0)


# ---- 5. clamps at rest: the matrix is assembled and factored once ---------------------------------------------------------
@pytest.fixture(scope="module")
def without_reuse(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tnl_reuse_off"))
    env = dict(os.environ, NODAL_TNL_REUSE="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "transient_diodes_child.py"), d] + list(child.RUNS),
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "transient diodes child ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    return {name: dict(np.load(os.path.join(d, name + ".npz"))) for name in child.RUNS}


@pytest.mark.parametrize("name", list(child.RUNS))
def test_clamps_at_rest_reuse_the_matrix(without_reuse, name, monkeypatch):
    monkeypatch.delenv("NODAL_TNL_REUSE", raising=False)
    got, off = child.outputs(name), without_reuse[name]
    print(f"{name}: Newton iterations {got['newton_iterations'].tolist()}, matrix updates {got['matrix_updates'].tolist()}, "
          f"with NODAL_TNL_REUSE=0 {off['matrix_updates'].tolist()}, solver iterations {got['iterations'].tolist()}")
    assert (got["info"] == 0).all() and (got["scaled_residual"] <= RESID_BAR).all()
    assert (got["matrix_updates"][1:] == 0).all() and got["matrix_updates"][0] == 1
    assert np.array_equal(off["matrix_updates"], off["newton_iterations"])  # (the knob: every iteration assembles)
    assert (got["iterations"] == (0 if name.startswith("dense") else 1)).all()
    for key in got:
        if key != "matrix_updates":
            assert np.array_equal(got[key], off[key], equal_nan=True), key


# ---- 6. edges ---------------------------------------------------------------------------------------------------------------
def fields(tr):
    env = tr.envelope
    return [tr.waveforms, tr.solutions, tr.info, tr.scaled_residual, tr.iterations, tr.currents, tr.final_currents,
            tr.newton_iterations, tr.matrix_updates, tr.diode_voltages, tr.diode_currents, tr.final_junctions] + \
        ([env.potential_min, env.potential_min_step, env.potential_max, env.potential_max_step] if env else [])


def same_bits(one, two):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(fields(one), fields(two)))


@pytest.mark.parametrize("sparse", [False, True])
def test_without_diodes_nothing_changes(sparse):
    rows, caps, inds, _, dt, steps, sources = tn.lu_transient_case(True)
    circ = circuit_of(rows, sparse)
    kw = dict(sources=sources, probes=["1", "30"], inductors=inds, current_probes=["l1"], keep_every=2, envelope=True)
    plain = circ.transient(caps, dt, steps, **kw)
    empty = circ.transient(caps, dt, steps, diodes=(), **kw)
    assert same_bits(plain, empty) and (empty.newton_iterations == 1).all() and (empty.matrix_updates == 0).all()
    assert empty.diode_voltages.shape == (steps + 1, 0) and len(empty.final_junctions) == 0


@pytest.mark.parametrize("sparse", [False, True])
def test_a_second_identical_call_gives_the_same_bits(sparse):
    rows, caps, inds, diodes, dt, steps, sources = tn.lu_transient_case(True)
    circ = circuit_of(rows, sparse)
    kw = dict(sources=sources, probes=["1", "30"], method="trapezoidal", inductors=inds, current_probes=["l1", "l2"],
              diodes=diodes, diode_probes=["d_fwd", "d_same"], keep_every=1, envelope=True, max_iter=MAX_ITER, **TIGHT)
    one = circ.transient(caps, dt, steps, **kw)
    kept = circ._transient_child[1], circ._transient_nl_dc[1]
    two = circ.transient(caps, dt, steps, **kw)
    assert (one.info == 0).all() and same_bits(one, two)
    assert (circ._transient_child[1], circ._transient_nl_dc[1]) == kept and two.timings[1] == 0.0, two.timings
    d = kw["diode_probes"].index("d_same")  # both leads on one node: exactly nothing
    assert (one.diode_voltages[:, d] == 0.0).all() and (one.diode_currents[:, d] == 0.0).all()
    circ.set_values(circ.values)
    assert circ._transient_child is None and circ._transient_nl_dc is None


@pytest.mark.parametrize("sparse", [False, True])
def test_too_few_iterations_give_info_2_and_leave_the_circuit_usable(sparse):
    rows, caps, inds, diodes, dt, steps, sources = tn.lu_transient_case(False)
    circ = circuit_of(rows, sparse)
    x0 = circ.operating_point(diodes, max_iter=MAX_ITER, **TIGHT).x  # (a start of its own: max_iter=1 is for the steps)
    kw = dict(sources=sources, probes=["1", "30"], initial=x0, diodes=diodes, diode_probes=["d_fwd"], keep_every=1,
              envelope=True, **TIGHT)
    with pytest.warns(RuntimeWarning, match="did not converge") as caught:
        tr = circ.transient(caps, dt, steps, max_iter=1, **kw)
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == 1
    first = int(np.argmax(tr.info == 2))
    print(f"sparse {sparse}: max_iter=1: info {tr.info.tolist()}, Newton iterations {tr.newton_iterations.tolist()}")
    assert (tr.info[:first] == 0).all() and (tr.info[first:] == 2).all() and tr.newton_iterations[first] == 1
    assert (tr.newton_iterations[first + 1:] == 0).all()
    assert np.isfinite(tr.waveforms[:first + 1]).all() and np.isnan(tr.waveforms[first + 1:]).all()
    assert np.isnan(tr.solutions[first:]).all() and np.isnan(tr.scaled_residual[first:]).all()
    assert np.isnan(tr.diode_voltages[first + 1:]).all() and np.isnan(tr.final_junctions).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        after = circ.transient(caps, dt, steps, max_iter=MAX_ITER, **kw)
        fresh = circuit_of(rows, sparse).transient(caps, dt, steps, max_iter=MAX_ITER, **kw)
    assert (after.info == 0).all() and same_bits(after, fresh)


def test_a_floating_island_on_the_sparse_path_gives_info_1():
    from scipy.sparse.linalg import MatrixRankWarning
    rows = tn.nr.grid_rows(9, [("a1", 0.5, 1)], extra=[["ri", "R", "1", "isl1", "isl2"], ["ai", "A", "0", "isl1", "isl2"]])
    circ = circuit_of(rows, True)
    assert circ.table.n > 64
    caps = [("c1", 1.0, "1", "g")]
    diodes = [("d1", I_SAT, N_VT, "1", "g")]
    with pytest.warns(MatrixRankWarning):
        tr = circ.transient(caps, 0.05, 3, probes=["1"], initial=np.zeros(circ.table.n), diodes=diodes, keep_every=1,
                            max_iter=MAX_ITER, **TIGHT)
    assert (tr.info == 1).all() and np.isnan(tr.waveforms[1:]).all() and np.isnan(tr.solutions).all()
    assert np.isnan(tr.final_junctions).all()


@pytest.mark.parametrize("sparse", [False, True])
def test_the_circuit_itself_is_untouched_and_record_raises(sparse):
    rows, caps, inds, diodes, dt, steps, sources = tn.rectifier_case()
    circ = circuit_of(rows, sparse)
    before = circ.solve().result.copy()
    values = np.array(circ.table.value)
    with pytest.raises(ValueError, match="adjoint"):
        circ.transient(caps, dt, steps, sources=sources, diodes=diodes, record=True)
    tr = circ.transient(caps, dt, steps, sources=sources, diodes=diodes, max_iter=MAX_ITER, **TIGHT)
    assert (tr.info == 0).all()
    assert np.array_equal(circ._handle.download_x(), before) and np.array_equal(np.array(circ.table.value), values)
    assert circ.table.ncomp == len(values)


def test_a_dc_start_that_does_not_converge_warns_once_and_gives_info_2():
    rows, caps, inds, diodes, dt, steps, _ = tn.lu_transient_case(True)
    circ = circuit_of(rows, True)
    with pytest.warns(RuntimeWarning, match="DC start did not converge") as caught:
        tr = circ.transient(caps, dt, steps, probes=["1"], inductors=inds, current_probes=["l1"], diodes=diodes,
                            diode_probes=["d_fwd"], keep_every=1, envelope=True, max_iter=1, **TIGHT)
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning)]) == 1
    assert (tr.info == 2).all() and (tr.newton_iterations == 0).all() and (tr.matrix_updates == 0).all()
    for field in (tr.waveforms, tr.solutions, tr.scaled_residual, tr.currents, tr.final_currents, tr.diode_voltages,
                  tr.diode_currents, tr.final_junctions, tr.envelope.potential_min):
        assert np.isnan(field).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert (circ.transient(caps, dt, steps, inductors=inds, diodes=diodes, max_iter=MAX_ITER, **TIGHT).info == 0).all()


# ---- the entry itself (nodal_transient_nl) ----------------------------------------------------------------------------------
def test_the_entry_without_diodes_is_nodal_transient_rlc_and_its_arguments_are_checked():
    from nodal_amd import _ffi
    rows, caps, inds, diodes, dt, steps, sources = tn.lu_transient_case(True)
    circ = circuit_of(rows, True)
    circ.transient(caps, dt, steps, sources=sources, inductors=inds, diodes=diodes, max_iter=MAX_ITER, **TIGHT)
    _, child, cap_rows, ind_rows, diode_rows = circ._transient_child
    h = child._handle
    src = np.array([circ.netlist.component_keys.index("a1")], dtype=np.int64)
    values = np.asarray(sources["a1"], dtype=np.float64)[:, None]
    x0, i0 = np.linspace(-0.2, 0.3, h.n), np.array([0.1, -0.2])
    pa, pb, cur = np.array([0, 5], dtype=np.int32), np.array([-1, 3], dtype=np.int32), np.array([1, 0], dtype=np.int32)
    common = dict(dense=False, method=0, keep_every=1, envelope=True)
    # (the diode rows hold the last linearisation: a legal linear network, the same for both calls)
    a = h.transient_rlc(cap_rows, ind_rows, src, values, x0, i0, pa, pb, cur, **common)
    none, nothing = np.zeros(0, dtype=np.int64), np.zeros(0)
    b = h.transient_nl(cap_rows, ind_rows, none, nothing, nothing, 1e-12, src, values, x0, i0, pa, pb, cur,
                       np.zeros(0, dtype=np.int32), max_iter=MAX_ITER, **TIGHT, **common)
    for q in (0, 1, 3, 4, 5, 6, 7):
        assert np.array_equal(a[q], b[q]), q
    assert all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
    assert (b[8]["newton"] == 1).all() and (b[8]["updates"] == 0).all()
    _, i_sat, n_vt, _, _ = resolve_diodes(circ.netlist, diodes)
    D = len(diodes)

    def call(rows_=diode_rows, sat=i_sat, nvt=n_vt, probe=(0,), max_iter=MAX_ITER, reltol=1e-3):
        return h.transient_nl(cap_rows, ind_rows, rows_, sat, nvt, 1e-12, src, values, x0, i0, pa, pb, cur,
                              np.asarray(probe, dtype=np.int32), max_iter=max_iter, reltol=reltol, vntol=1e-6, abstol=1e-12,
                              **common)

    bad_rows = diode_rows.copy()
    bad_rows[0] = src[0]  # an A row: not a resistor
    far_rows = diode_rows.copy()
    far_rows[0] = child.table.ncomp
    for kw in (dict(rows_=bad_rows), dict(rows_=far_rows), dict(sat=np.where(np.arange(D) == 1, 0.0, i_sat)),
               dict(nvt=np.where(np.arange(D) == 2, np.inf, n_vt)), dict(probe=(D,)), dict(probe=(-1,)), dict(max_iter=0),
               dict(reltol=-1.0)):
        with pytest.raises(_ffi.NodalHipError) as exc:
            call(**kw)
        assert exc.value.status == _ffi.E_INVALID, kw
    assert (call()[4] == 0).all()  # (and the handle is usable afterwards)
