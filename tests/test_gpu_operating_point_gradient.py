"""OperatingPoint.gradient (nodal_newton_gradient) on the device against the fp64 reference of
tests/operating_point_gradient_reference.py, evaluated at the DEVICE's own op.x: closed forms and a transposed child on
the dense-panel route, a grid with an E source on the sparse LU route, the same with a VCVS and a CCCS row (J not
symmetric), a 66 x 66 grid on the multigrid route; the contracts (same bits twice, no symbolic work the second time, the
circuit and the next operating_point untouched), the failure paths, and autograd.operating_point.

Every comparison with the reference is within the propagated bars of that module (worst_ratio <= 1): TOL normwise in
lambda and x through each formula plus 8 eps of its scale.  The operating points are found with TIGHT tolerances, so
that x is the operating point to roundoff (operating_point_residual <= RESID_BAR says so)."""
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd.operating_point import OperatingPoint
from tests import newton_reference as nr
from tests import operating_point_gradient_reference as og
from tests.newton_reference import I_SAT, N_VT, RESID_BAR, TIGHT, TOL, NewtonReference
from tests.test_operating_point_gradient_reference import FD_BAR

pytestmark = pytest.mark.gpu


def circuit_of(rows, sparse):
    return n.Circuit(n.Netlist.from_rows([list(r) for r in rows]), sparse=sparse, device=0)


def cotangent_of(size, seed=7):
    return np.random.default_rng(seed).standard_normal(size)


def check_against_reference(ref, op, grad, cot, label="", named=()):
    """the device's gradient against the reference evaluated at the device's own x; returns the reference's dict"""
    want = og.gradient(ref, op.x, cot)
    bars = want["bars"]
    ratios = {"values": og.worst_ratio(grad.values, want["values"], bars["values"]),
              "i_sat": og.worst_ratio(grad.i_sat, want["i_sat"], bars["i_sat"]),
              "n_vt": og.worst_ratio(grad.n_vt, want["n_vt"], bars["n_vt"]),
              "gmin": og.worst_ratio(grad.gmin, want["gmin"], bars["gmin"])}
    for name in named:
        ratios["source " + name] = og.worst_ratio(grad.source_values[name], want["sources"][name], bars["sources"][name])
    adjoint = np.abs(grad.adjoint - want["adjoint"]).max() / np.abs(want["adjoint"]).max()
    print(f"{label}: worst ratios {({k: float(f'{v:.2e}') for k, v in ratios.items()})}, adjoint {adjoint:.2e} normwise, "
          f"scaled residual {grad.scaled_residual:.2e}, operating-point residual {grad.operating_point_residual:.2e}, "
          f"timings {grad.timings}")
    assert grad.info == 0 and set(grad.source_values) == set(named)
    assert max(ratios.values()) <= 1.0, ratios
    assert adjoint <= TOL
    assert grad.scaled_residual <= 1e-12 and grad.operating_point_residual <= RESID_BAR
    assert len(grad.values) == len(ref.nl.component_keys)
    return want


def same_bits(g1, g2):
    return (np.array_equal(g1.values, g2.values) and np.array_equal(g1.i_sat, g2.i_sat) and np.array_equal(g1.n_vt, g2.n_vt)
            and g1.gmin == g2.gmin and g1.source_values == g2.source_values and np.array_equal(g1.adjoint, g2.adjoint)
            and g1.scaled_residual == g2.scaled_residual and g1.operating_point_residual == g2.operating_point_residual
            and g1.info == g2.info)


def run_and_check(circ, ref, diodes, cot, initial=None, sources=None, label="", solvable=True):
    """an operating point, its gradient and every contract of the file; returns (op, gradient, the reference's dict)"""
    before = circ.solve().result.copy() if solvable else None
    table = {name: np.array(getattr(circ.table, name)) for name in ("type", "value", "a", "b")}
    G, A = circ.G, circ.A
    G, A = (G.toarray() if hasattr(G, "toarray") else np.array(G)), np.array(A.toarray() if hasattr(A, "toarray") else A)
    op = circ.operating_point(diodes, sources=sources, initial=initial, **TIGHT)
    assert op.converged
    grad = op.gradient(cot, adjoints=True)
    want = check_against_reference(ref, op, grad, cot, label, named=tuple(sources or ()))
    # a second identical call: the same bits in every output, and no symbolic work
    again = op.gradient(cot, adjoints=True)
    assert same_bits(grad, again) and again.timings[1] == 0.0, again.timings
    assert op.gradient(cot).adjoint is None
    # operating_point after a gradient: the bits it returned before
    op2 = circ.operating_point(diodes, sources=sources, initial=initial, **TIGHT)
    assert np.array_equal(op2.x, op.x) and np.array_equal(op2.history.record, op.history.record)
    assert np.array_equal(op2.currents, op.currents) and op2.timings[1] == 0.0
    # the circuit itself is left as it was: its solution, table, G and A
    if solvable:
        assert np.array_equal(circ._handle.download_x(), before)
    for name, column in table.items():
        assert np.array_equal(np.array(getattr(circ.table, name)), column)
    circ._G = circ._A = None  # (exported anew from the device)
    G2, A2 = circ.G, circ.A
    assert np.array_equal(G2.toarray() if hasattr(G2, "toarray") else np.array(G2), G)
    assert np.array_equal(np.array(A2.toarray() if hasattr(A2, "toarray") else A2), A)
    return op, grad, want


# ---- the dense panel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("amps", [1e-6, 1.0])
def test_a_source_into_a_diode_meets_the_closed_forms(amps, sparse):
    rows, diodes = nr.source_diode_rows(amps), [("d1", I_SAT, N_VT, "1", "g")]
    ref = NewtonReference(rows, diodes, gmin=0.0, sources={"a1": amps}, **TIGHT)
    circ = circuit_of(rows, sparse)
    op = circ.operating_point(diodes, sources={"a1": amps}, gmin=0.0, **TIGHT)
    assert op.converged and set(op.history.route) == {"dense"}
    grad = op.gradient(np.ones(1), adjoints=True)
    want = check_against_reference(ref, op, grad, np.ones(1), f"I = {amps:g}, sparse {sparse}", named=("a1",))
    # the closed forms, L = v; x is the operating point to roundoff (TIGHT), so the reference's bars hold against them too
    dI, dsat, dnvt = og.source_diode_closed_forms(amps, I_SAT, N_VT)
    bars = want["bars"]
    print(f"I = {amps:g}: dL/dI {grad.source_values['a1']!r} / {dI!r}, dL/di_sat {grad.i_sat[0]!r} / {dsat!r}, "
          f"dL/dn_vt {grad.n_vt[0]!r} / {dnvt!r}")
    assert abs(grad.source_values["a1"] - dI) <= bars["sources"]["a1"]
    assert abs(grad.i_sat[0] - dsat) <= bars["i_sat"][0] and abs(grad.n_vt[0] - dnvt) <= bars["n_vt"][0]
    assert grad.of("d1") == (grad.i_sat[0], grad.n_vt[0]) and grad.of("a1") == grad.values[0]
    assert grad.values[0] == grad.source_values["a1"]  # (an A row's formula reads neither x nor the value)


@pytest.mark.parametrize("sparse", [False, True])
def test_a_source_behind_a_resistor_on_the_transposed_child(sparse):
    rows, diodes = nr.series_rows(5.0, 1000.0), [("d1", I_SAT, N_VT, "2", "g")]
    circ = circuit_of(rows, sparse)
    assert circ.table.B == 1 and circ.table.n == 3
    cot = cotangent_of(3)
    op, grad, _ = run_and_check(circ, NewtonReference(rows, diodes, **TIGHT), diodes, cot, label=f"E-R-diode, sparse {sparse}")
    assert set(op.history.route) == {"dense"}
    normalized = grad.normalized
    assert np.array_equal(normalized[0], grad.values * np.array(circ.table.value))
    assert normalized[1][0] == grad.i_sat[0] * I_SAT and normalized[2][0] == grad.n_vt[0] * N_VT
    # another operating_point call with other leads re-keys the companion child; the first result's gradient still works
    other = circ.operating_point([("dx", I_SAT, N_VT, "1", "g"), ("dy", 2 * I_SAT, N_VT, "2", "1")], **TIGHT)
    assert other.converged
    assert same_bits(op.gradient(cot, adjoints=True), grad)


# ---- the sparse LU route -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lu_inputs():
    rows, diodes, initial = nr.lu_case()
    return rows, diodes, initial, NewtonReference(rows, diodes, **TIGHT)


@pytest.mark.parametrize("sparse", [False, True])
def test_the_sparse_lu_route(lu_inputs, sparse):
    rows, diodes, initial, ref = lu_inputs
    circ = circuit_of(rows, sparse)
    assert circ.table.B == 1 and circ.table.K == 144
    op, grad, _ = run_and_check(circ, ref, diodes, cotangent_of(145), initial=initial, label=f"grid(12) + E, sparse {sparse}")
    assert set(op.history.route) <= {"lu", "direct"}
    d = op.diodes.index("d_same")  # both leads on one node: exactly nothing
    assert grad.i_sat[d] == 0.0 and grad.n_vt[d] == 0.0 and grad.of("d_same") == (0.0, 0.0)


def test_named_sources_get_their_derivatives(lu_inputs):
    rows, diodes, initial, _ = lu_inputs
    sources = {"e1": 3.5, "a2": -0.2}
    circ = circuit_of(rows, True)
    ref = NewtonReference(rows, diodes, sources=sources, **TIGHT)
    _, grad, want = run_and_check(circ, ref, diodes, cotangent_of(145, seed=8), initial=initial, sources=sources,
                                  label="grid(12) + E, e1 and a2 named")
    keys = list(circ.netlist.component_keys)
    for name in sources:  # (an A or E row's formula reads neither x nor the value: the row holds the same number)
        assert grad.source_values[name] == grad.values[keys.index(name)] == grad.of(name)


def test_without_symmetry_the_cross_term_lands_on_the_driver():
    rows, diodes, initial = og.nonsymmetric_case()
    ref = NewtonReference(rows, diodes, **TIGHT)
    circ = circuit_of(rows, True)
    op, grad, want = run_and_check(circ, ref, diodes, cotangent_of(ref.n), initial=initial, label="grid(12) + E + VCVS + CCCS")
    J = ref.jacobian(op.x)
    assert abs(J - J.T).max() > 0.1
    keys = list(circ.netlist.component_keys)
    at = keys.index("rh0_4")
    a, b, r = int(circ.table.a[at]), int(circ.table.b[at]), float(circ.table.value[at])
    lam, x = np.append(grad.adjoint, 0.0), np.append(op.x, 0.0)
    plain = (lam[a] - lam[b]) * (x[a] - x[b]) / r ** 2  # the R formula alone, without the CCCS row's term
    bar = want["bars"]["values"][at]
    print(f"rh0_4: {grad.values[at]!r}, reference {want['values'][at]!r}, without the cross term {plain!r}, bar {bar:.2e}")
    assert abs(grad.values[at] - want["values"][at]) <= bar < 1e-3 * abs(grad.values[at] - plain)


# ---- the multigrid route -------------------------------------------------------------------------------------------------
def test_the_multigrid_route():
    rows, diodes = nr.mg_case()
    ref = NewtonReference(rows, diodes, **TIGHT)
    circ = circuit_of(rows, True)
    assert circ.table.B == 0 and circ.table.K == 4355
    op, grad, _ = run_and_check(circ, ref, diodes, cotangent_of(4355), label="grid(66)")
    assert set(op.history.route) <= {"multigrid", "direct"} and "multigrid" in op.history.route
    assert grad.timings[1] == 0.0  # (the hierarchy's symbolic setup was the operating point's)


# ---- contracts -----------------------------------------------------------------------------------------------------------
def test_a_unit_cotangent_is_the_small_signal_sensitivity_of_the_source_rows(lu_inputs):
    """dL/d(source value) is lambda alone, and lambda solves the same transposed system as the adjoint of the ("e", node)
    output of the linearised circuit.  That holds ONLY for the rows whose formula does not read x -- the A and E rows:
    a resistor's formula multiplies lambda by x, and the linearised circuit's x is the last Newton step without the
    history currents, not the operating point."""
    rows, diodes, initial, ref = lu_inputs
    circ = circuit_of(rows, True)
    op = circ.operating_point(diodes, initial=initial, **TIGHT)
    node = "40"
    cot = np.zeros(145)
    cot[circ.netlist.nodenum[node]] = 1.0
    grad = op.gradient(cot)
    small = op.linearised()
    small.solve()
    sens = np.asarray(small.sensitivities([("e", node)]).values)[0]
    bars = og.gradient(ref, op.x, cot)["bars"]["values"]
    ty = np.asarray(circ.table.type)
    source_rows = np.flatnonzero((ty == n.constants.TYPE_CODE["A"]) | (ty == n.constants.TYPE_CODE["E"]))
    assert len(source_rows) == 3
    for i in source_rows:
        print(f"row {i}: gradient {grad.values[i]!r}, sensitivity of the linearised circuit {sens[i]!r}, bar {bars[i]:.2e}")
        assert abs(grad.values[i] - sens[i]) <= 2 * bars[i]  # (each of the two within its bar of the reference)
    resistors = np.flatnonzero(ty == n.constants.TYPE_CODE["R"])
    assert (np.abs(grad.values[resistors] - sens[resistors]) > 2 * bars[resistors]).any()


def test_without_diodes_it_is_the_linear_gradient(lu_inputs):
    rows = lu_inputs[0]
    circ = circuit_of(rows, True)
    cot = cotangent_of(145, seed=9)
    op = circ.operating_point([], **TIGHT)
    grad = op.gradient(cot, adjoints=True)
    ref = NewtonReference(rows, [], **TIGHT)
    want = check_against_reference(ref, op, grad, cot, "no diodes")
    linear = circ.gradient(cot, solutions=op.x)
    assert og.worst_ratio(linear.values, want["values"], want["bars"]["values"]) <= 1.0
    assert len(grad.i_sat) == 0 and len(grad.n_vt) == 0 and grad.gmin == 0.0


# ---- failure paths that fault nothing -----------------------------------------------------------------------------------
def test_an_x_that_is_no_operating_point_shows_in_its_residual(lu_inputs):
    rows, diodes, initial, _ = lu_inputs
    circ = circuit_of(rows, True)
    op = circ.operating_point(diodes, initial=initial, **TIGHT)
    _, child, diode_rows = circ._newton_child
    call = (diode_rows, op.i_sat, op.n_vt, op.gmin, op.source_rows, op.source_values)
    cot = cotangent_of(145)
    good = child._handle.newton_gradient(*call, op.x, cot, dense=False)
    bad = child._handle.newton_gradient(*call, op.x * 1.5, cot, dense=False)
    print(f"operating-point residual: {good['op_resid']:.2e} at op.x, {bad['op_resid']:.2e} at 1.5 op.x")
    assert good["op_resid"] <= RESID_BAR < bad["op_resid"]
    assert bad["info"] == 0 and (good["grad"][diode_rows] == 0.0).all() and not np.signbit(good["grad"][diode_rows]).any()
    # values that moved since the operating point was found show there too, through the public interface
    values = np.array(circ.values)
    values[list(circ.netlist.component_keys).index("rs")] *= 1.5
    circ.set_values(values)
    moved = op.gradient(cot)
    assert moved.operating_point_residual > RESID_BAR and moved.info == 0


@pytest.mark.parametrize("sparse", [False, True])
def test_a_singular_jacobian(sparse):
    """node 2 hangs on a diode alone; with gmin = 0 and 30 V of reverse bias exp(-30 / n_vt) underflows and g is exactly
    0: node 2 floats in J"""
    from scipy.sparse.linalg import MatrixRankWarning
    rows = [["a1", "A", "1", "1", "g"], ["r1", "R", "1", "1", "g"], ["a2", "A", "0", "2", "g"]]
    diodes = [("d1", I_SAT, N_VT, "2", "1")]
    circ = circuit_of(rows, sparse)
    op = circ.operating_point(diodes, **TIGHT)
    assert op.converged
    x = op.x.copy()
    x[circ.netlist.nodenum["2"]] = x[circ.netlist.nodenum["1"]] - 30.0
    floating = OperatingPoint(x, op.diodes, op.voltages, op.currents, op.conductances, True, 1, op.history, circuit=circ,
                              leads=op._leads, i_sat=op.i_sat, n_vt=op.n_vt, gmin=0.0, source_rows=op.source_rows,
                              source_values=op.source_values, source_columns=op.source_columns)
    if sparse:
        with pytest.warns(MatrixRankWarning) as caught:
            grad = floating.gradient(np.ones(2), adjoints=True)
        assert len([w for w in caught if issubclass(w.category, MatrixRankWarning)]) == 1
        assert grad.info > 0 and np.isnan(grad.values).all() and np.isnan(grad.i_sat).all() and np.isnan(grad.n_vt).all()
        assert np.isnan(grad.gmin) and np.isnan(grad.adjoint).all() and np.isnan(grad.scaled_residual)
        assert np.isfinite(grad.operating_point_residual)
    else:
        with pytest.raises((np.linalg.LinAlgError, n.UnconnectedCircuitError)):
            floating.gradient(np.ones(2))
    # the circuit and its child stay usable
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        grad = op.gradient(np.ones(2), adjoints=True)
    check_against_reference(NewtonReference(rows, diodes, **TIGHT), op, grad, np.ones(2), "after the singular call")


@pytest.mark.parametrize("sparse", [False, True])
def test_a_conductance_that_overflows(sparse):
    """100 V across a junction: exp(100 / n_vt) is inf, 1 / g is 0 -- the assembly reports it; every output is NaN with
    info 0, and the child stays usable"""
    rows, diodes = [["a1", "A", "1", "1", "g"], ["r1", "R", "1", "1", "g"]], [("d1", I_SAT, N_VT, "1", "g")]
    circ = circuit_of(rows, sparse)
    op = circ.operating_point(diodes, **TIGHT)
    _, child, diode_rows = circ._newton_child
    r = child._handle.newton_gradient(diode_rows, op.i_sat, op.n_vt, op.gmin, op.source_rows, op.source_values,
                                      np.array([100.0]), np.ones(1), dense=not sparse, adjoints=True)
    assert r["info"] == 0 and np.isnan(r["grad"]).all() and np.isnan(r["i_sat"]).all() and np.isnan(r["n_vt"]).all()
    assert np.isnan(r["gmin"]) and np.isnan(r["adjoint"]).all() and np.isnan(r["resid"]) and np.isnan(r["op_resid"])
    op2 = circ.operating_point(diodes, **TIGHT)
    assert np.array_equal(op2.x, op.x)
    check_against_reference(NewtonReference(rows, diodes, **TIGHT), op2, op2.gradient(np.ones(1), adjoints=True), np.ones(1),
                            f"after the overflow, sparse {sparse}")


def test_the_argument_checks_of_the_library(lu_inputs):
    from nodal_amd import _ffi
    rows, diodes, initial, _ = lu_inputs
    circ = circuit_of(rows, True)
    op = circ.operating_point(diodes, initial=initial, **TIGHT)
    _, child, diode_rows = circ._newton_child
    h, cot = child._handle, cotangent_of(145)
    none, keys = np.zeros(0, dtype=np.int64), list(circ.netlist.component_keys)
    not_r = diode_rows.copy()
    not_r[0] = keys.index("a1")
    far = diode_rows.copy()
    far[-1] = 10 ** 6
    resistor = np.array([keys.index("rs"), keys.index("rs")])
    for label, call in (("a diode row out of range", (far, op.i_sat, op.n_vt, 1e-12, none, np.zeros(0))),
                        ("a diode row that is not an R", (not_r, op.i_sat, op.n_vt, 1e-12, none, np.zeros(0))),
                        ("i_sat not positive", (diode_rows, -op.i_sat, op.n_vt, 1e-12, none, np.zeros(0))),
                        ("n_vt not finite", (diode_rows, op.i_sat, op.n_vt * np.inf, 1e-12, none, np.zeros(0))),
                        ("gmin negative", (diode_rows, op.i_sat, op.n_vt, -1.0, none, np.zeros(0))),
                        ("a source row that is a resistor", (diode_rows, op.i_sat, op.n_vt, 1e-12, resistor[:1], np.zeros(1))),
                        ("a source row named twice", (diode_rows, op.i_sat, op.n_vt, 1e-12,
                                                      np.array([keys.index("a1")] * 2), np.zeros(2)))):
        with pytest.raises(_ffi.NodalHipError) as caught:
            h.newton_gradient(*call, op.x, cot, dense=False)
        assert caught.value.status == _ffi.E_INVALID, label
    # and the handle is still good
    assert same_bits(op.gradient(cot, adjoints=True), op.gradient(cot, adjoints=True))


# ---- autograd ------------------------------------------------------------------------------------------------------------
def test_autograd_operating_point():
    import torch
    from nodal_amd import autograd
    rows, leads = nr.series_rows(5.0, 1000.0), [("d1", "2", "g")]
    circ = circuit_of(rows, True)
    node = circ.netlist.nodenum["2"]
    keys = list(circ.netlist.component_keys)

    def run(values, i_sat, n_vt, volts):
        return autograd.operating_point(circ, values, leads, i_sat, n_vt, source_names=("e1",), source_values=volts, **TIGHT)

    def leaves(e=5.0, r=1000.0, log_sat=np.log(I_SAT), nvt=N_VT):
        values = torch.tensor(np.array(circ.values), dtype=torch.float64)
        values[keys.index("r1")] = r
        log_sat = torch.tensor([log_sat], dtype=torch.float64, requires_grad=True)
        return (values.requires_grad_(True), log_sat, torch.tensor([nvt], dtype=torch.float64, requires_grad=True),
                torch.tensor([e], dtype=torch.float64, requires_grad=True))

    values, log_sat, nvt, volts = leaves()
    i_sat = torch.exp(log_sat).detach().requires_grad_(True)
    x = run(values, i_sat, nvt, volts)
    got = torch.autograd.grad(x[node], (values, i_sat, nvt, volts))
    # bit for bit the gradient object's numbers
    op = circ.operating_point([("d1", float(i_sat.detach()[0]), N_VT, "2", "g")], sources={"e1": 5.0}, **TIGHT)
    cot = np.zeros(3)
    cot[node] = 1.0
    grad = op.gradient(cot)
    expected = grad.values.copy()
    expected[keys.index("e1")] = 0.0  # (the run does not use the table value of a named source)
    assert np.array_equal(got[0].numpy(), expected) and np.array_equal(got[1].numpy(), grad.i_sat)
    assert np.array_equal(got[2].numpy(), grad.n_vt) and got[3].numpy().tolist() == [grad.source_values["e1"]]

    # central differences through the device's own forward pass, relative step 1e-6, at the bar of the CPU test
    def forward(**changed):
        v, ls, nv, e = leaves(**changed)
        with torch.no_grad():
            return float(run(v, torch.exp(ls), nv, e)[node])

    step = 1e-6
    checks = {"E": (float(got[3][0]), "e", 5.0), "R": (float(got[0][keys.index("r1")]), "r", 1000.0),
              "n_vt": (float(got[2][0]), "nvt", N_VT),
              "log i_sat": (float(got[1][0]) * float(i_sat.detach()[0]), "log_sat", float(np.log(I_SAT)))}
    for label, (adjoint, key, p) in checks.items():
        h = step * abs(p)
        fd = (forward(**{key: p + h}) - forward(**{key: p - h})) / (2 * h)
        print(f"d x[2] / d {label}: adjoint {adjoint!r}, central difference {fd!r}, relative {abs(adjoint - fd) / abs(fd):.1e}")
        assert abs(adjoint - fd) <= FD_BAR * abs(fd)
