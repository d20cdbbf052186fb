"""tests/transient_nl_reference.py held to a closed form, to itself (two linear solves per Newton step), to convergence on
every input of tests/test_gpu_transient_diodes.py within the max_iter that file passes, and to planted defects that its
two checks must catch.  No device."""
import numpy as np
import pytest

from tests import transient_nl_reference as tn
from tests.transient_nl_reference import I_SAT, N_VT, TIGHT, TOL, TransientDiodeReference

MAX_ITER = 50  # what the GPU tests pass


def test_the_reference_meets_the_closed_form_of_a_capacitor_discharging_into_a_diode():
    C, h, steps = 1e-3, 1e-4, 5
    ref = TransientDiodeReference(tn.rc_diode_rows(), [("c1", C, "1", "g")], [], [("d1", I_SAT, N_VT, "1", "g")], h, "euler",
                                  gmin=0.0, max_iter=MAX_ITER, **TIGHT)
    A = ref.rhs_steps({}, steps)
    X, _, its = ref.run(np.array([0.7]), np.zeros(0), A, both=True)
    v = tn.rc_diode_closed_form(0.7, C, I_SAT, N_VT, h, steps)
    # the closed form satisfies the step equation to the rounding of v itself: C / h = 10 A/V times a few ulps of 0.7 V
    step_defect = np.abs(C * np.diff(v) / h + I_SAT * np.expm1(v[1:] / N_VT))
    assert (step_defect <= 4 * (C / h) * np.spacing(0.7)).all(), step_defect
    print("closed form", v, "reference", X[:, 0], "iterations", its)
    assert ref.unconverged == 0 and (np.abs(X[:, 0] - v) <= 2 * TOL / 1000 * np.abs(v)).all()
    assert ref.newton.worst_disagreement <= TOL / 1000
    assert ref.parity(X, np.zeros(0), A)[0] <= 0.0 and ref.residual_excess(X, np.zeros(0), A)[0] <= 0.0


def _converges(case, method, both, label):
    rows, caps, inds, diodes, dt, steps, sources = case
    ref = TransientDiodeReference(rows, caps, inds, diodes, dt, method, max_iter=MAX_ITER, **TIGHT)
    x0, i0, dc_its = ref.dc_start()
    A = ref.rhs_steps(sources, steps)
    X, I, its = ref.run(x0, i0, A, both=both)
    print(f"{label} {method}: DC start {dc_its} iterations, steps {its.tolist()}, highest junction {ref.highest_junction:.3f} V, "
          f"two solves disagree by {ref.newton.worst_disagreement:.2e}")
    assert dc_its <= MAX_ITER and ref.unconverged == 0 and (its <= MAX_ITER).all()
    if both:
        assert ref.newton.worst_disagreement <= TOL / 1000
    excess, rel, _, _ = ref.parity(X, i0, A)
    rexcess, worst = ref.residual_excess(X, i0, A)
    print(f"{label} {method}: the reference against its own checks: parity {rel:.2e}, residual {worst:.2e}")
    assert excess <= 0.0 and rexcess <= 0.0
    return ref


@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
def test_the_rectifier_converges_in_every_step(method):
    _converges(tn.rectifier_case(), method, True, "rectifier")


@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
@pytest.mark.parametrize("with_inductors", [False, True])
def test_the_sparse_lu_case_converges_in_every_step(method, with_inductors):
    _converges(tn.lu_transient_case(with_inductors), method, True, f"lu, inductors {with_inductors}")


@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
def test_the_multigrid_case_converges_in_every_step(method):
    _converges(tn.mg_transient_case(), method, False, "mg")


@pytest.mark.parametrize("size", [4, 12])
def test_the_clamps_at_rest_stay_below_minus_two_volts_in_every_iterate(size):
    ref = _converges(tn.reuse_case(size), "euler", True, f"reuse({size})")
    assert ref.highest_junction <= -2.0
    # ... where 1 / g has the bits of 1 / gmin: the matrix does not move
    g = ref.newton.conductance(np.full(len(ref.newton.i_sat), ref.highest_junction))
    assert (g == ref.gmin).all()
    assert ref.n == (17 if size == 4 else 145)


@pytest.fixture(scope="module")
def planted():
    rows, caps, inds, diodes, dt, steps, sources = tn.lu_transient_case(with_inductors=True)
    ref = TransientDiodeReference(rows, caps, inds, diodes, dt, "euler", max_iter=MAX_ITER, **TIGHT)
    x0, i0, _ = ref.dc_start()
    return ref, x0, i0, ref.rhs_steps(sources, steps)


def test_the_checks_pass_on_the_clean_run(planted):
    ref, x0, i0, A = planted
    X, _, _ = ref.run(x0, i0, A)
    assert ref.parity(X, i0, A)[0] <= 0.0 and ref.residual_excess(X, i0, A)[0] <= 0.0


@pytest.mark.parametrize("defect", tn.DEFECTS)
def test_the_checks_fail_on_a_planted_defect(planted, defect):
    ref, x0, i0, A = planted
    X, _, its = ref.run(x0, i0, A, defect=defect)
    excess, rel, _, _ = ref.parity(X, i0, A)
    rexcess, worst = ref.residual_excess(X, i0, A)
    print(f"{defect}: iterations {its.tolist()}, parity error {rel:.2e}, residual {worst:.2e}")
    assert np.isfinite(X).all()
    assert excess > 0.0 and rexcess > 0.0
