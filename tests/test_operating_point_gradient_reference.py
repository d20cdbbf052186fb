"""tests/operating_point_gradient_reference.py held to closed forms and to central differences of the reference's own
tightly converged Newton run (no GPU): finite differences are what the reference is held to, and only where they can
decide; the reference adjoint is what the device is held to (tests/test_gpu_operating_point_gradient.py).

The central differences: newton_reference.lu_case() (n = 145, 13 diodes), L = c . x with a seeded normal c, relative step
1e-6 in the parameter, each side run with TIGHT tolerances and polished (nonlinear residual 2.3e-16 of its scale).
Compared are the conducting diodes (d_fwd, d_hard: i_sat and n_vt), rs, two grid resistors, a1, a2, e1 -- for a
reverse-biased diode a central difference in i_sat is below its own noise -- and, in a second run at gmin = 1e-2 where a
relative step in gmin moves L by more than its rounding, gmin as well.  Measured while this file was written, the largest
relative difference: 9.4e-8 on lu_case (rh0_0), 1.4e-7 at gmin = 1e-2 (rv5_5; gmin itself 1.2e-7), 1.3e-7 on
nonsymmetric_case() (f1).  FD_MEASURED is the largest of them, 1.4e-7, and FD_BAR ten times that, 1.4e-6.

Every planted defect misses FD_BAR on at least one parameter or misses the closed forms.  "no_transpose" shows on
nonsymmetric_case() (one VCVS and one CCCS row: J is not symmetric; the reference's Newton still converges on it),
"gmin_dropped_from_g" at gmin = 1e-2, "jacobian_at_last_vh" with the default (loose) Newton tolerances: there the
CORRECT reference at the loose x is outside FD_BAR of the central difference around the polished point as well, and inside
it after polishing -- the x of a converged run is only reltol-close to the operating point, and a J taken one step
behind is worse by the step's length: the documented reason nodal_newton_gradient re-linearises at x, and the reason a
caller who wants the fourth digit tightens the tolerances.
"""
import numpy as np
import pytest

from tests import newton_reference as nr
from tests import operating_point_gradient_reference as og
from tests.newton_reference import I_SAT, N_VT, TIGHT, NewtonReference

FD_MEASURED = 1.4e-7
FD_BAR = 10 * FD_MEASURED
DECIDABLE = [("i_sat", "d_fwd"), ("n_vt", "d_fwd"), ("i_sat", "d_hard"), ("n_vt", "d_hard"), ("value", "rs"),
             ("value", "rh0_0"), ("value", "rv5_5"), ("value", "a1"), ("value", "a2"), ("value", "e1")]
# nonsymmetric_case(): d_hard barely conducts there (its derivative is fifty times smaller: below the quotient's noise);
# the driver of the CCCS row, the two controlled sources and what stays decidable
DECIDABLE_NONSYMMETRIC = [("i_sat", "d_fwd"), ("n_vt", "d_fwd"), ("value", "rs"), ("value", "rh0_4"), ("value", "v1"),
                          ("value", "f1"), ("value", "a1"), ("value", "a2"), ("value", "e1")]
GMIN_LARGE = 1e-2


class Case:
    """a case at its polished operating point, the seeded cotangent and the central differences of its parameters"""

    def __init__(self, rows, diodes, initial, gmin, params, seed=7):
        self.rows, self.diodes, self.gmin, self.params = rows, diodes, gmin, params
        self.ref = NewtonReference(rows, diodes, gmin=gmin, **TIGHT)
        run = self.ref.run(initial)
        assert run["converged"]
        self.x = og.polish(self.ref, run["x"])
        res, scale = self.ref.residual(self.x)
        assert np.abs(res).max() <= 4e-16 * scale.max()
        self.cot = np.random.default_rng(seed).standard_normal(self.ref.n)
        self.keys = list(self.ref.nl.component_keys)
        self.fd = {p: og.central_difference(rows, diodes, gmin, p[0], p[1], self.cot, self.x) for p in params}

    def differences(self, grad, label=""):
        """relative difference from the central difference, per parameter"""
        out = {}
        for p in self.params:
            got = og.lookup(grad, p[0], p[1], self.ref.names, self.keys)
            out[p] = abs(got - self.fd[p]) / abs(self.fd[p])
            print(f"{label} {p[0]:6s} {p[1]:8s} adjoint {got: .9e}  central difference {self.fd[p]: .9e}  relative {out[p]:.1e}")
        return out


@pytest.fixture(scope="module")
def lu():
    rows, diodes, initial = nr.lu_case()
    return Case(rows, diodes, initial, 1e-12, DECIDABLE)


@pytest.fixture(scope="module")
def lu_large_gmin():
    rows, diodes, initial = nr.lu_case()
    return Case(rows, diodes, initial, GMIN_LARGE, DECIDABLE + [("gmin", "")])


@pytest.fixture(scope="module")
def nonsymmetric():
    rows, diodes, initial = og.nonsymmetric_case()
    return Case(rows, diodes, initial, 1e-12, DECIDABLE_NONSYMMETRIC)


# ---- closed forms ---------------------------------------------------------------------------------------------------
def closed_form_errors(amps, defect=None):
    """relative errors of (dL/dI, dL/di_sat, dL/dn_vt) for one source into one diode, gmin = 0, L = v"""
    rows, diodes = nr.source_diode_rows(amps), [("d1", I_SAT, N_VT, "1", "g")]
    ref = NewtonReference(rows, diodes, gmin=0.0, **TIGHT)
    run = ref.run()
    assert run["converged"]
    x = og.polish(ref, run["x"])
    grad = og.gradient(ref, x, np.ones(1), defect=defect, last_vh=run["vh"][-2])
    want = og.source_diode_closed_forms(amps, I_SAT, N_VT)
    got = (grad["sources"]["a1"], grad["i_sat"][0], grad["n_vt"][0])
    assert grad["companion"][0] == 0.0 or defect == "diode_rows_kept"
    return [abs(g - w) / abs(w) for g, w in zip(got, want)], grad


@pytest.mark.parametrize("amps", [1e-9, 1e-6, 1e-3, 1.0])
def test_the_reference_meets_the_closed_forms(amps):
    errors, grad = closed_form_errors(amps)
    print(f"I = {amps:g}: relative errors of dL/dI, dL/di_sat, dL/dn_vt: {errors}")
    # v = n_vt log1p(I / i_sat) carries eps |v| / n_vt = 30 eps relative into exp(v / n_vt): a few hundred eps in all
    assert max(errors) <= 1e-13
    # (and dL/dgmin = -lambda v = -dL/dI v, v the closed form of newton_reference)
    want = -og.source_diode_closed_forms(amps, I_SAT, N_VT)[0] * nr.source_diode_closed_form(amps, I_SAT, N_VT)
    assert abs(grad["gmin"] - want) <= 1e-13 * abs(want)


# ---- central differences --------------------------------------------------------------------------------------------
def test_the_reference_meets_central_differences(lu):
    worst = max(lu.differences(og.gradient(lu.ref, lu.x, lu.cot), "lu_case").values())
    print(f"lu_case: largest relative difference {worst:.2e} (measured {FD_MEASURED:g} when the bar was set, bar {FD_BAR:g})")
    assert worst <= FD_BAR


def test_the_reference_meets_central_differences_in_gmin(lu_large_gmin):
    case = lu_large_gmin
    worst = max(case.differences(og.gradient(case.ref, case.x, case.cot), f"gmin {GMIN_LARGE:g}").values())
    assert worst <= FD_BAR


def test_the_reference_meets_central_differences_without_symmetry(nonsymmetric):
    case = nonsymmetric
    J = case.ref.jacobian(case.x)
    assert abs(J - J.T).max() > 0.1  # (really not symmetric)
    grad = og.gradient(case.ref, case.x, case.cot)
    worst = max(case.differences(grad, "nonsymmetric").values())
    assert worst <= FD_BAR
    # the cross term of the CCCS row lands on its driving resistor: without it rh0_4 is off
    at = case.keys.index("rh0_4")
    table, _ = og.companion_table(case.ref, case.ref.conductance(case.ref.voltages(case.x)))
    a, b = int(table.a[at]), int(table.b[at])
    lam, x = np.append(grad["adjoint"], 0.0), np.append(case.x, 0.0)
    plain = (lam[a] - lam[b]) * (x[a] - x[b]) / table.value[at] ** 2
    assert abs(plain - case.fd[("value", "rh0_4")]) > 100 * FD_BAR * abs(case.fd[("value", "rh0_4")])


def test_companion_rows_are_not_parameters(lu):
    """the companion rows' table value is overwritten before every assembly: the reference's run does not even read it,
    so every difference quotient in it is exactly zero, and so is the reference gradient"""
    assert (og.gradient(lu.ref, lu.x, lu.cot)["companion"] == 0.0).all()


# ---- the planted defects ----------------------------------------------------------------------------------------------
def test_every_defect_is_caught(lu, lu_large_gmin, nonsymmetric):
    caught = {}
    for defect in og.DEFECTS:
        if defect == "jacobian_at_last_vh":
            continue  # (its own test below: it needs a loosely converged run)
        case = {"no_transpose": nonsymmetric, "gmin_dropped_from_g": lu_large_gmin}.get(defect, lu)
        grad = og.gradient(case.ref, case.x, case.cot, defect=defect)
        worst = max(case.differences(grad, defect).values())
        closed = max(closed_form_errors(1e-6, defect)[0])
        kept = float(np.abs(grad["companion"]).max())
        caught[defect] = (worst, closed, kept)
        print(f"{defect}: central differences {worst:.2e}, closed forms {closed:.2e}, companion rows {kept:.2e}")
        assert worst > FD_BAR or closed > 1e-13 or kept > 0.0, defect
    # each is caught by what it breaks
    assert caught["exp_not_expm1"][0] <= FD_BAR and caught["exp_not_expm1"][1] > 1e-13  # (forward bias: e >> 1)
    assert caught["nvt_sign"][0] > 1.0 and caught["nvt_sign"][1] > 1.0
    assert caught["no_transpose"][0] > FD_BAR
    assert caught["diode_rows_kept"][2] > 0.0
    assert caught["gmin_dropped_from_g"][0] > FD_BAR


def test_exp_in_place_of_expm1_shows_on_a_reverse_biased_diode():
    """where e << 1 the two differ by a factor: one source pulling a diode into reverse bias, against the closed form
    dL/di_sat = -n_vt I / (i_sat (i_sat + I)) with I = -i_sat / 2"""
    amps = -0.5 * I_SAT
    good, _ = closed_form_errors(amps)
    bad, _ = closed_form_errors(amps, "exp_not_expm1")
    print(f"I = -i_sat / 2: d/di_sat off by {good[1]:.2e} with expm1, {bad[1]:.2e} with exp")
    assert good[1] <= 1e-13 and bad[1] > 0.5


def test_a_jacobian_one_step_behind_needs_loose_tolerances_to_show(lu):
    rows, diodes, initial = nr.lu_case()
    loose = NewtonReference(rows, diodes)  # the default tolerances of Circuit.operating_point
    run = loose.run(initial)
    assert run["converged"]
    x_loose, last_vh = run["x"], run["vh"][-2]  # (the last step was linearised at vh[-2])
    behind = max(lu.differences(og.gradient(loose, x_loose, lu.cot, "jacobian_at_last_vh", last_vh), "one step behind").values())
    at_x = max(lu.differences(og.gradient(loose, x_loose, lu.cot), "at the loose x").values())
    polished = max(lu.differences(og.gradient(loose, og.polish(loose, x_loose), lu.cot), "polished").values())
    print(f"default tolerances: J at the last vh {behind:.2e}, J at the loose x {at_x:.2e}, after polishing {polished:.2e}")
    assert behind > FD_BAR and behind > at_x
    assert at_x > FD_BAR  # the loose x is reltol-close only ...
    assert polished <= FD_BAR  # ... and within the bar only after polishing
