"""The transistor reference (tests/transistor_reference.py) against a closed form and against itself, and the parity
check of tests/test_gpu_transistors.py against planted defects.  No GPU."""
import numpy as np
import pytest

from tests import newton_reference as nr
from tests import transistor_reference as tr
from tests.newton_reference import TIGHT, TOL
from tests.transistor_reference import TransistorReference, parity_errors

MAX_ITER = 100  # Circuit.operating_point's default, which the GPU tests run with


@pytest.fixture(scope="module")
def runs():
    """every input of the GPU tests, run once from zeros with both solves"""
    out = {}
    for name, case in tr.CASES.items():
        rows, diodes, transistors = case()
        ref = TransistorReference(rows, diodes, transistors, max_iter=MAX_ITER, **TIGHT)
        out[name] = (ref, ref.run(both=True))
    return out


@pytest.mark.parametrize("amps", [1e-9, 1e-6, 1e-3, 1.0])
def test_the_reference_meets_the_closed_form_of_a_diode_connected_transistor(amps):
    """Newton converges quadratically, so once a step is below reltol = 1e-10 the error is roundoff: a few ulp of v and
    of i_s (1 + 1 / beta_f), the latter times n_vt / v < 1 -- 1e-12 |v| leaves three decades"""
    rows, diodes, transistors = tr.diode_connected(amps)
    ref = TransistorReference(rows, diodes, transistors, gmin=0.0, **TIGHT)
    r = ref.run(both=True)
    v = tr.diode_connected_closed_form(amps)
    print(f"I = {amps:g}: {r['iterations']} iterations, v = {r['x'][0]!r}, closed form {v!r}")
    assert r["converged"] and abs(r["x"][0] - v) <= 1e-12 * abs(v)
    assert ref.worst_disagreement <= TOL / 1000
    i_c, i_b, i_e = ref.terminal_currents(r["x"])
    assert abs(i_c[0] + i_b[0] - amps) <= 1e-12 * amps and abs(i_e[0] + amps) <= 1e-12 * amps


@pytest.mark.parametrize("name", list(tr.CASES))
def test_the_reference_converges_on_the_inputs_of_the_gpu_tests(runs, name):
    ref, r = runs[name]
    print(f"{name}: n = {ref.n}, {r['iterations']} iterations, limited {r['limited']}, not converged {r['not_converged']}, "
          f"transports {r['transports_not_converged']}, two solves disagree by {ref.worst_disagreement:.2e}, "
          f"nearest threshold {r['margins'].min():.2e}")
    assert ref.n == tr.SIZES[name]
    assert r["converged"] and r["iterations"] <= MAX_ITER // 2
    assert ref.worst_disagreement <= TOL / 1000
    # the comparisons that lie in the band where the limiter's branch is undecidable: at most 1 % of them
    undecidable = r["margins"] <= 4 * TOL * np.abs(r["iterates"]).max(axis=1)[:, None]
    assert undecidable.sum() <= 0.01 * undecidable.size
    res, scale = ref.residual(r["x"])
    assert np.abs(res).max() / scale.max() <= nr.RESID_BAR + TIGHT["reltol"] + TIGHT["abstol"] / scale.max()
    i_c, i_b, i_e = ref.terminal_currents(r["x"])
    assert (np.abs(i_c + i_b + i_e) <= 4 * TOL * (np.abs(i_c) + np.abs(i_b) + np.abs(i_e))).all()


def test_the_common_emitter_stage_is_forward_active(runs):
    ref, r = runs["ce_amp"]
    i_c, i_b, _ = ref.terminal_currents(r["x"])
    v = ref.voltages(r["x"])
    print(f"ce_amp: I_C = {i_c[0]!r}, I_B = {i_b[0]!r}, I_C / I_B = {i_c[0] / i_b[0]!r}, v_be = {v[0]!r}, v_bc = {v[1]!r}")
    assert v[0] > 0.5 and v[1] < -1.0  # the base-emitter junction conducts, the base-collector junction is reverse biased
    assert abs(i_c[0] / i_b[0] - tr.BETA_F) <= 1e-3  # (beta_f, but for the reverse junction's leakage)


def test_every_region_is_visited(runs):
    """saturation has both junctions forward; reverse active has the base-collector junction alone forward and the
    emitter current at beta_r times the base current; a PNP's currents are an NPN's negated; a transistor with every
    lead on one node carries exactly nothing"""
    ref, r = runs["switch_sat"]
    v = ref.voltages(r["x"])
    assert v[0] > 0.5 and v[1] > 0.3
    ref, r = runs["reverse_active"]
    v = ref.voltages(r["x"])
    i_c, i_b, i_e = ref.terminal_currents(r["x"])
    assert v[0] < -1.0 and v[1] > 0.5 and i_e[0] > 0.0 and abs(i_e[0] / i_b[0] - tr.BETA_R) <= 1e-3
    ref, r = runs["pnp_follower"]
    i_c, i_b, i_e = ref.terminal_currents(r["x"])
    assert i_e[0] > 0.0 and i_c[0] < 0.0 and i_b[0] < 0.0
    ref, r = runs["lu_grid"]
    t = ref.transistor_names.index("q5")
    i_c, i_b, i_e = ref.terminal_currents(r["x"])
    assert i_c[t] == 0.0 and i_b[t] == 0.0 and i_e[t] == 0.0
    assert (r["vh"][:, ref.jf[t]] == 0.0).all() and (r["vh"][:, ref.jr[t]] == 0.0).all()


@pytest.mark.parametrize("name", list(tr.CASES))
def test_the_parity_check_passes_on_the_reference_itself(runs, name):
    ref, r = runs[name]
    ex, ev, left, total, counts = parity_errors(ref, r["iterates"], r["vh"], np.zeros(ref.n))
    assert ex <= 2 * TOL and ev <= 2 * TOL and left <= 0.01 * total
    assert [c[0] for c in counts] == r["not_converged"] and [c[1] for c in counts] == r["limited"]
    assert [c[3] for c in counts] == r["transports_not_converged"]


@pytest.mark.parametrize("defect, name", [("JT_sign", "ce_amp"), ("JT_sign", "reverse_active"), ("JT_sign", "lu_grid"),
                                          ("no_reverse_gm", "reverse_active"), ("no_reverse_gm", "switch_sat"),
                                          ("gm_rows_swapped", "ce_amp"), ("gm_rows_swapped", "reverse_active"),
                                          ("gm_rows_swapped", "lu_grid")])
def test_the_parity_check_bites_on_planted_defects(runs, defect, name):
    """a copy of the reference's own output with one step redone wrongly -- the last but one, where the transistors
    conduct: the check must see it.  (The reverse GM row of a forward-active transistor carries exp(v_bc / n_vt) of
    nothing, so its absence is planted where a base-collector junction conducts.)"""
    ref, r = runs[name]
    X, VH = r["iterates"].copy(), r["vh"].copy()
    k = len(X) - 2
    x, vh, _ = ref.one_step(None, VH[k], defect=defect)
    X[k], VH[k + 1] = x, vh
    ex, ev, left, total, counts = parity_errors(ref, X[:k + 1], VH[:k + 2], np.zeros(ref.n))
    print(f"{name}, {defect}: x error {ex:.2e}, vh error {ev:.2e}")
    assert ex > 2 * TOL or ev > 2 * TOL
