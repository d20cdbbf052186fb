"""Gradients through time without a device: the argument checks, the container, and the reference of the GPU tests
(tests/transient_gradient_reference.py) against itself -- its adjoint against central differences of its own forward
stepping, and against the closed form of one RC section."""
import numpy as np
import pytest

import nodal_amd as n
from nodal_amd.transient_gradient import (NO_RECORD, TransientGradient, TransientRecord,
                                          check_transient_gradient_arguments)
from tests import transient_gradient_reference as tg
from tests import transient_reference as tref


# ---- 1: arguments and container ---------------------------------------------------------------------------------------
def _record(steps=4):
    return TransientRecord(None, 0.1, np.ones(2), np.array([5, 6]), {}, 0, steps, ["1"], np.zeros(1, np.int32),
                           np.full(1, -1, np.int32), np.zeros(3), True)


def test_argument_checks():
    cot = check_transient_gradient_arguments(_record(), [[1.0]] * 5, 1)
    assert cot.shape == (5, 1) and cot.dtype == np.float64 and cot.flags.c_contiguous
    with pytest.raises(ValueError, match="no recorded transient: call transient\\(..., record=True\\) first"):
        check_transient_gradient_arguments(None, np.zeros((5, 1)), 1)
    assert NO_RECORD == "no recorded transient: call transient(..., record=True) first"
    for bad in (np.zeros((4, 1)), np.zeros((5, 2)), np.zeros(5)):
        with pytest.raises(ValueError, match="shape"):
            check_transient_gradient_arguments(_record(), bad, 1)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="finite"):
            check_transient_gradient_arguments(_record(), np.full((5, 1), bad), 1)
    assert check_transient_gradient_arguments(_record(0), np.zeros((1, 0)), 0).shape == (1, 0)


def test_record_with_the_trapezoidal_rule_raises():
    """the check comes before anything touches a device: a Circuit that was never assembled serves"""
    c = n.Circuit.__new__(n.Circuit)
    c._handle = type("H", (), {"n": 1})()
    c._transient_record = "stale"
    with pytest.raises(ValueError, match='record=True needs method="euler"'):
        c.transient([], 0.1, 3, method="trapezoidal", record=True)
    assert c._transient_record is None
    c._handle = None  # (nothing to give back)


def test_transient_gradient_without_a_record_raises():
    c = n.Circuit.__new__(n.Circuit)
    c._handle, c._transient_record = None, None
    with pytest.raises(ValueError, match="no recorded transient"):
        c.transient_gradient(np.zeros((3, 1)))


def test_container():
    g = TransientGradient(np.arange(3.0), np.ones(2), {"a1": np.zeros(4)}, np.zeros(5), np.zeros(4, np.int32), np.zeros(4),
                          timings=(0.0, 0.0, 1.5))
    assert len(g) == 4 and g.adjoints is None and g.source_values["a1"].shape == (4,) and g.timings[2] == 1.5
    assert g.start_values is None and g.values.tolist() == [0.0, 1.0, 2.0] and g.capacitors.shape == (2,) and g.initial.shape == (5,)


def test_the_blocks_of_the_device_order():
    assert tg.blocks(0) == [] and tg.blocks(1) == [(1, 1)] and tg.blocks(16) == [(16, 1)]
    assert tg.blocks(17) == [(17, 2), (1, 1)] and tg.blocks(18) == [(18, 3), (2, 1)]


# ---- 2: the reference's adjoint against central differences of its own forward stepping -----------------------------
def test_the_small_inputs_are_the_ones_the_bar_was_measured_on():
    cases = tg.small_cases()
    assert len(cases) == 26 and [c[0] for c in cases[-3:]] == ["edges", "grid(12)", "cfg5(12)"]


@pytest.mark.parametrize("dc_start", [True, False], ids=["dc", "initial"])
@pytest.mark.parametrize("k", range(26))
def test_adjoint_against_central_differences(k, dc_start):
    case = tg.small_case(k, dc_start)
    worst = tg.disagreement(case.adjoint, case.fd)
    print(case.name, "dc" if dc_start else "initial", "unknowns", case.ref.n, "|adjoint - central difference| / max:", worst)
    assert worst <= tg.CPU_DISAGREEMENT, case.name


# ---- 3: one RC section under Euler: the closed form ---------------------------------------------------------------------
@pytest.mark.parametrize("steps", [0, 1, 16, 33])
def test_rc_section_closed_form(steps):
    I, R, C, h = 0.7, 3.0, 0.02, 0.011
    rows, caps = tref.rc_rows(I, R), [("c1", C, "1", "g")]
    r = tg.TransientGradientReference(rows, caps, h)
    pairs = [(0, -1)]
    cot = np.random.default_rng(steps).uniform(-1.0, 1.0, size=(steps + 1, 1))
    W, X = tg.forward(rows, caps, h, steps, None, pairs, np.zeros(1))
    assert np.abs(W[:, 0] - tref.rc_euler_closed_form(I, R, C, h, steps)).max() <= 1e-15 * I * R * 4
    values, farads, _, initial = r.public(pairs, cot, X, np.zeros(0, dtype=np.int64), False)
    dR, dC, dI = tg.rc_euler_derivatives(I, R, C, h, steps)
    want = np.array([cot[:, 0] @ dI, cot[:, 0] @ dR]), np.array([cot[:, 0] @ dC])
    worst = max(tg.relative_miss(values, want[0]), tg.relative_miss(farads, want[1])) if steps else 0.0
    print("RC section, steps", steps, "|adjoint - closed form| / max:", worst)
    assert worst <= tg.RC_DISAGREEMENT
    if steps == 0:
        assert not values.any() and not farads.any() and initial.tolist() == [cot[0, 0]]
