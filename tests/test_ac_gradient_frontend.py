"""Gradients through frequency without a device: argument checking, the container, and tests/ac_gradient_reference.py
against itself -- its adjoint formulation against its central differences and against the closed forms."""
import math

import numpy as np
import pytest

from nodal_amd.ac_gradient import ACGradient, check_ac_gradient_arguments, sources_by_name
from tests import ac_gradient_reference as agr
from tests import ac_reference as acr
from tests.sensitivity_reference import T_A, T_E


# ---- argument checking ------------------------------------------------------------------------------------------------
def test_cotangents_are_checked():
    good = np.ones((3, 2), dtype=np.complex128)
    out = check_ac_gradient_arguments(good, 3, 2)
    assert out.dtype == np.complex128 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, good)
    assert check_ac_gradient_arguments(good.astype(np.complex64), 3, 2).dtype == np.complex128
    assert check_ac_gradient_arguments([[1j, 2.0]], 1, 2).shape == (1, 2)
    assert check_ac_gradient_arguments(np.zeros((0, 2), dtype=np.complex128), 0, 2).shape == (0, 2)
    with pytest.raises(TypeError, match="complex"):
        check_ac_gradient_arguments(np.ones((3, 2)), 3, 2)
    for shape in ((2, 3), (3,), (3, 2, 1), (6,)):
        with pytest.raises(ValueError, match="shape"):
            check_ac_gradient_arguments(np.ones(shape, dtype=np.complex128), 3, 2)
    for bad in (np.nan, np.inf, 1j * np.nan, -1j * np.inf):
        cot = good.copy()
        cot[1, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            check_ac_gradient_arguments(cot, 3, 2)


# ---- the container ----------------------------------------------------------------------------------------------------
def test_the_container_is_built_from_arrays():
    terms = np.array([[1 + 1j, 2.0, 0.5j], [3.0, -1j, 0.5]])
    by_name = sources_by_name(["r1", "a1", "e1", "a1"], [1, 2, 3], terms)
    assert by_name == {"a1": (4 + 1j) + (0.5 + 0.5j), "e1": 2 - 1j}
    g = ACGradient(np.arange(4.0), np.array([1.0, 2.0]), np.array([3.0]), by_name, terms, np.zeros((2, 1), dtype=complex),
                   np.zeros(2, dtype=np.int32), np.zeros((2, 2)), capacitor_names=["c1", "c2"], inductor_names=["l1"],
                   source_rows=np.array([1, 2, 3]), work=np.array([2, 4, 0]), timings=[0.0, 1.0, 2.0])
    assert len(g) == 2 and g.capacitors_by_name == {"c1": 1.0, "c2": 2.0} and g.inductors_by_name == {"l1": 3.0}
    assert g.sources["e1"] == 2 - 1j and g.adjoints is None and g.source_terms is terms and list(g.work) == [2, 4, 0]
    with pytest.raises(ValueError, match="one name"):
        ACGradient(np.zeros(1), np.zeros(2), np.zeros(0), {}, terms, None, np.zeros(0), None, capacitor_names=["c1"])
    empty = ACGradient(np.zeros(3), np.zeros(0), np.zeros(0), {}, np.zeros((0, 0), dtype=complex), np.zeros((0, 0), dtype=complex),
                       np.zeros(0, dtype=np.int32), np.zeros((0, 2)))
    assert len(empty) == 0 and empty.sources == {} and empty.capacitors_by_name == {}
    assert sources_by_name(["a1"], [], np.zeros((2, 0), dtype=complex)) == {}


# ---- the two formulations ---------------------------------------------------------------------------------------------
def test_the_small_cases_hold_every_type_and_both_kinds():
    ks = agr.small_cases()
    assert len(ks) == 27
    types, kinds = set(), set()
    for k in ks:
        c = agr.input_case(k)
        assert c.ref.n <= 64
        types |= set(c.ref.type.tolist())
        kinds |= set(c.ref.ac.kind.tolist())
    assert types == {0, 1, 2, 3, 4, 5} and kinds == {0, 1}


def test_the_adjoint_meets_the_central_differences():
    worst = 0.0
    for k in agr.small_cases():
        c = agr.input_case(k)
        d = agr.disagreement(c, c.values, c.react, c.by_name)
        print(f"{c.name}: |adjoint - central differences| {d:.2e}")
        worst = max(worst, d)
    print("the largest", worst, "MEASURED", agr.MEASURED)
    assert worst <= agr.CPU_DISAGREEMENT
    assert worst >= 0.1 * agr.MEASURED  # (MEASURED is the number obtained here, not a guess from above)


def test_the_differences_see_a_missing_transpose():
    """with A in place of A^T the adjoint formulation misses the central differences by far more than the bar"""
    c = agr.input_case(next(k for k in agr.small_cases() if agr.input_case(k).name == "random0"))
    values, react, terms, _, _, _ = c.ref.gradient(c.frequencies, c.sources, c.probes, c.cotangents, transpose=False)
    by_name = {c.ref.keys[i]: complex(terms[:, j].sum()) for j, i in enumerate(c.source_rows.tolist())}
    assert agr.disagreement(c, values, react, by_name) > 1e4 * agr.CPU_DISAGREEMENT


def test_source_rows_are_exactly_zero_in_the_reference():
    for k in agr.small_cases():
        c = agr.input_case(k)
        at = np.flatnonzero((c.ref.type == T_A) | (c.ref.type == T_E))
        assert (c.values[at] == 0.0).all() and not np.signbit(c.values[at]).any(), c.name
        assert (c.bars[0][at] == 0.0).all(), c.name
        assert all(v == 0.0 for i, v in zip(c.subset.tolist(), c.fd[0]) if i in at), c.name


# ---- closed forms -----------------------------------------------------------------------------------------------------
def test_rc_lowpass_closed_form():
    R, C, alpha = 2.0e3, 0.25e-6, 0.8 - 0.3j
    freqs = (1.0 / (2.0 * math.pi * R * C)) * np.logspace(-2, 2, 9)
    r = agr.ACGradientReference(acr.rc_lowpass_rows(R), [("c1", C, "out", "g")])
    pairs = r.pairs(["out"])
    W, _ = r.phasors(freqs, {"e1": alpha}, pairs)
    h2, dR, dC = agr.rc_lowpass_derivatives(freqs, R, C)
    assert np.allclose(np.abs(W[:, 0]) ** 2, abs(alpha) ** 2 * h2, rtol=1e-13, atol=0)
    # L = sum_f |W_f|^2: g = 2 W
    values, react, terms, _, _, _ = r.gradient(freqs, {"e1": alpha}, ["out"], 2.0 * W)
    a2 = abs(alpha) ** 2
    keys = r.keys
    assert abs(values[keys.index("r1")] - a2 * dR.sum()) <= 1e-12 * a2 * np.abs(dR).sum()
    assert abs(react[0] - a2 * dC.sum()) <= 1e-12 * a2 * np.abs(dC).sum()
    assert np.allclose(terms[:, 0], 2.0 * alpha * h2, rtol=1e-12, atol=0)  # d |alpha|^2 |H|^2 / d alpha, torch's convention
    assert values[keys.index("e1")] == 0.0


def test_series_rlc_closed_form():
    R, L, C = 5.0, 2.0e-3, 0.5e-6
    f0 = 1.0 / (2.0 * math.pi * math.sqrt(L * C))
    freqs = f0 * np.array([0.5, 0.9, 0.99, 1.0, 1.01, 1.1, 2.0])
    r = agr.ACGradientReference(acr.series_rlc_rows(R), [("c1", C, "b", "g")], [("l1", L, "in", "a")])
    probes = [("a", "b")]
    W, _ = r.phasors(freqs, {"e1": 1.0}, r.pairs(probes))
    v2, dR, dL, dC = agr.series_rlc_derivatives(freqs, R, L, C)
    assert np.allclose(np.abs(W[:, 0]) ** 2, v2, rtol=1e-12, atol=0)
    values, react, _, _, _, _ = r.gradient(freqs, {"e1": 1.0}, probes, 2.0 * W)
    assert abs(values[r.keys.index("r1")] - dR.sum()) <= 1e-11 * np.abs(dR).sum()
    assert abs(react[0] - dC.sum()) <= 1e-11 * np.abs(dC).sum()  # (the capacitor is the first element, the inductor the second)
    assert abs(react[1] - dL.sum()) <= 1e-11 * np.abs(dL).sum()
