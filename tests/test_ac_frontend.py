"""AC analysis without a device: the argument checks of nodal_amd/ac.py, the containers, and the reference the GPU tests
are measured against (tests/ac_reference.py) checked against itself and against closed forms."""
import math

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd.ac import ACPeaks, ACSweep, check_ac_arguments, resolve_amplitudes, resolve_reactive
from tests import ac_reference as acr
from tests.test_gpu_transient_inductors import _grid_case

ROWS = [["a1", "A", "1", "1", "g"], ["r1", "R", "2", "1", "2"], ["r2", "R", "3", "2", "g"], ["e1", "E", "1", "3", "g"],
        ["r3", "R", "1", "3", "2"]]


def test_frequencies():
    omega = check_ac_arguments([0.5, 10.0])
    assert omega.dtype == np.float64 and omega.tolist() == [2.0 * math.pi * 0.5, 2.0 * math.pi * 10.0]
    assert check_ac_arguments([]).shape == (0,)
    for bad in ([0.0], [-1.0], [float("nan")], [float("inf")], [[1.0, 2.0]], 3.0):
        with pytest.raises(ValueError):
            check_ac_arguments(bad)


def test_reactive_elements():
    nl = n.Netlist.from_rows(ROWS)
    names, kind, value, ia, ib = resolve_reactive(nl, [("c1", 2.0, "1", "g")], [("l1", 3.0, "g", "2"), ("l2", 1.0, "2", "g")])
    assert names == ["c1", "l1", "l2"] and kind.tolist() == [0, 1, 1] and value.tolist() == [2.0, 3.0, 1.0]
    assert kind.dtype == np.uint8 and ia.dtype == np.int32
    assert ia.tolist() == [nl.nodenum["1"], -1, nl.nodenum["2"]] and ib.tolist() == [-1, nl.nodenum["2"], -1]
    # two inductors in parallel, a loop of inductors: legal here (the transient's DC start refuses them)
    assert resolve_reactive(nl, (), [("l1", 1.0, "1", "2"), ("l2", 1.0, "1", "2"), ("l3", 1.0, "2", "1")])[0] == ["l1", "l2", "l3"]
    empty = resolve_reactive(nl)
    assert empty[0] == [] and all(a.shape == (0,) for a in empty[1:])
    with pytest.raises(ValueError, match="farads"):
        resolve_reactive(nl, [("c1", 0.0, "1", "g")])
    with pytest.raises(ValueError, match="henries"):
        resolve_reactive(nl, (), [("l1", float("inf"), "1", "g")])
    with pytest.raises(ValueError, match="both leads"):
        resolve_reactive(nl, [("c1", 1.0, "2", "2")])
    with pytest.raises(ValueError, match="both leads"):
        resolve_reactive(nl, (), [("l1", 1.0, "g", "g")])
    with pytest.raises(ValueError, match="given twice"):
        resolve_reactive(nl, [("x", 1.0, "1", "g")], [("x", 1.0, "2", "g")])
    with pytest.raises(ValueError, match="node_a, node_b"):
        resolve_reactive(nl, [("c1", 1.0, "1")])
    with pytest.raises(KeyError):
        resolve_reactive(nl, [("c1", 1.0, "1", "nowhere")])


def test_amplitudes():
    nl = n.Netlist.from_rows(ROWS)
    rows, amp = resolve_amplitudes(nl, {"e1": 1 + 2j, "a1": -0.5})
    assert rows.tolist() == [3, 0] and amp.tolist() == [1 + 2j, -0.5 + 0j] and amp.dtype == np.complex128
    none = resolve_amplitudes(nl, None)
    assert none[0].shape == (0,) and none[1].shape == (0,)
    assert resolve_amplitudes(nl, {})[0].shape == (0,)
    with pytest.raises(TypeError):
        resolve_amplitudes(nl, [("e1", 1.0)])
    with pytest.raises(KeyError):
        resolve_amplitudes(nl, {"zz": 1.0})
    with pytest.raises(ValueError, match="independent sources"):
        resolve_amplitudes(nl, {"r1": 1.0})
    with pytest.raises(ValueError, match="finite"):
        resolve_amplitudes(nl, {"e1": complex(float("nan"), 0.0)})


def test_the_two_formulations_agree():
    rows, caps, inds = _grid_case(12, ["e1", "e2"], 5, seed=31)
    r = acr.ACReference(rows, caps, inds)
    assert r.n == 145
    freqs = np.logspace(-4, 4, 17)
    amplitudes = {"e1": 1.0, "e2": 0.5 - 0.25j, "ld0": 2j, "ld1": -1.0 + 1j}
    Xc, Xi = r.sweep(freqs, amplitudes), r.sweep(freqs, amplitudes, method="interleaved")
    worst = max(np.abs(a - b).max() / np.abs(a).max() for a, b in zip(Xc, Xi))
    print("complex against interleaved real, worst difference over the largest unknown:", worst)
    assert worst <= 1e-13


def test_rc_lowpass_closed_form():
    R, C = 2.0, 0.25
    freqs = (1.0 / (2.0 * math.pi * R * C)) * np.logspace(-2, 2, 9)
    r = acr.ACReference(acr.rc_lowpass_rows(R), [("c1", C, "out", "g")])
    X = r.sweep(freqs, {"e1": 1.0})
    v, i = acr.rc_lowpass_closed_form(freqs, R, C)
    out = r.nl.nodenum["out"]
    assert np.abs(X[:, out] - v).max() <= 1e-14
    assert np.abs(r.currents(freqs, X)[:, 0] - i).max() <= 1e-14 * max(1.0, np.abs(i).max())
    assert abs(abs(X[4, out]) - math.sqrt(0.5)) <= 1e-14  # the -3 dB point


def test_series_rlc_closed_form():
    R, L, C = 0.5, 2.0, 0.125
    f0 = 1.0 / (2.0 * math.pi * math.sqrt(L * C))
    freqs = f0 * np.array([0.1, 0.5, 0.9, 0.99, 1.0, 1.01, 1.1, 2.0, 10.0])
    r = acr.ACReference(acr.series_rlc_rows(R), [("c1", C, "b", "g")], [("l1", L, "in", "a")])
    X = r.sweep(freqs, {"e1": 1.0})
    va, vb, i = acr.series_rlc_closed_form(freqs, R, L, C)
    scale = max(np.abs(va).max(), np.abs(vb).max())
    assert np.abs(X[:, r.nl.nodenum["a"]] - va).max() <= 1e-14 * scale
    assert np.abs(X[:, r.nl.nodenum["b"]] - vb).max() <= 1e-14 * scale
    cur = r.currents(freqs, X)
    assert np.abs(cur[:, 1] - i).max() <= 1e-14 * scale and np.abs(cur[:, 0] - i).max() <= 1e-14 * scale
    assert abs(i[4] - 1.0 / R) <= 1e-14 / R  # at resonance the reactances cancel


def test_containers():
    phasors = np.array([[1.0 + 0j, 1j], [-10.0 + 0j, 0.1 - 0.1j], [0j, -1j]])
    sw = ACSweep(np.array([1.0, 2.0, 3.0]), 2.0 * math.pi * np.array([1.0, 2.0, 3.0]), phasors, [("1", "g"), ("2", "1")],
                 np.zeros(3, dtype=np.int32), np.zeros(3), peaks=ACPeaks(np.array([2.0]), np.array([1], dtype=np.int32)))
    assert len(sw) == 3 and sw.currents.shape == (3, 0) and sw.solutions is None and sw.solution_indices.shape == (0,)
    assert sw.peaks.magnitude.tolist() == [2.0] and sw.peaks.frequency_index.tolist() == [1]
    db, deg = sw.magnitude_db(), sw.phase_deg()
    assert db[0].tolist() == [0.0, 0.0] and db[1, 0] == 20.0 and db[2, 0] == -math.inf
    assert abs(db[1, 1] - 20.0 * math.log10(0.1 * math.sqrt(2.0))) <= 1e-13
    assert deg[0].tolist() == [0.0, 90.0] and deg[1, 0] == 180.0 and abs(deg[1, 1] + 45.0) <= 1e-13 and deg[2, 1] == -90.0
    assert n.ACSweep is ACSweep and n.ACPeaks is ACPeaks and n.resolve_reactive is resolve_reactive
