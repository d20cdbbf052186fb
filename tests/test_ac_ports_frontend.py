"""AC port analysis without a device: the argument checks and the container of nodal_amd/ac_ports.py, and the reference
the GPU tests are measured against (tests/ac_port_reference.py) checked against itself -- its two formulations -- and
against closed forms.

Bars: the two formulations agree to 1e-13 of the largest unknown among the P solutions of a frequency (measured: 4.9e-16
of max|Z| on the grid case, 2.7e-15 on the inputs), the closed forms hold to 1e-14 of the same scale."""
import math

import numpy as np
import pytest

import nodal
import nodal_amd as n
from nodal_amd.ac_ports import ACPortPeaks, ACPortSweep, check_ac_port_arguments
from tests import ac_port_reference as apr
from tests.ac_reference import ACReference
from tests.test_gpu_branches import INPUTS
from tests.test_gpu_transient_inductors import _grid_case
from tests.transient_rl_reference import seeded_mix


def _agreement(pr, freqs, tag):
    Xc, Zc = pr.sweep(freqs, "complex")
    Xi, Zi = pr.sweep(freqs, "interleaved")
    z, x = apr.worst_ratio(Zi, Zc, Xc, tol=1e-13), apr.worst_ratio(Xi, Xc, Xc, tol=1e-13)
    print(tag, "complex against interleaved over 1e-13 of the solutions' scale: Z", z, "solutions", x)
    assert z <= 1.0 and x <= 1.0, tag
    assert np.isfinite(Zc).all() and (apr.scales(Xc) > 0).all(), tag  # (nonsingular at every frequency)
    return Zc


@pytest.mark.parametrize("k", range(29), ids=[name for name, _ in INPUTS])
def test_the_two_formulations_agree(k):
    name, rows = INPUTS[k]
    caps, inds = seeded_mix(rows, k)
    r = ACReference(rows, caps, inds)
    _agreement(apr.ACPortReference(r, apr.seeded_ports(r.nl, 5, 2000 + k)), apr.INPUT_FREQS, name)


def test_the_two_formulations_agree_on_the_grid():
    rows, caps, inds = _grid_case(12, ["e1", "e2"], 5, seed=31)
    r = ACReference(rows, caps, inds)
    assert r.n == 145 and r.K == 143 and len(INPUTS) == 29
    pr = apr.ACPortReference(r, apr.seeded_ports(r.nl, 33, 7))
    Z = _agreement(pr, apr.GRID_FREQS, "grid(12), 33 ports")
    rec = max(np.abs(z - z.T).max() / np.abs(z).max() for z in Z)
    print("grid(12), 33 ports: reciprocity of the reference", rec)
    assert rec <= 1e-13  # (R, L, C and E sources switched off: reciprocal)


def test_t_network_closed_form():
    R1, R2, C = 3.0, 5.0, 0.25
    freqs = np.logspace(-2, 2, 9)
    r = ACReference(apr.t_network_rows(R1, R2), [("c1", C, "m", "g")])
    pr = apr.ACPortReference(r, ["a", "b"])
    want = apr.t_network_closed_form(freqs, R1, R2, C)
    for method in ("complex", "interleaved"):
        X, Z = pr.sweep(freqs, method)
        assert apr.worst_ratio(Z, want, X, tol=1e-14) <= 1.0, method


def test_tank_closed_form():
    R, L, C = 40.0, 2.0, 0.125
    f0 = 1.0 / (2.0 * math.pi * math.sqrt(L * C))
    freqs = f0 * np.array([0.1, 0.5, 0.9, 0.99, 1.0, 1.01, 1.1, 2.0, 10.0])
    r = ACReference(apr.tank_rows(R), [("c1", C, "t", "g")], [("l1", L, "t", "g")])
    pr = apr.ACPortReference(r, ["t"])
    want = apr.tank_closed_form(freqs, R, L, C)
    assert abs(want[4] - R) <= 1e-13 * R  # at resonance the tank is its resistor
    for method in ("complex", "interleaved"):
        X, Z = pr.sweep(freqs, method)
        assert apr.worst_ratio(Z[:, 0, 0], want, X, tol=1e-14) <= 1.0, method


# ---- the container ----------------------------------------------------------------------------------------------------
def _sweep(z, info=None, ports=None):
    z = np.asarray(z, dtype=np.complex128)
    F, P = z.shape[0], z.shape[1]
    freqs = np.arange(1.0, F + 1.0)
    info = np.zeros(F, dtype=np.int32) if info is None else np.asarray(info, dtype=np.int32)
    return ACPortSweep(freqs, 2.0 * math.pi * freqs, ports or [(str(p), "g") for p in range(P)], z, info, np.zeros((F, P)))


def test_container_y_and_s():
    rng = np.random.default_rng(5)
    F, P = 4, 3
    z = rng.normal(size=(F, P, P)) + 1j * rng.normal(size=(F, P, P)) + 4.0 * np.eye(P)
    sw = _sweep(z)
    assert len(sw) == F and sw.peaks is None and sw.work == (0, 0, 0) and sw.ports == [("0", "g"), ("1", "g"), ("2", "g")]
    assert np.abs(sw.y() @ z - np.eye(P)).max() <= 1e-13
    # a per-port reference against the formula, matrix by matrix
    z0 = np.array([50.0, 75.0, 10.0])
    R, root = np.diag(z0), np.diag(np.sqrt(z0))
    want = np.array([np.linalg.inv(root) @ (zf - R) @ np.linalg.inv(zf + R) @ root for zf in z])
    assert np.abs(sw.s(z0) - want).max() <= 1e-13
    assert np.abs(sw.s(50.0) - sw.s([50.0, 50.0, 50.0])).max() == 0.0
    # a one-port: (Z - z0) / (Z + z0), and the default z0 is 50 ohms
    one = _sweep(z[:, :1, :1])
    assert np.abs(one.s(75.0)[:, 0, 0] - (z[:, 0, 0] - 75.0) / (z[:, 0, 0] + 75.0)).max() <= 1e-14
    assert np.array_equal(one.s(), one.s(50.0))
    assert abs(_sweep([[[50.0]]]).s()[0, 0, 0]) == 0.0  # a matched load reflects nothing
    for bad in (0.0, -50.0, float("nan"), float("inf"), [50.0, 50.0], [50.0, 50.0, 0.0], np.ones((3, 3)), "fifty", None, 50j):
        with pytest.raises(ValueError, match="z0"):
            sw.s(bad)
    # a singular Z: a port between a node and itself
    zero = z.copy()
    zero[:, 1, :] = 0.0
    zero[:, :, 1] = 0.0
    with pytest.raises(np.linalg.LinAlgError):
        _sweep(zero).y()
    assert n.ACPortSweep is ACPortSweep and nodal.ACPortSweep is ACPortSweep and nodal.ACPortPeaks is ACPortPeaks


def test_container_with_a_singular_frequency():
    z = np.array([[[2.0, 1.0], [1.0, 3.0]], [[np.nan, np.nan], [np.nan, np.nan]], [[2.0 + 8j, 1.0], [1.5, 3.0]],
                  [[0.0, 0.0], [0.0, 0.0]]], dtype=np.complex128)
    sw = _sweep(z, info=[0, 1, 0, 0])
    assert np.array_equal(sw.driving_point()[[0, 2, 3]], np.array([[2.0, 3.0], [2.0 + 8j, 3.0], [0.0, 0.0]]))
    assert np.isnan(sw.driving_point()[1]).all()
    rec = sw.reciprocity()
    assert rec[0] == 0.0 and np.isnan(rec[1]) and rec[2] == 0.5 / abs(2.0 + 8j) and rec[3] == 0.0
    mag, at = sw.peak_impedance()
    assert mag.tolist() == [abs(2.0 + 8j), 3.0] and at.tolist() == [2, 0]  # (among exact ties the first frequency)
    y = _sweep(z[:3], info=[0, 1, 0]).y()
    assert np.isnan(y[1]).all() and np.abs(y[0] @ z[0] - np.eye(2)).max() <= 1e-15 and np.abs(y[2] @ z[2] - np.eye(2)).max() <= 1e-15
    s = _sweep(z[:3], info=[0, 1, 0]).s(2.0)
    assert np.isnan(s[1]).all() and np.isfinite(s[[0, 2]]).all()
    none = _sweep(z[1:2], info=[1])
    mag, at = none.peak_impedance()
    assert np.isnan(mag).all() and at.tolist() == [-1, -1] and np.isnan(none.y()).all() and np.isnan(none.s()).all()
    empty = _sweep(np.zeros((2, 0, 0)))
    assert empty.y().shape == (2, 0, 0) and empty.s().shape == (2, 0, 0) and empty.reciprocity().tolist() == [0.0, 0.0]
    assert empty.driving_point().shape == (2, 0) and empty.peak_impedance()[0].shape == (0,)
    peaks = ACPortPeaks(np.ones(3), np.zeros(3, dtype=np.int32), np.ones(3, dtype=np.int32))
    assert peaks.magnitude.shape == peaks.port.shape == peaks.frequency_index.shape == (3,)


# ---- the arguments ----------------------------------------------------------------------------------------------------
def test_arguments():
    nl = n.Netlist.from_rows(apr.t_network_rows(1.0, 2.0) + [["r3", "R", "1.0", "m", "g"]])
    omega, pairs, ia, ib = check_ac_port_arguments(nl, [1.0, 2.0], ["a", ("a", "b"), ("g", "m"), ["b", "b"]])
    assert omega.tolist() == [2.0 * math.pi, 2.0 * math.pi * 2.0]
    assert pairs == [("a", "g"), ("a", "b"), ("g", "m"), ("b", "b")]
    num = nl.nodenum
    assert ia.tolist() == [num["a"], num["a"], -1, num["b"]] and ib.tolist() == [-1, num["b"], num["m"], num["b"]]
    assert ia.dtype == ib.dtype == np.int32
    none = check_ac_port_arguments(nl, [], [])
    assert none[0].shape == (0,) and none[1] == [] and none[2].shape == none[3].shape == (0,)
    for bad in (("a", "b", "m"), ("a",), ()):
        with pytest.raises(ValueError, match="Port"):
            check_ac_port_arguments(nl, [1.0], [bad])
    for bad in ("nowhere", ("a", "nowhere"), ("nowhere", "g")):
        with pytest.raises(KeyError, match="nowhere"):
            check_ac_port_arguments(nl, [1.0], [bad])
    for bad in ([0.0], [-1.0], [float("nan")], [float("inf")], [[1.0, 2.0]], 1.0):
        with pytest.raises(ValueError, match="frequencies"):
            check_ac_port_arguments(nl, bad, ["a"])
    assert callable(n.Circuit.ac_ports) and nodal.Circuit.ac_ports is n.Circuit.ac_ports
