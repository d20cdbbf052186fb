"""Noise analysis without a device: the argument checks of nodal_amd/noise.py, the container, and the reference the GPU
tests are measured against (tests/noise_reference.py) checked against itself -- its two formulations, and what a
forgotten transpose would give -- and against closed forms.

grid(60) is left out of the comparison of the two formulations here: its direct formulation is 7080 right-hand sides per
frequency, 18 s on a CPU.  Measured once by that route (sparse LU, blocks of 512 right-hand sides, refined), in the
normwise terms of the reference: 6.9e-16 on amplitude densities, 5.2e-16 on contributions."""
import math

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd.noise import BOLTZMANN, NoiseSweep, check_noise_arguments, trapezoid_weights
from tests import noise_reference as nr
from tests.test_gpu_branches import INPUTS
from tests.test_gpu_transient_inductors import _grid_case
from tests.transient_rl_reference import seeded_mix

FREQS = [0.01, 0.3, 10.0]
SMALL = [k for k, (name, _) in enumerate(INPUTS) if name != "grid(60)"]


def test_arguments():
    assert check_noise_arguments(300, False, [2.0, 1.0]) == 300.0 and isinstance(check_noise_arguments(300, False, []), float)
    assert check_noise_arguments(77.5, True, [1.0, 2.0, 4.0]) == 77.5 and check_noise_arguments(1.0, True, [3.0]) == 1.0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            check_noise_arguments(bad, False, [1.0])
    for bad in ([2.0, 1.0], [1.0, 1.0], [1.0, 2.0, 2.0]):
        with pytest.raises(ValueError, match="strictly increasing"):
            check_noise_arguments(300.0, True, bad)
    assert BOLTZMANN == 1.380649e-23 == nr.BOLTZMANN


def test_trapezoid_weights():
    trapz = getattr(np, "trapezoid", None) or np.trapz
    rng = np.random.default_rng(3)
    for count in (2, 3, 9, 40):
        f = np.cumsum(rng.uniform(0.1, 5.0, size=count))
        y = rng.uniform(-1.0, 1.0, size=(count, 4))
        w = trapezoid_weights(f)
        assert w.shape == (count,) and abs(w.sum() - (f[-1] - f[0])) <= 1e-14 * f[-1]
        assert np.abs(w @ y - trapz(y, f, axis=0)).max() <= 1e-14 * (f[-1] - f[0])
        assert np.abs(nr.trapezoid(f, y) - trapz(y, f, axis=0)).max() <= 1e-14 * (f[-1] - f[0])
    assert trapezoid_weights([1.0, 3.0]).tolist() == [1.0, 1.0] and trapezoid_weights([1.0, 2.0, 4.0]).tolist() == [0.5, 1.5, 1.0]
    assert trapezoid_weights([5.0]).tolist() == [0.0] and trapezoid_weights([]).shape == (0,)
    assert n.trapezoid_weights is trapezoid_weights


def test_container():
    freqs = np.array([1.0, 2.0, 4.0])
    density = np.array([[4.0, 0.0], [16.0, 0.0], [4.0, 0.0]])
    contrib = np.array([[3.0, 0.0, 29.0, 3.0], [0.0, 0.0, 0.0, 0.0]])
    sw = NoiseSweep(freqs, 2.0 * math.pi * freqs, [("1", "g"), ("2", "2")], density, np.zeros(3, dtype=np.int32), np.zeros((3, 2)),
                    contributions=contrib, names=["r1", "e1", "r2", "r3"])
    assert len(sw) == 3 and sw.gain is None and sw.input_density is None and sw.outputs == [("1", "g"), ("2", "2")]
    assert sw.amplitude_density().tolist() == [[2.0, 0.0], [4.0, 0.0], [2.0, 0.0]]
    assert sw.integrated().tolist() == [30.0, 0.0] and sw.rms().tolist() == [math.sqrt(30.0), 0.0]
    assert sw.top(0, 2) == [("r2", 29.0), ("r1", 3.0)] and sw.top(0, 9)[2:] == [("r3", 3.0), ("e1", 0.0)]  # (ties: table order)
    assert sw.top(1, 1) == [("r1", 0.0)] and sw.top(0, 0) == []
    with pytest.raises(ValueError, match="contributions"):
        NoiseSweep(freqs, None, [], density, np.zeros(3), np.zeros((3, 2))).top(0)
    assert n.NoiseSweep is NoiseSweep


def _case(k):
    name, rows = INPUTS[k]
    caps, inds = seeded_mix(rows, k)
    r = nr.NoiseReference(rows, caps, inds)
    return name, r, nr.two_outputs(r.nl)


def _agreement(r, freqs, outputs, tag):
    ca, _ = r.adjoint(freqs, outputs, 300.0)
    cd = r.direct(freqs, outputs, 300.0)
    amp = nr.amplitude_miss(nr.density(ca), nr.density(cd), 1.0)
    con = nr.call_miss(r.integrated_contributions(freqs, ca), r.integrated_contributions(freqs, cd), 1.0)
    print(tag, "adjoint against direct: amplitude densities", amp, "contributions", con)
    assert amp <= 1e-13 and con <= 1e-13, tag
    quiet = np.setdiff1d(np.arange(r.ncomp), r.noisy)
    assert not ca[:, :, quiet].any() and not cd[:, :, quiet].any()


@pytest.mark.parametrize("k", SMALL, ids=[INPUTS[k][0] for k in SMALL])
def test_the_two_formulations_agree(k):
    name, r, outputs = _case(k)
    _agreement(r, FREQS, outputs, name)


def test_the_two_formulations_agree_on_the_grid():
    rows, caps, inds = _grid_case(12, ["e1", "e2"], 5, seed=31)
    r = nr.NoiseReference(rows, caps, inds)
    assert r.n == 145 and len(SMALL) == 28
    _agreement(r, FREQS, nr.two_outputs(r.nl), "grid(12) with two E sources")


@pytest.mark.parametrize("name", ["cfg5(24)", "doc/buffer"])
def test_the_transpose_matters(name):
    """With A in place of A^T the amplitude densities are off by more than 1e-3 of the largest: a forgotten transpose
    cannot pass the device suite's 1e-9.  (Measured: cfg5(24) 1.3e-3, doc/buffer 1.0.)"""
    k = [i[0] for i in INPUTS].index(name)
    _, r, outputs = _case(k)
    right, _ = r.adjoint(FREQS, outputs, 300.0)
    wrong, _ = r.adjoint(FREQS, outputs, 300.0, transpose=False)
    miss = nr.amplitude_miss(nr.density(wrong), nr.density(right), 1.0)
    print(name, "A in place of A^T: miss over the largest amplitude density", miss)
    assert miss > 1e-3


def test_rc_parallel_closed_form():
    R, C, T = 2.0e3, 0.25e-6, 300.0
    freqs = (1.0 / (2.0 * math.pi * R * C)) * np.logspace(-2, 2, 9)
    r = nr.NoiseReference(nr.rc_parallel_rows(R), [("c1", C, "out", "g")])
    want = nr.rc_parallel_density(freqs, R, C, T)
    for c in (r.adjoint(freqs, ["out"], T)[0], r.direct(freqs, ["out"], T)):
        assert np.abs(nr.density(c)[:, 0] - want).max() <= 1e-13 * want.max() and (np.abs(nr.density(c)[:, 0] - want) <= 1e-13 * want).all()
    assert abs(want[4] - 2.0 * BOLTZMANN * T * R) <= 1e-13 * want[4]  # at the corner: half the density of the resistor alone


def test_divider_closed_form():
    R1, R2, T = 3.0e3, 1.0e3, 300.0
    r = nr.NoiseReference(nr.divider_rows(R1, R2))
    S, H, (c1, c2) = nr.divider_closed_form(R1, R2, T)
    assert abs(S - 4.0 * BOLTZMANN * T * 750.0) <= 1e-15 * S and H == 0.25 and abs(c1 + c2 - S) <= 1e-15 * S
    c, gain = r.adjoint([1.0, 100.0], ["out", ("out", "out")], T, input="e1")
    keys = list(r.nl.component_keys)
    for f in range(2):
        assert abs(nr.density(c)[f, 0] - S) <= 1e-13 * S and abs(gain[f, 0] - H) <= 1e-13 * H
        assert abs(c[f, 0, keys.index("r1")] - c1) <= 1e-13 * c1 and abs(c[f, 0, keys.index("r2")] - c2) <= 1e-13 * c2
        assert not c[f, 1].any() and gain[f, 1] == 0
    assert np.abs(nr.density(r.direct([1.0, 100.0], ["out"], T))[:, 0] - S).max() <= 1e-13 * S
