"""Noise analysis: the thermal-noise density at chosen outputs of an RLC network over a list of frequencies.

The third of a simulator's small-signal analyses (SPICE's `.noise`, after `.ac` and `.tran`): how many V/sqrt(Hz) appear at
an output, and which resistors put them there.  A resistor R at the temperature T is a current source of the density
4 k_B T / R in parallel with it; what it adds at an output is that density times the squared magnitude of the transfer
impedance from its leads to the output.  Direct solves would need one per resistor.  With A(w) = G + j B(w) the matrix of
`Circuit.ac`, one ADJOINT solve per output, A(w)^T y = e(out+) - e(out-), gives every resistor's transfer at once -- it is
y(a) - y(b) across the resistor's leads -- and the gain from an input source besides, H = y^T s.  `Circuit.noise` hands
the whole sweep to `nodal_ac_noise` (csrc/noise.hip): one numeric factorisation per frequency whatever the number of
outputs, one pass over the component table on the device per block of sixteen outputs, and the contributions integrated
over the frequencies on the device, so that [P, ncomp] numbers come down and never [F, P, ncomp].

Only resistors with a positive value make noise here: sources, dependent elements, capacitors and inductors are
noiseless, and one temperature holds for the whole network.

`check_noise_arguments` and `trapezoid_weights` need no device, and `NoiseSweep` is a plain container that can be built
from arrays.
"""

import math

import numpy as np

BOLTZMANN = 1.380649e-23  # J / K, the exact SI value


def check_noise_arguments(temperature, contributions, frequencies):
    """The temperature of Circuit.noise as a float: ValueError unless it is finite and > 0 (kelvin).  With
    `contributions` the frequencies (Hz) must be strictly increasing, because the contributions are integrated over
    them: ValueError otherwise."""
    temperature = float(temperature)
    if not (temperature > 0.0 and math.isfinite(temperature)):
        raise ValueError(f"temperature must be positive and finite (kelvin), not {temperature}")
    if contributions:
        f = np.asarray(frequencies, dtype=np.float64)
        if f.ndim == 1 and len(f) > 1 and not (np.diff(f) > 0.0).all():
            raise ValueError("frequencies must be strictly increasing when contributions are integrated over them")
    return temperature


def trapezoid_weights(frequencies):
    """w [F] with sum(w * y) the trapezoid rule of y over `frequencies` (Hz): half the distance to each neighbour.
    A single frequency, or none, integrates to zero."""
    f = np.asarray(frequencies, dtype=np.float64).reshape(-1)
    w = np.zeros(len(f), dtype=np.float64)
    if len(f) > 1:
        half = 0.5 * np.diff(f)
        w[:-1] += half
        w[1:] += half
    return w


class NoiseSweep:
    """Result of Circuit.noise.

    frequencies [F] in Hz and omega [F] in rad/s; outputs as passed; density [F, P] in V^2/Hz, the thermal noise of
    every resistor summed at each output; gain complex128 [F, P], the transfer from the input source to each output, and
    input_density [F, P] = density / |gain|^2 in the input's unit squared per Hz, both None without an input;
    contributions [P, ncomp] in V^2 in the order of `netlist.component_keys`, every component's share of integrated(),
    exactly 0.0 for whatever makes no noise, or None, and names, those keys (what top() reports); info [F]: 0 solved, > 0 singular at that frequency (sparse path:
    NaN in its rows, and NaN in every integrated quantity); scaled_residual [F, P] of every output's real system of twice
    the size, computed on the device.  timings: nodal_last_timings of the call, [0] the host ms of the transposed
    system's pattern and symbolic analysis (0.0: both were kept from an earlier call), [1] the ms of the numeric
    factorisations, [2] the whole call on the device."""

    def __init__(self, frequencies, omega, outputs, density, info, scaled_residual, gain=None, input_density=None,
                 contributions=None, names=None, timings=None):
        self.frequencies = frequencies
        self.omega = omega
        self.outputs = list(outputs)
        self.density = density
        self.info = info
        self.scaled_residual = scaled_residual
        self.gain = gain
        self.input_density = input_density
        self.contributions = contributions
        self.names = names
        self.timings = timings

    def __len__(self):
        return len(self.info)

    def amplitude_density(self):
        """sqrt(density), [F, P] in V/sqrt(Hz)."""
        return np.sqrt(self.density)

    def integrated(self):
        """The mean square noise voltage of each output over the band the frequencies span, [P] in V^2: the trapezoid
        rule over `density`.  NaN when a frequency was singular."""
        return trapezoid_weights(self.frequencies) @ self.density if len(self.frequencies) else np.zeros(len(self.outputs))

    def rms(self):
        """sqrt(integrated()), [P] in volts."""
        return np.sqrt(self.integrated())

    def top(self, p, count=10):
        """The `count` largest contributors to output p as [(name, integrated contribution in V^2)], largest first;
        ties keep the table's order.  ValueError when the sweep was made without contributions."""
        if self.contributions is None:
            raise ValueError("the sweep was made without contributions: pass contributions=True")
        row = self.contributions[p]
        order = np.argsort(-row, kind="stable")[:max(int(count), 0)]
        names = self.names if self.names is not None else list(range(len(row)))
        return [(names[k], float(row[k])) for k in order.tolist()]
