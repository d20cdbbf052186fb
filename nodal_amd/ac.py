"""AC analysis: the steady state of an RLC network over a list of frequencies, solved on the device.

The first question asked of a network with capacitors and inductors: impedance against frequency, the resonance of a
decoupling network, the -3 dB point of a filter (SPICE's `.ac`).  At the angular frequency w a capacitor C is the
admittance j w C and an inductor L the admittance 1 / (j w L), so with B(w) the matrix that stamps every reactive
element like a conductance of its susceptance (w C, or -1 / (w L)) the phasors solve (G + j B) x = s.  `Circuit.ac`
hands the whole sweep to `nodal_ac_sweep` (csrc/ac.hip), which solves the real system of twice the size per frequency on
the circuit's own device context: the reactive elements are arguments, not table rows, so nothing is uploaded or
assembled again, and the pattern and the symbolic analysis of the doubled system are kept between calls.  With the
reference the only ways to the same numbers are a transient run per frequency, long enough to settle, with an amplitude
fit afterwards, or exporting G and solving G + j B per frequency on the host.

The excitation is small-signal: every independent source is off except the ones that are named, each with a complex
amplitude that stays constant over the sweep.

`check_ac_arguments` and `resolve_reactive` need no device, and `ACSweep` / `ACPeaks` are plain containers that can be
built from arrays.
"""

import math

import numpy as np

from .ports import _port_node

CAPACITOR, INDUCTOR = 0, 1


def check_ac_arguments(frequencies):
    """The frequencies of Circuit.ac, in Hz, as omega = 2.0 * math.pi * f in rad/s, float64 [F].  ValueError for anything
    but a flat sequence and for a frequency that is not finite and > 0."""
    f = np.asarray(frequencies, dtype=np.float64)
    if f.ndim != 1:
        raise ValueError(f"frequencies must be a flat sequence, not of shape {f.shape}")
    for value in f.tolist():
        if not (value > 0.0 and math.isfinite(value)):
            raise ValueError(f"frequencies must be positive and finite, not {value}")
    return np.asarray([2.0 * math.pi * value for value in f.tolist()], dtype=np.float64).reshape(len(f))


def resolve_reactive(netlist, capacitors=(), inductors=()):
    """`capacitors` and `inductors`, sequences of (name, value, node_a, node_b) as Circuit.transient takes them, as
    (names, kind uint8 [E], value float64 [E], ia, ib int32 [E]): the capacitors (kind 0, farads) first, then the
    inductors (kind 1, henries), -1 for the ground node.  KeyError for a label the netlist does not have (reactive
    elements introduce no nodes), ValueError for a value <= 0 or not finite, for node_a == node_b and for a name given
    twice.  Loops of inductors are legal here: there is no DC start."""
    names, kind, values, ia, ib = [], [], [], [], []
    for code, what, unit, elements in ((CAPACITOR, "Capacitor", "farads", capacitors), (INDUCTOR, "Inductor", "henries", inductors)):
        for element in elements:
            if len(element) != 4:
                raise ValueError(f"{what} {element!r} is not (name, {unit}, node_a, node_b)")
            name, value, a, b = element
            value = float(value)
            if not (value > 0.0 and math.isfinite(value)):
                raise ValueError(f"{what} {name}: {unit} must be positive and finite, not {value}")
            na, nb = _port_node(netlist, a), _port_node(netlist, b)
            if na == nb:
                raise ValueError(f"{what} {name}: both leads on node {a}")
            if name in names:
                raise ValueError(f"{what} {name} is given twice")
            names.append(name)
            kind.append(code)
            values.append(value)
            ia.append(na)
            ib.append(nb)
    count = len(names)
    return (names, np.asarray(kind, dtype=np.uint8).reshape(count), np.asarray(values, dtype=np.float64).reshape(count),
            np.asarray(ia, dtype=np.int32).reshape(count), np.asarray(ib, dtype=np.int32).reshape(count))


def resolve_amplitudes(netlist, sources):
    """`sources` of Circuit.ac, a mapping of names of A / E components to complex amplitudes (None: every source off),
    as (rows int64 [R], amplitudes complex128 [R]).  TypeError / KeyError / ValueError as solve_sources gives them; a
    name the netlist defines more than once drives every row that carries it."""
    from .sweep import resolve_sources
    if sources is None:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.complex128)
    if not hasattr(sources, "items"):
        raise TypeError("sources must map component names to complex amplitudes")
    amplitudes = {}
    for name, value in sources.items():
        value = complex(value)
        if not (math.isfinite(value.real) and math.isfinite(value.imag)):
            raise ValueError(f"The amplitude of {name} must be finite, not {value}")
        amplitudes[name] = value
    rows, re = resolve_sources(netlist, {name: [value.real] for name, value in amplitudes.items()})
    _, im = resolve_sources(netlist, {name: [value.imag] for name, value in amplitudes.items()})
    if not len(rows):
        return rows, np.zeros(0, dtype=np.complex128)
    return rows, re[0] + 1j * im[0]


class ACPeaks:
    """Per node the largest magnitude of its potential over the solved frequencies and the index of a frequency that
    attains it (among exact ties the lowest; frequencies with info > 0 are left out; NaN and -1 when every one is)."""

    def __init__(self, magnitude, frequency_index):
        self.magnitude = magnitude
        self.frequency_index = frequency_index


class ACSweep:
    """Result of Circuit.ac.

    frequencies [F] in Hz and omega [F] in rad/s; phasors complex128 [F, P], the probes' voltages; probes as passed;
    currents complex128 [F, Q], the currents of the elements named in current_probes, from lead a to lead b; solutions
    complex128 [F // keep_every, K+B] or None and solution_indices, the frequencies they belong to; peaks (ACPeaks) or
    None; info [F]: 0 solved, > 0 singular at that frequency (sparse path: NaN in its rows); scaled_residual [F] of the
    real system of twice the size, computed on the device.  timings: nodal_last_timings of the call, [0] the host ms of
    the doubled system's pattern and symbolic analysis (0.0: both were kept from an earlier call), [1] the ms of the
    numeric factorisations, [2] the whole call on the device."""

    def __init__(self, frequencies, omega, phasors, probes, info, scaled_residual, currents=None, current_probes=(),
                 solutions=None, solution_indices=None, peaks=None, timings=None):
        self.frequencies = frequencies
        self.omega = omega
        self.phasors = phasors
        self.probes = list(probes)
        self.info = info
        self.scaled_residual = scaled_residual
        self.currents = currents if currents is not None else np.zeros((len(frequencies), 0), dtype=np.complex128)
        self.current_probes = list(current_probes)
        self.solutions = solutions
        self.solution_indices = solution_indices if solution_indices is not None else np.zeros(0, dtype=np.int64)
        self.peaks = peaks
        self.timings = timings

    def __len__(self):
        return len(self.info)

    def magnitude_db(self):
        """20 log10 |phasors|, [F, P]; -inf where a phasor is exactly zero."""
        with np.errstate(divide="ignore"):
            return 20.0 * np.log10(np.abs(self.phasors))

    def phase_deg(self):
        """The phasors' arguments in degrees, (-180, 180], [F, P]."""
        return np.degrees(np.angle(self.phasors))
