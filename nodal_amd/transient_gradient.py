"""Gradients through time: the derivative of a loss of the transient waveforms with respect to every component value,
every capacitance, every swept source value and the initial state.

Someone who sizes decoupling capacitors or wire widths against a droop waveform gets the waveform from
`Circuit.transient`; its derivative by finite differences costs two full transient runs per component.  The steps of a
transient are coupled through the capacitors, so `Circuit.gradient` -- independent members -- does not apply.  The adjoint
of backward Euler is the same time stepping run backwards with the transposed matrix: `Circuit.transient(...,
record=True)` keeps the states on the device, and `Circuit.transient_gradient` hands the cotangents of the probe
waveforms to `nodal_transient_gradient` (csrc/transient_gradient.hip), which costs about one more transient run.  With
the reference the only way to the same numbers is finite differences over its host loop of rebuild and solve per step
(reference nodal/nodal.py:306-336).

`check_transient_gradient_arguments` needs no device, and `TransientGradient` is a plain container that can be built
from arrays.
"""

import numpy as np

NO_RECORD = "no recorded transient: call transient(..., record=True) first"


class TransientRecord:
    """What Circuit.transient(..., record=True) remembers for the gradient: the device context that holds the tape
    (`child`), dt, the farads [C] and their companion rows in the child's table, the swept rows' columns by name, steps,
    the probes as passed and as node indices, and x0 with whether it was the DC operating point."""

    def __init__(self, child, dt, farads, cap_rows, columns, nsrc, steps, probes, pa, pb, x0, dc_start):
        self.child, self.dt, self.farads, self.cap_rows = child, dt, farads, cap_rows
        self.columns, self.nsrc, self.steps = columns, nsrc, steps
        self.probes, self.pa, self.pb = list(probes), pa, pb
        self.x0, self.dc_start = x0, dc_start


def check_transient_gradient_arguments(record, wave_cotangents, nprobes):
    """The cotangents of Circuit.transient_gradient as float64 [steps + 1, nprobes].  ValueError when `record` is None
    (nothing recorded, or set_values() since), for another shape and for entries that are not finite."""
    if record is None:
        raise ValueError(NO_RECORD)
    cot = np.ascontiguousarray(wave_cotangents, dtype=np.float64)
    want = (record.steps + 1, int(nprobes))
    if cot.shape != want:
        raise ValueError(f"wave_cotangents must have shape {want}, not {cot.shape}")
    if not np.isfinite(cot).all():
        raise ValueError("wave_cotangents must be finite")
    return cot


class TransientGradient:
    """Result of Circuit.transient_gradient, for a loss L of the probe waveforms.

    values [ncomp]: dL / d value of table row i (rows in the order of `netlist.component_keys`, as
    Circuit.gradient(...).values): the part through the steps and, when the run started from the DC operating point,
    the part through that start (start_values [ncomp] alone; zeros with `initial=`); at a swept source the sum over the
    steps comes on top, nodal_gradient's convention.  capacitors [C]: dL / dC in the order the
    capacitors were passed.  source_values: name -> [steps], entry k-1 the derivative with respect to the value in
    force at t_k.  initial [K+B]: dL / dx_0.  info [steps]: 0 solved, > 0 singular (sparse path: NaN); scaled_residual
    [steps] of the backward solves, computed on the device; adjoints [steps, K+B] (lambda_1 .. lambda_steps) or None;
    timings: nodal_last_timings of the backward sweep, [0] the ms of matrix work done once (0.0: kept or not needed),
    [2] the whole call on the device."""

    def __init__(self, values, capacitors, source_values, initial, info, scaled_residual, adjoints=None, timings=None,
                 start_values=None):
        self.values = values
        self.capacitors = capacitors
        self.source_values = dict(source_values)
        self.initial = initial
        self.info = info
        self.scaled_residual = scaled_residual
        self.adjoints = adjoints
        self.timings = timings
        self.start_values = start_values

    def __len__(self):
        return len(self.info)
