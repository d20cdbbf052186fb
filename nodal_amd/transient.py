"""Transient analysis: capacitors stepped in time on the device.

The dynamic counterpart of an IR-drop study: decoupling capacitors hang on the network, the load currents switch, and
the question is how far each node droops and when.  Under backward Euler a capacitor C between nodes a and b, stepped
with h, is a conductance C / h from a to b plus a history current rebuilt from the previous solution; under the
trapezoidal rule the conductance is 2 C / h.  So the transient matrix is that of the SAME netlist with one extra `R` row
per capacitor (`ComponentTable.with_rows_appended`), the existing assembly stamps it, and `Circuit.transient` hands the
steps to `nodal_transient` (csrc/transient.hip): one multigrid hierarchy or one factorisation serves every step, and the
history currents, probes and envelope are formed on the device.  With the reference the only way to the same numbers is
a host loop that rebuilds `Circuit(netlist with companion rows)` and solves it per step (reference nodal/nodal.py:306-336).

`check_transient_arguments`, `resolve_capacitors` and `companion_table` need no device, and `Transient` is a plain
container that can be built from arrays.
"""

import math

import numpy as np

from . import constants as c
from .ports import _port_node

METHODS = {"euler": 0, "trapezoidal": 1}


def check_transient_arguments(dt, steps, method, initial, n):
    """The scalar arguments of Circuit.transient.  Returns (dt, steps, method code, initial float64 [n] or None);
    ValueError for dt <= 0 or not finite, steps < 0, an unknown method, `initial` of another shape, and for the
    trapezoidal rule with `initial` given: it needs the capacitor currents at t_0, which are zero exactly when the
    start is a DC operating point."""
    dt = float(dt)
    if not (dt > 0.0 and math.isfinite(dt)):
        raise ValueError(f"dt must be positive and finite, not {dt}")
    if int(steps) != steps or steps < 0:
        raise ValueError(f"steps must be a non-negative integer, not {steps}")
    if method not in METHODS:
        raise ValueError(f"method must be one of {sorted(METHODS)}, not {method!r}")
    x0 = None
    if initial is not None:
        if method == "trapezoidal":
            raise ValueError('method="trapezoidal" starts from the DC operating point (the capacitor currents at t_0 '
                             'must be zero): leave `initial` out, or use method="euler"')
        x0 = np.ascontiguousarray(initial, dtype=np.float64)
        if x0.shape != (n,):
            raise ValueError(f"initial must have shape ({n},), not {x0.shape}")
    return dt, int(steps), METHODS[method], x0


def resolve_capacitors(netlist, capacitors):
    """`capacitors`, a sequence of (name, farads, node_a, node_b), as (names, farads float64 [C], ia, ib int32 [C]),
    -1 for the ground node.  KeyError for a label the netlist does not have (capacitors introduce no nodes),
    ValueError for farads <= 0 or not finite and for node_a == node_b."""
    names, farads, ia, ib = [], [], [], []
    for cap in capacitors:
        if len(cap) != 4:
            raise ValueError(f"Capacitor {cap!r} is not (name, farads, node_a, node_b)")
        name, value, a, b = cap
        value = float(value)
        if not (value > 0.0 and math.isfinite(value)):
            raise ValueError(f"Capacitor {name}: farads must be positive and finite, not {value}")
        na, nb = _port_node(netlist, a), _port_node(netlist, b)
        if na == nb:
            raise ValueError(f"Capacitor {name}: both leads on node {a}")
        names.append(name)
        farads.append(value)
        ia.append(na)
        ib.append(nb)
    return (names, np.asarray(farads, dtype=np.float64).reshape(len(names)),
            np.asarray(ia, dtype=np.int32).reshape(len(names)), np.asarray(ib, dtype=np.int32).reshape(len(names)))


def companion_table(table, farads, ia, ib, dt, method_code):
    """The table with one companion `R` row per capacitor appended: value dt / C (Euler) or dt / (2 C) (trapezoidal).
    Returns (table, rows int64 [C]): the appended rows' indices; the original rows keep theirs."""
    scale = 2.0 if method_code == METHODS["trapezoidal"] else 1.0
    values = dt / (scale * np.asarray(farads, dtype=np.float64))
    types = np.full(len(values), c.TYPE_CODE["R"], dtype=np.uint8)
    return table.with_rows_appended(types, values, ia, ib), np.arange(table.ncomp, table.ncomp + len(values), dtype=np.int64)


class TransientEnvelope:
    """Per node the lowest and highest potential over steps 1..steps and a step that attains each (among exact ties the
    lowest; steps with info > 0 are left out; NaN and -1 when every step is)."""

    def __init__(self, potential_min, potential_min_step, potential_max, potential_max_step):
        self.potential_min = potential_min
        self.potential_min_step = potential_min_step
        self.potential_max = potential_max
        self.potential_max_step = potential_max_step


class Transient:
    """Result of Circuit.transient.

    t [steps + 1]; waveforms [steps + 1, P], row 0 read from the initial state; probes as passed; solutions
    [steps // keep_every, K+B] or None and solution_steps, the steps they belong to; envelope (TransientEnvelope) or None;
    info [steps]: 0 solved, > 0 singular (sparse path: NaN); scaled_residual [steps], computed on the device; iterations
    [steps].  timings: nodal_last_timings of the call, [0] the ms of the matrix work done once (0.0: it was kept from an
    earlier call), [2] the whole call on the device."""

    def __init__(self, t, waveforms, probes, info, scaled_residual, iterations, solutions=None, solution_steps=None,
                 envelope=None, timings=None):
        self.t = t
        self.waveforms = waveforms
        self.probes = list(probes)
        self.info = info
        self.scaled_residual = scaled_residual
        self.iterations = iterations
        self.solutions = solutions
        self.solution_steps = solution_steps if solution_steps is not None else np.zeros(0, dtype=np.int64)
        self.envelope = envelope
        self.timings = timings

    def __len__(self):
        return len(self.info)
