"""Nonlinear DC analysis: the operating point of a network with diodes, by Newton's method on the device.

Clamp diodes on a power grid, a rectifier, an ESD network: the first question after "linear DC" is the DC operating point
with junctions in the network.  A diode (name, i_sat, n_vt, anode, cathode) carries

    i(v) = i_sat (exp(v / n_vt) - 1) + gmin v,    v = x(anode) - x(cathode),

counted positive from anode to cathode; n_vt is in volts (emission coefficient times thermal voltage).  Linearised at a
junction voltage vh it is a conductance g = i_sat exp(vh / n_vt) / n_vt + gmin from anode to cathode plus a current
J = g vh - i(vh) injected into the anode and drawn from the cathode, so the Newton matrix is that of the SAME netlist
with one extra `R` row per diode (`ComponentTable.with_rows_appended`, as transient()'s capacitors), and an iteration is
"change D values, assemble, solve".  `Circuit.operating_point` hands the loop to `nodal_newton_dc` (csrc/newton.hip):
the diode pass, SPICE's junction limiting and the convergence test run on the device, the value column never leaves it,
and the assembly's symbolic phase, the sparse LU's analysis and the multigrid hierarchy's symbolic setup are kept over
the iterations and over later calls.  With the reference the only way to the same numbers is a host loop that rebuilds
`Circuit(netlist with companion rows)` and solves it per iteration (reference nodal/nodal.py:306-336).

`resolve_diodes`, `check_operating_point_arguments` and `companion_table` need no device, and `OperatingPoint` is a plain
container that can be built from arrays.
"""

import math

import numpy as np

from . import constants as c
from .ports import _port_node


def resolve_diodes(netlist, diodes):
    """`diodes`, a sequence of (name, i_sat, n_vt, anode, cathode), as (names, i_sat float64 [D], n_vt float64 [D], ia,
    ib int32 [D]), -1 for the ground node.  ValueError for a label the netlist does not have (diodes introduce no
    nodes), for i_sat or n_vt that is not positive and finite, for a name given twice and for a name that a component
    of the netlist carries.  A diode with both leads on one node is legal and carries nothing."""
    names, i_sat, n_vt, ia, ib = [], [], [], [], []
    taken = set(netlist.component_keys)
    for diode in diodes:
        if len(diode) != 5:
            raise ValueError(f"Diode {diode!r} is not (name, i_sat, n_vt, anode, cathode)")
        name, sat, nvt, a, b = diode
        sat, nvt = float(sat), float(nvt)
        if not (sat > 0.0 and math.isfinite(sat)):
            raise ValueError(f"Diode {name}: i_sat must be positive and finite, not {sat}")
        if not (nvt > 0.0 and math.isfinite(nvt)):
            raise ValueError(f"Diode {name}: n_vt must be positive and finite, not {nvt}")
        if name in names:
            raise ValueError(f"Diode {name} is given twice")
        if name in taken:
            raise ValueError(f"Diode {name} has the name of a component of the netlist")
        try:
            na, nb = _port_node(netlist, a), _port_node(netlist, b)
        except KeyError as exc:
            raise ValueError(f"Diode {name}: {exc.args[0]}") from None
        names.append(name)
        i_sat.append(sat)
        n_vt.append(nvt)
        ia.append(na)
        ib.append(nb)
    count = len(names)
    return (names, np.asarray(i_sat, dtype=np.float64).reshape(count), np.asarray(n_vt, dtype=np.float64).reshape(count),
            np.asarray(ia, dtype=np.int32).reshape(count), np.asarray(ib, dtype=np.int32).reshape(count))


def check_operating_point_arguments(max_iter, reltol, vntol, abstol, gmin, initial, n):
    """The scalar arguments of Circuit.operating_point.  Returns (max_iter, reltol, vntol, abstol, gmin, initial float64
    [n] or None); ValueError for max_iter < 1, a negative or not finite tolerance or gmin, and an `initial` of another
    shape or with entries that are not finite."""
    if int(max_iter) != max_iter or max_iter < 1:
        raise ValueError(f"max_iter must be a positive integer, not {max_iter}")
    out = []
    for label, value in (("reltol", reltol), ("vntol", vntol), ("abstol", abstol), ("gmin", gmin)):
        value = float(value)
        if not (value >= 0.0 and math.isfinite(value)):
            raise ValueError(f"{label} must be finite and not negative, not {value}")
        out.append(value)
    x0 = None
    if initial is not None:
        x0 = np.ascontiguousarray(initial, dtype=np.float64)
        if x0.shape != (n,):
            raise ValueError(f"initial must have shape ({n},), not {x0.shape}")
        if not np.isfinite(x0).all():
            raise ValueError("initial has entries that are not finite")
    return (int(max_iter), *out, x0)


def companion_table(table, i_sat, n_vt, ia, ib, gmin=0.0):
    """The table with one companion `R` row per diode appended.  Returns (table, rows int64 [D]): the appended rows'
    indices; the original rows keep theirs.  A row's value is 1 / (i_sat / n_vt + gmin), the linearisation at v = 0 --
    a placeholder that makes the table a legal one: the device overwrites it before every assembly.  A diode with both
    leads on one node gets a row between ground and ground, which stamps nothing at all."""
    i_sat, n_vt = np.asarray(i_sat, dtype=np.float64), np.asarray(n_vt, dtype=np.float64)
    ia, ib = np.array(ia, dtype=np.int32).reshape(-1), np.array(ib, dtype=np.int32).reshape(-1)
    same = ia == ib
    ia[same] = -1
    ib[same] = -1
    values = 1.0 / (i_sat / n_vt + gmin)
    types = np.full(len(values), c.TYPE_CODE["R"], dtype=np.uint8)
    first = table.ncomp
    return table.with_rows_appended(types, values, ia, ib), np.arange(first, first + len(values), dtype=np.int64)


ROUTES = {0: "dense", 1: "lu", 2: "multigrid", 3: "direct"}


class NewtonHistory:
    """The iterations of an operating point, one entry per iteration: not_converged (diodes that failed the test),
    limited (diodes whose voltage the junction limiting changed), max_step (max |v - vh|), scaled_residual of the
    iteration's linear solve, info (0 solved, > 0 singular), iterations of the linear solver, and route ("dense", "lu",
    "multigrid", or "direct": the sparse direct solve took the step over)."""

    def __init__(self, record, info, iterations, route):
        record = np.asarray(record, dtype=np.float64).reshape(-1, 4)
        self.record = record
        with np.errstate(invalid="ignore"):
            self.not_converged = np.nan_to_num(record[:, 0], nan=-1.0).astype(np.int64)
            self.limited = np.nan_to_num(record[:, 1], nan=-1.0).astype(np.int64)
        self.max_step = record[:, 2].copy()
        self.scaled_residual = record[:, 3].copy()
        self.info = np.asarray(info, dtype=np.int32)
        self.iterations = np.asarray(iterations, dtype=np.int32)
        self.route = [ROUTES.get(int(r), "none") for r in route]

    def __len__(self):
        return len(self.info)


class OperatingPoint:
    """Result of Circuit.operating_point.

    x [K+B]: the last iterate; diodes: the names; voltages, currents, conductances [D]: v, i(v) and g(v) = di/dv of
    every diode there; converged; iterations; history (NewtonHistory); scaled_residual: that of the last iteration's
    linear solve; timings: nodal_last_timings of the call, [0] the host ms of the matrix work summed over the
    iterations, [1] the part of it that was symbolic (0.0: everything symbolic was kept), [2] the whole call.  With
    keep_iterates: iterates [iterations, K+B], x_1 .. , and limited_voltages [iterations + 1, D], vh_0 .. ."""

    def __init__(self, x, diodes, voltages, currents, conductances, converged, iterations, history, timings=None,
                 iterates=None, limited_voltages=None, circuit=None, leads=None):
        self.x = x
        self.diodes = list(diodes)
        self.voltages = voltages
        self.currents = currents
        self.conductances = conductances
        self.converged = bool(converged)
        self.iterations = int(iterations)
        self.history = history
        self.timings = timings
        self.iterates = iterates
        self.limited_voltages = limited_voltages
        self._circuit = circuit
        self._leads = leads

    @property
    def scaled_residual(self):
        return float(self.history.scaled_residual[-1]) if len(self.history) else float("nan")

    def linearised(self):
        """The small-signal circuit at this operating point: a Circuit on the same netlist whose table has every diode
        as a resistor 1 / conductance behind the netlist's rows.  Its ac(), noise(), thevenin(sources=False) and the
        rest are the small-signal analyses at this point; its solve() is the last Newton step WITHOUT the diodes'
        history currents, not the operating point.  ValueError for a result without its circuit, or when a conductance
        is zero or not finite (a reverse-biased junction with gmin=0 whose exponential underflowed)."""
        if self._circuit is None:
            raise ValueError("this OperatingPoint was not made by Circuit.operating_point")
        g = np.asarray(self.conductances, dtype=np.float64)
        if not (np.isfinite(g).all() and (g > 0.0).all()):
            raise ValueError("a conductance is zero or not finite: no small-signal resistor stands for that diode")
        ia, ib = (np.array(lead, dtype=np.int32) for lead in self._leads)
        same = ia == ib  # (a diode between a node and itself: a row between ground and ground stamps nothing)
        ia[same] = -1
        ib[same] = -1
        circuit = self._circuit
        types = np.full(len(g), c.TYPE_CODE["R"], dtype=np.uint8)
        return type(circuit)._clone_of(circuit, circuit.table.with_rows_appended(types, 1.0 / g, ia, ib))
