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

Gradients through the operating point.  At the answer F(x, p) = G(p) x + S i(S^T x; theta) - A(p) = 0, so a loss L(x) has
dL/dp = -lambda^T dF/dp with J^T lambda = dL/dx, J = G + S diag(g(v)) S^T at v = S^T x: ONE linear solve with the matrix a
Newton iteration assembles, linearised at the answer itself.  `OperatingPoint.gradient` hands the cotangent to
`nodal_newton_gradient` (csrc/newton_gradient.hip) and returns an `OperatingPointGradient`: a number per component, two
per diode (i_sat, n_vt), one for gmin and one per source named in the call.  The other routes are finite differences, two
Newton runs per parameter, and `linearised().gradient(...)`, which answers another question: its x is the last Newton
step without the history currents, and its companion resistors are constants.

`resolve_diodes`, `check_operating_point_arguments`, `companion_table` and `check_cotangent` need no device, and
`OperatingPoint` and `OperatingPointGradient` are plain containers that can be built from arrays.
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


def check_cotangent(cotangent, n):
    """`cotangent` = dL/dx as float64 [n]; ValueError for another shape or entries that are not finite."""
    cot = np.ascontiguousarray(cotangent, dtype=np.float64)
    if cot.shape != (n,):
        raise ValueError(f"cotangent must have shape ({n},), not {cot.shape}")
    if not np.isfinite(cot).all():
        raise ValueError("cotangent has entries that are not finite")
    return cot


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
    keep_iterates: iterates [iterations, K+B], x_1 .. , and limited_voltages [iterations + 1, D], vh_0 .. .

    What gradient() needs beside x is remembered when Circuit.operating_point makes the result: i_sat, n_vt [D] and
    gmin of the diodes, source_rows / source_values (the table rows and the one value each of the sources named in the
    call) and source_columns (name -> the entries of source_rows that carry it).  A result built from arrays alone
    has None there and no circuit."""

    def __init__(self, x, diodes, voltages, currents, conductances, converged, iterations, history, timings=None,
                 iterates=None, limited_voltages=None, circuit=None, leads=None, i_sat=None, n_vt=None, gmin=None,
                 source_rows=None, source_values=None, source_columns=None):
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
        self.i_sat = i_sat
        self.n_vt = n_vt
        self.gmin = gmin
        self.source_rows = source_rows
        self.source_values = source_values
        self.source_columns = source_columns

    @property
    def scaled_residual(self):
        return float(self.history.scaled_residual[-1]) if len(self.history) else float("nan")

    def gradient(self, cotangent, adjoints=False):
        """The gradient of a scalar loss L(x) through this operating point, by the adjoint method on the device
        (nodal_newton_gradient): `cotangent` [K+B] = dL/dx.  One linear solve with J^T, J = G + S diag(g(v)) S^T the
        matrix of a Newton iteration linearised at x ITSELF -- the run's last linearisation is at the limited voltages
        one step behind, which with default tolerances is an error in the fourth digit -- and then a formula per
        table row, two per diode and one for gmin.  Returns an OperatingPointGradient.

        The gradient is taken at the circuit's values IN FORCE: after set_values() the matrix is the new one while x
        is this result's, and `operating_point_residual` -- the scaled residual of x in the nonlinear equations, at
        roundoff for a converged result -- is how a caller sees that they moved (or that the run had not converged).
        ValueError for a cotangent of another shape or with entries that are not finite, for a result without its
        circuit and for one whose x is not finite (a lost run).  Singular networks behave as in Circuit.gradient():
        the dense path raises LinAlgError / UnconnectedCircuitError, the sparse path returns NaN with info > 0 and
        warns once.  A second call repeats no symbolic work (`timings[1] == 0.0`) and gives the same bits; the circuit
        itself is left as it was."""
        if self._circuit is None or self.i_sat is None:
            raise ValueError("this OperatingPoint was not made by Circuit.operating_point")
        x = np.ascontiguousarray(self.x, dtype=np.float64)
        cot = check_cotangent(cotangent, len(x))
        if not np.isfinite(x).all():
            raise ValueError("this operating point is not finite (a lost run): there is nothing to differentiate")
        return self._circuit._operating_point_gradient(self, x, cot, adjoints)

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


class OperatingPointGradient:
    """Result of OperatingPoint.gradient: the implicit part of dL/dp, what the loss owes to the operating point's
    dependence on the parameters.

    values [ncomp]: dL / d value of table row i, in the order of `netlist.component_keys` (the array handed in may
    carry the diodes' companion rows behind them: they are cut off); diodes: the names; i_sat, n_vt [D]: dL/di_sat and
    dL/dn_vt of every diode; gmin: dL/dgmin (a float); source_values: name -> dL / d value of a source named in the
    operating_point call (a float); adjoint [K+B] (lambda) or None; scaled_residual of the solve J^T lambda = dL/dx;
    operating_point_residual: the scaled residual of x in the nonlinear equations at the circuit's values in force;
    info: 0 solved, > 0 singular (sparse path: NaN); timings: nodal_last_timings of the call."""

    def __init__(self, netlist, values, diodes, i_sat, n_vt, gmin, source_values, info, scaled_residual,
                 operating_point_residual, adjoint=None, timings=None, table=None, diode_i_sat=None, diode_n_vt=None):
        self._netlist = netlist
        self.values = np.asarray(values, dtype=np.float64)[:len(netlist.component_keys)]
        self.diodes = list(diodes)
        self.i_sat = np.asarray(i_sat, dtype=np.float64)
        self.n_vt = np.asarray(n_vt, dtype=np.float64)
        self.gmin = float(gmin)
        self.source_values = {name: float(value) for name, value in dict(source_values).items()}
        self.info = int(info)
        self.scaled_residual = float(scaled_residual)
        self.operating_point_residual = float(operating_point_residual)
        self.adjoint = adjoint
        self.timings = timings
        self._table = table
        self._diode_i_sat, self._diode_n_vt = diode_i_sat, diode_n_vt
        self._rows = None

    @property
    def names(self):
        return list(self._netlist.component_keys)

    def of(self, name):
        """(dL/di_sat, dL/dn_vt) for a diode's name; dL / d value for a component's name -- one the netlist defines
        more than once: the sum over its rows, as Gradient.of."""
        if name in self.diodes:
            d = self.diodes.index(name)
            return float(self.i_sat[d]), float(self.n_vt[d])
        if self._rows is None:
            from .sweep import _row_map
            self._rows = _row_map(self._netlist)
        return float(self.values[self._rows[name]].sum())

    @property
    def normalized(self):
        """(values * component value [ncomp], i_sat * dL/di_sat [D], n_vt * dL/dn_vt [D]): the change of the loss per
        relative change of each parameter.  ValueError when the container was built without the diodes' parameters."""
        if self._diode_i_sat is None or self._diode_n_vt is None:
            raise ValueError("this OperatingPointGradient was built without the diodes' i_sat and n_vt")
        if self._table is None:
            from .circuit import Circuit
            self._table = Circuit._lower(self._netlist)
        value = np.asarray(self._table.value, dtype=np.float64)[:len(self.values)]
        return (self.values * value, self.i_sat * np.asarray(self._diode_i_sat, dtype=np.float64),
                self.n_vt * np.asarray(self._diode_n_vt, dtype=np.float64))
