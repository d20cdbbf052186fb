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

Bipolar transistors.  In the transport form of Ebers-Moll a transistor (name, "npn" | "pnp", i_s, beta_f, beta_r, n_vt,
collector, base, emitter) is two junction diodes with i_sat = i_s / beta_f (base-emitter) and i_s / beta_r
(base-collector) plus one transport current

    i_T = i_s (exp(v_f / n_vt) - exp(v_r / n_vt))

from collector to emitter that the two junction voltages control; a PNP is the same with every direction reversed,
which is nothing but another choice of leads.  The junctions join the call's diodes behind the caller's, and the
transport's linearisation is two `GM` table rows (gmf on the forward junction's voltage, -gmr on the reverse one's)
plus a history current, so the Newton matrix is the netlist's with one `R` row per junction and two `GM` rows per
transistor (`transistor_companion_table`) and the loop is `nodal_newton_dc_bjt`.  No Early effect, high injection,
ohmic resistances or charge storage.  `OperatingPoint.linearised()` is then the hybrid-pi model.  The same transistors
step in time in `Circuit.transient(transistors=...)` (`nodal_transient_nl_bjt`, transient.py): its DC start is this
analysis with the capacitors open and the inductors shorted, and its child's table holds the same two `GM` rows per
transistor behind the capacitors', inductors' and junctions' rows (`transient.bjt_companion_table`).

`resolve_diodes`, `resolve_transistors`, `check_operating_point_arguments`, `companion_table`,
`transistor_companion_table` and `check_cotangent` need no device, and `OperatingPoint` and `OperatingPointGradient` are
plain containers that can be built from arrays.
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


KINDS = {"npn": 1.0, "pnp": -1.0}


def resolve_transistors(netlist, transistors, first=0):
    """`transistors`, a sequence of (name, "npn" | "pnp", i_s, beta_f, beta_r, n_vt, collector, base, emitter), as
    (names, sign float64 [T] (+1 NPN, -1 PNP), junctions, ta, tb int32 [T], junction int32 [T, 2], i_s float64 [T]).
    `junctions` are the two junction diodes per transistor as resolve_diodes takes them, forward then reverse: an NPN's
    (name.be, i_s / beta_f, n_vt, base, emitter) and (name.bc, i_s / beta_r, n_vt, base, collector), a PNP's
    (name.eb, .., emitter, base) and (name.cb, .., collector, base).  They go BEHIND the caller's `first` diodes:
    junction[t] = (first + 2 t, first + 2 t + 1).  ta, tb: the transport's leads a (where i_T enters the element: an
    NPN's collector, a PNP's emitter) and b, -1 for the ground node.  ValueError as resolve_diodes (a label the netlist
    does not have, a name given twice, a name that a component of the netlist carries), for a kind other than the two
    and for i_s, beta_f, beta_r or n_vt that is not positive and finite.  A transistor with leads on one node is legal."""
    names, sign, junctions, ta, tb, i_s = [], [], [], [], [], []
    taken = set(netlist.component_keys)
    for transistor in transistors:
        if len(transistor) != 9:
            raise ValueError(f"Transistor {transistor!r} is not (name, kind, i_s, beta_f, beta_r, n_vt, collector, base, "
                             "emitter)")
        name, kind, sat, bf, br, nvt, col, base, emit = transistor
        if kind not in KINDS:
            raise ValueError(f"Transistor {name}: kind must be 'npn' or 'pnp', not {kind!r}")
        sat, bf, br, nvt = float(sat), float(bf), float(br), float(nvt)
        for label, value in (("i_s", sat), ("beta_f", bf), ("beta_r", br), ("n_vt", nvt)):
            if not (value > 0.0 and math.isfinite(value)):
                raise ValueError(f"Transistor {name}: {label} must be positive and finite, not {value}")
        if name in names:
            raise ValueError(f"Transistor {name} is given twice")
        if name in taken:
            raise ValueError(f"Transistor {name} has the name of a component of the netlist")
        try:
            nc, ne = _port_node(netlist, col), _port_node(netlist, emit)
            _port_node(netlist, base)
        except KeyError as exc:
            raise ValueError(f"Transistor {name}: {exc.args[0]}") from None
        if kind == "npn":
            junctions += [(f"{name}.be", sat / bf, nvt, base, emit), (f"{name}.bc", sat / br, nvt, base, col)]
            a, b = nc, ne
        else:
            junctions += [(f"{name}.eb", sat / bf, nvt, emit, base), (f"{name}.cb", sat / br, nvt, col, base)]
            a, b = ne, nc
        names.append(name)
        sign.append(KINDS[kind])
        ta.append(a)
        tb.append(b)
        i_s.append(sat)
    count = len(names)
    junction = (int(first) + np.arange(2 * count, dtype=np.int32)).reshape(count, 2)
    return (names, np.asarray(sign, dtype=np.float64).reshape(count), junctions,
            np.asarray(ta, dtype=np.int32).reshape(count), np.asarray(tb, dtype=np.int32).reshape(count), junction,
            np.asarray(i_s, dtype=np.float64).reshape(count))


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


def _grounded_where_same(ia, ib):
    """copies of the leads with every pair on one node moved to ground and ground: such a row stamps nothing"""
    ia, ib = np.array(ia, dtype=np.int32).reshape(-1), np.array(ib, dtype=np.int32).reshape(-1)
    same = ia == ib
    ia[same] = -1
    ib[same] = -1
    return ia, ib


def _with_transport_rows(table, ia, ib, ta, tb, junction, forward, reverse):
    """`table` with two `GM` rows per transport appended, forward then reverse: leads a, b the transport's, control
    leads c, d the (grounded-where-same) leads ia, ib of its junctions, values forward[t] and reverse[t].  Returns
    (table, gm_rows int64 [T, 2])."""
    ia, ib = _grounded_where_same(ia, ib)
    ta, tb = _grounded_where_same(ta, tb)
    junction = np.asarray(junction, dtype=np.int64).reshape(-1, 2)
    count = len(junction)
    a, b = np.repeat(ta, 2), np.repeat(tb, 2)
    cc, dd = ia[junction.reshape(-1)], ib[junction.reshape(-1)]
    values = np.stack([np.asarray(forward, dtype=np.float64).reshape(count),
                       np.asarray(reverse, dtype=np.float64).reshape(count)], axis=1).reshape(-1)
    types = np.full(2 * count, c.T_GM, dtype=np.uint8)
    first = table.ncomp
    out = table.with_controlled_rows_appended(types, values, a, b, cc, dd)
    return out, np.arange(first, first + 2 * count, dtype=np.int64).reshape(count, 2)


def transistor_companion_table(table, i_sat, n_vt, ia, ib, ta, tb, junction, i_s, gmin=0.0):
    """companion_table for a call with transistors: behind the `R` row of every diode (the junctions among them) two
    `GM` rows per transport -- the forward one reads its junction junction[t, 0], the reverse one junction[t, 1]; both
    carry the transport's leads ta[t], tb[t] as a, b and the junction row's leads as c, d.  Returns (table, rows int64
    [D], gm_rows int64 [T, 2]).  The values are the linearisation at v = 0, i_s / n_vt and -i_s / n_vt, placeholders
    that the device overwrites before every assembly.  A transport whose leads a and b are one node gets rows between
    ground and ground, which stamp nothing, as a junction on one node gets control leads ground and ground."""
    out, rows = companion_table(table, i_sat, n_vt, ia, ib, gmin)
    junction = np.asarray(junction, dtype=np.int64).reshape(-1, 2)
    n_vt, i_s = np.asarray(n_vt, dtype=np.float64), np.asarray(i_s, dtype=np.float64)
    out, gm_rows = _with_transport_rows(out, ia, ib, ta, tb, junction, i_s / n_vt[junction[:, 0]],
                                        -i_s / n_vt[junction[:, 1]])
    return out, rows, gm_rows


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
    "multigrid", or "direct": the sparse direct solve took the step over); transistors_not_converged (transports that
    failed theirs; zeros for a record of four words)."""

    def __init__(self, record, info, iterations, route):
        record = np.asarray(record, dtype=np.float64)
        # (a fifth word from a call that may carry transistors: the transports that failed their test)
        record = record.reshape(-1, 5 if record.ndim == 2 and record.shape[1] == 5 else 4)
        self.record = record
        with np.errstate(invalid="ignore"):
            self.transistors_not_converged = (np.nan_to_num(record[:, 4], nan=-1.0).astype(np.int64) if record.shape[1] == 5
                                              else np.zeros(len(record), dtype=np.int64))
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
    has None there and no circuit.

    With transistors (T of them; `diodes`, `voltages`, `currents`, `conductances` stay the CALLER's D diodes only):
    transistors: the names; junction_voltages [T, 2]: the forward (base-emitter) and reverse (base-collector) junction
    voltages, positive when the junction conducts; collector_currents, base_currents, emitter_currents [T]: positive
    INTO the terminal; transconductances [T, 2]: gmf and gmr of the transport current.  With keep_iterates
    limited_voltages has D + 2 T columns, the junctions' behind the caller's diodes.  `transport` holds what
    linearised() needs of them: (leads a, leads b, junction [T, 2], the junctions' conductances [2 T])."""

    def __init__(self, x, diodes, voltages, currents, conductances, converged, iterations, history, timings=None,
                 iterates=None, limited_voltages=None, circuit=None, leads=None, i_sat=None, n_vt=None, gmin=None,
                 source_rows=None, source_values=None, source_columns=None, transistors=(), junction_voltages=None,
                 collector_currents=None, base_currents=None, emitter_currents=None, transconductances=None,
                 transport=None):
        self.transistors = list(transistors)
        self.junction_voltages = junction_voltages
        self.collector_currents = collector_currents
        self.base_currents = base_currents
        self.emitter_currents = emitter_currents
        self.transconductances = transconductances
        self._transport = transport
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
        if self.transistors:
            raise ValueError("the adjoint with transistors is not implemented")
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
        is zero or not finite (a reverse-biased junction with gmin=0 whose exponential underflowed).

        With transistors it is the hybrid-pi model: every junction a resistor 1 / g like a diode, and behind them every
        transport as its two `GM` rows, gmf on the forward junction's voltage and -gmr on the reverse one's; ac(),
        ac_ports() and solve() run on it.  A `GM` row has no term in branches(), sensitivities() or gradient(): they
        give 0.0 for it, which is what the kernels do with such a row today."""
        if self._circuit is None:
            raise ValueError("this OperatingPoint was not made by Circuit.operating_point")
        circuit = self._circuit
        return type(circuit)._clone_of(circuit, self.linearised_table(circuit.table))

    def linearised_table(self, table):
        """linearised()'s table, from `table` (the circuit's): needs no device.  ValueError as linearised()."""
        g = np.asarray(self.conductances, dtype=np.float64)
        if self._transport is not None:
            g = np.concatenate([g, np.asarray(self._transport[3], dtype=np.float64)])
        if not (np.isfinite(g).all() and (g > 0.0).all()):
            raise ValueError("a conductance is zero or not finite: no small-signal resistor stands for that diode")
        # (a diode between a node and itself: a row between ground and ground stamps nothing)
        ia, ib = _grounded_where_same(*self._leads)
        types = np.full(len(g), c.TYPE_CODE["R"], dtype=np.uint8)
        out = table.with_rows_appended(types, 1.0 / g, ia, ib)
        if self._transport is not None:
            ta, tb, junction, _ = self._transport
            gm = np.asarray(self.transconductances, dtype=np.float64).reshape(-1, 2)
            if not np.isfinite(gm).all():
                raise ValueError("a transconductance is not finite: no small-signal row stands for that transistor")
            out, _ = _with_transport_rows(out, ia, ib, ta, tb, junction, gm[:, 0], -gm[:, 1])
        return out


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
