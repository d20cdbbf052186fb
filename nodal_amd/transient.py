"""Transient analysis: capacitors and inductors stepped in time on the device.

The dynamic counterpart of an IR-drop study: decoupling capacitors hang on the network, the load currents switch, and
the question is how far each node droops and when.  Under backward Euler a capacitor C between nodes a and b, stepped
with h, is a conductance C / h from a to b plus a history current rebuilt from the previous solution; under the
trapezoidal rule the conductance is 2 C / h.  So the transient matrix is that of the SAME netlist with one extra `R` row
per capacitor (`ComponentTable.with_rows_appended`), the existing assembly stamps it, and `Circuit.transient` hands the
steps to `nodal_transient` (csrc/transient.hip): one multigrid hierarchy or one factorisation serves every step, and the
history currents, probes and envelope are formed on the device.  With the reference the only way to the same numbers is
a host loop that rebuilds `Circuit(netlist with companion rows)` and solves it per step (reference nodal/nodal.py:306-336).

An inductor L between a and b is again a conductance, h / L (Euler) or h / (2 L) (trapezoidal), plus a history current,
so it is one more companion `R` row behind the capacitors'; its state is its current i, positive from a to b through the
element, kept per inductor on the device (`nodal_transient_rlc`).  At DC an inductor is a short: with inductors the start
is the solution of the netlist with one zero-volt `E` row per inductor (`dc_table`), whose branch unknown is the current
INTO lead a out of the element, so i_0 is its negative.

With diodes (`Circuit.transient(diodes=...)`, `nodal_transient_nl`, csrc/transient_nl.hip) every step is a Newton
iteration on the device: the diodes' companion rows stand behind the inductors' (`diode_companion_table`), the step's
sources and history currents are formed once and held fixed, and an iteration whose junction conductances did not move
by a bit re-uses the factorisation or the hierarchy.  Out of scope: adaptive time steps, junction capacitance, the
adjoint of such a run, a presolve route, and a hierarchy kept as a preconditioner while only level 0 follows the matrix.

With bipolar transistors (`Circuit.transient(transistors=...)`, `nodal_transient_nl_bjt`) the same Newton iteration
carries operating_point.py's Ebers-Moll transports: the two junctions of every transistor join the diodes behind the
caller's, two `GM` rows per transistor stand behind all the diodes' rows (`bjt_companion_table`), and a step has
converged when no diode and no transport fails.  Such a run assembles in every iteration: a transconductance has no gmin
floor, so its bits move whenever a junction voltage moves.  No charge storage, Early effect or ohmic resistances: a fixed
junction capacitance is a `capacitors` entry.

`check_transient_arguments`, `resolve_capacitors`, `resolve_inductors`, `companion_table`, `diode_companion_table`,
`bjt_companion_table`, `check_diode_probes`, `check_transistor_probes` and `dc_table` need no device,
and `Transient` is a plain container that can be built from arrays.
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


def resolve_inductors(netlist, inductors):
    """`inductors`, a sequence of (name, henries, node_a, node_b), as (names, henries float64 [L], ia, ib int32 [L]),
    -1 for the ground node.  KeyError for a label the netlist does not have (inductors introduce no nodes), ValueError
    for henries <= 0 or not finite, for node_a == node_b, for a name given twice and for a loop made of inductors alone
    (ground is one node; two inductors in parallel are such a loop): at DC every inductor is a short, and a loop of
    shorts makes the start singular whatever the rest of the network is."""
    names, henries, ia, ib = [], [], [], []
    parent = {}

    def find(x):  # union-find over the inductors' leads
        root = x
        while parent.setdefault(root, root) != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for ind in inductors:
        if len(ind) != 4:
            raise ValueError(f"Inductor {ind!r} is not (name, henries, node_a, node_b)")
        name, value, a, b = ind
        value = float(value)
        if not (value > 0.0 and math.isfinite(value)):
            raise ValueError(f"Inductor {name}: henries must be positive and finite, not {value}")
        na, nb = _port_node(netlist, a), _port_node(netlist, b)
        if na == nb:
            raise ValueError(f"Inductor {name}: both leads on node {a}")
        if name in names:
            raise ValueError(f"Inductor {name} is given twice")
        ra, rb = find(na), find(nb)
        if ra == rb:
            raise ValueError(f"Inductor {name} closes a loop of inductors: the DC start (every inductor a short) is singular")
        parent[ra] = rb
        names.append(name)
        henries.append(value)
        ia.append(na)
        ib.append(nb)
    return (names, np.asarray(henries, dtype=np.float64).reshape(len(names)),
            np.asarray(ia, dtype=np.int32).reshape(len(names)), np.asarray(ib, dtype=np.int32).reshape(len(names)))


def check_inductor_arguments(names, initial, initial_currents, current_probes):
    """`initial_currents` and `current_probes` of Circuit.transient.  Returns (i0 float64 [L] or None: the DC start
    supplies it, cur_index int32 [Q]); ValueError for initial_currents without `initial` or of another shape, KeyError
    for a probe that is not the name of an inductor."""
    count = len(names)
    i0 = None
    if initial_currents is not None:
        if initial is None:
            raise ValueError("initial_currents needs `initial`: the DC start supplies the inductor currents itself")
        i0 = np.ascontiguousarray(initial_currents, dtype=np.float64)
        if i0.shape != (count,):
            raise ValueError(f"initial_currents must have shape ({count},), not {i0.shape}")
    elif initial is not None:
        i0 = np.zeros(count, dtype=np.float64)
    index = {name: j for j, name in enumerate(names)}
    for name in current_probes:
        if name not in index:
            raise KeyError(f"current probe {name!r} is not the name of an inductor")
    return i0, np.asarray([index[name] for name in current_probes], dtype=np.int32).reshape(len(current_probes))


def companion_table(table, farads, ia, ib, dt, method_code, henries=None, la=None, lb=None):
    """The table with one companion `R` row per capacitor appended: value dt / C (Euler) or dt / (2 C) (trapezoidal).
    Returns (table, rows int64 [C]): the appended rows' indices; the original rows keep theirs.  With `henries` [L] (and
    the inductors' leads la, lb) one row per inductor follows the capacitors': value L / dt or 2 L / dt; then the
    result is (table, capacitor rows [C], inductor rows [L])."""
    scale = 2.0 if method_code == METHODS["trapezoidal"] else 1.0
    values = dt / (scale * np.asarray(farads, dtype=np.float64))
    ncap, first = len(values), table.ncomp
    if henries is not None:
        values = np.concatenate([values, scale * np.asarray(henries, dtype=np.float64) / dt])
        ia = np.concatenate([np.asarray(ia, dtype=np.int32).reshape(ncap), np.asarray(la, dtype=np.int32).reshape(-1)])
        ib = np.concatenate([np.asarray(ib, dtype=np.int32).reshape(ncap), np.asarray(lb, dtype=np.int32).reshape(-1)])
    types = np.full(len(values), c.TYPE_CODE["R"], dtype=np.uint8)
    out, rows = table.with_rows_appended(types, values, ia, ib), np.arange(first, first + len(values), dtype=np.int64)
    return (out, rows) if henries is None else (out, rows[:ncap], rows[ncap:])


def diode_companion_table(table, farads, ia, ib, dt, method_code, henries, la, lb, i_sat, n_vt, da, db, gmin=0.0):
    """The table of a transient run with diodes: the capacitors' companion rows, then the inductors', then one per
    diode (operating_point.companion_table: a placeholder value the device overwrites before every assembly, a diode with
    both leads on one node between ground and ground).  Returns (table, capacitor rows [C], inductor rows [L], diode
    rows [D]); the original rows keep their indices."""
    from .operating_point import companion_table as diode_rows_appended
    table, cap_rows, ind_rows = companion_table(table, farads, ia, ib, dt, method_code, henries, la, lb)
    table, diode_rows = diode_rows_appended(table, i_sat, n_vt, da, db, gmin)
    return table, cap_rows, ind_rows, diode_rows


def bjt_companion_table(table, farads, ia, ib, dt, method_code, henries, la, lb, i_sat, n_vt, da, db, ta, tb, junction, i_s,
                        gmin=0.0):
    """The table of a transient run with bipolar transistors: diode_companion_table's rows -- the capacitors', the
    inductors', then one per diode, the transistors' junctions among them (i_sat, n_vt, da, db [D + 2 T]) -- and behind
    them two `GM` rows per transport as operating_point.transistor_companion_table lays them out: the forward one reads
    junction[t, 0], the reverse one junction[t, 1]; both carry the transport's leads ta[t], tb[t] as a, b and the
    (grounded-where-same) leads of the junction's row as c, d.  Returns (table, capacitor rows [C], inductor rows [L],
    diode rows [D + 2 T], gm_rows [T, 2]); the original rows keep their indices.  The GM values are the linearisation at
    v = 0, i_s / n_vt and -i_s / n_vt, placeholders that the device overwrites before every assembly."""
    from .operating_point import _with_transport_rows
    table, cap_rows, ind_rows, diode_rows = diode_companion_table(table, farads, ia, ib, dt, method_code, henries, la, lb,
                                                                  i_sat, n_vt, da, db, gmin)
    junction = np.asarray(junction, dtype=np.int64).reshape(-1, 2)
    n_vt, i_s = np.asarray(n_vt, dtype=np.float64), np.asarray(i_s, dtype=np.float64)
    table, gm_rows = _with_transport_rows(table, da, db, ta, tb, junction, i_s / n_vt[junction[:, 0]],
                                          -i_s / n_vt[junction[:, 1]])
    return table, cap_rows, ind_rows, diode_rows, gm_rows


def check_transistor_probes(names, transistor_probes):
    """`transistor_probes` of Circuit.transient as int32 [Q] indices into the transistors `names`; ValueError for a
    probe that is not the name of a transistor (also: any probe when there are no transistors) and for a name given
    twice."""
    index = {name: j for j, name in enumerate(names)}
    seen = set()
    for name in transistor_probes:
        if name not in index:
            raise ValueError(f"transistor probe {name!r} is not the name of a transistor")
        if name in seen:
            raise ValueError(f"transistor probe {name!r} is given twice")
        seen.add(name)
    return np.asarray([index[name] for name in transistor_probes], dtype=np.int32).reshape(len(transistor_probes))


def check_diode_probes(names, diode_probes):
    """`diode_probes` of Circuit.transient as int32 [Q] indices into the diodes `names`; KeyError for a probe that is
    not the name of a diode (also: any probe when there are no diodes)."""
    index = {name: j for j, name in enumerate(names)}
    for name in diode_probes:
        if name not in index:
            raise KeyError(f"diode probe {name!r} is not the name of a diode")
    return np.asarray([index[name] for name in diode_probes], dtype=np.int32).reshape(len(diode_probes))


def dc_table(table, la, lb):
    """The table in which every inductor is a short: one zero-volt `E` row per inductor appended, each with a branch
    unknown of its own (ComponentTable.with_branch_rows_appended): K + B + L unknowns, the first K + B the circuit's.
    The branch unknown of an `E` row is the current that enters lead a from the element, so the inductor's current from
    a to b is its negative."""
    count = len(la)
    return table.with_branch_rows_appended(np.full(count, c.TYPE_CODE["E"], dtype=np.uint8), np.zeros(count), la, lb)


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
    earlier call), [2] the whole call on the device.  currents [steps + 1, Q]: the currents of the inductors named in
    current_probes, from lead a to lead b, row 0 the start's; final_currents [L]: every inductor's after the last step
    (NaN when a step was singular), what `initial_currents` of a continuing call takes.

    With diodes (nodal_transient_nl): info 2 marks a step whose Newton loop did not converge (it and every later step:
    NaN); newton_iterations [steps] and matrix_updates [steps]: a step's Newton iterations and those of them whose
    matrix work ran; diode_voltages, diode_currents [steps + 1, Q]: v and i(v) of the diodes named in diode_probes, row 0
    the start's; final_junctions [D]: the limited junction voltages after the last step.  scaled_residual is the largest
    of a step's linear solves (one per Newton iteration), iterations those of its last, timings as OperatingPoint's.  Without diodes: one iteration per solved
    step, no update, empty arrays.

    With transistors (nodal_transient_nl_bjt): transistor_probes as passed; junction_voltages [steps + 1, Q, 2]: the
    forward and reverse junction voltages of the transistors named there (an NPN's v_be, v_bc; a PNP's v_eb, v_cb), row 0
    the start's; collector_currents, base_currents, emitter_currents [steps + 1, Q]: positive INTO the terminal, formed
    as Circuit.operating_point forms them; final_junctions has D + 2 T entries, the transistors' junctions behind the
    caller's diodes; matrix_updates equals newton_iterations (no re-use with transistors).  The diode outputs keep
    covering the caller's diodes only.  Without transistors: empty arrays."""

    def __init__(self, t, waveforms, probes, info, scaled_residual, iterations, solutions=None, solution_steps=None,
                 envelope=None, timings=None, currents=None, current_probes=(), final_currents=None,
                 newton_iterations=None, matrix_updates=None, diode_voltages=None, diode_currents=None, diode_probes=(),
                 final_junctions=None, transistor_probes=(), junction_voltages=None, collector_currents=None,
                 base_currents=None, emitter_currents=None):
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
        self.currents = currents if currents is not None else np.zeros((len(t), 0), dtype=np.float64)
        self.current_probes = list(current_probes)
        self.final_currents = final_currents if final_currents is not None else np.zeros(0, dtype=np.float64)
        solved = (np.asarray(info) == 0).astype(np.int32)
        self.newton_iterations = newton_iterations if newton_iterations is not None else solved
        self.matrix_updates = matrix_updates if matrix_updates is not None else np.zeros(len(solved), dtype=np.int32)
        empty = np.zeros((len(t), 0), dtype=np.float64)
        self.diode_voltages = diode_voltages if diode_voltages is not None else empty
        self.diode_currents = diode_currents if diode_currents is not None else empty.copy()
        self.diode_probes = list(diode_probes)
        self.final_junctions = final_junctions if final_junctions is not None else np.zeros(0, dtype=np.float64)
        self.transistor_probes = list(transistor_probes)
        self.junction_voltages = (junction_voltages if junction_voltages is not None
                                  else np.zeros((len(t), 0, 2), dtype=np.float64))
        self.collector_currents = collector_currents if collector_currents is not None else empty.copy()
        self.base_currents = base_currents if base_currents is not None else empty.copy()
        self.emitter_currents = emitter_currents if emitter_currents is not None else empty.copy()

    def __len__(self):
        return len(self.info)
