"""Source sweeps: one network solved for many settings of its independent sources.

A SPICE-style `.dc` sweep of a supply, or the load vectors of a power-grid IR-drop study, keeps G
fixed and changes only A.  The reference can only rebuild and re-solve the circuit per setting
(reference nodal/nodal.py:306-336: `Circuit(netlist)` + `.solve()`); `Circuit.solve_sources`
hands every setting to `nodal_solve_sources` at once, which solves them against one factorisation
or one multigrid hierarchy (include/nodal_hip.h).

`resolve_sources` -- names to table rows, argument checks -- needs no device.
"""

import numpy as np

SWEEPABLE = ("A", "E")  # the only types whose value enters A and not G


def _row_map(netlist):
    """name -> table rows carrying it (the table has one row per entry of component_keys)."""
    if getattr(netlist, "_fast", False):
        # natively parsed netlists have no duplicated names (fastparse.Irregular): one row each
        return {name: [row] for name, row in netlist._row_of.items()}
    rows = {}
    for row, key in enumerate(netlist.component_keys):
        rows.setdefault(key, []).append(row)
    return rows


def _type_of(netlist, name, row):
    if getattr(netlist, "_fast", False):
        return str(netlist._type[row])
    return netlist.components[name].type  # a duplicated name: the last definition, on every row (lowering.py)


def resolve_sources(netlist, sources):
    """Table rows and member values of a source sweep.

    `sources` maps component names to sequences of M values (the same M for every name).  Returns
    (rows int64 [R], values float64 [M, R]): a name that the netlist defines more than once
    contributes every row that carries it, all with the same values.  Raises KeyError for a name
    the netlist does not have, ValueError for a component that is not an independent source or for
    sequences of different lengths."""
    if not hasattr(sources, "items"):
        raise TypeError("sources must map component names to sequences of values")
    names = list(sources)
    if not names:
        return np.zeros(0, dtype=np.int64), np.zeros((0, 0), dtype=np.float64)
    row_map = _row_map(netlist)
    rows, columns, length = [], [], None
    for name in names:
        if name not in row_map:
            raise KeyError(name)
        found = row_map[name]
        ctype = _type_of(netlist, name, found[0])
        if ctype not in SWEEPABLE:
            raise ValueError(
                f"Component {name} is of type {ctype}: only independent sources (A, E) can be swept; "
                "a sweep of resistor or gain values is a value sweep (nodal_amd.batch)")
        vals = np.asarray(sources[name], dtype=np.float64)
        if vals.ndim != 1:
            raise ValueError(f"Values of {name} must be a flat sequence")
        if length is None:
            length = len(vals)
        elif len(vals) != length:
            raise ValueError(f"Sweep lengths differ: {names[0]} has {length} values, {name} has {len(vals)}")
        for row in found:
            rows.append(row)
            columns.append(vals)
    values = np.ascontiguousarray(np.stack(columns, axis=1)) if length else np.zeros((0, len(rows)))
    return np.asarray(rows, dtype=np.int64), values


def check_sweep_options(branches, keep_solutions):
    """The argument rule of Circuit.solve_sources: without the members' solutions the envelope is the only answer."""
    if not keep_solutions and not branches:
        raise ValueError("keep_solutions=False needs branches=True: the sweep would return nothing")


class SourceSweep:
    """Result of Circuit.solve_sources: `result[m]` is what `Circuit(netlist with member m's source
    values).solve().result` gives; `sw[m]` is that Solution; `info[m]` 0 solved, > 0 singular
    (sparse path: a NaN row); `scaled_residual[m]` = ||G x_m - A_m||_inf / (||G||_inf ||x_m||_inf +
    ||A_m||_inf), computed on the device.  `envelope` (solve_sources(branches=True)): the worst case over
    the members, a branches.Envelope, else None.  A sweep made with keep_solutions=False has `result` None."""

    def __init__(self, result, info, scaled_residual, netlist, currents, envelope=None):
        self.result = result
        self.info = info
        self.scaled_residual = scaled_residual
        self.envelope = envelope
        self._netlist = netlist
        self._currents = currents

    def __len__(self):
        return len(self.info)

    def __getitem__(self, m):
        from .circuit import Solution
        if self.result is None:
            raise ValueError("the sweep was made with keep_solutions=False: no member solutions were kept")
        return Solution(self.result[m], self._netlist, self._currents)

    def __iter__(self):
        return (self[m] for m in range(len(self)))
