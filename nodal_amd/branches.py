"""Branch currents, power and the worst-case envelope of a source sweep.

The reference answers with node potentials and the currents of the components that own a branch
unknown (`Solution`, reference nodal/nodal.py:401-434); what flows through a resistor or what a
component dissipates is a loop over `Solution.result` that its users write themselves.
`Circuit.branches()` computes it on the device (`nodal_branches`, csrc/branch.hip), and
`Circuit.solve_sources(..., branches=True)` keeps, per component and per node, the worst case over
the members of a sweep (`nodal_solve_sources_branches`).

Conventions, per table row (one row per entry of `netlist.component_keys`, in that order):

    voltage = e(a) - e(b)                       first lead minus second lead, ground = 0
    current   R: voltage / value, flowing from lead a to lead b through the resistor
              A: its value; E, VCVS, VCCS, CCVS, CCCS: the `i(name)` of `Solution`.
              For every type but R the current flows from b to a inside the component, into node a
              (the reference's stamps: A[a] += J; G[a, K + k] = -1).
    power     what the component absorbs: voltage * current for R, -(voltage * current) otherwise

`Branches` and `Envelope` are plain containers: they can be built from arrays with no device.
"""

import numpy as np

from . import constants as c


def _table_of(netlist):
    from .circuit import Circuit
    return Circuit._lower(netlist)


def _node_labels(netlist):
    labels = [None] * netlist.nums["kcl"]
    for label, index in netlist.nodenum.items():
        labels[index] = label
    return labels


def _largest(values, count):
    """indices of the `count` largest entries, largest first, the lower index first among equals; NaNs never"""
    values = np.asarray(values, dtype=np.float64)
    valid = np.flatnonzero(~np.isnan(values))
    count = min(int(count), len(valid))
    if count <= 0:
        return np.zeros(0, dtype=np.int64)
    picked = valid
    if count < len(valid):
        # everything at least as large as the count-th largest, then cut: ties resolve by index
        kth = len(valid) - count
        bar = values[valid][np.argpartition(values[valid], kth)[kth]]
        picked = valid[values[valid] >= bar]
    order = np.lexsort((picked, -values[picked]))
    return picked[order][:count]


class Branches:
    """Per-component voltage, current and absorbed power of one solution, in table row order, and
    the two power totals.  `br[name]` -> (voltage, current, power)."""

    def __init__(self, netlist, voltage, current, power, dissipated, absorbed_by_sources, table=None):
        self._netlist = netlist
        self.voltage = voltage
        self.current = current
        self.power = power
        self.dissipated = dissipated
        self.absorbed_by_sources = absorbed_by_sources
        self._table = table
        self._names = self._rows = None

    @property
    def names(self):
        if self._names is None:
            self._names = list(self._netlist.component_keys)
        return self._names

    def _row_map(self):
        if self._rows is None:
            from .sweep import _row_map
            self._rows = _row_map(self._netlist)
        return self._rows

    def rows(self, name):
        """every table row that carries `name` (a name defined more than once has several)"""
        return list(self._row_map()[name])

    def __len__(self):
        return len(self.voltage)

    def __getitem__(self, name):
        row = self._row_map()[name][-1]
        return float(self.voltage[row]), float(self.current[row]), float(self.power[row])

    def kcl_residual(self):
        """Net current into every non-ground node, [K]: sum over the rows with a == node of s * current minus
        the sum over the rows with b == node, s = +1 for R and -1 otherwise.  Zero, up to rounding and the
        solver's residual, for a solution.  Computed on the host from `current`: a check, not a hot path."""
        table = self._table if self._table is not None else _table_of(self._netlist)
        self._table = table
        K = self._netlist.nums["kcl"]
        signed = np.where(np.asarray(table.type) == c.T_R, 1.0, -1.0) * np.asarray(self.current, dtype=np.float64)
        a, b = np.asarray(table.a), np.asarray(table.b)
        net = np.zeros(K + 1)  # (slot K: the ground lead)
        np.add.at(net, np.where(a < 0, K, a), signed)
        np.subtract.at(net, np.where(b < 0, K, b), signed)
        return net[:K]

    def __str__(self):
        # values as Solution prints them (the shortest round-trip repr), names in sorted order
        last = {name: rows[-1] for name, rows in self._row_map().items()}
        v = np.asarray(self.voltage, dtype=np.float64).tolist()
        i = np.asarray(self.current, dtype=np.float64).tolist()
        p = np.asarray(self.power, dtype=np.float64).tolist()
        lines = []
        for name in sorted(last):
            row = last[name]
            lines += [f"v({name}) \t= {v[row]!r}", f"i({name}) \t= {i[row]!r}", f"p({name}) \t= {p[row]!r}"]
        return "\n".join(lines)


class Envelope:
    """Worst case over the members of a source sweep that were solved (info == 0):

    current_absmax [ncomp], current_member [ncomp]: the largest |current| through every component and a
    member that attains it; potential_min / potential_max [K] with potential_min_member /
    potential_max_member; dissipated [M], absorbed_by_sources [M] per member (NaN for a member that is
    left out).  Among exact ties the lowest member index is reported; with no member solved the
    values are NaN and the members -1."""

    def __init__(self, netlist, current_absmax, current_member, potential_min, potential_min_member,
                 potential_max, potential_max_member, dissipated, absorbed_by_sources):
        self._netlist = netlist
        self.current_absmax = current_absmax
        self.current_member = current_member
        self.potential_min = potential_min
        self.potential_min_member = potential_min_member
        self.potential_max = potential_max
        self.potential_max_member = potential_max_member
        self.dissipated = dissipated
        self.absorbed_by_sources = absorbed_by_sources
        self._names = None

    @classmethod
    def empty(cls, netlist, ncomp, members=0):
        """the envelope of a sweep without a solved member"""
        K = netlist.nums["kcl"]
        nan, none = (lambda k: np.full(k, np.nan)), (lambda k: np.full(k, -1, dtype=np.int32))
        return cls(netlist, nan(ncomp), none(ncomp), nan(K), none(K), nan(K), none(K), nan(members), nan(members))

    @property
    def names(self):
        if self._names is None:
            self._names = list(self._netlist.component_keys)
        return self._names

    def worst_current(self, count=10):
        """the `count` components carrying the largest |current| in any member: (name, value, member),
        largest first (the earlier table row first among equals)"""
        names = self.names
        return [(names[i], float(self.current_absmax[i]), int(self.current_member[i]))
                for i in _largest(self.current_absmax, count)]

    def worst_drop(self, count=10):
        """the `count` nodes with the largest |potential| in any member: (node label, signed potential,
        member), largest magnitude first (the lower node index first among equals; at a node whose extremes
        have the same magnitude the minimum is reported)"""
        lo, hi = np.asarray(self.potential_min, dtype=np.float64), np.asarray(self.potential_max, dtype=np.float64)
        use_hi = np.abs(hi) > np.abs(lo)
        value = np.where(use_hi, hi, lo)
        member = np.where(use_hi, self.potential_max_member, self.potential_min_member)
        labels = _node_labels(self._netlist)
        return [(labels[j], float(value[j]), int(member[j])) for j in _largest(np.abs(value), count)]
