"""Adjoint sensitivities: how much every component value decides a chosen output.

The derivative of an output -- a node potential, a voltage between two nodes, the current through a
component -- with respect to the value of EVERY component of the netlist: what tolerance analysis,
worst-case design and any optimisation over component values are built on.  With the reference the
only way to it is finite differences, two `Circuit(netlist)` + `.solve()` per component (reference
nodal/nodal.py:306-336); `Circuit.sensitivities` gets the whole gradient of an output from one extra
solve with the transposed matrix and one pass over the component table (`nodal_sensitivities`,
csrc/sensitivity.hip), sixteen outputs to a block.

Outputs:

    ("e", node)                     the potential of a node (the ground node is allowed: all zeros)
    ("v", node_plus, node_minus)    the voltage between two nodes (either may be ground)
    ("i", component)                the current `Circuit.branches()` reports for that component, same
                                    orientation; not for a current source (its current is its value)

`resolve_outputs` -- names to indices, argument checks -- needs no device, and `Sensitivities` is a
plain container that can be built from arrays.
"""

import numpy as np

from .sweep import _row_map, _type_of

KIND_NODES, KIND_CURRENT = 0, 1


def _node_index(netlist, label):
    """index of a node among the unknowns, -1 for the ground node; KeyError for a label the netlist does not have"""
    if label == netlist.ground:
        return -1
    if label in netlist.nodenum:
        return int(netlist.nodenum[label])
    text = str(label)
    if text == str(netlist.ground):
        return -1
    if text in netlist.nodenum:
        return int(netlist.nodenum[text])
    raise KeyError(label)


def resolve_outputs(netlist, outputs):
    """The outputs of Circuit.sensitivities as the arrays nodal_sensitivities takes.

    Returns (kind, p, q2), int32 [M] each: kind 0 = e(p) - e(q2) with node indices (-1 ground), kind 1 =
    the current of table row p (q2 = -1).  Raises KeyError for a node or component the netlist does not
    have, ValueError for a malformed specification, for ("i", name) of a current source and for
    ("i", name) of a name the netlist defines more than once (which row is meant?)."""
    kind, p, q2 = [], [], []
    row_map = None
    for spec in outputs:
        if isinstance(spec, (str, bytes)) or not hasattr(spec, "__len__") or len(spec) < 1:
            raise ValueError(f"Output {spec!r} is not one of ('e', node), ('v', node, node), ('i', component)")
        what = spec[0]
        if what == "e" and len(spec) == 2:
            kind.append(KIND_NODES)
            p.append(_node_index(netlist, spec[1]))
            q2.append(-1)
        elif what == "v" and len(spec) == 3:
            kind.append(KIND_NODES)
            p.append(_node_index(netlist, spec[1]))
            q2.append(_node_index(netlist, spec[2]))
        elif what == "i" and len(spec) == 2:
            if row_map is None:
                row_map = _row_map(netlist)
            name = spec[1]
            if name not in row_map:
                raise KeyError(name)
            rows = row_map[name]
            if len(rows) != 1:
                raise ValueError(f"Component {name} is defined {len(rows)} times: its current is not one output")
            ctype = _type_of(netlist, name, rows[0])
            if ctype == "A":
                raise ValueError(f"Component {name} is a current source: its current is its value, not an output")
            kind.append(KIND_CURRENT)
            p.append(int(rows[0]))
            q2.append(-1)
        else:
            raise ValueError(f"Output {spec!r} is not one of ('e', node), ('v', node, node), ('i', component)")
    as_i32 = lambda v: np.asarray(v, dtype=np.int32).reshape(len(v))  # noqa: E731
    return as_i32(kind), as_i32(p), as_i32(q2)


class Sensitivities:
    """Result of Circuit.sensitivities.

    values [M, ncomp]: values[m, i] = d output m / d value of table row i (rows in the order of
    `netlist.component_keys`); outputs: the specifications; output_values [M]: the outputs themselves;
    info [M]: 0 solved, > 0 singular (sparse path: a NaN row); scaled_residual [M] of the adjoint solves
    G^T lambda = c, computed on the device; adjoints [M, K+B] (the lambdas) or None."""

    def __init__(self, netlist, outputs, values, output_values, info, scaled_residual, adjoints=None, table=None):
        self._netlist = netlist
        self.outputs = list(outputs)
        self.values = values
        self.output_values = output_values
        self.info = info
        self.scaled_residual = scaled_residual
        self.adjoints = adjoints
        self._table = table
        self._names = self._rows = self._value = None

    def __len__(self):
        return len(self.outputs)

    @property
    def names(self):
        if self._names is None:
            self._names = list(self._netlist.component_keys)
        return self._names

    @property
    def component_values(self):
        """the value column the derivatives are taken with respect to, [ncomp]"""
        if self._value is None:
            if self._table is None:
                from .circuit import Circuit
                self._table = Circuit._lower(self._netlist)
            self._value = np.asarray(self._table.value, dtype=np.float64)
        return self._value

    def of(self, name):
        """d output / d value of component `name`, [M].  A name the netlist defines more than once: the sum
        over its rows, which is the derivative with respect to the value they share."""
        if self._rows is None:
            self._rows = _row_map(self._netlist)
        rows = self._rows[name]
        return np.asarray(self.values)[:, rows].sum(axis=1)

    @property
    def normalized(self):
        """values * component value: the change of the output per relative change of the component, [M, ncomp]"""
        return np.asarray(self.values) * self.component_values[None, :]

    def worst_case(self, tolerance):
        """sum_i |values[m, i] * value_i| * tolerance_i, [M]: the first-order worst-case excursion of every
        output when component i may be off by the relative tolerance_i (a scalar, or [ncomp])."""
        tol = np.asarray(tolerance, dtype=np.float64)
        if tol.ndim not in (0, 1) or (tol.ndim == 1 and len(tol) != np.asarray(self.values).shape[1]):
            raise ValueError("tolerance must be a scalar or one value per component")
        return (np.abs(self.normalized) * tol).sum(axis=1)

    def top(self, m, count=10):
        """the `count` components output m depends on most: (name, normalized sensitivity), largest
        magnitude first (the earlier table row first among equals; NaNs never)"""
        from .branches import _largest
        row = self.normalized[m]
        names = self.names
        return [(names[i], float(row[i])) for i in _largest(np.abs(row), count)]
