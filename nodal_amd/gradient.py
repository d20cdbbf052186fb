"""Loss gradients: the derivative of a scalar loss of the solution with respect to every component value.

An optimiser, a calibration or a fit wants the gradient of a scalar loss L(x) of the whole solution, often summed
over the load cases of a source sweep, L = sum_m L_m(x_m).  `Circuit.sensitivities` would need one ("e", node)
output -- one adjoint solve, one [ncomp] row -- per unknown the loss touches; the chain rule needs one adjoint solve
per member, with the right-hand side c_m = dL/dx_m, and one number per component.  `Circuit.gradient` hands the
cotangents c_m to `nodal_gradient` (csrc/gradient.hip), which solves the members sixteen to a block and sums the
per-row formulas over them on the device.  With the reference the only way to the same numbers is finite
differences, two `Circuit(netlist)` + `.solve()` per component (reference nodal/nodal.py:306-336).

`check_gradient_arguments` -- shapes, the single-solve and the sweep form -- needs no device, and `Gradient` is a
plain container that can be built from arrays.
"""

import numpy as np

from .sweep import _row_map, resolve_sources


def check_gradient_arguments(netlist, n, cotangents, sources=None, solutions=None):
    """The arguments of Circuit.gradient as the arrays nodal_gradient takes.

    Single solve: cotangents [n], no sources; solutions None (the solution on the device) or [n].  Sweep: sources as
    passed to solve_sources (M values per name), solutions [M, n] (SourceSweep.result), cotangents [M, n].  Returns (cotangents [M, n], rows int64 [R],
    solutions [M, n] or None, columns: name -> the columns of `rows` that carry it).  Raises ValueError for shapes
    that do not fit, and what sweep.resolve_sources raises for the sources."""
    cot = np.asarray(cotangents, dtype=np.float64)
    if sources is None and solutions is None:
        if cot.shape != (n,):
            raise ValueError(f"cotangents must have shape ({n},) for the single solve, not {cot.shape}")
        return np.ascontiguousarray(cot.reshape(1, n)), np.zeros(0, dtype=np.int64), None, {}
    if sources is None:  # one solution the caller kept, in place of the one on the device
        x = np.asarray(solutions, dtype=np.float64)
        if cot.shape != (n,) or x.shape != (n,):
            raise ValueError(f"without sources, cotangents and solutions must have shape ({n},), "
                             f"not {cot.shape} and {x.shape}")
        one = lambda v: np.ascontiguousarray(v.reshape(1, n))  # noqa: E731
        return one(cot), np.zeros(0, dtype=np.int64), one(x), {}
    if solutions is None:
        raise ValueError("a sweep's gradient needs `solutions` (SourceSweep.result) beside `sources`")
    rows, values = resolve_sources(netlist, sources)
    M = values.shape[0]
    x = np.asarray(solutions, dtype=np.float64)
    if x.shape != (M, n):
        raise ValueError(f"solutions must have shape ({M}, {n}), not {x.shape}")
    if cot.shape != (M, n):
        raise ValueError(f"cotangents must have shape ({M}, {n}), not {cot.shape}")
    row_map = _row_map(netlist)
    columns, at = {}, 0
    for name in sources:  # (the order resolve_sources lays the rows out in)
        columns[name] = list(range(at, at + len(row_map[name])))
        at += len(row_map[name])
    return np.ascontiguousarray(cot), rows, np.ascontiguousarray(x), columns


class Gradient:
    """Result of Circuit.gradient.

    values [ncomp]: dL / d value of table row i (rows in the order of `netlist.component_keys`), the implicit part:
    what the loss owes to the solution's dependence on the values; at a swept source the sum over the members, the
    derivative with respect to a value they would all share.  source_values: name -> [M], member m's derivative with
    respect to its own value of that swept source.  info [M]: 0 solved, > 0 singular (sparse path: NaN);
    scaled_residual [M] of the adjoint solves G^T lambda_m = dL/dx_m, computed on the device; adjoints [M, K+B] (the
    lambdas) or None."""

    def __init__(self, netlist, values, source_values, info, scaled_residual, adjoints=None, table=None):
        self._netlist = netlist
        self.values = values
        self.source_values = dict(source_values)
        self.info = info
        self.scaled_residual = scaled_residual
        self.adjoints = adjoints
        self._table = table
        self._names = self._rows = self._value = None

    def __len__(self):
        return len(self.info)

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
        """dL / d value of component `name`.  A name the netlist defines more than once: the sum over its rows, which
        is the derivative with respect to the value they share."""
        if self._rows is None:
            self._rows = _row_map(self._netlist)
        return float(np.asarray(self.values)[self._rows[name]].sum())

    @property
    def normalized(self):
        """values * component value: the change of the loss per relative change of the component, [ncomp]"""
        return np.asarray(self.values) * self.component_values
