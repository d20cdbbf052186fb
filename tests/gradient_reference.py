"""The sums every gradient test is measured against (never product code).

Everything per member comes from tests/sensitivity_reference.py -- the oracle's G, an LU of G and of G^T, the per-row
`formulas`, their scale `formulas_abs` and the bar `parity_bars`; this module only sums them over the members of a
sweep:

    grad[i]         = sum_m formulas(table, lam_m, x_m)[i],              G^T lam_m = c_m,  G x_m = A_m
    source[m][j]    = formulas(table, lam_m, x_m)[rows[j]]
    bar(grad)       = sum_m parity_bars(table, lam_m, x_m, None) + M EPS sum_m formulas_abs(table, lam_m, x_m)
    bar(source m j) = parity_bars(table, lam_m, x_m, None)[rows[j]]

The first term of bar(grad) is the project's bar for solutions through the bilinear formula, member by member; the
second is one rounding per addition of the member sum.  The members' right-hand sides come by linearity in the source
values from one oracle build per swept source: A(v) = A(v0) + sum_j (v_j - v0_j) (A(v0 + e_j) - A(v0)).
"""
import numpy as np

import nodal_amd as n
from nodal_amd.sweep import resolve_sources
from oracle import nodal_oracle as oracle
from tests import sensitivity_reference as ref
from tests.sensitivity_reference import EPS


def source_names(rows, limit):
    """the first `limit` independent sources (A, E) of the rows whose names are defined once"""
    keys = [r[0] for r in rows if r]
    out = [r[0] for r in rows if r and r[1] in ("A", "E") and keys.count(r[0]) == 1]
    return out[:limit]


def sweep_values(names, M, seed):
    """member values that differ by factors, not by rounding"""
    rng = np.random.default_rng(seed)
    return {name: rng.uniform(-5.0, 5.0, size=M) for name in names}


class SweepReference:
    """ref.Reference of a netlist plus the members of a source sweep: x_m from an LU of the oracle's G"""

    def __init__(self, rows, sparse, transposed=True):
        self.rows = rows
        self.nl = n.Netlist.from_rows(rows)
        self.r = ref.Reference(self.nl, sparse, transposed=transposed)
        self.table = self.r.table
        self.sparse = sparse
        if sparse:
            import scipy.sparse.linalg as spla
            self._lu = spla.splu(self.r.G)
        self._unit = {}

    def solve(self, A):
        return self._lu.solve(A) if self.sparse else np.linalg.solve(self.r.G, A)

    def _unit_rhs(self, name):
        """A(v0 + e_name) - A(v0): one oracle build per swept source"""
        if name not in self._unit:
            rows = [[r[0], r[1], repr(float(r[2]) + 1.0), *r[3:]] if r and r[0] == name else r for r in self.rows]
            _, A, _ = oracle.build_model(n.Netlist.from_rows(rows), self.sparse)
            self._unit[name] = np.asarray(A, dtype=np.float64).ravel() - self.r.A
        return self._unit[name]

    def members(self, sources):
        """x [M, n] of the members of a sweep (sources: name -> [M])"""
        base = {r[0]: float(r[2]) for r in self.rows if r and r[0] in sources}
        M = len(next(iter(sources.values())))
        xs = []
        for m in range(M):
            A = self.r.A.copy()
            for name, vals in sources.items():
                A += (float(vals[m]) - base[name]) * self._unit_rhs(name)
            xs.append(self.solve(A))
        return np.array(xs).reshape(M, len(self.r.A))

    def adjoints(self, cotangents):
        return np.array([self.r.adjoint(c) for c in cotangents]).reshape(len(cotangents), len(self.r.A))


def gradient_sum(table, lams, xs, value=None):
    """(grad [ncomp], per member [M, ncomp]) of the formulas"""
    per = np.array([ref.formulas(table, lam, x, value) for lam, x in zip(lams, xs)]).reshape(len(lams), table.ncomp)
    grad = np.zeros(table.ncomp)
    for row in per:  # (member order, as the device adds them)
        grad = grad + row
    return grad, per


def gradient_bars(table, lams, xs, value=None):
    """(bar of grad [ncomp], bars per member [M, ncomp])"""
    per = np.array([ref.parity_bars(table, lam, x, None, value) for lam, x in zip(lams, xs)]).reshape(len(lams), table.ncomp)
    scale = np.zeros(table.ncomp)
    for lam, x in zip(lams, xs):
        scale = scale + ref.formulas_abs(table, lam, x, value)
    return per.sum(axis=0) + len(lams) * EPS * scale, per


def worst_ratio(got, want, bar):
    """max |got - want| / bar (inf where the bar is 0 and the values differ; NaN counts as a miss)"""
    off = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(all="ignore"):
        ratio = np.where(bar > 0, off / bar, np.where(off > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return float(ratio.max(initial=0.0))


def check_gradient(sr, grad, cotangents, xs, sources, tag, value=None):
    """the bars on grad.values and on every member's source values; returns the worst ratio"""
    table = sr.table
    lams = sr.adjoints(cotangents)
    want, per = gradient_sum(table, lams, xs, value)
    bar, per_bar = gradient_bars(table, lams, xs, value)
    assert (np.asarray(grad.info) == 0).all(), tag
    assert np.asarray(grad.values).shape == (table.ncomp,)
    worst = worst_ratio(grad.values, want, bar)
    print(tag, "members", len(lams), "worst |grad - want| / bar:", worst)
    assert worst <= 1.0, (tag, worst)
    if sources:
        tab_rows, _ = resolve_sources(sr.nl, sources)
        at = 0
        for name in sources:
            j = int(tab_rows[at])  # (names defined once: one row each)
            at += 1
            w = worst_ratio(grad.source_values[name], per[:, j], per_bar[:, j])
            assert w <= 1.0, (tag, name, w)
            worst = max(worst, w)
    return worst, lams
