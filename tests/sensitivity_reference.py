"""The numpy restatement every sensitivity test is measured against (never product code).

G, A come from the oracle's build_model, x and lambda from an LU (numpy.linalg.solve small, splu large), and the
per-row formulas are evaluated here from the columns of the lowered table:

    dy/dv_i = lambda^T (dA/dv_i - dG/dv_i x) + dy/dv_i|explicit,      G^T lambda = c,  y = c^T x

    R           (L(a) - L(b)) (X(a) - X(b)) / v^2  + for every CCVS / CCCS row j driven by it
                L(m_j) v_j (X(c_j) - X(d_j)) / v^2
    A           L(a) - L(b)
    E           L(m)
    VCVS        L(m) (X(c) - X(d))                 (VCCS rows carry this type)
    CCVS, CCCS  -L(m) (X(c) - X(d)) / Rd

X / L read +0.0 for the ground lead, m = K + k, Rd = value[drv] (1 without a driver).  The output ("i", resistor) has
c = (e_a - e_b) / v and the explicit term -y / v at its own row: it belongs to that row's formula for that output,
in `formulas` and in `formulas_abs` alike (there as (|X(a)| + |X(b)|) / v^2).

`formulas_abs` is the scale the bars are built from: the same formulas with every entry of lambda and x replaced by
its absolute value and every difference by a sum -- zero only where a row cannot contribute at all.
"""
import numpy as np

from nodal_amd.lowering import lower
from oracle import nodal_oracle as oracle

EPS = 2.0 ** -52
TOL = 1e-9  # the project's bar for solutions, normwise (tests/test_gpu_sweep.py)
T_R, T_A, T_E, T_VCVS, T_CCVS, T_CCCS = range(6)


def table_of(nl):
    return lower(nl)


def _columns(table):
    cols = {name: np.asarray(getattr(table, name)) for name in ("type", "a", "b", "c", "d", "drv", "k")}
    cols["m"] = np.where(cols["k"] >= 0, table.K + cols["k"], -1)
    return cols


def _evaluate(table, lam, x, value, explicit_row, absolute):
    t = _columns(table)
    v = np.asarray(table.value if value is None else value, dtype=np.float64)
    L, X = np.append(np.asarray(lam, dtype=np.float64), 0.0), np.append(np.asarray(x, dtype=np.float64), 0.0)
    if absolute:
        L, X, v = np.abs(L), np.abs(X), np.abs(v)
    sign = 1.0 if absolute else -1.0
    dL = L[t["a"]] + sign * L[t["b"]]
    dX = X[t["a"]] + sign * X[t["b"]]
    dXc = X[t["c"]] + sign * X[t["d"]]
    Lm = L[t["m"]]
    Rd = np.where(t["drv"] >= 0, v[np.where(t["drv"] >= 0, t["drv"], 0)], 1.0)
    ty = t["type"]
    with np.errstate(all="ignore"):
        s = np.zeros(table.ncomp)
        s = np.where(ty == T_R, dL * dX / (v * v), s)
        s = np.where(ty == T_A, dL, s)
        s = np.where(ty == T_E, Lm, s)
        s = np.where(ty == T_VCVS, Lm * dXc, s)
        s = np.where((ty == T_CCVS) | (ty == T_CCCS), sign * Lm * dXc / Rd, s)
        # the resistors that drive CCVS / CCCS rows, in table order
        for j in np.flatnonzero(((ty == T_CCVS) | (ty == T_CCCS)) & (t["drv"] >= 0)):
            i = t["drv"][j]
            if ty[i] == T_R:
                s[i] += Lm[j] * v[j] * dXc[j] / (v[i] * v[i])
        if explicit_row is not None and ty[explicit_row] == T_R:
            s[explicit_row] += sign * dX[explicit_row] / (v[explicit_row] * v[explicit_row])
    return s


def formulas(table, lam, x, value=None, explicit_row=None):
    """dy / d value of every table row, [ncomp]"""
    return _evaluate(table, lam, x, value, explicit_row, False)


def formulas_abs(table, lam, x, value=None, explicit_row=None):
    """the same without cancellation, [ncomp] (lam / x may be all-ones vectors scaled by a norm)"""
    return _evaluate(table, lam, x, value, explicit_row, True)


def output_vector(nl, table, spec, value=None):
    """c [n] of an output specification and the row whose formula carries its explicit term (or None); the test's
    own reading of the specification, from nodenum and component_keys"""
    n = table.K + table.B
    v = np.asarray(table.value if value is None else value, dtype=np.float64)
    c = np.zeros(n)

    def node(label):
        return -1 if label == nl.ground else nl.nodenum[label]

    if spec[0] in ("e", "v"):
        p = node(spec[1])
        q = node(spec[2]) if spec[0] == "v" else -1
        if p >= 0:
            c[p] += 1.0
        if q >= 0:
            c[q] -= 1.0
        return c, None
    rows = [i for i, key in enumerate(nl.component_keys) if key == spec[1]]
    assert spec[0] == "i" and len(rows) == 1
    i = rows[0]
    ty = int(np.asarray(table.type)[i])
    assert ty != T_A
    if ty == T_R:
        a, b = int(np.asarray(table.a)[i]), int(np.asarray(table.b)[i])
        if a >= 0:
            c[a] += 1.0 / v[i]
        if b >= 0:
            c[b] -= 1.0 / v[i]
        return c, i
    c[table.K + int(np.asarray(table.k)[i])] += 1.0
    return c, None


def node_labels(nl):
    labels = [None] * nl.nums["kcl"]
    for label, index in nl.nodenum.items():
        labels[index] = label
    return labels


def all_outputs(nl, table):
    """every unknown (node potentials as "e", branch unknowns as "i" of their row), the current of every other row that
    is admissible (not a current source, a name defined once), two "v" forms (one against ground) and the ground node"""
    keys = list(nl.component_keys)
    once = {key for key in keys if keys.count(key) == 1}
    labels = node_labels(nl)
    out = [("e", label) for label in labels]
    ty = np.asarray(table.type)
    out += [("i", key) for i, key in enumerate(keys) if key in once and ty[i] != T_A]
    out.append(("e", nl.ground))
    if labels:
        out.append(("v", labels[0], nl.ground))
        out.append(("v", labels[-1], labels[0]))
    return out


def sample_outputs(nl, table, count, seed):
    """a seeded sample of `count` outputs of all three kinds (at least one of each where the network has them)"""
    rng = np.random.default_rng(seed)
    keys = list(nl.component_keys)
    labels = node_labels(nl)
    ty = np.asarray(table.type)
    rows = [i for i in range(len(keys)) if ty[i] != T_A]
    out = []
    for q in range(count):
        which = q % 3
        if which == 0:
            out.append(("e", labels[int(rng.integers(len(labels)))]))
        elif which == 1:
            a, b = (int(u) for u in rng.integers(len(labels), size=2))
            out.append(("v", labels[a], labels[b] if q % 2 else nl.ground))
        else:
            out.append(("i", keys[rows[int(rng.integers(len(rows)))]]))
    return out


class Reference:
    """G (dense ndarray or csc), x and the LU of G^T for one netlist"""

    def __init__(self, nl, sparse, transposed=True):
        self.nl = nl
        self.table = table_of(nl)
        G, A, _ = oracle.build_model(nl, sparse)
        self.A = np.asarray(A, dtype=np.float64).ravel()
        self.sparse = sparse
        if sparse:
            import scipy.sparse.linalg as spla
            self.G = G.tocsc()
            self.x = spla.splu(self.G).solve(self.A)
            # (transposed=False: the test that the transpose is really taken evaluates the formulas with G in its place)
            self._lu = spla.splu(self.G.T.tocsc() if transposed else self.G)
            self.norm1 = float(abs(self.G).sum(axis=0).max())
        else:
            self.G = np.asarray(G, dtype=np.float64)
            self.x = np.linalg.solve(self.G, self.A)
            self._Gt = self.G.T if transposed else self.G
            self.norm1 = float(np.abs(self.G).sum(axis=0).max()) if self.G.size else 0.0

    def adjoint(self, c):
        return self._lu.solve(c) if self.sparse else np.linalg.solve(self._Gt, c)

    def adjoint_residual(self, lam, c):
        """||G^T lam - c||_inf / (||G||_1 ||lam||_inf + ||c||_inf)"""
        r = (self.G.T @ lam) - c
        den = self.norm1 * np.abs(lam).max(initial=0.0) + np.abs(c).max(initial=0.0)
        return float(np.abs(r).max(initial=0.0) / den) if den > 0 else 0.0

    def output(self, spec):
        """(y, c, explicit row, lambda, sensitivities [ncomp]) of one output"""
        c, row = output_vector(self.nl, self.table, spec)
        lam = self.adjoint(c)
        return float(c @ self.x), c, row, lam, formulas(self.table, lam, self.x, explicit_row=row)


def parity_bars(table, lam, x, row, value=None):
    """Per table row: the project's bar for solutions (TOL, normwise) propagated through the bilinear formula -- an
    error of TOL |lam|_inf in every entry of lam and of TOL |x|_inf in every entry of x, to first order -- plus
    8 eps of the formula's own scale."""
    ones_l = np.full(len(lam), np.abs(lam).max(initial=0.0))
    ones_x = np.full(len(x), np.abs(x).max(initial=0.0))
    return (TOL * (formulas_abs(table, ones_l, x, value, row) + formulas_abs(table, lam, ones_x, value, row))
            + 8 * EPS * formulas_abs(table, lam, x, value, row))
