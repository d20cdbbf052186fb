"""The numpy / scipy restatement every transient-gradient test is measured against (never product code).

Forward stepping, matrices and right-hand sides are those of tests/transient_reference.py (backward Euler, companion
form: M = the oracle's matrix of the netlist with one R row r_i = h / C_i per capacitor); the per-row formulas, their
scale and the bars are those of tests/sensitivity_reference.py.  This module adds the backward stepping

    lambda_{steps+1} = 0,    M^T lambda_k = c_k + S (g o S^T lambda_{k+1}),   k = steps .. 1

with an LU of M^T and one refinement step (transient_reference._solver), c_k = sum_p w[k][p] (e(a_p) - e(b_p)), and

    grad[i]              = sum_k formulas(table with companion rows, lambda_k, x_k)[i]        rows of the netlist
    grad[cap row i]      = the same R formula  -  sum_k (S^T lambda_k)_i (S^T x_{k-1})_i / r_i^2
    grad_sources[k-1][j] = formulas(., lambda_k, .)[rows[j]]
    grad_x0              = c_0 + S (g o S^T lambda_1)
    dL/dC_i              = -(h / C_i^2) grad[cap row i]
    DC start             values += formulas(table, mu, x_0),  G^T mu = grad_x0      (sensitivity_reference.Reference)

summed in the device's stated order: descending k, sixteen steps to a block, per block the sixteen table terms and then
the sixteen history terms of the capacitors.

Two INDEPENDENT formulations of the same derivatives: the adjoint above, and central differences of the reference's own
forward stepping (`run`, and `dc` for the DC start) in every component value, capacitance,
swept source value and entry of the initial state (central_differences states the steps).  Measured on the CPU, as the
largest difference over the largest entry of each array: 7.2e-9 over small_cases() below (23 networks of at most 64
unknowns with every component type, the edge network, grid(12) with two loads, cfg5(12); DC start and `initial=`
alike) -- the floor of the differences in the capacitances, the values agree to 7e-10 -- and the adjoint meets the
closed form of one RC section under Euler to 1.1e-14.  tests/test_transient_gradient_frontend.py asserts both with one
decade of margin; the device's end-to-end bar is ten times the measured value as well.
"""
import functools
import types

import numpy as np

import nodal_amd as n
from tests import sensitivity_reference as sref
from tests.sensitivity_reference import EPS, TOL, formulas, formulas_abs, parity_bars  # noqa: F401
from tests.gradient_reference import gradient_bars, worst_ratio  # noqa: F401
from tests.transient_reference import TransientReference, _solver

BLOCK = 16
FD_STEP = 1e-4
MEASURED = 7.2e-9                   # |adjoint - central differences| on the CPU (the module's docstring)
CPU_DISAGREEMENT = 10 * MEASURED    # asserted on the CPU: one decade of margin
DEVICE_END_TO_END = 10 * MEASURED   # the device's result against the same central differences
RC_DISAGREEMENT = 1.1e-13           # measured 1.1e-14, one decade of margin


def blocks(steps):
    """(k_hi, k_lo) of the device's blocks, in its order"""
    out, k_hi = [], steps
    while k_hi >= 1:
        k_lo = max(1, k_hi - BLOCK + 1)
        out.append((k_hi, k_lo))
        k_hi = k_lo - 1
    return out


class TransientGradientReference:
    """rows: the netlist; capacitors: (name, farads, node_a, node_b); dt.  Backward Euler."""

    def __init__(self, rows, capacitors, dt):
        self.r = r = TransientReference(rows, capacitors, dt, "euler")
        r._companion()
        self.n, self.K = r.n, r.K
        self._back = _solver(r.G_aug.T)
        t = r.table
        nc = len(r.g)
        cat = lambda col, tail: np.concatenate([np.asarray(col), tail])  # noqa: E731
        minus = np.full(nc, -1, dtype=np.int64)
        # the lowered table with the companion rows behind its own (R rows: a, b and the value are all they carry)
        self.table = types.SimpleNamespace(
            ncomp=t.ncomp + nc, K=t.K, B=t.B, type=cat(t.type, np.zeros(nc, dtype=np.int64)), value=cat(t.value, 1.0 / r.g),
            a=cat(t.a, r.ia), b=cat(t.b, r.ib), c=cat(t.c, minus), d=cat(t.d, minus), drv=cat(t.drv, minus), k=cat(t.k, minus))
        self.cap_rows = np.arange(t.ncomp, t.ncomp + nc)
        self.ncomp = t.ncomp

    # -- pieces -------------------------------------------------------------------------------------------------------
    def seed(self, pairs, w):
        """c_k from row k of the cotangents; pairs: the probes' node indices (a, b), -1 ground"""
        c = np.zeros(self.n + 1)
        for (a, b), v in zip(pairs, w):
            if a != b:
                c[a] += v
                c[b] -= v
        return c[:self.n]

    def history(self, lam):
        return self.r.inject(self.r.g * self.r.voltages(lam))

    def adjoints(self, pairs, cot):
        """lambda_1 .. lambda_steps [steps, n] of the reference's own backward stepping"""
        steps = len(cot) - 1
        lam, nxt = np.zeros((steps, self.n)), None
        for k in range(steps, 0, -1):
            b = self.seed(pairs, cot[k]) + (self.history(nxt) if nxt is not None else 0.0)
            lam[k - 1] = nxt = self._back(b)
        return lam

    def one_step_back(self, lam_dev, pairs, cot):
        """the reference's lambda_k from the DEVICE's lambda_{k+1}, k = 1 .. steps: [steps, n]"""
        steps = len(cot) - 1
        out = np.zeros((steps, self.n))
        for k in range(steps, 0, -1):
            b = self.seed(pairs, cot[k]) + (self.history(lam_dev[k]) if k < steps else 0.0)
            out[k - 1] = self._back(b)
        return out

    def cap_history_term(self, lam, x_prev):
        return self.r.voltages(lam) * self.r.voltages(x_prev) * self.r.g ** 2

    def cap_history_abs(self, lam, x_prev):
        L, X = np.append(np.abs(lam), 0.0), np.append(np.abs(x_prev), 0.0)
        return (L[self.r.ia] + L[self.r.ib]) * (X[self.r.ia] + X[self.r.ib]) * self.r.g ** 2

    # -- the sums, in the device's order ------------------------------------------------------------------------------
    def sums(self, lam, X):
        """grad [ncomp + C] of the table with companion rows from lambda_1 .. lambda_steps and x_0 .. x_steps"""
        grad = np.zeros(self.table.ncomp)
        for k_hi, k_lo in blocks(len(lam)):
            for k in range(k_hi, k_lo - 1, -1):
                grad = grad + formulas(self.table, lam[k - 1], X[k])
            for k in range(k_hi, k_lo - 1, -1):
                grad[self.cap_rows] = grad[self.cap_rows] - self.cap_history_term(lam[k - 1], X[k - 1])
        return grad

    def sums_abs(self, lam, X):
        """sum_k formulas_abs, with (|S^T lambda_k|)(|S^T x_k| + |S^T x_{k-1}|) / r^2 at the companion rows"""
        scale = np.zeros(self.table.ncomp)
        for k in range(1, len(lam) + 1):
            scale = scale + formulas_abs(self.table, lam[k - 1], X[k])
            scale[self.cap_rows] += self.cap_history_abs(lam[k - 1], X[k - 1])
        return scale

    def solution_bars(self, lam, X):
        """sum_k parity_bars: the project's bar for solutions through the bilinear formulas, the history term included"""
        bar = np.zeros(self.table.ncomp)
        for k in range(1, len(lam) + 1):
            bar = bar + parity_bars(self.table, lam[k - 1], X[k], None)
            ones_l = np.full(self.n, np.abs(lam[k - 1]).max(initial=0.0))
            ones_x = np.full(self.n, np.abs(X[k - 1]).max(initial=0.0))
            bar[self.cap_rows] += (TOL * (self.cap_history_abs(ones_l, X[k - 1]) + self.cap_history_abs(lam[k - 1], ones_x))
                                   + 8 * EPS * self.cap_history_abs(lam[k - 1], X[k - 1]))
        return bar

    def sources(self, lam, rows):
        """grad_sources [steps, len(rows)]: the A / E formula reads lambda alone"""
        zero = np.zeros(self.n)
        return np.array([formulas(self.table, l, zero)[rows] for l in lam]).reshape(len(lam), len(rows))

    def sources_abs(self, lam, rows):
        zero = np.zeros(self.n)
        return np.array([formulas_abs(self.table, l, zero)[rows] for l in lam]).reshape(len(lam), len(rows))

    def grad_x0(self, pairs, cot, lam):
        return self.seed(pairs, cot[0]) + (self.history(lam[0]) if len(lam) else 0.0)

    def grad_x0_abs(self, pairs, cot, lam):
        """the scale of grad_x0: every +-w and every +-g (S^T lambda_1) taken with its absolute value"""
        c = np.zeros(self.n + 1)
        for (a, b), v in zip(pairs, cot[0]):
            if a != b:
                c[a] += abs(v)
                c[b] += abs(v)
        if len(lam):
            L = np.append(np.abs(lam[0]), 0.0)
            J = self.r.g * (L[self.r.ia] + L[self.r.ib])
            np.add.at(c, self.r.ia, J)
            np.add.at(c, self.r.ib, J)
        return c[:self.n]

    # -- the public result --------------------------------------------------------------------------------------------
    def dc_chain(self, gx0, x0=None):
        """formulas(table, mu, x_0) with G^T mu = grad_x0: the derivative through the DC start, [ncomp]"""
        ref = sref.Reference(self.r.nl, True)
        return formulas(ref.table, ref.adjoint(gx0), ref.x if x0 is None else x0)

    def public(self, pairs, cot, X, rows, dc_start):
        """(values [ncomp], capacitors [C], source values [steps, len(rows)], initial [n]) by the reference's own adjoint"""
        lam = self.adjoints(pairs, cot)
        grad = self.sums(lam, X)
        gx0 = self.grad_x0(pairs, cot, lam)
        values = grad[:self.ncomp] + (self.dc_chain(gx0, X[0]) if dc_start else 0.0)
        return values, -(self.r.dt / self.r.farads ** 2) * grad[self.cap_rows], self.sources(lam, rows), gx0


def probe_pairs(nl, probes):
    """node indices (a, b) of probes given as (plus, minus) labels or single labels against ground"""
    def index(label):
        return -1 if (label == nl.ground or str(label) == str(nl.ground)) else int(nl.nodenum[label])
    return [(index(p[0]), index(p[1])) if isinstance(p, (tuple, list)) else (index(p), -1) for p in probes]


def waveforms(X, pairs):
    xe = np.hstack([X, np.zeros((len(X), 1))])
    return np.array([[0.0 if a == b else xe[k, a] - xe[k, b] for a, b in pairs] for k in range(len(X))]).reshape(len(X), len(pairs))


def forward(rows, capacitors, dt, steps, sources, pairs, initial):
    """the waveforms [steps + 1, P] of the reference's own forward stepping; initial None: from its DC solution"""
    r = TransientReference(rows, capacitors, dt, "euler")
    x0 = r.dc() if initial is None else np.asarray(initial, dtype=np.float64)
    X = r.run(x0, r.rhs_steps(sources, steps))
    return waveforms(X, pairs), X


def central_differences(loss, rows, capacitors, dt, steps, sources, pairs, initial, step=FD_STEP, subset=None, initial_subset=None):
    """dL/d(values [ncomp], farads [C], source values {name: [steps]}, initial [n] or None) of loss(waveforms), each by
    central differences with the steps `step` and `step` / 2 relative to the entry (absolute where the entry is 0),
    combined by Richardson's rule -- for source values and the initial state, in which a loss that is linear in the
    waveforms is linear, by one central difference with the step 1e-2; subset: the rows
    of the netlist the values are differentiated for, initial_subset: the entries of the initial state (None: all)"""
    rows = [list(r) for r in rows]
    comp = list(range(len(rows))) if subset is None else list(subset)  # (text rows are table rows in the tests' inputs)

    def L(rows_=rows, caps_=capacitors, sources_=sources, initial_=initial):
        return float(loss(forward(rows_, caps_, dt, steps, sources_, pairs, initial_)[0]))

    def diff(at, make):
        d = []
        for rel in (step, step / 2):
            h = rel * (abs(at) if at != 0 else 1.0)
            d.append((L(**make(at + h)) - L(**make(at - h))) / (2 * h))
        return (4.0 * d[1] - d[0]) / 3.0  # (Richardson's rule, as tests/test_sensitivity_frontend.py)

    def diff_linear(at, make):  # (the waveforms are linear in the sources and in x_0: exact at any step, so a long one)
        h = 1e-2 * (abs(at) if at != 0 else 1.0)
        return (L(**make(at + h)) - L(**make(at - h))) / (2 * h)

    def with_row(i, v):
        out = [list(r) for r in rows]
        out[i][2] = repr(float(v))
        return out

    def with_cap(j, v):
        return [(c[0], v if q == j else c[1], c[2], c[3]) for q, c in enumerate(capacitors)]

    def with_source(name, k, v):
        out = {key: np.array(vals, dtype=np.float64) for key, vals in sources.items()}
        out[name][k] = v
        return out

    def with_initial(i, v):
        out = np.array(initial, dtype=np.float64)
        out[i] = v
        return out

    values = np.array([diff(float(rows[i][2]), lambda v, i=i: dict(rows_=with_row(i, v))) for i in comp])
    farads = np.array([diff(float(c[1]), lambda v, j=j: dict(caps_=with_cap(j, v))) for j, c in enumerate(capacitors)])
    swept = {name: np.array([diff_linear(float(vals[k]), lambda v, name=name, k=k: dict(sources_=with_source(name, k, v)))
                             for k in range(steps)]) for name, vals in (sources or {}).items()}
    init = None
    if initial is not None:
        init = np.array([diff_linear(float(initial[i]), lambda v, i=i: dict(initial_=with_initial(i, v))) for i in (range(len(initial)) if initial_subset is None else initial_subset)])
    return values.reshape(len(comp)), farads.reshape(len(capacitors)), swept, init


def relative_miss(got, want):
    """max |got - want| over the largest |want| (0 for empty arrays, inf for NaN)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if want.size == 0:
        return 0.0
    miss = np.abs(got - want).max()
    top = np.abs(want).max()
    if np.isnan(miss):
        return np.inf
    return float(miss / top) if top > 0 else (0.0 if miss == 0 else np.inf)


# ---- one RC section under Euler from a discharged capacitor: v_k = I R (1 - q^-k), q = 1 + h / (R C) -----------------
def rc_euler_derivatives(I, R, C, h, steps):
    """(dv_k/dR, dv_k/dC, dv_k/dI), k = 0 .. steps"""
    k = np.arange(steps + 1, dtype=np.float64)
    q = 1.0 + h / (R * C)
    decay, slope = q ** -k, k * q ** -(k + 1.0)  # (d q^-k / dq = -k q^-(k+1))
    dR = I * (1.0 - decay) + I * R * slope * (-h / (R * R * C))
    dC = I * R * slope * (-h / (R * C * C))
    dI = R * (1.0 - decay)
    return dR, dC, dI


# ---- the inputs of the tests ------------------------------------------------------------------------------------------
def seeded_case(rows, steps, ncaps, seed, caps=None):
    """capacitors (transient_reference.seeded_capacitors unless given), every A / E source whose name is defined once
    swept with seeded values, three seeded probes -- node to ground, ground to node, node to node -- and seeded
    cotangents [steps + 1, 3]: (capacitors, sources, probes, cotangents)"""
    from tests.gradient_reference import source_names
    from tests.transient_reference import seeded_capacitors
    rows = [list(r) for r in rows]
    nl = n.Netlist.from_rows(rows)
    rng = np.random.default_rng(1000 + seed)
    nodes = sorted(nl.nodenum, key=lambda s: nl.nodenum[s])
    pick = lambda: nodes[int(rng.integers(len(nodes)))]  # noqa: E731
    probes = [(pick(), nl.ground), (nl.ground, pick()), (pick(), pick())]
    sources = {name: rng.uniform(-5.0, 5.0, size=steps) for name in source_names(rows, 1 << 30)}
    caps = seeded_capacitors(rows, ncaps, seed=seed) if caps is None else caps
    return caps, sources, probes, rng.uniform(-1.0, 1.0, size=(steps + 1, len(probes)))


def small_grid_rows():
    from nodal_amd import generators as gen
    return list(gen.grid_rows(12)) + [["ld0", "A", "1", "40", "g"], ["ld1", "A", "1", "97", "g"]]


def edge_rows():
    """a six-node ladder with a VCVS on its last rung: every edge of the probe and capacitor lists on one small network"""
    rows = [["a1", "A", "0.8", "1", "g"], ["e1", "E", "1.5", "6", "g"]]
    rows += [[f"s{k}", "R", repr(1.0 + 0.25 * k), str(k), str(k + 1)] for k in range(1, 6)]
    rows += [[f"t{k}", "R", repr(3.0 + k), str(k), "g"] for k in (1, 2, 3, 4, 5)]
    return rows


EDGE_CAPACITORS = [("p1", 0.7, "2", "3"), ("p2", 1.9, "2", "3"),   # two in parallel on one pair
                   ("gf", 1.1, "g", "4"),                            # the ground lead first
                   ("np", 0.6, "5", "g")]                            # node 5: capacitors but no probe
EDGE_PROBES = [("1", "g"), ("g", "3"),                                # ground in either orientation
               ("3", "2"), ("2", "g"),                                # two probes on node 2 (and two on node 3)
               ("4", "4"),                                            # a == b: its cotangent must change nothing
               ("1", "6")]                                            # nodes 1 and 6: probes but no capacitor


# ---- the small inputs: the adjoint above and the central differences, computed once and shared ----------------------
DT = 0.4


def cfg5_rows():
    from nodal_amd import generators as gen
    rows = gen.cfg5_rows(12)
    nl = n.Netlist.from_rows(rows)
    assert nl.nums["kcl"] + nl.nums["be"] == 156  # (more than 64 unknowns: the sparse LU of the transposed child)
    return rows


@functools.lru_cache(maxsize=None)
def small_cases():
    """(name, rows, steps, seeded capacitors, given capacitors, given probes): the networks of the sensitivity tests'
    central differences (every component type, at most 64 unknowns: the dense panel), the edge network, and one input
    per sparse LU route"""
    from tests.test_sensitivity_frontend import FD_INPUTS
    return tuple([(name, rows, 6, 7, None, None) for name, rows in FD_INPUTS]
                 + [("edges", edge_rows(), 5, 0, EDGE_CAPACITORS, EDGE_PROBES),
                    ("grid(12)", small_grid_rows(), 17, 7, None, None), ("cfg5(12)", cfg5_rows(), 17, 7, None, None)])


@functools.lru_cache(maxsize=None)
def small_case(k, dc_start):
    """Case k of small_cases with its seeded capacitors, sources, probes, cotangents and (dc_start False) initial state;
    `adjoint` and `fd`: (values, capacitors, source values [steps, R], initial or None) by the reference's own adjoint
    and by central differences -- the values at the swept rows WITHOUT the sum over the steps (no step uses the table
    value of a swept source), and on networks of more than 64 unknowns on `subset` only: 24 seeded rows and every row
    that is not a resistor, and the initial state on 24 seeded `entries` (two to four forward runs each; the others are
    rows and entries of the same kind)."""
    from nodal_amd.sweep import resolve_sources
    name, rows, steps, ncaps, caps, probes = small_cases()[k]
    rows = [list(r) for r in rows]
    caps, sources, seeded_probes, cot = seeded_case(rows, steps, ncaps, k, caps)
    probes = seeded_probes if probes is None else probes
    rng = np.random.default_rng(k)
    cot = rng.uniform(-1.0, 1.0, size=(steps + 1, len(probes)))
    r = TransientGradientReference(rows, caps, DT)
    assert len(rows) == r.ncomp, "text rows are table rows in these inputs"
    pairs = probe_pairs(r.r.nl, probes)
    x0 = None if dc_start else rng.uniform(-1.0, 1.0, size=r.n)
    _, X = forward(rows, caps, DT, steps, sources, pairs, x0)
    table_rows, _ = resolve_sources(r.r.nl, sources)
    values, farads, swept, initial = r.public(pairs, cot, X, table_rows, dc_start)
    values = values.copy()
    values[table_rows] -= swept.sum(axis=0)
    subset = np.arange(len(rows))
    if r.n > 64:
        other = [i for i, row in enumerate(rows) if row[1] != "R"]
        subset = np.array(sorted(set(other) | set(rng.choice(len(rows), size=24, replace=False).tolist())))
    entries = np.arange(r.n) if r.n <= 64 else np.sort(rng.choice(r.n, size=24, replace=False))
    fv, fc, fs, fi = central_differences(lambda W: float((cot * W).sum()), rows, caps, DT, steps, sources, pairs, x0,
                                         subset=subset.tolist(), initial_subset=entries.tolist())
    fs = np.stack([fs[name] for name in sources], axis=1) if sources else np.zeros((steps, 0))
    return types.SimpleNamespace(name=name, rows=rows, steps=steps, capacitors=caps, sources=sources, probes=probes,
                                 pairs=pairs, cotangents=cot, initial=x0, X=X, table_rows=table_rows, subset=subset, ref=r,
                                 entries=entries,
                                 adjoint=(values[subset], farads, swept, None if dc_start else initial[entries]),
                                 fd=(fv, fc, fs, fi))


def disagreement(got, want):
    """the largest relative_miss over (values, capacitors, source values, initial); None entries are left out"""
    return max(relative_miss(g, w) for g, w in zip(got, want) if w is not None and g is not None)
