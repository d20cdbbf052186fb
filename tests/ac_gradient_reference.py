"""The numpy / scipy restatement every AC-gradient test is measured against (never product code), on tests/ac_reference.py.

A(w) = G + j B(w) is the AC reference's matrix, A x_f = s the forward system with the named sources at their complex
amplitudes and every other one off, W[f][p] = x_f(a_p) - x_f(b_p) the probe phasors.  The loss is the seeded
least-squares loss

    L = sum w[f][p] |W[f][p] - t[f][p]|^2,        g = dL/dRe W + j dL/dIm W = 2 w (W - t)

and two INDEPENDENT formulations give its derivatives:

  adjoint   c_f = sum_p conj(g[f][p]) (e(a_p) - e(b_p)), A(w_f)^T y_f = c_f by scipy's complex sparse LU of the TRANSPOSED
            matrix and one step of refinement, and dL = sum_f Re(y_f^T (ds - dA x_f)) evaluated per table row from
            sensitivity_reference's columns with complex lam = y_f and x = x_f:
                R           Re(D U) / v^2, plus Re(L(m_j) v_j (X(c_j) - X(d_j))) / v^2 for every CCVS / CCCS row j it drives
                VCVS        Re(L(m) U)                              CCVS, CCCS   -Re(L(m) U) / Rd
                A, E        exactly +0.0 (the forward sweep never reads their table value)
                capacitor   w Im(D U)                               inductor     Im(D U) / (w L^2)
                amplitude   conj(D_j), D_j = L(a) - L(b) (A row), L(m) (E row)
  central   central differences of the reference's own forward sweep in every table value, every capacitance and
            inductance, and the real and the imaginary part of every amplitude.  A changed table value reaches G as the
            change of that row's stamps (and of the CCVS / CCCS rows it drives) added to the oracle's G (G_of): assembling
            all of G anew rounds the change away where a conductance is added to far larger ones.  Steps: FD_STEP = 1e-2,
            FD_STEP / 2 and FD_STEP / 4 relative to the entry (absolute where the entry is 0), combined by Richardson's
            rule (64 D(h/4) - 20 D(h/2) + D(h)) / 45, whose error is O(h^6); for the amplitudes, in which the loss is a
            quadratic, one central difference with the relative step 1e-2 (exact for a quadratic).  L(v + h) - L(v - h)
            is evaluated without the cancellation of two nearly equal losses (loss_difference).  The rounding that is
            left grows as 1 / h: on the grids the two formulations disagree by 8e-9 of the largest entry at the step
            1e-4 and by 8e-12 at 1e-2, where the small inputs are at the rule's own error (6e-11 and 6e-12; measured on
            the CPU).  The A / E rows are not differenced: the forward sweep replaces their values by the amplitudes
            before it reads anything.

Bars.  parity_bars is the complex restatement of sensitivity_reference.parity_bars: an error of TOL |y|_inf in every entry
of y and of TOL |x|_inf in every entry of x carried through the bilinear formulas, plus 8 eps of the formula's scale (the
formulas with every phasor replaced by its magnitude and every difference by a sum), summed over the frequencies;
TOL = 1e-9 is the project's bar.  The two first-order terms stand beside the product of the two errors,
TOL^2 |y|_inf |x|_inf: where x and y both vanish at every lead of an element -- a capacitor across a voltage source that is
off -- the first-order terms and the scale are exactly zero, and a dense LU that leaves 1e-17 at both leads would miss a
bar of 0 by 1e-37.  Nowhere else does the product count (it is 1e-9 of the first-order terms).

MEASURED is the disagreement of the two formulations on the CPU, the largest difference over the largest entry of each
array (array_miss): 6.3e-12 over small_cases() below -- the 27 inputs of the branches suite with at most 64 unknowns, which
between them hold every component type, each with its seeded capacitors and inductors (seeded_mix), three frequencies,
two probes and the first independent source driven.  The worst is edge/vccs_standalone.
tests/test_ac_gradient_frontend.py asserts it with one decade of margin (CPU_DISAGREEMENT), and the device's end-to-end
bar against the same central differences (DEVICE_END_TO_END) is ten times the measured value as well: the decade covers
the differences' own floor.  On the larger inputs, differenced on fd_subset, the same measure gives 4.2e-12 (grid(60)),
9.0e-14 (cfg5(24)), 8.1e-12 (grid(24) with two loads) and 1.5e-12 (grid(12) with two E sources).
"""
import functools
import math
import types

import numpy as np
import scipy.sparse as sp

import nodal_amd as n
from oracle import nodal_oracle as oracle
from tests import ac_reference as acr
from tests import sensitivity_reference as sref
from tests.ac_reference import _index
from tests.noise_reference import two_outputs
from tests.sensitivity_reference import EPS, TOL, T_A, T_CCCS, T_CCVS, T_E, T_R, T_VCVS
from tests.transient_gradient_reference import relative_miss  # noqa: F401

FD_STEP = 1e-2
MEASURED = 6.3e-12                  # |adjoint - central differences| on the CPU (the module's docstring)
CPU_DISAGREEMENT = 10 * MEASURED    # asserted on the CPU: one decade of margin
DEVICE_END_TO_END = 10 * MEASURED   # the device's result against the same central differences
CASE_FREQS = [0.01, 0.3, 10.0]


def _solve(M, b):
    M = sp.csc_matrix(M)
    if M.shape[0] <= 64:
        return np.linalg.solve(M.toarray(), b)
    return acr._refined(M)(b)


def _phasor_terms(table, lam, x, value, absolute):
    """the per-row formulas with complex lam, x ([n] each): Re(D U) / den per row, the cross terms in table order; with
    `absolute` the same with magnitudes and sums -- the formula's scale.  A / E rows and rows without a term: 0."""
    t = sref._columns(table)
    v = np.asarray(table.value if value is None else value, dtype=np.float64)
    L, X = np.append(np.asarray(lam), 0.0), np.append(np.asarray(x), 0.0)
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
        s = np.where(ty == T_R, np.real(dL * dX) / (v * v), s)
        s = np.where(ty == T_VCVS, np.real(Lm * dXc), s)
        s = np.where((ty == T_CCVS) | (ty == T_CCCS), sign * np.real(Lm * dXc) / Rd, s)
        for j in np.flatnonzero(((ty == T_CCVS) | (ty == T_CCCS)) & (t["drv"] >= 0)):
            i = t["drv"][j]
            if ty[i] == T_R:
                s[i] += np.real(Lm[j] * dXc[j]) * v[j] / (v[i] * v[i])
    return s


class ACGradientReference:
    """rows: the netlist; capacitors, inductors: (name, value, node_a, node_b)."""

    def __init__(self, rows, capacitors=(), inductors=()):
        self.rows = [list(r) for r in rows]
        self.ac = acr.ACReference(self.rows, capacitors, inductors)
        self.nl, self.n, self.K = self.ac.nl, self.ac.n, self.ac.K
        self.table = self.ac.base.table
        self.ncomp = int(self.table.ncomp)
        self.type = np.asarray(self.table.type, dtype=np.int64).reshape(self.ncomp)
        self.keys = list(self.nl.component_keys)
        self.ncap = int((self.ac.kind == 0).sum())

    # -- pieces -----------------------------------------------------------------------------------------------------
    def first_source(self):
        """the first A / E row's name, in table order, or None"""
        return next((self.keys[i] for i in range(self.ncomp) if self.type[i] in (T_A, T_E)), None)

    def source_rows(self, names):
        """the table rows that carry one of `names`, ascending (what resolve_amplitudes drives)"""
        return np.array([i for i in range(self.ncomp) if self.keys[i] in names and self.type[i] in (T_A, T_E)], dtype=np.int64)

    def pairs(self, probes):
        out = [(p, self.nl.ground) if not isinstance(p, (tuple, list)) else tuple(p) for p in probes]
        return [(_index(self.nl, a), _index(self.nl, b)) for a, b in out]

    def G_of(self, values):
        """G with the value column replaced: the oracle's G of the netlist plus the CHANGE of the stamps of the rows whose
        value differs (and of the CCVS / CCCS rows they drive), G_S(values) - G_S(table values), both from the oracle's
        vectorised stamp of the lowered table with every other row masked (typed A: a current source stamps nothing into
        G).  Assembling the whole of G anew would round the change away wherever a row's conductance is added to larger
        ones -- in edge/self_loop_r_bits the 3.3 S of r1 go under in the 1e17 S of the self-loop, and G(1, 1) would not
        move at all.  Where the vectorised stamp refuses a table (a SET stamp that coincides with another), the oracle's
        own build of the text rows with the values written into them (such inputs have one text row per table row)"""
        values, base = np.asarray(values, dtype=np.float64), np.asarray(self.table.value, dtype=np.float64)
        changed = values != base
        drv = np.asarray(self.table.drv)
        keep = changed | ((drv >= 0) & changed[np.where(drv >= 0, drv, 0)])
        masked = np.where(keep, np.asarray(self.table.type), T_A).astype(np.uint8)

        def part(column):
            t = self.table.with_values(column)
            t.type = masked
            return sp.csr_matrix(oracle.assemble_fast(t)[0])
        try:
            return sp.csr_matrix(self.ac.G + (part(values) - part(base)))
        except AssertionError:
            assert len(self.rows) == self.ncomp and all(float(r[2]) == v for r, v in zip(self.rows, self.table.value))
            rows = [[r[0], r[1], repr(float(v))] + r[3:] for r, v in zip(self.rows, values)]
            return sp.csr_matrix(oracle.build_model(n.Netlist.from_rows(rows), True)[0])

    def matrix(self, omega, G=None, react=None):
        value = self.ac.value if react is None else np.asarray(react, dtype=np.float64)
        b = np.where(self.ac.kind == 0, omega * value, -1.0 / (omega * value))
        B = self.ac.S @ sp.diags(b) @ self.ac.S.T if len(value) else sp.csr_matrix((self.n, self.n))
        return sp.csc_matrix(sp.csc_matrix(self.ac.G if G is None else G, dtype=np.complex128) + 1j * B)

    def phasors(self, frequencies, amplitudes, pairs, values=None, react=None):
        """(W [F, P], X [F, n]) of the reference's own forward sweep"""
        G = None if values is None else self.G_of(values)
        s = self.ac.rhs(amplitudes)
        X = np.array([_solve(self.matrix(2.0 * math.pi * float(f), G, react), s) for f in frequencies]).reshape(len(frequencies), self.n)
        Xe = np.hstack([X, np.zeros((len(X), 1))])
        W = np.array([[Xe[f, a] - Xe[f, b] if a != b else 0.0 for a, b in pairs] for f in range(len(X))], dtype=np.complex128)
        return W.reshape(len(X), len(pairs)), X

    def seed(self, pairs, g):
        """c_f from row f of the cotangents, added in probe order"""
        c = np.zeros(self.n + 1, dtype=np.complex128)
        for (a, b), v in zip(pairs, g):
            if a != b:
                c[a] += np.conj(v)
                c[b] -= np.conj(v)
        return c[:self.n]

    def adjoints(self, frequencies, pairs, cot, transpose=True):
        """Y [F, n]; transpose=False solves with A in place of A^T: the mistake the suites must be able to see"""
        out = []
        for f, hz in enumerate(frequencies):
            A = self.matrix(2.0 * math.pi * float(hz))
            out.append(_solve(A.T if transpose else A, self.seed(pairs, cot[f])))
        return np.array(out).reshape(len(frequencies), self.n)

    # -- the formulas -----------------------------------------------------------------------------------------------
    def table_terms(self, y, x, absolute=False):
        return _phasor_terms(self.table, y, x, None, absolute)

    def react_terms(self, omega, y, x, absolute=False):
        L, X = np.append(y, 0.0), np.append(x, 0.0)
        ia, ib, v = self.ac.ia, self.ac.ib, self.ac.value
        coef = np.where(self.ac.kind == 0, omega, 1.0 / (omega * v * v))
        if absolute:
            return coef * (np.abs(L[ia]) + np.abs(L[ib])) * (np.abs(X[ia]) + np.abs(X[ib]))
        return coef * np.imag((L[ia] - L[ib]) * (X[ia] - X[ib]))

    def source_terms(self, y, rows, absolute=False):
        t = sref._columns(self.table)
        L = np.append(y, 0.0)
        if absolute:
            L = np.abs(L)
            return np.array([L[t["a"][i]] + L[t["b"][i]] if self.type[i] == T_A else L[t["m"][i]] for i in rows]).reshape(len(rows))
        return np.conj(np.array([L[t["a"][i]] - L[t["b"][i]] if self.type[i] == T_A else L[t["m"][i]] for i in rows],
                                dtype=np.complex128)).reshape(len(rows))

    def gradient(self, frequencies, amplitudes, probes, cot, transpose=True):
        """the adjoint formulation: (values [ncomp], reactive [E], source terms [F, R], W [F, P], X, Y), the sums over the
        frequencies in ascending index"""
        pairs = self.pairs(probes)
        W, X = self.phasors(frequencies, amplitudes, pairs)
        Y = self.adjoints(frequencies, pairs, cot, transpose)
        rows = self.source_rows(set(amplitudes or {}))
        values, react = np.zeros(self.ncomp), np.zeros(len(self.ac.value))
        terms = np.zeros((len(frequencies), len(rows)), dtype=np.complex128)
        for f, hz in enumerate(frequencies):
            values = values + self.table_terms(Y[f], X[f])
            react = react + self.react_terms(2.0 * math.pi * float(hz), Y[f], X[f])
            terms[f] = self.source_terms(Y[f], rows)
        return values, react, terms, W, X, Y

    def parity_bars(self, frequencies, X, Y, rows):
        """(values [ncomp], reactive [E], source terms [F, R]): an error of TOL |y|_inf in every entry of y and of
        TOL |x|_inf in every entry of x carried through the bilinear formulas -- the two first-order terms and the
        product of the two errors (module docstring) -- plus 8 eps of the formula's scale, summed over the frequencies"""
        values, react = np.zeros(self.ncomp), np.zeros(len(self.ac.value))
        terms = np.zeros((len(frequencies), len(rows)))
        for f, hz in enumerate(frequencies):
            w = 2.0 * math.pi * float(hz)
            y, x = np.abs(Y[f]), np.abs(X[f])
            ones_y, ones_x = np.full(self.n, y.max(initial=0.0)), np.full(self.n, x.max(initial=0.0))
            for total, F in ((values, self.table_terms), (react, lambda l, u, a: self.react_terms(w, l, u, a))):
                total += TOL * (F(ones_y, x, True) + F(y, ones_x, True)) + TOL * TOL * F(ones_y, ones_x, True) + 8 * EPS * F(y, x, True)
            terms[f] = TOL * self.source_terms(ones_y, rows, True) + 8 * EPS * self.source_terms(y, rows, True)
        return values, react, terms

    # -- central differences ----------------------------------------------------------------------------------------
    def loss(self, W, weights, targets):
        return float((weights * np.abs(W - targets) ** 2).sum())

    def probe(self, x, pairs):
        xe = np.append(x, 0.0)
        return np.array([xe[a] - xe[b] if a != b else 0.0 for a, b in pairs], dtype=np.complex128).reshape(len(pairs))

    def loss_difference(self, frequencies, amplitudes, pairs, weights, targets, plus, minus):
        """L(plus) - L(minus) of two forward sweeps that differ in the table values or the reactive values (dicts of
        `values`, `react`), without the cancellation of two nearly equal losses: with A+ x+ = s = A- x-,
        x+ - x- = -A+^-1 (A+ - A-) x- and |W+ - t|^2 - |W- - t|^2 = Re(conj(W+ - W-) (W+ + W- - 2 t)), both exact"""
        Gp, Gm = (None if side.get("values") is None else self.G_of(side["values"]) for side in (plus, minus))
        s = self.ac.rhs(amplitudes)
        total = 0.0
        for f, hz in enumerate(frequencies):
            w = 2.0 * math.pi * float(hz)
            Ap, Am = self.matrix(w, Gp, plus.get("react")), self.matrix(w, Gm, minus.get("react"))
            xm = _solve(Am, s)
            Wm, dW = self.probe(xm, pairs), self.probe(_solve(Ap, -((Ap - Am) @ xm)), pairs)
            total += float((weights[f] * np.real(np.conj(dW) * (2.0 * Wm + dW - 2.0 * targets[f]))).sum())
        return total

    def central_differences(self, frequencies, amplitudes, probes, weights, targets, subset=None, step=FD_STEP):
        """(values [len(subset)], reactive [E], amplitudes {name: complex}) of the loss by central differences of the
        forward sweep; subset: the table rows differenced (None: all); A / E rows are exactly 0 (the module's docstring)"""
        pairs = self.pairs(probes)
        amplitudes = {name: complex(v) for name, v in (amplitudes or {}).items()}
        base_v, base_r = np.array(self.table.value, dtype=np.float64), np.array(self.ac.value, dtype=np.float64)

        def L(amps):
            return self.loss(self.phasors(frequencies, amps, pairs)[0], weights, targets)

        def diff(at, make):
            d = []
            for rel in (step, step / 2, step / 4):
                h = rel * (abs(at) if at != 0 else 1.0)
                d.append(self.loss_difference(frequencies, amplitudes, pairs, weights, targets, make(at + h), make(at - h)) / (2 * h))
            return (64.0 * d[2] - 20.0 * d[1] + d[0]) / 45.0

        def replaced(base, i, v):
            out = base.copy()
            out[i] = v
            return out

        comp = list(range(self.ncomp)) if subset is None else list(subset)
        values = np.array([0.0 if self.type[i] in (T_A, T_E) else
                           diff(base_v[i], lambda v, i=i: dict(values=replaced(base_v, i, v))) for i in comp]).reshape(len(comp))
        react = np.array([diff(base_r[q], lambda v, q=q: dict(react=replaced(base_r, q, v))) for q in range(len(base_r))]).reshape(len(base_r))
        amps = {}
        for name, at in amplitudes.items():
            h = 1e-2 * (abs(at) if at != 0 else 1.0)
            parts = [(L({**amplitudes, name: at + d}) - L({**amplitudes, name: at - d})) / (2 * h) for d in (h, 1j * h)]
            amps[name] = complex(parts[0], parts[1])
        return values, react, amps


def seeded_loss(W, seed):
    """(weights [F, P] in [0.5, 1.5], targets complex [F, P] of the size of the largest phasor, g = 2 w (W - t))"""
    rng = np.random.default_rng(4000 + seed)
    top = np.abs(W).max(initial=0.0)
    top = top if top > 0 else 1.0
    weights = rng.uniform(0.5, 1.5, size=W.shape)
    targets = top * (rng.uniform(-1.0, 1.0, size=W.shape) + 1j * rng.uniform(-1.0, 1.0, size=W.shape))
    return weights, targets, 2.0 * weights * (W - targets)


def fd_subset(r, seed, count=12):
    """the table rows the central differences are taken for: all of them up to 64 unknowns; beyond, `count` seeded rows
    and `count` seeded rows that are neither resistors nor independent sources (two to four sweeps each: the others
    are rows of the same kinds)"""
    if r.n <= 64:
        return np.arange(r.ncomp)
    rng = np.random.default_rng(seed)
    other = np.flatnonzero((r.type != T_R) & (r.type != T_A) & (r.type != T_E))
    pick = rng.choice(r.ncomp, size=min(count, r.ncomp), replace=False).tolist()
    pick += rng.choice(other, size=min(count, len(other)), replace=False).tolist()
    return np.array(sorted(set(pick)), dtype=np.int64)


def case_of(rows, capacitors, inductors, frequencies, probes, sources, seed, fd=True):
    """Everything the tests compare against, computed once: the reference, the seeded loss and its cotangents, the
    adjoint formulation with its bars, and (fd) the central differences on fd_subset"""
    r = ACGradientReference(rows, capacitors, inductors)
    amplitudes = dict(sources or {})
    pairs = r.pairs(probes)
    W, _ = r.phasors(frequencies, amplitudes, pairs)
    weights, targets, cot = seeded_loss(W, seed)
    values, react, terms, W, X, Y = r.gradient(frequencies, amplitudes, probes, cot)
    src_rows = r.source_rows(set(amplitudes))
    by_name = {}
    for j, i in enumerate(src_rows.tolist()):
        by_name[r.keys[i]] = by_name.get(r.keys[i], 0j) + complex(terms[:, j].sum())
    case = types.SimpleNamespace(ref=r, rows=r.rows, capacitors=list(capacitors), inductors=list(inductors),
                                 frequencies=list(frequencies), probes=list(probes), sources=amplitudes or None, pairs=pairs,
                                 weights=weights, targets=targets, cotangents=cot, values=values, react=react, terms=terms,
                                 by_name=by_name, W=W, X=X, Y=Y, source_rows=src_rows,
                                 bars=r.parity_bars(frequencies, X, Y, src_rows), subset=None, fd=None)
    if fd:
        case.subset = fd_subset(r, seed)
        case.fd = r.central_differences(frequencies, amplitudes, probes, weights, targets, subset=case.subset.tolist())
    return case


def array_miss(got, want, bars):
    """relative_miss: the largest difference over the largest expected entry of the array.  An array in which every
    entry, expected and obtained, lies within its parity bar has no largest entry to measure against -- what stands there
    is the rounding of solves that are good to TOL normwise, not a derivative (doc/test_1: a source pins every probe):
    it counts as 0, and as inf where only the expected entries lie within the bars"""
    got, want, bars = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bars, dtype=np.float64)
    if want.size and (np.abs(want) <= bars).all():
        return 0.0 if (np.abs(got) <= bars).all() else np.inf
    return relative_miss(got, want)


def disagreement(case, values, react, by_name):
    """the largest array_miss of (values on the subset, reactive, amplitudes by name) against the case's central
    differences"""
    fv, fr, fa = case.fd
    names = sorted(fa)
    bar_of = {k: sum(case.bars[2][:, j].sum() for j, i in enumerate(case.source_rows.tolist()) if case.ref.keys[i] == k) for k in names}
    return max(array_miss(np.asarray(values)[case.subset], fv, case.bars[0][case.subset]), array_miss(react, fr, case.bars[1]),
               array_miss(np.array([[by_name[k].real, by_name[k].imag] for k in names]).ravel(),
                          np.array([[fa[k].real, fa[k].imag] for k in names]).ravel(),
                          np.array([[bar_of[k], bar_of[k]] for k in names]).ravel()))


# ---- the small inputs: both formulations, computed once and shared -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def input_case(k):
    """input k of the branches suite with seeded_mix elements, CASE_FREQS, two_outputs and the first source at 1 - 0.5j"""
    from tests.test_gpu_branches import INPUTS
    from tests.transient_rl_reference import seeded_mix
    name, rows = INPUTS[k]
    caps, inds = seeded_mix(rows, k)
    probe = ACGradientReference(rows, caps, inds)
    source = probe.first_source()
    case = case_of(rows, caps, inds, CASE_FREQS, two_outputs(probe.nl), {source: 1.0 - 0.5j} if source else None, k)
    case.name = name
    return case


def small_cases():
    """the indices of the inputs with at most 64 unknowns: 27 of the 29"""
    from tests.test_gpu_branches import INPUTS

    def unknowns(rows):
        nl = n.Netlist.from_rows([list(r) for r in rows])
        return nl.nums["kcl"] + nl.nums["be"]
    return [k for k, (_, rows) in enumerate(INPUTS) if unknowns(rows) <= 64]


# ---- closed forms -----------------------------------------------------------------------------------------------------
def rc_lowpass_derivatives(frequencies, R, C):
    """(|H|^2, d|H|^2/dR, d|H|^2/dC) of H = v_out / v_in = 1 / (1 + j w R C), per frequency"""
    w = 2.0 * math.pi * np.asarray(frequencies, dtype=np.float64)
    den = 1.0 + (w * R * C) ** 2
    return 1.0 / den, -2.0 * w * w * R * C * C / den ** 2, -2.0 * w * w * R * R * C / den ** 2


def series_rlc_derivatives(frequencies, R, L, C):
    """(|v_R|^2, its derivatives in R, L, C) of the voltage across the resistor of ac_reference.series_rlc_rows at the
    amplitude 1: |v_R|^2 = R^2 / (R^2 + X^2), X = w L - 1 / (w C)"""
    w = 2.0 * math.pi * np.asarray(frequencies, dtype=np.float64)
    X = w * L - 1.0 / (w * C)
    den = R * R + X * X
    return (R * R / den, 2.0 * R * X * X / den ** 2, -2.0 * R * R * X * w / den ** 2,
            -2.0 * R * R * X / (w * C * C) / den ** 2)
