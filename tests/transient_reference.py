"""The numpy / scipy restatement every transient test is measured against (never product code).

G comes from the oracle's build_model; the right-hand side is restated from the columns of the lowered table (an A row
puts +v on lead a and -v on lead b, an E row v on its branch row) and checked against the oracle's A at the netlist's
own values.  The capacitance matrix C comes from the capacitor list.  Two INDEPENDENT formulations step in time:

  state space   (networks whose only unknowns are potentials)
                Euler        (G + C/h) x_k   = A_k + C x_{k-1} / h
                trapezoidal  (G/2 + C/h) x_k = (C/h - G/2) x_{k-1} + (A_k + A_{k-1}) / 2
  companion     (any network) the oracle's matrix of the netlist with one extra R row per capacitor, value h / C
                (Euler) or h / (2 C) (trapezoidal), and per capacitor the history current J_k into lead a, out of
                lead b:  Euler J_k = g v_{k-1};  trapezoidal J_k = 2 g v_{k-1} - J_{k-1}, J_1 = g v_0.

On the CPU the two agree to 3e-15 of the largest potential on grid(100) with 10 049 capacitors over 33 steps, for both
methods, and the closed form of one RC section under Euler holds to 9e-16 (tests/test_transient_frontend.py asserts
both), so the project's normwise bar TOL = 1e-9 leaves six decades for the device.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import nodal_amd as n
from nodal_amd.lowering import lower
from oracle import nodal_oracle as oracle
from tests.sensitivity_reference import TOL  # noqa: F401  (the project's bar for solutions, normwise)

T_R, T_A, T_E = 0, 1, 2


def _index(nl, label):
    if label == nl.ground or str(label) == str(nl.ground):
        return -1
    return int(nl.nodenum[label] if label in nl.nodenum else nl.nodenum[str(label)])


def _solver(M):
    M = sp.csc_matrix(M)
    if M.shape[0] <= 64:
        dense = M.toarray()
        return lambda b: np.linalg.solve(dense, b)
    lu, Mr = spla.splu(M), sp.csr_matrix(M)

    def solve(b):  # (one step of refinement: the LU's own rounding is not to show in the comparisons)
        x = lu.solve(b)
        return x + lu.solve(b - Mr @ x)
    return solve


class TransientReference:
    """rows: the netlist; capacitors: (name, farads, node_a, node_b); dt; method "euler" or "trapezoidal"."""

    def __init__(self, rows, capacitors, dt, method):
        assert method in ("euler", "trapezoidal")
        self.rows, self.dt, self.method = [list(r) for r in rows], float(dt), method
        self.nl = n.Netlist.from_rows(self.rows)
        self.table = lower(self.nl)
        self.K, self.B = self.table.K, self.table.B
        self.n = self.K + self.B
        G, A, _ = oracle.build_model(self.nl, True)
        self.G = sp.csr_matrix(G)
        self.A0 = self.rhs({})
        assert np.array_equal(self.A0, np.asarray(A.todense() if sp.issparse(A) else A, dtype=np.float64).ravel())
        self.names = [c[0] for c in capacitors]
        self.farads = np.array([float(c[1]) for c in capacitors], dtype=np.float64).reshape(len(capacitors))
        self.ia = np.array([_index(self.nl, c[2]) for c in capacitors], dtype=np.int64).reshape(len(capacitors))
        self.ib = np.array([_index(self.nl, c[3]) for c in capacitors], dtype=np.int64).reshape(len(capacitors))
        self.g = (2.0 if method == "trapezoidal" else 1.0) * self.farads / self.dt
        self._aug = self._state = None

    # -- the right-hand side for given source values ---------------------------------------------------------------
    def rhs(self, values):
        """A with the named sources at `values` (name -> value), the others at the netlist's"""
        t = self.table
        v = np.array(t.value, dtype=np.float64)
        for row, key in enumerate(self.nl.component_keys):
            if key in values:
                v[row] = values[key]
        A = np.zeros(self.n + 1)
        for row in range(t.ncomp):  # (table order, as a sequential program stamps)
            if t.type[row] == T_A:
                A[t.a[row]] += v[row]
                A[t.b[row]] -= v[row]
            elif t.type[row] == T_E:
                A[t.K + t.k[row]] += v[row]
        return A[:self.n]  # (index -1, the ground lead, fell on the slot that is dropped)

    def rhs_steps(self, sources, steps):
        return [self.rhs({name: vals[k] for name, vals in (sources or {}).items()}) for k in range(steps)]

    # -- the capacitance matrix ---------------------------------------------------------------------------------------
    def capacitance(self):
        C = sp.lil_matrix((self.n + 1, self.n + 1))
        for c, a, b in zip(self.farads, self.ia, self.ib):
            C[a, a] += c
            C[b, b] += c
            C[a, b] -= c
            C[b, a] -= c
        return sp.csr_matrix(C)[:self.n, :self.n]

    # -- companion stepping ---------------------------------------------------------------------------------------------
    def augmented_rows(self):
        """the netlist with one companion R row per capacitor behind its own rows"""
        labels = {v: k for k, v in self.nl.nodenum.items()}
        name = lambda i: self.nl.ground if i < 0 else labels[int(i)]  # noqa: E731
        return self.rows + [[f"cap__{j}", "R", repr(float(1.0 / self.g[j])), name(self.ia[j]), name(self.ib[j])]
                            for j in range(len(self.g))]

    def _companion(self):
        if self._aug is None:
            aug = n.Netlist.from_rows(self.augmented_rows())
            # Capacitors introduce no nodes, and the circuit keeps its ground and its numbering: the parser, which
            # picks the ground by degree when there is no "g" and numbers nodes as it meets them, is overruled.
            assert set(aug.nodenum) | {aug.ground} == set(self.nl.nodenum) | {self.nl.ground}
            assert aug.anomnum == self.nl.anomnum and all(aug.nums[q] == self.nl.nums[q] for q in ("kcl", "be"))
            aug.ground, aug.nodenum = self.nl.ground, self.nl.nodenum
            G, _, _ = oracle.build_model(aug, True)
            self.G_aug = sp.csr_matrix(G)
            self._aug = _solver(self.G_aug)
        return self._aug

    def voltages(self, x):
        xe = np.append(np.asarray(x, dtype=np.float64), 0.0)
        return xe[self.ia] - xe[self.ib]

    def history(self, x_prev, J_prev=None):
        """J_k from x_{k-1} (and, trapezoidal, J_{k-1}; None: the start, J_1 = g v_0)"""
        gv = self.g * self.voltages(x_prev)
        if self.method == "euler" or J_prev is None:
            return gv
        return 2.0 * gv - J_prev

    def inject(self, J):
        b = np.zeros(self.n + 1)
        np.add.at(b, self.ia, J)
        np.add.at(b, self.ib, -J)
        return b[:self.n]

    def advance(self, x_prev, A_k, J_prev=None):
        """one companion step: (x_k, J_k)"""
        J = self.history(x_prev, J_prev)
        return self._companion()(A_k + self.inject(J)), J

    def run(self, x0, A_steps):
        """companion stepping from x0: X [steps + 1, n]"""
        X, J = [np.asarray(x0, dtype=np.float64)], None
        for A_k in A_steps:
            x, J = self.advance(X[-1], A_k, J)
            X.append(x)
        return np.array(X)

    def rebuilt_histories(self, X):
        """J_1 .. J_steps from the solutions X[0 .. steps - 1] somebody else computed (the one-step parity)"""
        out, J = [], None
        for x in X[:-1]:
            J = self.history(x, J)
            out.append(J)
        return out

    def one_step_from(self, X, A_steps):
        """X_ref[k] = the reference's step from X[k - 1] (and the histories rebuilt from X[0 .. k - 1]), k = 1 .. steps"""
        solve = self._companion()
        return np.array([solve(A_k + self.inject(J)) for A_k, J in zip(A_steps, self.rebuilt_histories(X))])

    # -- state-space stepping -------------------------------------------------------------------------------------------
    def run_state_space(self, x0, A_steps, A_start=None):
        """X [steps + 1, n]; A_start: the right-hand side in force at t_0 (the trapezoidal rule reads it)"""
        assert self.B == 0, "state-space stepping: potentials only"
        C, h = self.capacitance(), self.dt
        A_prev = self.A0 if A_start is None else A_start
        if self.method == "euler":
            solve, right = _solver(self.G + C / h), C / h
        else:
            solve, right = _solver(self.G / 2 + C / h), C / h - self.G / 2
        X = [np.asarray(x0, dtype=np.float64)]
        for A_k in A_steps:
            b = right @ X[-1] + (A_k if self.method == "euler" else (A_k + A_prev) / 2)
            X.append(solve(b))
            A_prev = A_k
        return np.array(X)

    def dc(self, A=None):
        return _solver(self.G)(self.A0 if A is None else A)


# ---- one RC section: a current source I into a node with R and C to ground ------------------------------------------
def rc_rows(I, R):
    return [["a1", "A", repr(float(I)), "1", "g"], ["r1", "R", repr(float(R)), "1", "g"]]


def rc_euler_closed_form(I, R, C, h, steps):
    """v_k = I R (1 - (1 + h / RC)^-k) from a discharged capacitor, k = 0 .. steps"""
    k = np.arange(steps + 1, dtype=np.float64)
    return I * R * (1.0 - (1.0 + h / (R * C)) ** -k)


def rc_trapezoidal_closed_form(I0, I1, R, C, h, steps):
    """from the DC point v_0 = I0 R with the source stepped to I1 at t_1: v_1 = ((1 - a) v_0 + a R (I0 + I1)) / (1 + a),
    then v_k = I1 R + (v_1 - I1 R) rho^(k - 1), a = h / (2 R C), rho = (1 - a) / (1 + a)"""
    a = h / (2.0 * R * C)
    v = np.empty(steps + 1)
    v[0] = I0 * R
    if steps >= 1:
        v1 = ((1.0 - a) * v[0] + a * R * (I0 + I1)) / (1.0 + a)
        k = np.arange(1, steps + 1, dtype=np.float64)
        v[1:] = I1 * R + (v1 - I1 * R) * ((1.0 - a) / (1.0 + a)) ** (k - 1.0)
    return v


def seeded_capacitors(rows, count, seed, to_ground=0.5):
    """`count` capacitors on a seeded sample of node pairs and node-to-ground leads of the netlist `rows`"""
    import random
    rng = random.Random(seed)
    nl = n.Netlist.from_rows([list(r) for r in rows])
    nodes = sorted(nl.nodenum, key=lambda s: nl.nodenum[s])
    caps = []
    for j in range(count):
        a = rng.choice(nodes)
        if rng.random() < to_ground or len(nodes) < 2:
            pair = (a, nl.ground) if rng.random() < 0.5 else (nl.ground, a)
        else:
            b = rng.choice([x for x in nodes if x != a])
            pair = (a, b)
        caps.append((f"cx{j}", rng.uniform(0.2, 3.0), *pair))
    return caps
