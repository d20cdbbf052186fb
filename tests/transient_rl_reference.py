"""The numpy / scipy restatement the transient tests WITH INDUCTORS are measured against (never product code).

Built on tests/transient_reference.py, which supplies the oracle's matrices, the right-hand sides and the capacitors'
history currents.  Inductor j has L_j henries between a and b, its current i counts positive from a to b through the
element, and v = x(a) - x(b).  Two INDEPENDENT formulations step in time:

  companion  the oracle's matrix of the netlist with one extra R row per capacitor and then per inductor (value L / h
             for Euler, 2 L / h for the trapezoidal rule, g = 1 / value) and per inductor the history current J_k into
             lead a, out of lead b:
                 Euler        J_k = -i_{k-1},                   i_k = i_{k-1} + g v_k
                 trapezoidal  J_k = -(i_{k-1} + g v_{k-1}),     i_k = i_{k-1} + g (v_k + v_{k-1})
  branch     the inductor currents as extra unknowns, [[M, S], [S^T, -D]] [x_k; i_k] = [b_k; r_k]: M and b_k the
             capacitor-companion matrix and right-hand side, S the inductors' incidence (+1 at a, -1 at b),
                 Euler        D = diag(L / h),   r_k = -D i_{k-1}
                 trapezoidal  D = diag(2 L / h), r_k = -D i_{k-1} - S^T x_{k-1}

The DC start is the oracle's solve of the netlist with one row ["ind__j", "E", "0.0", a, b] per inductor appended: an
inductor is a short there.  The oracle's E row puts -1 into G[a, m]: its branch unknown is the current that ENTERS lead
a from the element, so i_0 = -(that unknown).

On the CPU the two agree to 1e-15 of the largest potential and of the largest current on grid(12) with 149 seeded
capacitors and 9 seeded inductors over 33 steps, for both methods (measured: 2.7e-16 and 4.1e-16), and the closed form
of one RL section under Euler holds to 5e-16 (measured: 2.5e-16; tests/test_transient_inductors_frontend.py asserts
both), so the project's normwise bar TOL = 1e-9 leaves six decades for the device.
"""
import numpy as np
import scipy.sparse as sp

import nodal_amd as n
from oracle import nodal_oracle as oracle
from tests import transient_reference as ref
from tests.transient_reference import TOL, _index, _solver  # noqa: F401

# the component types whose stamp is a branch equation on the potentials of their own leads (the oracle stamps a VCCS as
# it stamps a VCVS): a short across a chain of them has no DC solution
VOLTAGE_DEFINED = ("E", "VCVS", "VCCS", "CCVS")


class RLReference:
    """rows: the netlist; capacitors, inductors: (name, value, node_a, node_b); dt; method "euler" or "trapezoidal"."""

    def __init__(self, rows, capacitors, inductors, dt, method):
        self.cap = ref.TransientReference(rows, capacitors, dt, method)
        c = self.cap
        self.rows, self.nl, self.n, self.dt, self.method = c.rows, c.nl, c.n, c.dt, method
        count = len(inductors)
        self.names = [i[0] for i in inductors]
        self.henries = np.array([float(i[1]) for i in inductors], dtype=np.float64).reshape(count)
        self.la = np.array([_index(self.nl, i[2]) for i in inductors], dtype=np.int64).reshape(count)
        self.lb = np.array([_index(self.nl, i[3]) for i in inductors], dtype=np.int64).reshape(count)
        self.value = (2.0 if method == "trapezoidal" else 1.0) * self.henries / self.dt  # the companion rows' ohms: D
        self.g = 1.0 / self.value
        self._full = self._branch = None

    def rhs_steps(self, sources, steps):
        return self.cap.rhs_steps(sources, steps)

    def _label(self, i):
        labels = {v: k for k, v in self.nl.nodenum.items()}
        return self.nl.ground if i < 0 else labels[int(i)]

    def _oracle_matrix(self, rows, branches):
        """the oracle's G, A of `rows` with the circuit's ground and numbering kept (the parser is overruled as
        TransientReference._companion does); `branches`: the names whose branch unknowns follow the circuit's"""
        aug = n.Netlist.from_rows([list(r) for r in rows])
        assert set(aug.nodenum) | {aug.ground} == set(self.nl.nodenum) | {self.nl.ground}
        assert aug.nums["kcl"] == self.nl.nums["kcl"] and aug.nums["be"] == self.nl.nums["be"] + len(branches)
        B = self.nl.nums["be"]
        aug.ground, aug.nodenum = self.nl.ground, self.nl.nodenum
        aug.anomnum = {**self.nl.anomnum, **{name: B + j for j, name in enumerate(branches)}}
        G, A, _ = oracle.build_model(aug, True)
        return sp.csr_matrix(G), np.asarray(A, dtype=np.float64).ravel()

    # -- the DC start: every inductor a zero-volt E row ----------------------------------------------------------------
    def dc_rows(self):
        return self.rows + [[f"ind__{j}", "E", "0.0", self._label(self.la[j]), self._label(self.lb[j])]
                            for j in range(len(self.g))]

    def dc_system(self):
        return self._oracle_matrix(self.dc_rows(), [f"ind__{j}" for j in range(len(self.g))])

    def dc_start(self):
        """(x_0 [n], i_0 [L]) at the netlist's own source values"""
        G, A = self.dc_system()
        e = _solver(G)(A)
        return e[:self.n], -e[self.n:]

    # -- companion stepping -----------------------------------------------------------------------------------------------
    def augmented_rows(self):
        """the netlist with the capacitors' companion rows and then the inductors' behind its own"""
        return self.cap.augmented_rows() + [[f"ind__{j}", "R", repr(float(self.value[j])), self._label(self.la[j]),
                                             self._label(self.lb[j])] for j in range(len(self.g))]

    def _companion(self):
        if self._full is None:
            self.G_full, _ = self._oracle_matrix(self.augmented_rows(), [])
            self._full = _solver(self.G_full)
        return self._full

    def voltages(self, x):
        xe = np.append(np.asarray(x, dtype=np.float64), 0.0)
        return xe[self.la] - xe[self.lb]

    def inject(self, J):
        b = np.zeros(self.n + 1)
        np.add.at(b, self.la, J)
        np.add.at(b, self.lb, -J)
        return b[:self.n]

    def history(self, x_prev, i_prev):
        if self.method == "euler":
            return -np.asarray(i_prev, dtype=np.float64)
        return -(i_prev + self.g * self.voltages(x_prev))

    def advance(self, x_prev, i_prev, A_k, Jc_prev=None):
        """one companion step: (x_k, i_k, the capacitors' J_k)"""
        Jc = self.cap.history(x_prev, Jc_prev)
        JL = self.history(x_prev, i_prev)
        x = self._companion()(A_k + self.cap.inject(Jc) + self.inject(JL))
        return x, -JL + self.g * self.voltages(x), Jc

    def run(self, x0, i0, A_steps):
        """companion stepping: (X [steps + 1, n], I [steps + 1, L])"""
        X, I, Jc = [np.asarray(x0, dtype=np.float64)], [np.asarray(i0, dtype=np.float64)], None
        for A_k in A_steps:
            x, i, Jc = self.advance(X[-1], I[-1], A_k, Jc)
            X.append(x)
            I.append(i)
        return np.array(X), np.array(I).reshape(len(X), len(self.g))

    def one_step_from(self, X, I, A_steps):
        """(X_ref[k], I_ref[k]) = the reference's step from X[k - 1], I[k - 1] (and the capacitors' histories rebuilt
        from X[0 .. k - 1]), k = 1 .. steps"""
        solve = self._companion()
        Xr, Ir = [], []
        for k, (A_k, Jc) in enumerate(zip(A_steps, self.cap.rebuilt_histories(X)), start=1):
            JL = self.history(X[k - 1], I[k - 1])
            x = solve(A_k + self.cap.inject(Jc) + self.inject(JL))
            Xr.append(x)
            Ir.append(-JL + self.g * self.voltages(x))
        return np.array(Xr), np.array(Ir).reshape(len(Xr), len(self.g))

    # -- branch stepping: the currents as unknowns ----------------------------------------------------------------------
    def incidence(self):
        S = sp.lil_matrix((self.n + 1, len(self.g)))
        for j, (a, b) in enumerate(zip(self.la, self.lb)):
            S[a, j] += 1.0
            S[b, j] -= 1.0
        return sp.csr_matrix(S)[:self.n, :]

    def run_branch(self, x0, i0, A_steps):
        """(X [steps + 1, n], I [steps + 1, L])"""
        self.cap._companion()
        M, S, D = self.cap.G_aug, self.incidence(), sp.diags(self.value)
        solve = _solver(sp.bmat([[M, S], [S.T, -D]], format="csc"))
        X, I, Jc = [np.asarray(x0, dtype=np.float64)], [np.asarray(i0, dtype=np.float64)], None
        for A_k in A_steps:
            Jc = self.cap.history(X[-1], Jc)
            r = -(D @ I[-1])
            if self.method == "trapezoidal":
                r = r - S.T @ X[-1]
            e = solve(np.concatenate([A_k + self.cap.inject(Jc), r]))
            X.append(e[:self.n])
            I.append(e[self.n:])
        return np.array(X), np.array(I).reshape(len(X), len(self.g))


# ---- one RL section: a current source I into a node with R and L to ground, i_0 = 0 -----------------------------------
def rl_rows(I, R):
    return ref.rc_rows(I, R)


def rl_euler_closed_form(I, R, L, h, steps):
    """(v_k, i_k), k = 0 .. steps, from x_0 = I R (all of I through R) and i_0 = 0:
    v_k = I R (1 + h R / L)^-k, i_k = I (1 - (1 + h R / L)^-k)"""
    k = np.arange(steps + 1, dtype=np.float64)
    decay = (1.0 + h * R / L) ** -k
    return I * R * decay, I * (1.0 - decay)


def seeded_inductors(rows, count, seed, to_ground=0.5):
    """up to `count` inductors on a seeded sample of node pairs and node-to-ground leads of the netlist `rows`, none of
    which closes a loop with the others or with the voltage-defined branches (VOLTAGE_DEFINED) of the parsed netlist,
    those an OPMODEL row expands to included: a loop of shorts and voltage sources has no DC solution"""
    import random
    rng = random.Random(seed)
    nl = n.Netlist.from_rows([list(r) for r in rows])
    nodes = sorted(nl.nodenum, key=lambda s: nl.nodenum[s])
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            x = parent[x]
        return x

    for key in nl.component_keys:
        comp = nl.components[key]
        if comp.type in VOLTAGE_DEFINED:
            parent[find(str(comp.anode))] = find(str(comp.bnode))
    out = []
    for _ in range(20 * count):
        if len(out) == count:
            break
        a = rng.choice(nodes)
        if rng.random() < to_ground or len(nodes) < 2:
            pair = (a, nl.ground) if rng.random() < 0.5 else (nl.ground, a)
        else:
            pair = (a, rng.choice([x for x in nodes if x != a]))
        ra, rb = find(str(pair[0])), find(str(pair[1]))
        if ra == rb:
            continue
        parent[ra] = rb
        out.append((f"lx{len(out)}", rng.uniform(0.2, 3.0), *pair))
    return out


def seeded_mix(rows, k):
    """the capacitors and inductors the one-step parity hangs on input k of the branches suite: 5 and (up to) 4"""
    return ref.seeded_capacitors(rows, 5, seed=k), seeded_inductors(rows, 4, seed=300 + k)


def grid12_mix():
    """grid(12) with two loads, a capacitor on every node and six between nodes, nine seeded inductors"""
    import random
    from nodal_amd import generators as gen
    rng = random.Random(7)
    rows = list(gen.grid_rows(12)) + [["ld0", "A", "1", "40", "g"], ["ld1", "A", "1", "97", "g"]]
    nl = n.Netlist.from_rows(rows)
    nodes = sorted(nl.nodenum, key=nl.nodenum.get)
    caps = [(f"cg{k}", rng.uniform(0.5, 2.0), node, "g") for k, node in enumerate(nodes)]
    caps += [(f"cc{k}", rng.uniform(0.5, 2.0), *rng.sample(nodes, 2)) for k in range(6)]
    return rows, caps, seeded_inductors(rows, 9, seed=3)
