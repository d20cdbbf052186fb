"""The numpy / scipy restatement the transient tests WITH DIODES are measured against (never product code).

Built on tests/transient_rl_reference.py (the oracle's companion matrix M of the netlist with one R row per capacitor and
then per inductor, the right-hand sides A_k and the history currents) and on tests/newton_reference.py (the diode model,
the incidence S of the diodes, SPICE's junction limiting and the convergence test).  Step k solves, for x_k,

    M x_k + S i(S^T x_k) = base_k,    base_k = A_k + the capacitors' and the inductors' history currents from x_{k-1}

by Newton's method from vh^0 = S^T x_{k-1}: linearise at vh^j, solve (M + S diag(g) S^T) x = base_k + S J, limit, test;
base_k is formed once per step and the inductor currents advance once per step, from the converged x_k.

Two checks are made of somebody else's solutions X [steps + 1, n] (the device's, keep_every=1):

  step parity  the states are REBUILT from X -- the capacitors' J by the recurrence from J_0 = g v_0, the inductors'
               currents from i_0 -- and every step is solved from X[k - 1] to the reference's OWN convergence, whatever
               path the device's iteration took: no limiter threshold can make a comparison undecidable
  residual     the nonlinear KCL defect of step k in fp64 against its scale; for backward Euler in the state-space form
               G x_k + C (x_k - x_{k-1}) / h + S_L i_k + S i(S^T x_k) - A_k with i_k = i_{k-1} + (h / L) S_L^T x_k, which
               knows nothing of companion rows; for the trapezoidal rule M x_k + S i(S^T x_k) - base_k

`run` is the whole loop on the host, with the defects tests/test_transient_nl_reference.py plants.
"""
import numpy as np
import scipy.sparse as sp
from scipy.special import lambertw

from tests import newton_reference as nr
from tests.newton_reference import I_SAT, N_VT, RESID_BAR, TIGHT, TOL, NewtonReference  # noqa: F401
from tests.transient_rl_reference import RLReference

DEFECTS = ("history_from_iterate", "J_sign", "inductor_per_iteration")


class TransientDiodeReference:
    """rows: the netlist; capacitors, inductors: (name, value, node_a, node_b); diodes: (name, i_sat, n_vt, anode,
    cathode); dt; method; the tolerances as Circuit.transient takes them."""

    def __init__(self, rows, capacitors, inductors, diodes, dt, method, gmin=1e-12, reltol=1e-3, vntol=1e-6, abstol=1e-12,
                 max_iter=50):
        self.rl = RLReference(rows, capacitors, inductors, dt, method)
        self.cap = self.rl.cap
        self.n, self.dt, self.method = self.rl.n, float(dt), method
        self.newton = NewtonReference(rows, diodes, gmin=gmin, reltol=reltol, vntol=vntol, abstol=abstol, max_iter=max_iter)
        self.G = self.newton.G  # the netlist's own matrix
        self.rl._companion()
        self.M = sp.csr_matrix(self.rl.G_full)
        self.newton.G = self.M  # (one_step then solves with M + S diag(g) S^T)
        self.gmin, self.reltol, self.vntol, self.abstol, self.max_iter = gmin, reltol, vntol, abstol, max_iter
        self.highest_junction = -np.inf  # over every linearisation point of every step solved
        self.most_iterations = 0
        self.unconverged = 0

    def rhs_steps(self, sources, steps):
        return self.rl.rhs_steps(sources, steps)

    # -- the start ------------------------------------------------------------------------------------------------------
    def dc_start(self, x_guess=None):
        """the nonlinear DC operating point with capacitors open, inductors shorts and diodes in, at the netlist's own
        source values: (x_0 [n], i_0 [L], Newton iterations)"""
        G, A = self.rl.dc_system()
        dc = NewtonReference.__new__(NewtonReference)
        dc.__dict__.update(self.newton.__dict__)
        L = len(self.rl.g)
        dc.G, dc.A, dc.n = sp.csr_matrix(G), A, self.n + L
        dc.S = sp.vstack([self.newton.S, sp.csr_matrix((L, self.newton.S.shape[1]))], format="csr")
        r = dc.run(x_guess)
        assert r["converged"], "the reference's DC start did not converge"
        return r["x"][:self.n], -r["x"][self.n:], r["iterations"]

    # -- one step ---------------------------------------------------------------------------------------------------------
    def base(self, A_k, Jc, JL):
        return A_k + self.cap.inject(Jc) + self.rl.inject(JL)

    def solve_step(self, x_prev, base, both=False, defect=None, rebase=None):
        """Newton's method on M x + S i(S^T x) = base from vh^0 = S^T x_prev: (x, iterations, converged).  rebase(x): a
        planted defect's right-hand side for the iterations after the first."""
        nw = self.newton
        nw.A = base
        x, vh = np.asarray(x_prev, dtype=np.float64), nw.voltages(x_prev)
        for j in range(self.max_iter):
            self.highest_junction = max(self.highest_junction, float(vh.max(initial=-np.inf)))
            x, vh, flags = nw.one_step(x, vh, both=both, defect="J_sign" if defect == "J_sign" else None)
            if not flags["not_converged"].any():
                self.most_iterations = max(self.most_iterations, j + 1)
                return x, j + 1, True
            if rebase is not None:
                nw.A = rebase(x)
        self.unconverged += 1
        return x, self.max_iter, False

    # -- the whole loop, and its planted defects --------------------------------------------------------------------------
    def run(self, x0, i0, A_steps, defect=None, both=False):
        """(X [steps + 1, n], I [steps + 1, L], Newton iterations [steps])"""
        assert defect is None or defect in DEFECTS
        rl, cap = self.rl, self.cap
        X, I, Jc, its = [np.asarray(x0, dtype=np.float64)], [np.asarray(i0, dtype=np.float64).reshape(len(rl.g))], None, []
        for A_k in A_steps:
            Jc_prev, i_prev = Jc, I[-1]
            Jc, JL = cap.history(X[-1], Jc_prev), rl.history(X[-1], i_prev)
            rebase = None
            if defect == "history_from_iterate":  # the capacitors' history from the Newton iterate, not from x_{k-1}
                rebase = lambda x, A_k=A_k, Jc_prev=Jc_prev, JL=JL: self.base(A_k, cap.history(x, Jc_prev), JL)  # noqa: E731
            if defect == "inductor_per_iteration":  # the inductor lane after every iteration
                state = {"i": i_prev, "J": JL}

                def rebase(x, A_k=A_k, Jc=Jc, state=state):
                    state["i"] = -state["J"] + rl.g * rl.voltages(x)
                    state["J"] = rl.history(x, state["i"])
                    return self.base(A_k, Jc, state["J"])
            x, it, _ = self.solve_step(X[-1], self.base(A_k, Jc, JL), both=both, defect=defect, rebase=rebase)
            X.append(x)
            I.append(-JL + rl.g * rl.voltages(x))
            its.append(it)
        return np.array(X), np.array(I).reshape(len(X), len(rl.g)), np.array(its)

    # -- the two checks of somebody else's solutions ----------------------------------------------------------------------
    def rebuilt_states(self, X, i0):
        """per step k = 1 .. steps: (the capacitors' J_k, the inductors' J_k, i_{k-1}) from X[0 .. k - 1] and i_0, and the
        currents I [steps + 1, L] they imply"""
        rl = self.rl
        I, out = [np.asarray(i0, dtype=np.float64).reshape(len(rl.g))], []
        for k, Jc in enumerate(self.cap.rebuilt_histories(X), start=1):
            JL = rl.history(X[k - 1], I[-1])
            out.append((Jc, JL, I[-1]))
            I.append(-JL + rl.g * rl.voltages(X[k]))
        return out, np.array(I).reshape(len(X), len(rl.g))

    def parity(self, X, i0, A_steps, both=False):
        """(worst of |X[k] - ref_k| - ((2 TOL + reltol) max |X[k]| + vntol) over the steps, i.e. <= 0 passes; the worst
        error relative to max |X[k]|; the reference's iterations per step; I rebuilt [steps + 1, L])"""
        states, I = self.rebuilt_states(X, i0)
        excess, rel, its = -np.inf, 0.0, []
        for k, (A_k, (Jc, JL, _)) in enumerate(zip(A_steps, states), start=1):
            x, it, ok = self.solve_step(X[k - 1], self.base(A_k, Jc, JL), both=both)
            its.append(it if ok else -1)
            err, top = float(np.abs(X[k] - x).max()), float(np.abs(X[k]).max())
            excess = max(excess, err - ((2 * TOL + self.reltol) * top + self.vntol))
            rel = max(rel, err / max(top, np.finfo(float).tiny))
        return excess, rel, its, I

    def residual(self, X, i0, A_steps):
        """per step (max |r|, max scale): the nonlinear KCL defect of X[k] and its scale"""
        rl, cap, nw, h = self.rl, self.cap, self.newton, self.dt
        states, I = self.rebuilt_states(X, i0)
        out = []
        if self.method == "euler":
            C, SL = cap.capacitance(), rl.incidence()
            i = np.asarray(i0, dtype=np.float64).reshape(len(rl.g))
            for k, A_k in enumerate(A_steps, start=1):
                x, xp = X[k], X[k - 1]
                i = i + (h / rl.henries) * (SL.T @ x)
                idio = nw.current(nw.voltages(x))
                r = self.G @ x + C @ (x - xp) / h + SL @ i + nw.S @ idio - A_k
                scale = abs(self.G) @ np.abs(x) + abs(C) @ (np.abs(x) + np.abs(xp)) / h + abs(SL) @ np.abs(i) + \
                    abs(nw.S) @ np.abs(idio) + np.abs(A_k)
                out.append((float(np.abs(r).max()), float(scale.max())))
            return out
        for k, (A_k, (Jc, JL, _)) in enumerate(zip(A_steps, states), start=1):
            x = X[k]
            idio, b = nw.current(nw.voltages(x)), self.base(A_k, Jc, JL)
            r = self.M @ x + nw.S @ idio - b
            scale = abs(self.M) @ np.abs(x) + abs(nw.S) @ np.abs(idio) + np.abs(A_k) + np.abs(cap.inject(Jc)) + np.abs(rl.inject(JL))
            out.append((float(np.abs(r).max()), float(scale.max())))
        return out

    def residual_excess(self, X, i0, A_steps):
        """worst of r / scale - (RESID_BAR + reltol + abstol / scale) over the steps (<= 0 passes), and the worst r / scale"""
        pairs = self.residual(X, i0, A_steps)
        excess = max((r / s - (RESID_BAR + self.reltol + self.abstol / s) for r, s in pairs), default=-np.inf)
        return excess, max((r / s for r, s in pairs), default=0.0)


# ---- closed form: a capacitor and a diode from one node to ground, nothing else (gmin = 0), backward Euler -------------
def rc_diode_rows():
    """the netlist needs a component: a resistor of 1e300 ohms carries nothing that fp64 can see"""
    return [["rbig", "R", "1e300", "1", "g"]]


def rc_diode_closed_form(v0, C, i_sat, n_vt, h, steps):
    """C (v_k - v_{k-1}) / h + i_sat (exp(v_k / n_vt) - 1) = 0:
    v_k = u - n_vt W((h i_sat / (C n_vt)) exp(u / n_vt)),  u = v_{k-1} + h i_sat / C"""
    v = [float(v0)]
    for _ in range(steps):
        u = v[-1] + h * i_sat / C
        v.append(u - n_vt * float(lambertw((h * i_sat / (C * n_vt)) * np.exp(u / n_vt)).real))
    return np.array(v)


# ---- the inputs of the GPU tests (tests/test_gpu_transient_diodes.py; tests/test_transient_nl_reference.py runs them) ----
def rectifier_case():
    """half-wave rectifier: E behind R, the diode in series, R || C as the load; E a sampled sine over 32 steps.  B = 1,
    n = 4: the dense panel.  Returns (rows, capacitors, inductors, diodes, dt, steps, sources)."""
    rows = nr.series_rows(0.0, 10.0) + [["rl", "R", "1000", "3", "g"]]
    steps, dt = 32, 1e-3
    wave = 5.0 * np.sin(2.0 * np.pi * np.arange(1, steps + 1) / steps)
    return rows, [("cl", 1e-4, "3", "g")], [], [("d1", I_SAT, N_VT, "2", "3")], dt, steps, {"e1": wave}


def _node_caps(rows, farads=1.0):
    import nodal_amd as n
    nl = n.Netlist.from_rows([list(r) for r in rows])
    return [(f"cn{k}", farads, node, "g") for k, node in enumerate(sorted(nl.nodenum, key=nl.nodenum.get))]


def lu_transient_case(with_inductors=False):
    """newton_reference.lu_case() (n = 145, B = 1: the sparse LU route) with 1 F from every node to ground, h = 0.05, 16
    steps, a1 swept in blocks of four between 1.5 and -2.0; with_inductors: 20 H between nodes 2 and 14 and 30 H from
    node 13 to ground, next to the swept source and large enough to hold their currents while it switches (tenths of a
    volt across them: an inductor lane run once too often shows)."""
    rows, diodes, _ = nr.lu_case()
    inductors = [("l1", 20.0, "2", "14"), ("l2", 30.0, "13", "g")] if with_inductors else []
    return rows, _node_caps(rows), inductors, diodes, 0.05, 16, {"a1": np.repeat([1.5, -2.0, 1.5, -2.0], 4)}


def mg_transient_case():
    """newton_reference.mg_case() (n = 4355, B = 0: the multigrid route) with 1 F on every node, h = 0.05, 8 steps; a0, a1,
    a3 go from their netlist values to -1.2, 0.9, -1.0 after step 4."""
    rows, diodes = nr.mg_case()
    now = {r[0]: float(r[2]) for r in rows if r[0] in ("a0", "a1", "a3")}
    then = {"a0": -1.2, "a1": 0.9, "a3": -1.0}
    sources = {name: np.array([now[name]] * 4 + [then[name]] * 4) for name in now}
    return rows, _node_caps(rows), [], diodes, 0.05, 8, sources


def reuse_case(size):
    """clamps at rest: grid(size) with a rail "vdd" held at 5 V by an E source (100 ohms from the rail into node 3), two
    switching loads of a few hundred mA, and clamp diodes from nodes up to the rail: the grid's potentials stay within a
    volt of ground, so every junction stays below -2 V (tests/test_transient_nl_reference.py asserts it of every
    linearisation point).  size 4: n = 17, the dense panel; size 12: n = 145, the sparse LU route."""
    last = size * size - 1
    mid = last // 2
    rows = nr.grid_rows(size, [("ld0", 0.2, mid), ("ld1", -0.1, last - 1)],
                        extra=[["e1", "E", "5", "vdd", "g"], ["rr", "R", "100", "vdd", "3"]])
    diodes = [(f"dz{k}", I_SAT, N_VT, str(k), "vdd") for k in (1, 2, mid, last - 1)] + [("dzg", I_SAT, N_VT, "g", "vdd")]
    sources = {"ld0": np.array([0.2, 0.4, 0.4, -0.3, -0.3, 0.1]), "ld1": np.array([-0.1, -0.1, 0.3, 0.3, -0.2, -0.2])}
    return rows, _node_caps(rows, 0.5), [], diodes, 0.05, 6, sources
