"""The numpy / scipy restatement the operating point with bipolar transistors is measured against (never product code).

Written from the formulas of the model alone, on top of tests/newton_reference.py's NewtonReference.  A transistor
(name, "npn" | "pnp", i_s, beta_f, beta_r, n_vt, collector, base, emitter) is, in the transport form of Ebers-Moll,

    junction f:  a diode with i_sat = i_s / beta_f,  NPN base -> emitter,    PNP emitter -> base
    junction r:  a diode with i_sat = i_s / beta_r,  NPN base -> collector,  PNP collector -> base
    transport:   i_T = i_s (exp(v_f / n_f) - exp(v_r / n_r))  through the element from lead a to lead b,
                 NPN a = collector, b = emitter;  PNP a = emitter, b = collector

The junctions are diodes of the parent class behind the caller's own (limiting, gmin and test included); the transport
has no gmin, no limiting and no state.  One Newton step from (x_k, vh_k), vhf = vh[jf], vhr = vh[jr]:

    ef = exp(vhf / n_f),  er = exp(vhr / n_r),  gmf = i_s ef / n_f,  gmr = i_s er / n_r,  iT = i_s ef - i_s er
    JT = gmf vhf - gmr vhr - iT
    (G + S diag(g) S^T + P (diag(gmf) E_f - diag(gmr) E_r) S^T) x_{k+1} = A + S J + P JT

P the transports' incidence (+1 at a, -1 at b, ground dropped), E_f / E_r the [T, D] selections of the junctions.  After
the solve, with the raw vf, vr of x_{k+1}:

    iT(v) = i_s exp(vf / n_f) - i_s exp(vr / n_r),  ihat = iT + gmf (vf - vhf) - gmr (vr - vhr)
    converged(t) = |iT(v) - ihat| <= reltol max(|iT(v)|, |ihat|) + abstol

and the loop has converged when no diode and no transport fails.  Terminal currents, positive INTO the terminal, of an
NPN: I_C = iT - i_r, I_B = i_f + i_r, I_E = -(iT + i_f); a PNP's are those negated.
"""
import numpy as np
import scipy.sparse as sp

from tests import newton_reference as nr
from tests.newton_reference import I_SAT, N_VT, NewtonReference, _index, pnjlim

BETA_F, BETA_R = 100.0, 1.0


def npn(name, collector, base, emitter, i_s=I_SAT, n_vt=N_VT):
    return (name, "npn", i_s, BETA_F, BETA_R, n_vt, str(collector), str(base), str(emitter))


def pnp(name, collector, base, emitter, i_s=I_SAT, n_vt=N_VT):
    return (name, "pnp", i_s, BETA_F, BETA_R, n_vt, str(collector), str(base), str(emitter))


class TransistorReference(NewtonReference):
    """rows, diodes and the tolerances as NewtonReference takes them; transistors as above.  The junction diodes stand
    behind the caller's D0 diodes: junction f of transistor t is diode D0 + 2 t, junction r diode D0 + 2 t + 1."""

    def __init__(self, rows, diodes, transistors, **kwargs):
        diodes = list(diodes)
        self.D0, self.T = len(diodes), len(transistors)
        junctions, leads, sign = [], [], []
        for name, kind, i_s, bf, br, n_vt, col, base, emit in transistors:
            if kind == "npn":
                junctions += [(name + ".be", i_s / bf, n_vt, base, emit), (name + ".bc", i_s / br, n_vt, base, col)]
                leads.append((col, emit))
                sign.append(1.0)
            else:
                assert kind == "pnp"
                junctions += [(name + ".eb", i_s / bf, n_vt, emit, base), (name + ".cb", i_s / br, n_vt, col, base)]
                leads.append((emit, col))
                sign.append(-1.0)
        super().__init__(rows, diodes + junctions, **kwargs)
        T = self.T
        self.transistor_names = [t[0] for t in transistors]
        self.sign = np.array(sign, dtype=np.float64).reshape(T)
        self.i_s = np.array([float(t[2]) for t in transistors], dtype=np.float64).reshape(T)
        self.jf = self.D0 + 2 * np.arange(T, dtype=np.int64)
        self.jr = self.jf + 1
        self.n_f, self.n_r = self.n_vt[self.jf], self.n_vt[self.jr]
        self.ta = np.array([_index(self.nl, a) for a, _ in leads], dtype=np.int64).reshape(T)
        self.tb = np.array([_index(self.nl, b) for _, b in leads], dtype=np.int64).reshape(T)
        P = sp.lil_matrix((self.n + 1, T))
        for t in range(T):  # (index -1, the ground lead, falls on the row that is dropped)
            P[self.ta[t], t] += 1.0
            P[self.tb[t], t] -= 1.0
        self.P = sp.csr_matrix(P)[:self.n, :]
        D = len(self.i_sat)
        self.E_f = sp.csr_matrix((np.ones(T), (np.arange(T), self.jf)), shape=(T, D))
        self.E_r = sp.csr_matrix((np.ones(T), (np.arange(T), self.jr)), shape=(T, D))

    # -- the transport ---------------------------------------------------------------------------------------------------
    def transport(self, v):
        """(iT, gmf, gmr) at the junction voltages v [D]"""
        with np.errstate(over="ignore", invalid="ignore"):
            ef, er = np.exp(v[self.jf] / self.n_f), np.exp(v[self.jr] / self.n_r)
            return self.i_s * ef - self.i_s * er, self.i_s * ef / self.n_f, self.i_s * er / self.n_r

    def transport_block(self, gmf, gmr, swapped=False):
        E_f, E_r = (self.E_r, self.E_f) if swapped else (self.E_f, self.E_r)
        return self.P @ (sp.diags(gmf) @ E_f - sp.diags(gmr) @ E_r) @ self.S.T

    def jacobian(self, x):
        v = self.voltages(x)
        _, gmf, gmr = self.transport(v)
        return sp.csr_matrix(self.matrix(self.conductance(v)) + self.transport_block(gmf, gmr))

    def terminal_currents(self, x):
        """(I_C, I_B, I_E) [T], positive into the terminal"""
        v = self.voltages(x)
        i = self.current(v)
        iT, _, _ = self.transport(v)
        i_f, i_r = i[self.jf], i[self.jr]
        return self.sign * (iT - i_r), self.sign * (i_f + i_r), -self.sign * (iT + i_f)

    # -- one step --------------------------------------------------------------------------------------------------------
    def one_step(self, x_k, vh_k, both=False, defect=None):
        """NewtonReference.one_step with the transports; flags gain transports_not_converged [T].  defect plants a
        mistake: "JT_sign", "no_reverse_gm" (the reverse GM row stamps nothing), "gm_rows_swapped" (each GM row reads
        the other junction)."""
        vh_k = np.asarray(vh_k, dtype=np.float64)
        g, i, J = self.linearise(vh_k)
        iT, gmf, gmr = self.transport(vh_k)
        vhf, vhr = vh_k[self.jf], vh_k[self.jr]
        JT = gmf * vhf - gmr * vhr - iT
        if defect == "JT_sign":
            JT = -JT
        stamped_gmr = np.zeros_like(gmr) if defect == "no_reverse_gm" else gmr
        M = sp.csr_matrix(self.matrix(g) + self.transport_block(gmf, stamped_gmr, swapped=defect == "gm_rows_swapped"))
        x = self.solve(M, self.A + self.S @ J + self.P @ JT, both=both)
        v = self.voltages(x)
        vh, limited = pnjlim(v, vh_k, self.n_vt, self.v_crit)
        with np.errstate(all="ignore"):
            iv = self.current(v)
            iTv, _, _ = self.transport(v)
        ihat = i + g * (v - vh_k)
        ok = (np.abs(v - vh_k) <= self.reltol * np.maximum(np.abs(v), np.abs(vh_k)) + self.vntol) & \
             (np.abs(iv - ihat) <= self.reltol * np.maximum(np.abs(iv), np.abs(ihat)) + self.abstol)
        iThat = iT + gmf * (v[self.jf] - vhf) - gmr * (v[self.jr] - vhr)
        ok_t = np.abs(iTv - iThat) <= self.reltol * np.maximum(np.abs(iTv), np.abs(iThat)) + self.abstol
        margin = np.minimum(np.abs(v - self.v_crit), np.abs(np.abs(v - vh_k) - 2.0 * self.n_vt))
        return x, vh, {"limited": limited, "not_converged": ~ok, "transports_not_converged": ~ok_t, "v": v, "margin": margin}

    def run(self, x0=None, both=False):
        """NewtonReference.run's dict with transports_not_converged [r]; converged: no diode and no transport failed"""
        x = np.zeros(self.n) if x0 is None else np.asarray(x0, dtype=np.float64)
        vh = self.voltages(x)
        X, VH, lim, bad, tbad, margins = [], [vh], [], [], [], []
        converged = False
        for _ in range(self.max_iter):
            x, vh, flags = self.one_step(x, vh, both=both)
            X.append(x)
            VH.append(vh)
            lim.append(int(flags["limited"].sum()))
            bad.append(int(flags["not_converged"].sum()))
            tbad.append(int(flags["transports_not_converged"].sum()))
            margins.append(flags["margin"])
            if bad[-1] == 0 and tbad[-1] == 0:
                converged = True
                break
        return {"x": x, "iterates": np.array(X), "vh": np.array(VH), "limited": lim, "not_converged": bad,
                "transports_not_converged": tbad, "converged": converged, "iterations": len(X), "margins": np.array(margins)}

    # -- at an answer ----------------------------------------------------------------------------------------------------
    def residual(self, x):
        """(r, scale): the nonlinear KCL defect G x - A + S i + P i_T per row and its scale |G||x| + |A| + |S||i| +
        |P||i_T|"""
        x = np.asarray(x, dtype=np.float64)
        v = self.voltages(x)
        i = self.current(v)
        iT, _, _ = self.transport(v)
        r = self.G @ x - self.A + self.S @ i + self.P @ iT
        scale = abs(self.G) @ np.abs(x) + np.abs(self.A) + abs(self.S) @ np.abs(i) + abs(self.P) @ np.abs(iT)
        return r, scale


def parity_errors(ref, X, VH, x0):
    """tests/test_newton_reference.py's one-step parity with the transports' count: the reference advances somebody's
    (x_k, vh_k) by one step and is compared with that somebody's x_{k+1}, vh_{k+1}.  Returns (worst x error /
    |x_{k+1}|_inf, worst vh error / max(|x_{k+1}|_inf, |vh_{k+1}|_inf), comparisons left out, comparisons, per iterate
    (diodes not converged, limited, left out, transports not converged) of the reference): a diode whose raw v lies
    within 4 TOL |x|_inf of a limiter threshold is left out of the vh comparison and of the counts."""
    ex = ev = 0.0
    left = total = 0
    counts = []
    for k in range(len(X)):
        x, vh, flags = ref.one_step(None, VH[k])
        xs = np.abs(X[k]).max()
        ex = max(ex, np.abs(x - X[k]).max() / xs)
        decidable = flags["margin"] > 4 * nr.TOL * xs
        left += int((~decidable).sum())
        total += len(decidable)
        if decidable.any():
            scale = max(xs, np.abs(VH[k + 1]).max())
            ev = max(ev, np.abs(vh - VH[k + 1])[decidable].max() / scale)
        counts.append((int(flags["not_converged"].sum()), int(flags["limited"].sum()), int((~decidable).sum()),
                       int(flags["transports_not_converged"].sum())))
    return ex, ev, left, total, counts


# ---- the inputs of the GPU tests (tests/test_gpu_transistors.py; tests/test_transistor_reference.py runs them too) ------
def _e(name, volts, node):
    return [name, "E", repr(float(volts)), str(node), "g"]


def _r(name, ohms, a, b):
    return [name, "R", repr(float(ohms)), str(a), str(b)]


def ce_amp():
    """a common-emitter stage with a divider at the base and emitter degeneration: forward active (n = 5)"""
    rows = [_e("e1", 10, 1), _r("r1", 47e3, 1, 2), _r("r2", 10e3, 2, "g"), _r("rc", 4.7e3, 1, 3), _r("re", 1e3, 4, "g")]
    return rows, [], [npn("q1", 3, 2, 4)]


def switch_sat():
    """a saturated switch: both junctions forward (n = 4)"""
    rows = [_e("e1", 5, 1), _r("rb", 1e3, 1, 2), _r("rc", 1e3, 1, 3)]
    return rows, [], [npn("q1", 3, 2, "g")]


def reverse_active():
    """collector and emitter exchanged: the reverse GM row carries the current (n = 4)"""
    rows = [_e("e1", 5, 1), _r("rb", 10e3, 1, 2), _r("rc", 1e3, 1, 3)]
    return rows, [], [npn("q1", "g", 2, 3)]


def mirror():
    """a current mirror: the first transistor has its collector tied to its base (n = 4)"""
    rows = [_e("e1", 5, 1), _r("r1", 4.3e3, 1, 2), _r("r2", 1e3, 1, 3)]
    return rows, [], [npn("q1", 2, 2, "g"), npn("q2", 3, 2, "g")]


def pnp_follower():
    """a PNP emitter follower (n = 5)"""
    rows = [_e("e1", 5, 1), _e("e2", 2, 2), _r("r1", 1e3, 1, 3)]
    return rows, [], [pnp("q1", "g", 2, 3)]


def diff_pair():
    """a differential pair with 10 mV between the bases and a resistor as its tail (n = 11)"""
    rows = [_e("e1", 10, 1), _e("e2", -10, 9), _e("e3", 0.01, 2), _e("e4", 0, 3), _r("r1", 5e3, 1, 4), _r("r2", 5e3, 1, 5),
            _r("rt", 9.3e3, 6, 9)]
    return rows, [], [npn("q1", 4, 2, 6), npn("q2", 5, 3, 6)]


def lu_grid():
    """newton_reference's lu_case() -- grid(12) + E with its thirteen diodes -- and five transistors: to ground, between
    three nodes, a PNP, a diode-connected one and one with every lead on one node (n = 145 > 64: the sparse LU route)"""
    rows, diodes, _ = nr.lu_case()
    transistors = [npn("q1", 5, 17, "g"), npn("q2", 40, 41, 42), pnp("q3", 100, 88, "g"), npn("q4", 60, 60, "g"),
                   npn("q5", 77, 77, 77)]
    return rows, diodes, transistors


CASES = {"ce_amp": ce_amp, "switch_sat": switch_sat, "reverse_active": reverse_active, "mirror": mirror,
         "pnp_follower": pnp_follower, "diff_pair": diff_pair, "lu_grid": lu_grid}
SIZES = {"ce_amp": 5, "switch_sat": 4, "reverse_active": 4, "mirror": 4, "pnp_follower": 5, "diff_pair": 11, "lu_grid": 145}


def diode_connected(amps):
    """a current source into node 1 and an NPN with collector and base on it, the emitter grounded: with gmin = 0 the
    closed form is newton_reference.source_diode_closed_form(amps, i_s (1 + 1 / beta_f), n_vt)"""
    return nr.source_diode_rows(amps), [], [npn("q1", 1, 1, "g")]


def diode_connected_closed_form(amps):
    return nr.source_diode_closed_form(amps, I_SAT * (1.0 + 1.0 / BETA_F), N_VT)
