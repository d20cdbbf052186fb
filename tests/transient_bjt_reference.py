"""The numpy / scipy restatement the transient tests WITH BIPOLAR TRANSISTORS are measured against (never product code).

tests/transient_nl_reference.py's TransientDiodeReference whose Newton object is tests/transistor_reference.py's
TransistorReference on the companion matrix M: the junctions of every transistor are diodes behind the caller's own, and
step k solves, for x_k,

    M x_k + S i(S^T x_k) + P iT(S^T x_k) = base_k,    base_k = A_k + the capacitors' and the inductors' history currents

by Newton's method from vh^0 = S^T x_{k-1}: linearise the diodes AND the transports at vh^j, solve
(M + S diag(g) S^T + P (diag(gmf) E_f - diag(gmr) E_r) S^T) x = base_k + S J + P JT, limit the junctions, test; a step
has converged when no diode and no transport fails.  base_k is formed once per step, the inductor currents advance once
per step from the converged x_k, and a transport has no memory: P iT joins the nonlinear residual and |P| |iT| its scale.

`run` is the whole loop on the host with the defects tests/test_transient_bjt_reference.py plants: the three of
TransistorReference.one_step and "frozen", transports linearised at the step's FIRST vh in every iteration of the step
(a transport lane run once per step where it belongs into every iteration).
"""
import numpy as np
import scipy.sparse as sp

from tests import newton_reference as nr
from tests import transient_nl_reference as tn
from tests import transistor_reference as tref
from tests.newton_reference import I_SAT, N_VT, RESID_BAR, TIGHT, TOL, pnjlim  # noqa: F401
from tests.transient_nl_reference import TransientDiodeReference
from tests.transient_rl_reference import RLReference
from tests.transistor_reference import BETA_F, BETA_R, TransistorReference, npn, pnp  # noqa: F401

DEFECTS = ("JT_sign", "no_reverse_gm", "gm_rows_swapped", "frozen")


class TransientTransistorReference(TransientDiodeReference):
    """rows: the netlist; capacitors, inductors: (name, value, node_a, node_b); diodes: (name, i_sat, n_vt, anode,
    cathode); transistors: (name, kind, i_s, beta_f, beta_r, n_vt, collector, base, emitter); dt; method; the tolerances
    as Circuit.transient takes them."""

    def __init__(self, rows, capacitors, inductors, diodes, transistors, dt, method, gmin=1e-12, reltol=1e-3, vntol=1e-6,
                 abstol=1e-12, max_iter=50):
        self.rl = RLReference(rows, capacitors, inductors, dt, method)
        self.cap = self.rl.cap
        self.n, self.dt, self.method = self.rl.n, float(dt), method
        self.newton = TransistorReference(rows, diodes, transistors, gmin=gmin, reltol=reltol, vntol=vntol, abstol=abstol,
                                          max_iter=max_iter)
        self.G = self.newton.G  # the netlist's own matrix
        self.rl._companion()
        self.M = sp.csr_matrix(self.rl.G_full)
        self.newton.G = self.M  # (one_step then solves with M + S diag(g) S^T + the transports' block)
        self.gmin, self.reltol, self.vntol, self.abstol, self.max_iter = gmin, reltol, vntol, abstol, max_iter
        self.highest_junction = -np.inf
        self.most_iterations = 0
        self.unconverged = 0

    # -- the start ------------------------------------------------------------------------------------------------------
    def dc_start(self, x_guess=None):
        """the nonlinear DC operating point with capacitors open, inductors shorts (zero-volt E rows), diodes and
        transistors in, at the netlist's own source values: (x_0 [n], i_0 [L], Newton iterations).  S and P are padded
        with zero rows for the inductors' branch unknowns."""
        G, A = self.rl.dc_system()
        nw = self.newton
        dc = TransistorReference.__new__(TransistorReference)
        dc.__dict__.update(nw.__dict__)
        L = len(self.rl.g)
        dc.G, dc.A, dc.n = sp.csr_matrix(G), A, self.n + L
        dc.S = sp.vstack([nw.S, sp.csr_matrix((L, nw.S.shape[1]))], format="csr")
        dc.P = sp.vstack([nw.P, sp.csr_matrix((L, nw.P.shape[1]))], format="csr")
        r = dc.run(x_guess)
        assert r["converged"], "the reference's DC start did not converge"
        return r["x"][:self.n], -r["x"][self.n:], r["iterations"]

    # -- one step ---------------------------------------------------------------------------------------------------------
    def _frozen_step(self, vh_k, vh_t, both):
        """TransistorReference.one_step with the transports linearised at vh_t instead of vh_k (the planted defect)"""
        nw = self.newton
        g, i, J = nw.linearise(vh_k)
        iT, gmf, gmr = nw.transport(vh_t)
        vhf, vhr = vh_t[nw.jf], vh_t[nw.jr]
        JT = gmf * vhf - gmr * vhr - iT
        M = sp.csr_matrix(nw.matrix(g) + nw.transport_block(gmf, gmr))
        x = nw.solve(M, nw.A + nw.S @ J + nw.P @ JT, both=both)
        v = nw.voltages(x)
        vh, limited = pnjlim(v, vh_k, nw.n_vt, nw.v_crit)
        with np.errstate(all="ignore"):
            iv = nw.current(v)
            iTv, _, _ = nw.transport(v)
        ihat = i + g * (v - vh_k)
        ok = (np.abs(v - vh_k) <= nw.reltol * np.maximum(np.abs(v), np.abs(vh_k)) + nw.vntol) & \
             (np.abs(iv - ihat) <= nw.reltol * np.maximum(np.abs(iv), np.abs(ihat)) + nw.abstol)
        iThat = iT + gmf * (v[nw.jf] - vhf) - gmr * (v[nw.jr] - vhr)
        ok_t = np.abs(iTv - iThat) <= nw.reltol * np.maximum(np.abs(iTv), np.abs(iThat)) + nw.abstol
        return x, vh, {"limited": limited, "not_converged": ~ok, "transports_not_converged": ~ok_t, "v": v}

    def solve_step(self, x_prev, base, both=False, defect=None, rebase=None):
        """Newton's method on M x + S i(S^T x) + P iT(S^T x) = base from vh^0 = S^T x_prev: (x, iterations, converged);
        converged needs every diode AND every transport to pass"""
        assert rebase is None
        nw = self.newton
        nw.A = base
        x, vh = np.asarray(x_prev, dtype=np.float64), nw.voltages(x_prev)
        vh_first = vh
        for j in range(self.max_iter):
            self.highest_junction = max(self.highest_junction, float(vh.max(initial=-np.inf)))
            if defect == "frozen":
                x, vh, flags = self._frozen_step(vh, vh_first, both)
            else:
                x, vh, flags = nw.one_step(x, vh, both=both, defect=defect)
            if not flags["not_converged"].any() and not flags["transports_not_converged"].any():
                self.most_iterations = max(self.most_iterations, j + 1)
                return x, j + 1, True
        self.unconverged += 1
        return x, self.max_iter, False

    # -- the whole loop, and its planted defects --------------------------------------------------------------------------
    def run(self, x0, i0, A_steps, defect=None, both=False):
        """(X [steps + 1, n], I [steps + 1, L], Newton iterations [steps]); a factorisation that a planted defect makes
        singular raises (RuntimeError from SuperLU) or leaves NaN behind"""
        assert defect is None or defect in DEFECTS
        rl, cap = self.rl, self.cap
        X, I, Jc, its = [np.asarray(x0, dtype=np.float64)], [np.asarray(i0, dtype=np.float64).reshape(len(rl.g))], None, []
        for A_k in A_steps:
            Jc, JL = cap.history(X[-1], Jc), rl.history(X[-1], I[-1])
            x, it, _ = self.solve_step(X[-1], self.base(A_k, Jc, JL), both=both, defect=defect)
            X.append(x)
            I.append(-JL + rl.g * rl.voltages(x))
            its.append(it)
        return np.array(X), np.array(I).reshape(len(X), len(rl.g)), np.array(its)

    # -- the nonlinear residual of somebody else's solutions (parity is the parent's, through solve_step) -----------------
    def residual(self, X, i0, A_steps):
        """per step (max |r|, max scale): transient_nl_reference's defect with P iT added, and |P| |iT| to its scale"""
        rl, cap, nw, h = self.rl, self.cap, self.newton, self.dt
        states, I = self.rebuilt_states(X, i0)
        out = []
        if self.method == "euler":
            C, SL = cap.capacitance(), rl.incidence()
            i = np.asarray(i0, dtype=np.float64).reshape(len(rl.g))
            for k, A_k in enumerate(A_steps, start=1):
                x, xp = X[k], X[k - 1]
                i = i + (h / rl.henries) * (SL.T @ x)
                v = nw.voltages(x)
                idio, iT = nw.current(v), nw.transport(v)[0]
                r = self.G @ x + C @ (x - xp) / h + SL @ i + nw.S @ idio + nw.P @ iT - A_k
                scale = abs(self.G) @ np.abs(x) + abs(C) @ (np.abs(x) + np.abs(xp)) / h + abs(SL) @ np.abs(i) + \
                    abs(nw.S) @ np.abs(idio) + abs(nw.P) @ np.abs(iT) + np.abs(A_k)
                out.append((float(np.abs(r).max()), float(scale.max())))
            return out
        for k, (A_k, (Jc, JL, _)) in enumerate(zip(A_steps, states), start=1):
            x = X[k]
            v = nw.voltages(x)
            idio, iT, b = nw.current(v), nw.transport(v)[0], self.base(A_k, Jc, JL)
            r = self.M @ x + nw.S @ idio + nw.P @ iT - b
            scale = abs(self.M) @ np.abs(x) + abs(nw.S) @ np.abs(idio) + abs(nw.P) @ np.abs(iT) + np.abs(A_k) + \
                np.abs(cap.inject(Jc)) + np.abs(rl.inject(JL))
            out.append((float(np.abs(r).max()), float(scale.max())))
        return out

    # -- the transistors' outputs at somebody else's solution ---------------------------------------------------------------
    def junction_voltages(self, x):
        """[T, 2]: forward, reverse"""
        nw = self.newton
        v = nw.voltages(x)
        return np.stack([v[nw.jf], v[nw.jr]], axis=1)

    def terminal_currents(self, x):
        """(I_C, I_B, I_E) [T], positive into the terminal"""
        return self.newton.terminal_currents(x)


# ---- the inputs of the GPU tests (tests/test_gpu_transient_transistors.py; test_transient_bjt_reference.py runs them) ----
# every case: (rows, capacitors, inductors, diodes, transistors, dt, steps, sources)
def _e(name, volts, a, b="g"):
    return [name, "E", repr(float(volts)), str(a), str(b)]


def _r(name, ohms, a, b):
    return [name, "R", repr(float(ohms)), str(a), str(b)]


def inverter_case():
    """a resistor-loaded NPN inverter driven by a pulse, with load, Miller and base capacitors (n = 6: the dense
    panel).  The output goes from 5 V into saturation (0.07 V, the reverse junction at +0.63 V) and back."""
    rows = [_e("vcc", 5, 1), _e("ein", 0, "in"), _r("rb", 10e3, "in", 2), _r("rc", 1e3, 1, 3)]
    caps = [("cl", 1e-9, "3", "g"), ("cm", 1e-10, "2", "3"), ("cb", 1e-10, "2", "g")]
    return rows, caps, [], [], [npn("q1", 3, 2, "g")], 2e-6, 24, {"ein": np.repeat([0.0, 5.0, 0.0], 8)}


def pushpull_case():
    """a complementary emitter follower between +-5 V rails, driven by a sine through 100 ohms, into an inductor and
    R || C, with a clamp diode from the output to the positive rail (n = 10: the dense panel): a PNP, a diode and an
    inductor in one call"""
    rows = [_e("ep", 5, "p"), _e("em", -5, "m"), _e("ein", 0, "in"), _r("rs", 100, "in", "b"), _r("re", 1, "e", "x"),
            _r("rl", 100, "o", "g")]
    steps = 32
    wave = 3.0 * np.sin(2.0 * np.pi * np.arange(1, steps + 1) / steps)
    return (rows, [("cl", 1e-6, "o", "g")], [("l1", 1e-4, "x", "o")], [("dc", I_SAT, N_VT, "o", "p")],
            [npn("qn", "p", "b", "e"), pnp("qp", "m", "b", "e")], 1e-5, steps, {"ein": wave})


def lu_bjt_case(with_inductors=False):
    """transient_nl_reference.lu_transient_case with transistor_reference.lu_grid()'s five transistors (n = 145: the
    sparse LU route).  With the inductors the transistors barely conduct (v_f <= 0.53 V): the check of the inductor lane
    beside the transports on that route."""
    rows, caps, inds, diodes, dt, steps, sources = tn.lu_transient_case(with_inductors)
    return rows, caps, inds, diodes, tref.lu_grid()[2], dt, steps, sources


def lu_inverter_case(with_inductors=False):
    """lu_bjt_case plus inverter_case's inverter on nodes of its own ("vcc", "in", "qb", "qc") and a sixth transistor
    (n = 151: the sparse LU route): it saturates, with diodes and transistors in one call.  The 1 F node capacitors
    stand on the grid's nodes only; the inverter's are scaled to the step of 0.05."""
    rows, caps, inds, diodes, transistors, dt, steps, sources = lu_bjt_case(with_inductors)
    rows = rows + [_e("vcc", 5, "vcc"), _e("ein", 0, "in"), _r("rb", 10e3, "in", "qb"), _r("rc", 1e3, "vcc", "qc")]
    caps = caps + [("cl", 2.5e-5, "qc", "g"), ("cm", 2.5e-6, "qb", "qc"), ("cb", 2.5e-6, "qb", "g")]
    sources = dict(sources, ein=np.repeat([0.0, 5.0, 0.0], [4, 6, 6]))
    return rows, caps, inds, diodes, transistors + [npn("q6", "qc", "qb", "g")], dt, steps, sources


CASES = {"inverter": inverter_case, "pushpull": pushpull_case, "lu_bjt": lambda: lu_bjt_case(False),
         "lu_bjt_l": lambda: lu_bjt_case(True), "lu_inverter": lambda: lu_inverter_case(False),
         "lu_inverter_l": lambda: lu_inverter_case(True)}
SIZES = {"inverter": 6, "pushpull": 10, "lu_bjt": 145, "lu_bjt_l": 145, "lu_inverter": 151, "lu_inverter_l": 151}


def diode_connected_closed_form(v0, C, h, steps):
    """rc_diode_rows(), a capacitor from node 1 to ground and an NPN with collector and base on node 1, the emitter
    grounded, gmin = 0: the reverse junction sits at exactly 0 V and carries nothing, the forward junction i_s / beta_f
    and the transport i_s, so the node sees one diode with i_sat = i_s (1 + 1 / beta_f)"""
    return tn.rc_diode_closed_form(v0, C, I_SAT * (1.0 + 1.0 / BETA_F), N_VT, h, steps)
