"""The numpy / scipy restatement every operating-point test is measured against (never product code).

Written from the formulas of the diode model alone; G and A come from the oracle's build_model (a change of source values
is a netlist with other value strings, built again).  A diode (name, i_sat, n_vt, anode, cathode) carries

    i(v) = i_sat (exp(v / n_vt) - 1) + gmin v,   v = x(anode) - x(cathode)

from anode to cathode.  One Newton step from (x_k, vh_k), vh the limited junction voltages:

    e = exp(vh / n_vt),  g = i_sat e / n_vt + gmin,  i = i_sat (e - 1) + gmin vh,  J = g vh - i
    (G + S diag(g) S^T) x_{k+1} = A + S J                       S: the incidence of the diodes, ground dropped
    v = S^T x_{k+1},  v_crit = n_vt ln(n_vt / (sqrt(2) i_sat))
    limited = v > v_crit and |v - vh| > 2 n_vt
        vh > 0:   a = 1 + (v - vh) / n_vt,  vh' = vh + n_vt ln a if a > 0 else v_crit
        vh <= 0:  vh' = n_vt ln(v / n_vt)
    else vh' = v
    converged(d) = |v - vh| <= reltol max(|v|, |vh|) + vntol  and
                   |i(v) - ihat| <= reltol max(|i(v)|, |ihat|) + abstol,   ihat = i + g (v - vh)

Each step can be solved twice, by LAPACK on the dense matrix and by SuperLU with one step of refinement; on the inputs of
the GPU tests the two agree to a few 1e-16 of the largest unknown (tests/test_newton_reference.py asserts TOL / 1000), so
the project's normwise bar TOL = 1e-9 leaves six decades for the device.
"""
import random

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import nodal_amd as n
from oracle import nodal_oracle as oracle
from tests.sensitivity_reference import TOL  # noqa: F401  (the project's bar for solutions, normwise)

RESID_BAR = 1e-12  # the transient tests' bar for the scaled residual of one solve
TIGHT = dict(reltol=1e-10, vntol=1e-13, abstol=1e-16)
SQRT2 = float(np.sqrt(2.0))


def _index(nl, label):
    if label == nl.ground or str(label) == str(nl.ground):
        return -1
    return int(nl.nodenum[label] if label in nl.nodenum else nl.nodenum[str(label)])


def _flat(A):
    return np.asarray(A.todense() if sp.issparse(A) else A, dtype=np.float64).ravel()


def diode_current(v, i_sat, n_vt, gmin):
    return i_sat * (np.exp(v / n_vt) - 1.0) + gmin * v


def diode_conductance(v, i_sat, n_vt, gmin):
    return i_sat * np.exp(v / n_vt) / n_vt + gmin


def pnjlim(v, vh, n_vt, v_crit):
    """(vh', limited) elementwise"""
    v, vh = np.asarray(v, dtype=np.float64), np.asarray(vh, dtype=np.float64)
    limited = (v > v_crit) & (np.abs(v - vh) > 2.0 * n_vt)
    out = v.copy()
    with np.errstate(all="ignore"):
        a = 1.0 + (v - vh) / n_vt
        forward = np.where(a > 0.0, vh + n_vt * np.log(np.where(a > 0.0, a, 1.0)), v_crit)
        cold = n_vt * np.log(v / n_vt)
    pick = np.where(vh > 0.0, forward, cold)
    out[limited] = pick[limited]
    return out, limited


class NewtonReference:
    """rows: the netlist; diodes: (name, i_sat, n_vt, anode, cathode); sources: name -> value in force (None: the
    netlist's); tolerances as Circuit.operating_point takes them."""

    def __init__(self, rows, diodes, gmin=1e-12, reltol=1e-3, vntol=1e-6, abstol=1e-12, sources=None, max_iter=100):
        self.rows = [list(r) for r in rows]
        if sources:
            self.rows = [[r[0], r[1], repr(float(sources[r[0]])), *r[3:]] if r[0] in sources else r for r in self.rows]
        self.nl = n.Netlist.from_rows([list(r) for r in self.rows])
        G, A, _ = oracle.build_model(self.nl, True)
        self.G = sp.csr_matrix(G)
        self.A = _flat(A)
        self.n = self.G.shape[0]
        self.gmin, self.reltol, self.vntol, self.abstol, self.max_iter = gmin, reltol, vntol, abstol, max_iter
        D = len(diodes)
        self.names = [d[0] for d in diodes]
        self.i_sat = np.array([float(d[1]) for d in diodes], dtype=np.float64).reshape(D)
        self.n_vt = np.array([float(d[2]) for d in diodes], dtype=np.float64).reshape(D)
        self.ia = np.array([_index(self.nl, d[3]) for d in diodes], dtype=np.int64).reshape(D)
        self.ib = np.array([_index(self.nl, d[4]) for d in diodes], dtype=np.int64).reshape(D)
        self.v_crit = self.n_vt * np.log(self.n_vt / (SQRT2 * self.i_sat))
        S = sp.lil_matrix((self.n + 1, D))
        for d in range(D):  # (index -1, the ground lead, falls on the row that is dropped)
            S[self.ia[d], d] += 1.0
            S[self.ib[d], d] -= 1.0
        self.S = sp.csr_matrix(S)[:self.n, :]
        self.worst_disagreement = 0.0  # of the two solves, normwise, over every step taken with both=True

    # -- the model ---------------------------------------------------------------------------------------------------
    def voltages(self, x):
        return self.S.T @ np.asarray(x, dtype=np.float64)

    def current(self, v):
        return diode_current(v, self.i_sat, self.n_vt, self.gmin)

    def conductance(self, v):
        return diode_conductance(v, self.i_sat, self.n_vt, self.gmin)

    def linearise(self, vh):
        """(g, i, J) at vh"""
        e = np.exp(vh / self.n_vt)
        g = self.i_sat * e / self.n_vt + self.gmin
        i = self.i_sat * (e - 1.0) + self.gmin * vh
        return g, i, g * vh - i

    def matrix(self, g):
        return sp.csr_matrix(self.G + self.S @ sp.diags(g) @ self.S.T)

    def jacobian(self, x):
        return self.matrix(self.conductance(self.voltages(x)))

    # -- one step --------------------------------------------------------------------------------------------------------
    def solve(self, M, b, both=False):
        """SuperLU with one step of refinement; both=True: LAPACK on the dense matrix as well, the disagreement filed"""
        lu = spla.splu(sp.csc_matrix(M))
        x = lu.solve(b)
        x = x + lu.solve(b - M @ x)
        if both:
            xd = np.linalg.solve(M.toarray(), b)
            scale = max(np.abs(x).max(), np.abs(xd).max(), np.finfo(float).tiny)
            self.worst_disagreement = max(self.worst_disagreement, float(np.abs(x - xd).max() / scale))
        return x

    def one_step(self, x_k, vh_k, both=False, defect=None):
        """(x_{k+1}, vh_{k+1}, flags) from (x_k, vh_k); only vh_k enters (x_k is the iterate it was limited from).
        flags: limited, not_converged [D] bool, v the raw voltages, margin [D] the distance of v from the nearest
        threshold of the limiter.  defect plants a mistake: "J_sign", "no_limiting", "g_without_gmin"."""
        vh_k = np.asarray(vh_k, dtype=np.float64)
        g, i, J = self.linearise(vh_k)
        if defect == "J_sign":
            J = -J
        if defect == "g_without_gmin":
            g = g - self.gmin
        x = self.solve(self.matrix(g), self.A + self.S @ J, both=both)
        v = self.voltages(x)
        vh, limited = pnjlim(v, vh_k, self.n_vt, self.v_crit)
        if defect == "no_limiting":
            vh, limited = v.copy(), np.zeros(len(v), dtype=bool)
        with np.errstate(all="ignore"):
            iv = self.current(v)
        ihat = i + g * (v - vh_k)
        ok = (np.abs(v - vh_k) <= self.reltol * np.maximum(np.abs(v), np.abs(vh_k)) + self.vntol) & \
             (np.abs(iv - ihat) <= self.reltol * np.maximum(np.abs(iv), np.abs(ihat)) + self.abstol)
        margin = np.minimum(np.abs(v - self.v_crit), np.abs(np.abs(v - vh_k) - 2.0 * self.n_vt))
        return x, vh, {"limited": limited, "not_converged": ~ok, "v": v, "margin": margin}

    def run(self, x0=None, both=False):
        """the full iteration: dict(x, iterates [r, n], vh [r + 1, D], limited, not_converged [r], converged, iterations)"""
        x = np.zeros(self.n) if x0 is None else np.asarray(x0, dtype=np.float64)
        vh = self.voltages(x)
        X, VH, lim, bad, margins = [], [vh], [], [], []
        converged = False
        for _ in range(self.max_iter):
            x, vh, flags = self.one_step(x, vh, both=both)
            X.append(x)
            VH.append(vh)
            lim.append(int(flags["limited"].sum()))
            bad.append(int(flags["not_converged"].sum()))
            margins.append(flags["margin"])
            if bad[-1] == 0:
                converged = True
                break
        return {"x": x, "iterates": np.array(X), "vh": np.array(VH), "limited": lim, "not_converged": bad,
                "converged": converged, "iterations": len(X), "margins": np.array(margins)}

    # -- at an answer ----------------------------------------------------------------------------------------------------
    def residual(self, x):
        """(r, scale): the nonlinear KCL defect G x - A + S i(S^T x) per row and its scale |G||x| + |A| + |S||i|"""
        x = np.asarray(x, dtype=np.float64)
        i = self.current(self.voltages(x))
        r = self.G @ x - self.A + self.S @ i
        scale = abs(self.G) @ np.abs(x) + np.abs(self.A) + abs(self.S) @ np.abs(i)
        return r, scale


# ---- closed forms -------------------------------------------------------------------------------------------------------
def source_diode_rows(I):
    """a current source I into node 1 (the diode from node 1 to ground is the only other element)"""
    return [["a1", "A", repr(float(I)), "1", "g"]]


def source_diode_closed_form(I, i_sat, n_vt):
    """gmin = 0: I = i_sat (exp(v / n_vt) - 1)"""
    return n_vt * np.log1p(I / i_sat)


def series_rows(E, R):
    """E from ground to node 1, R from node 1 to node 2 (the diode from node 2 to ground closes the loop): B = 1"""
    return [["e1", "E", repr(float(E)), "1", "g"], ["r1", "R", repr(float(R)), "1", "2"]]


def series_closed_form(E, R, i_sat, n_vt):
    """gmin = 0: the root of (E - v) / R = i_sat (exp(v / n_vt) - 1), by bisection and a few Newton steps in long
    double -- an independent route to the same number"""
    f = lambda v: (E - v) / R - i_sat * np.expm1(v / n_vt)  # noqa: E731
    lo, hi = 0.0, float(E)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if f(mid) > 0.0:
            lo = mid
        else:
            hi = mid
    v = np.longdouble(0.5 * (lo + hi))
    for _ in range(3):
        fv = (np.longdouble(E) - v) / R - i_sat * np.expm1(v / np.longdouble(n_vt))
        v = v - fv / (-1.0 / np.longdouble(R) - i_sat / np.longdouble(n_vt) * np.exp(v / np.longdouble(n_vt)))
    return float(v)


# ---- the inputs of the GPU tests (tests/test_gpu_operating_point.py; tests/test_newton_reference.py runs them too) ----
I_SAT, N_VT = 1e-14, 0.02585


def grid_rows(N, sources, extra=()):
    """grid(N) with unit resistors, `sources`: (name, amperes, node) current sources into nodes, and `extra` rows"""
    last = N * N - 1
    label = lambda k: "g" if k == last else str(k + 1)  # noqa: E731
    rows = []
    for r in range(N):
        for col in range(N):
            k = r * N + col
            if col + 1 < N:
                rows.append([f"rh{r}_{col}", "R", "1", label(k), label(k + 1)])
            if r + 1 < N:
                rows.append([f"rv{r}_{col}", "R", "1", label(k), label(k + N)])
    rows += [list(row) for row in extra]
    rows += [[name, "A", repr(float(amps)), str(node), "g"] for name, amps, node in sources]
    return rows


def lu_case():
    """grid(12) (n = 143 potentials) and one E source behind a resistor, B = 1, with thirteen diodes: forward and
    reverse to ground, an anti-parallel pair, between two nodes, on the E source's node, one with both leads on a node.
    Returns (rows, diodes, initial): `initial` puts the diode on node 30 at 1.2 V, eighteen n_vt above its v_crit of 0.73 V
    (Newton comes down from there by about one n_vt per iteration)."""
    rows = grid_rows(12, [("a1", 0.5, 1), ("a2", -0.3, 77)],
                     extra=[["e1", "E", "3", "src", "g"], ["rs", "R", "2", "src", "40"]])
    rng = random.Random(12)
    diodes = [("d_fwd", I_SAT, N_VT, "1", "g"), ("d_rev", I_SAT, N_VT, "g", "2"),
              ("d_ap1", 2e-14, 0.03, "14", "15"), ("d_ap2", 2e-14, 0.03, "15", "14"),
              ("d_mid", 1e-12, 0.04, "40", "52"), ("d_src", I_SAT, N_VT, "g", "src"),
              ("d_same", I_SAT, N_VT, "60", "60"), ("d_hard", I_SAT, N_VT, "30", "g"),
              ("d_neg", 1e-13, N_VT, "g", "77")]
    for j in range(4):
        a, b = rng.sample(range(1, 143), 2)
        diodes.append((f"d_r{j}", I_SAT * 10 ** rng.uniform(0, 3), N_VT * rng.uniform(1.0, 2.0), str(a), str(b)))
    nl = n.Netlist.from_rows([list(r) for r in rows])
    initial = np.zeros(len(nl.nodenum) + len(nl.anomnum))
    initial[_index(nl, "30")] = 1.2
    return rows, diodes, initial


def mg_case():
    """grid(66) (n = 4355 > 4096, B = 0) with six current sources and fifty seeded diodes to ground and between
    neighbours.  Returns (rows, diodes)."""
    N = 66
    rng = random.Random(66)
    nodes = rng.sample(range(1, N * N - 1), 6)
    rows = grid_rows(N, [(f"a{j}", amps, node) for j, (amps, node) in
                         enumerate(zip((0.8, -0.6, 0.4, 1.0, -0.9, 0.7), nodes))])
    diodes = []
    for j in range(50):
        k = rng.randrange(1, N * N - 2)
        sat, nvt = I_SAT * 10 ** rng.uniform(0, 2), N_VT * rng.uniform(1.0, 1.5)
        if j < 6:  # (one on every source node, forward for a source that pushes and for one that pulls)
            diodes.append((f"d{j}", sat, nvt, str(nodes[j]), "g") if j % 2 == 0 else (f"d{j}", sat, nvt, "g", str(nodes[j])))
        elif rng.random() < 0.5:
            diodes.append((f"d{j}", sat, nvt, str(k), "g") if rng.random() < 0.5 else (f"d{j}", sat, nvt, "g", str(k)))
        else:
            step = 1 if k % N != 0 else N  # (k and k + 1 are neighbours unless k ends a row; k + N is the node below)
            other = k + step if k + step < N * N else k - N
            diodes.append((f"d{j}", sat, nvt, str(k), str(other)))
    return rows, diodes
