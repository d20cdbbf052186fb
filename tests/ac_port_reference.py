"""The numpy / scipy restatement the AC port tests are measured against (never product code).

Built on tests/ac_reference.ACReference: G from the oracle's model of the netlist, B(w) by incidence.  Port q is the
ordered pair of node indices (a_q, b_q), -1 the ground node; S [n, P] has +1 at a_q and -1 at b_q of column q (ground
dropped, zeros in the branch rows).  Per frequency G + j B is factored ONCE with scipy, the P unit injections are solved
with one step of refinement, and the P solutions X [n, P] and Z = S^T X are returned -- in both formulations of
ac_reference.py, complex and interleaved real.

Measured on the CPU with the seeds below: the two agree to 4.9e-16 of max|Z| per frequency on grid(12) with 33 ports over
17 frequencies (reciprocity 3.3e-16) and to 2.7e-15 on 28 of the 29 inputs of the branches suite; on the remaining one
(edge/ccvs_ctrl_on_leads) every port voltage vanishes identically and only a 1 A branch current is left in the solutions,
which is why every bar here scales by the largest unknown of the P solutions of a frequency and not by max|Z|."""
import math
import random

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests.ac_reference import ROTATE, TOL, ACReference, _index  # noqa: F401

INPUT_FREQS = [0.01, 0.3, 10.0]
GRID_FREQS = np.logspace(-4, 4, 17)


def node_labels(nl):
    return sorted(nl.nodenum, key=nl.nodenum.get)


def seeded_ports(nl, count, seed):
    """`count` ports (a, b) as labels: a among the nodes, b among the nodes and ground, a drawn before b"""
    labels = node_labels(nl)
    K = len(labels)
    rng = random.Random(seed)
    pairs = []
    for _ in range(count):
        a = rng.randrange(K)
        b = rng.randrange(-1, K)
        pairs.append((labels[a], nl.ground if b < 0 else labels[b]))
    return pairs


def _refined_block(M):
    """X = M^-1 B for a block of right-hand sides by ONE sparse LU and one step of refinement"""
    lu, Mr = spla.splu(sp.csc_matrix(M)), sp.csr_matrix(M)

    def solve(B):
        X = lu.solve(B)
        return X + lu.solve(B - Mr @ X)
    return solve


class ACPortReference:
    """r: an ACReference; ports: (node_plus, node_minus) labels or single labels against ground."""

    def __init__(self, r, ports):
        self.r, self.n, self.K = r, r.n, r.K
        pairs = [tuple(p) if isinstance(p, (tuple, list)) else (p, r.nl.ground) for p in ports]
        self.ports = pairs
        self.ia = np.array([_index(r.nl, a) for a, _ in pairs], dtype=np.int64).reshape(len(pairs))
        self.ib = np.array([_index(r.nl, b) for _, b in pairs], dtype=np.int64).reshape(len(pairs))
        S = np.zeros((self.n + 1, len(pairs)))
        for q, (a, b) in enumerate(zip(self.ia, self.ib)):  # (index -1, the ground lead, falls on the row that is dropped)
            S[a, q] += 1.0
            S[b, q] -= 1.0
        self.S = S[:self.n]

    def solutions(self, f, method="complex"):
        """X [n, P] complex at the frequency f (Hz)"""
        omega = 2.0 * math.pi * float(f)
        if not len(self.ports):
            return np.zeros((self.n, 0), dtype=np.complex128)
        if method == "complex":
            M = sp.csc_matrix(self.r.G, dtype=np.complex128) + 1j * self.r.B(omega)
            return _refined_block(M)(self.S.astype(np.complex128))
        M = sp.kron(self.r.G, sp.identity(2)) + sp.kron(self.r.B(omega), sp.csr_matrix(ROTATE))
        B = np.zeros((2 * self.n, len(self.ports)))
        B[0::2] = self.S
        X = _refined_block(M)(B)
        return X[0::2] + 1j * X[1::2]

    def sweep(self, frequencies, method="complex"):
        """(X [F, n, P], Z [F, P, P]) with Z = S^T X"""
        X = np.array([self.solutions(f, method) for f in frequencies]).reshape(len(frequencies), self.n, len(self.ports))
        return X, np.einsum("np,fnq->fpq", self.S, X)


def scales(X):
    """per frequency the largest magnitude among all unknowns of the P solutions: what every bar scales by"""
    return np.array([np.abs(x).max(initial=0.0) for x in X])


def worst_ratio(got, want, X, tol=TOL):
    """per frequency the largest miss of `got` against `want` over tol times scales(X); the worst frequency (0 / 0 is 0)"""
    worst = 0.0
    for g, w, s in zip(got, want, scales(X)):
        if np.size(w):
            miss, bar = np.abs(np.asarray(g) - np.asarray(w)).max(), tol * s
            worst = max(worst, miss / bar if bar > 0 else (0.0 if miss == 0 else np.inf))
    return worst


# ---- closed forms -----------------------------------------------------------------------------------------------------
def t_network_rows(R1, R2):
    """R1 a-m, R2 b-m; the capacitor goes m-g.  The 1 A source a-g brings the ground node into the netlist (reactive
    elements introduce no nodes) and stamps nothing into G: it is off in a port analysis, like every independent source.
    At DC a, b and m float, at any frequency they do not."""
    return [["r1", "R", repr(float(R1)), "a", "m"], ["r2", "R", repr(float(R2)), "b", "m"], ["a0", "A", "1.0", "a", "g"]]


def t_network_closed_form(frequencies, R1, R2, C):
    """Z [F, 2, 2] seen from the ports a and b: [[R1 + zc, zc], [zc, R2 + zc]] with zc = 1 / (j w C)"""
    w = 2.0 * math.pi * np.asarray(frequencies, dtype=np.float64)
    zc = 1.0 / (1j * w * C)
    return np.stack([np.stack([R1 + zc, zc], axis=1), np.stack([zc, R2 + zc], axis=1)], axis=1)


def tank_rows(R):
    """R t-g; the capacitor and the inductor go t-g as well"""
    return [["r1", "R", repr(float(R)), "t", "g"]]


def tank_closed_form(frequencies, R, L, C):
    """Z [F] of the parallel RLC tank: 1 / (1 / R + j w C + 1 / (j w L)), R at resonance"""
    w = 2.0 * math.pi * np.asarray(frequencies, dtype=np.float64)
    return 1.0 / (1.0 / R + 1j * w * C + 1.0 / (1j * w * L))
