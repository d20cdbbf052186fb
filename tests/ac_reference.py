"""The numpy / scipy restatement every AC test is measured against (never product code).

G comes from the oracle's build_model of the netlist the circuit is built from, so the circuit's numbering holds
(tests/transient_reference.py, which also restates the right-hand side from the lowered table and checks it against the
oracle's A).  s_r and s_i are that right-hand side with every A / E value replaced by the real (imaginary) part of its
amplitude, 0 for a source that is not named.  B(w) = S diag(b) S^T by incidence, S the reactive elements' incidence (+1
at lead a, -1 at lead b, ground dropped), b = w C for a capacitor and -1 / (w L) for an inductor.  Two INDEPENDENT
formulations solve a frequency:

  complex      (G + j B) x = s_r + j s_i, scipy's complex sparse LU and one step of refinement
  interleaved  the real system of twice the size, kron(G, I_2) + kron(B, [[0, -1], [1, 0]]) on (re, im) pairs: what the
               device solves

On the CPU the two agree to 5.4e-16 of the largest unknown on grid(12) with two E sources, a capacitor on every node and
five inductors over 17 frequencies from 1e-4 to 1e4 Hz (tests/test_ac_frontend.py asserts 1e-13), and the closed forms of
the RC low-pass and the series RLC hold to 1e-14, so the project's normwise bar TOL = 1e-9 leaves four decades for the
device.
"""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import transient_reference as ref
from tests.transient_reference import TOL, _index  # noqa: F401

ROTATE = np.array([[0.0, -1.0], [1.0, 0.0]])  # multiplication by j on a (re, im) pair


def _refined(M):
    """x = M^-1 b by a sparse LU and one step of refinement (the LU's own rounding is not to show in the comparisons)"""
    lu, Mr = spla.splu(sp.csc_matrix(M)), sp.csr_matrix(M)

    def solve(b):
        x = lu.solve(b)
        return x + lu.solve(b - Mr @ x)
    return solve


class ACReference:
    """rows: the netlist; capacitors, inductors: (name, value, node_a, node_b)."""

    def __init__(self, rows, capacitors=(), inductors=()):
        self.base = ref.TransientReference(rows, [], 1.0, "euler")
        self.nl, self.n, self.K, self.G = self.base.nl, self.base.n, self.base.K, self.base.G
        elements = [(0,) + tuple(c) for c in capacitors] + [(1,) + tuple(i) for i in inductors]
        count = len(elements)
        self.names = [e[1] for e in elements]
        self.kind = np.array([e[0] for e in elements], dtype=np.int64).reshape(count)
        self.value = np.array([float(e[2]) for e in elements], dtype=np.float64).reshape(count)
        self.ia = np.array([_index(self.nl, e[3]) for e in elements], dtype=np.int64).reshape(count)
        self.ib = np.array([_index(self.nl, e[4]) for e in elements], dtype=np.int64).reshape(count)
        S = sp.lil_matrix((self.n + 1, count))
        for q, (a, b) in enumerate(zip(self.ia, self.ib)):  # (index -1, the ground lead, falls on the row that is dropped)
            S[a, q] += 1.0
            S[b, q] -= 1.0
        self.S = sp.csr_matrix(S)[:self.n, :]

    def source_names(self):
        comps = self.nl.components
        return sorted({key for key in self.nl.component_keys if comps[key].type in ("A", "E")})

    def susceptances(self, omega):
        return np.where(self.kind == 0, omega * self.value, -1.0 / (omega * self.value))

    def B(self, omega):
        return sp.csr_matrix(self.S @ sp.diags(self.susceptances(omega)) @ self.S.T) if len(self.value) else sp.csr_matrix((self.n, self.n))

    def rhs(self, amplitudes):
        """s = s_r + j s_i: every A / E source at its amplitude (name -> complex), the ones not named off"""
        amplitudes = {name: complex(v) for name, v in (amplitudes or {}).items()}
        assert set(amplitudes) <= set(self.source_names())
        re = {name: amplitudes.get(name, 0j).real for name in self.source_names()}
        im = {name: amplitudes.get(name, 0j).imag for name in self.source_names()}
        return self.base.rhs(re) + 1j * self.base.rhs(im)

    def solve_complex(self, omega, s):
        return _refined(sp.csc_matrix(self.G, dtype=np.complex128) + 1j * self.B(omega))(np.asarray(s, dtype=np.complex128))

    def solve_interleaved(self, omega, s):
        M = sp.kron(self.G, sp.identity(2)) + sp.kron(self.B(omega), sp.csr_matrix(ROTATE))
        b = np.empty(2 * self.n)
        b[0::2], b[1::2] = np.real(s), np.imag(s)
        x = _refined(M)(b)
        return x[0::2] + 1j * x[1::2]

    def sweep(self, frequencies, amplitudes, method="complex"):
        """X [F, n] complex at the frequencies (Hz)"""
        s = self.rhs(amplitudes)
        solve = self.solve_complex if method == "complex" else self.solve_interleaved
        return np.array([solve(2.0 * math.pi * float(f), s) for f in frequencies]).reshape(len(frequencies), self.n)

    def voltages(self, X):
        Xe = np.hstack([np.asarray(X, dtype=np.complex128), np.zeros((len(X), 1))])
        return Xe[:, self.ia] - Xe[:, self.ib]

    def currents(self, frequencies, X):
        """[F, E]: j b_q (x(a) - x(b)), from lead a to lead b through each element"""
        b = np.array([self.susceptances(2.0 * math.pi * float(f)) for f in frequencies]).reshape(len(frequencies), len(self.value))
        return 1j * b * self.voltages(X)


# ---- closed forms -----------------------------------------------------------------------------------------------------
def rc_lowpass_rows(R):
    """E 1 V in-g, R in-out; the capacitor goes out-g"""
    return [["e1", "E", "1.0", "in", "g"], ["r1", "R", repr(float(R)), "in", "out"]]


def rc_lowpass_closed_form(frequencies, R, C, amplitude=1.0):
    """(v_out, the capacitor's current out -> g) = (a / (1 + j w R C), j w C v_out)"""
    w = 2.0 * math.pi * np.asarray(frequencies, dtype=np.float64)
    v = amplitude / (1.0 + 1j * w * R * C)
    return v, 1j * w * C * v


def series_rlc_rows(R):
    """E 1 V in-g, R a-b; the inductor goes in-a and the capacitor b-g (reactive elements introduce no nodes, so the
    resistor sits in the middle: at DC a and b float, at any frequency they do not)"""
    return [["e1", "E", "1.0", "in", "g"], ["r1", "R", repr(float(R)), "a", "b"]]


def series_rlc_closed_form(frequencies, R, L, C, amplitude=1.0):
    """(v_a, v_b, the loop current in -> a -> b -> g) of the series circuit: i = a / (R + j w L + 1 / (j w C))"""
    w = 2.0 * math.pi * np.asarray(frequencies, dtype=np.float64)
    i = amplitude / (R + 1j * w * L + 1.0 / (1j * w * C))
    return amplitude - 1j * w * L * i, i / (1j * w * C), i
