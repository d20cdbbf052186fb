"""The numpy / scipy restatement every noise test is measured against (never product code), on tests/ac_reference.py.

A(w) = G + j B(w) is the AC reference's matrix.  A table row of type R with value R_k > 0 and leads a != b is a noise
current source of the density 4 k_B T / R_k across its leads; every other row makes no noise.  Output p is the node pair
(oa, ob).  Two INDEPENDENT formulations give what row k adds at output p, c_k(f, p):

  adjoint   y_p = A^-T (e(oa) - e(ob)) by scipy's complex sparse LU of the TRANSPOSED matrix and one step of refinement,
            one solve per output; c_k = 4 k_B T / R_k |y_p(a) - y_p(b)|^2.  The gain from an input source is y_p^T s.
  direct    z_k = A^-1 (e(a) - e(b)), the response to a unit current through resistor k, one solve per resistor on the
            matrix itself (sparse LU, many right-hand sides, refined); c_k = 4 k_B T / R_k |z_k(oa) - z_k(ob)|^2.  No
            transpose appears anywhere.

The density is the sum over k, the integrated contribution of k the trapezoid rule of c_k over the frequencies in Hz.

Bars, normwise as in the AC suite (TOL = 1e-9 on the device): amplitude densities sqrt(S) of a frequency against the
largest expected one among that frequency's outputs; the contributions of a call against the call's largest expected
contribution; gains against the largest expected |H| of the frequency; 0 / 0 counts as 0.  A relative bar on the density
itself would be wrong: an output pinned by an ideal source has a density that is pure rounding (1e-56 against 1e-20).
On the CPU the two formulations agree in these terms to 2.2e-15 (amplitude densities) and 5.4e-15 (contributions) over
the inputs of the branches suite and the AC suite's grid(12) (tests/test_noise_frontend.py asserts 1e-13).
"""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import ac_reference as acr
from tests.ac_reference import TOL, _index  # noqa: F401

BOLTZMANN = 1.380649e-23  # J / K, the exact SI value
T_R = 0
CHUNK = 512  # right-hand sides of one direct solve


def node_labels(nl):
    return sorted(nl.nodenum, key=nl.nodenum.get)


def two_outputs(nl):
    """the outputs of the suites: the first node against ground, the last node against the first"""
    labels = node_labels(nl)
    return [labels[0], (labels[-1], labels[0])]


def trapezoid(frequencies, y):
    """the trapezoid rule of y [F, ...] over the frequencies, written out"""
    f = np.asarray(frequencies, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    total = np.zeros(y.shape[1:])
    for k in range(len(f) - 1):
        total = total + 0.5 * (f[k + 1] - f[k]) * (y[k] + y[k + 1])
    return total


class NoiseReference:
    """rows: the netlist; capacitors, inductors: (name, value, node_a, node_b)."""

    def __init__(self, rows, capacitors=(), inductors=()):
        self.ac = acr.ACReference(rows, capacitors, inductors)
        self.nl, self.n, self.K = self.ac.nl, self.ac.n, self.ac.K
        t = self.ac.base.table
        self.ncomp = int(t.ncomp)
        self.type = np.asarray(t.type, dtype=np.int64).reshape(self.ncomp)
        self.value = np.asarray(t.value, dtype=np.float64).reshape(self.ncomp)
        self.a = np.asarray(t.a, dtype=np.int64).reshape(self.ncomp)
        self.b = np.asarray(t.b, dtype=np.int64).reshape(self.ncomp)
        self.noisy = np.flatnonzero((self.type == T_R) & (self.value > 0.0) & (self.a != self.b))

    def pairs(self, outputs):
        out = [(o, self.nl.ground) if not isinstance(o, (tuple, list)) else tuple(o) for o in outputs]
        return (np.array([_index(self.nl, o[0]) for o in out], dtype=np.int64).reshape(len(out)),
                np.array([_index(self.nl, o[1]) for o in out], dtype=np.int64).reshape(len(out)))

    def matrix(self, omega):
        return sp.csc_matrix(sp.csc_matrix(self.ac.G, dtype=np.complex128) + 1j * self.ac.B(omega))

    def _unit(self, ia, ib):
        """columns e(ia[q]) - e(ib[q]), ground dropped"""
        E = np.zeros((self.n + 1, len(ia)), dtype=np.complex128)
        for q, (a, b) in enumerate(zip(ia, ib)):
            E[a, q] += 1.0
            E[b, q] -= 1.0
        return E[:self.n]

    @staticmethod
    def _solve(M, rhs):
        lu, Mr = spla.splu(sp.csc_matrix(M)), sp.csr_matrix(M)
        x = lu.solve(rhs)
        return x + lu.solve(rhs - Mr @ x)

    def _scale(self, temperature):
        return 4.0 * BOLTZMANN * float(temperature) / self.value[self.noisy]

    def adjoint(self, frequencies, outputs, temperature=300.0, input=None, transpose=True):
        """(contributions per frequency [F, P, ncomp], gain [F, P] complex or None); transpose=False solves with A in
        place of A^T: the mistake the suites must be able to see"""
        oa, ob = self.pairs(outputs)
        F, P = len(frequencies), len(oa)
        c = np.zeros((F, P, self.ncomp))
        gain = np.zeros((F, P), dtype=np.complex128) if input is not None else None
        s = self.ac.rhs({input: 1.0}) if input is not None else None
        rhs = self._unit(oa, ob)
        for f, hz in enumerate(frequencies):
            A = self.matrix(2.0 * math.pi * float(hz))
            Y = self._solve(A.T if transpose else A, rhs)  # [n, P]
            Ye = np.vstack([Y, np.zeros((1, P))])
            d = Ye[self.a[self.noisy], :] - Ye[self.b[self.noisy], :]
            c[f][:, self.noisy] = (self._scale(temperature)[:, None] * (d.real ** 2 + d.imag ** 2)).T
            if gain is not None:
                gain[f] = Y.T @ s  # (nothing is conjugated)
        return c, gain

    def direct(self, frequencies, outputs, temperature=300.0):
        """contributions per frequency [F, P, ncomp], one column of A^-1 (e(a) - e(b)) per resistor"""
        oa, ob = self.pairs(outputs)
        F, P = len(frequencies), len(oa)
        c = np.zeros((F, P, self.ncomp))
        scale = self._scale(temperature)
        for f, hz in enumerate(frequencies):
            A = self.matrix(2.0 * math.pi * float(hz))
            lu, Ar = spla.splu(A), sp.csr_matrix(A)
            for k0 in range(0, len(self.noisy), CHUNK):
                ks = self.noisy[k0:k0 + CHUNK]
                rhs = self._unit(self.a[ks], self.b[ks])
                Z = lu.solve(rhs)
                Z = Z + lu.solve(rhs - Ar @ Z)
                Ze = np.vstack([Z, np.zeros((1, len(ks)))])
                t = Ze[oa, :] - Ze[ob, :]  # [P, chunk]
                c[f][:, ks] = scale[k0:k0 + CHUNK][None, :] * (t.real ** 2 + t.imag ** 2)
        return c

    def integrated_contributions(self, frequencies, c):
        return trapezoid(frequencies, c)


def density(c):
    """[F, P] from the contributions per frequency [F, P, ncomp]"""
    return c.sum(axis=2)


# ---- the bars ---------------------------------------------------------------------------------------------------------
def ratio(miss, bar):
    return miss / bar if bar > 0 else (0.0 if miss == 0 else np.inf)


def amplitude_miss(got_density, want_density, tol):
    """per frequency the largest miss of sqrt(S) over tol times the largest expected sqrt(S) of that frequency; the worst"""
    worst = 0.0
    for g, w in zip(np.sqrt(got_density), np.sqrt(want_density)):
        if len(w):
            worst = max(worst, ratio(np.abs(g - w).max(), tol * np.abs(w).max()))
    return worst


def call_miss(got, want, tol):
    """the largest miss of a call over tol times the call's largest expected magnitude"""
    got, want = np.asarray(got), np.asarray(want)
    return ratio(np.abs(got - want).max(), tol * np.abs(want).max()) if want.size else 0.0


def gain_miss(got, want, tol):
    worst = 0.0
    for g, w in zip(got, want):
        if len(w):
            worst = max(worst, ratio(np.abs(g - w).max(), tol * np.abs(w).max()))
    return worst


# ---- closed forms -----------------------------------------------------------------------------------------------------
def rc_parallel_rows(R):
    """R from out to ground; the capacitor goes beside it.  No source at all."""
    return [["r1", "R", repr(float(R)), "out", "g"]]


def rc_parallel_density(frequencies, R, C, temperature):
    """S_out = 4 k_B T R / (1 + (w R C)^2); over all frequencies it integrates to k_B T / C"""
    w = 2.0 * math.pi * np.asarray(frequencies, dtype=np.float64)
    return 4.0 * BOLTZMANN * temperature * R / (1.0 + (w * R * C) ** 2)


def divider_rows(R1, R2):
    """E 1 V in-g, R1 in-out, R2 out-g"""
    return [["e1", "E", "1.0", "in", "g"], ["r1", "R", repr(float(R1)), "in", "out"], ["r2", "R", repr(float(R2)), "out", "g"]]


def divider_closed_form(R1, R2, temperature):
    """(S_out, H, the contributions of (r1, r2) to S_out): S_out = 4 k_B T (R1 || R2), H = R2 / (R1 + R2).  The source
    pins `in`, so either resistor's noise current enters `out` and sees Z = R1 || R2: the shares are 4 k_B T / R1 Z^2
    and 4 k_B T / R2 Z^2 -- with Z^2 = R1^2 R2^2 / (R1 + R2)^2 they stand as R2 : R1, and they sum to S_out"""
    Z = R1 * R2 / (R1 + R2)
    kt4 = 4.0 * BOLTZMANN * temperature
    return kt4 * Z, R2 / (R1 + R2), (kt4 / R1 * Z * Z, kt4 / R2 * Z * Z)
