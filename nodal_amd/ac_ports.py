"""AC port analysis: the impedance matrix Z(jw) of an RLC network seen from chosen ports, over a list of frequencies.

The question `ac.py` opens with -- impedance against frequency, the resonance of a decoupling network -- asked of several
ports at once: driving-point impedance profiles of a power grid with its decoupling capacitors, transfer impedances
between injection sites, the Y- and S-parameters of a filter.  With A(w) = G + j B(w) the matrix of `Circuit.ac` and
port q the ordered pair (node_plus, node_minus), x_q solves A(w) x_q = e(plus_q) - e(minus_q) with every independent
source off, and

    Z[f][p][q]   volts at port p per ampere entering node_plus of port q and leaving its node_minus at frequency f
                 (the sign of `Circuit.thevenin`).

`Circuit.ac` answers it one port and one call at a time, for a source that is in the netlist already, with a numeric
factorisation of the doubled system per call and frequency; `Circuit.thevenin` gives the P x P matrix at DC only.
`Circuit.ac_ports` hands the sweep to `nodal_ac_ports` (csrc/ac_ports.hip): one factorisation per frequency whatever the
number of ports, the ports pushed through the factors sixteen at a time, the solutions read at the port nodes on the
device -- F x P x P complex numbers come down, not F x P x 2n.

`check_ac_port_arguments` needs no device, and `ACPortSweep` / `ACPortPeaks` are plain containers that can be built from
arrays; the methods are numpy calls on P x P matrices, nothing on the hot path.
"""

import math

import numpy as np

from .ac import check_ac_arguments
from .ports import _as_pair, resolve_ports


def check_ac_port_arguments(netlist, frequencies, ports):
    """The frequencies and ports of Circuit.ac_ports as (omega float64 [F], the (node_plus, node_minus) labels, ia, ib
    int32 [P], -1 for the ground node): frequencies as Circuit.ac takes them, ports as Circuit.thevenin takes them.
    ValueError for frequencies that are not a flat sequence of finite values > 0 and for a malformed port, KeyError for
    a node the netlist does not have."""
    omega = check_ac_arguments(frequencies)
    pairs = [_as_pair(netlist, port) for port in ports]
    ia, ib = resolve_ports(netlist, pairs)
    return omega, pairs, ia, ib


class ACPortPeaks:
    """Per node the largest |x_q(i)| over all ports q and all solved frequencies -- the worst transfer impedance
    magnitude from any port to that node --, the port and the frequency index that attain it (among exact ties the
    lowest frequency, then the lowest port; frequencies with info > 0 are left out; NaN, -1 and -1 when every one is)."""

    def __init__(self, magnitude, port, frequency_index):
        self.magnitude = magnitude
        self.port = port
        self.frequency_index = frequency_index


class ACPortSweep:
    """Result of Circuit.ac_ports.

    frequencies [F] in Hz and omega [F] in rad/s; ports: the (node_plus, node_minus) labels; z complex128 [F, P, P];
    info [F]: 0 solved, > 0 singular at that frequency (sparse path: NaN in its rows); scaled_residual [F, P] of every
    column's real system of twice the size, computed on the device; peaks (ACPortPeaks) or None; work: three ints --
    numeric factorisations, applications of the sparse factors to a block of up to sixteen columns, columns redone
    alone; timings: nodal_last_timings of the call, as ACSweep's."""

    def __init__(self, frequencies, omega, ports, z, info, scaled_residual, peaks=None, work=(0, 0, 0), timings=None):
        self.frequencies = np.asarray(frequencies, dtype=np.float64)
        count = len(self.frequencies)
        self.omega = omega
        self.ports = list(ports)
        self.z = np.asarray(z, dtype=np.complex128).reshape(count, len(self.ports), len(self.ports))
        self.info = np.asarray(info, dtype=np.int32).reshape(count)
        self.scaled_residual = np.asarray(scaled_residual, dtype=np.float64).reshape(count, len(self.ports))
        self.peaks = peaks
        self.work = tuple(int(w) for w in work)
        self.timings = timings

    def __len__(self):
        return len(self.info)

    def driving_point(self):
        """Z_pp(f), the impedance seen into every port with the others open: the diagonals, complex128 [F, P]."""
        return np.diagonal(self.z, axis1=1, axis2=2).copy()

    def reciprocity(self):
        """Per frequency max |Z - Z^T| / max |Z|, [F]: 0 (to rounding) for a network of R, L and C, not for one with
        dependent sources; 0.0 for an empty or all-zero Z, NaN for a frequency with info > 0."""
        out = np.zeros(len(self))
        for f, z in enumerate(self.z):
            if z.size == 0:
                continue
            scale = np.abs(z).max()
            if scale != 0.0:  # (NaN for a singular frequency: it is not 0.0)
                out[f] = np.abs(z - z.T).max() / scale
        return out

    def _solved(self):
        return np.flatnonzero(self.info == 0)

    def y(self):
        """The short-circuit admittance matrices Y(f) = Z(f)^-1, complex128 [F, P, P]: numpy's batched inverse on the
        host.  Frequencies with info > 0 stay NaN; LinAlgError when a solved Z is singular (a port between a node and
        itself, two ports that are the same pair)."""
        out = np.full(self.z.shape, np.nan + 1j * np.nan, dtype=np.complex128)
        solved = self._solved()
        if len(solved) and self.z.shape[1]:
            out[solved] = np.linalg.inv(self.z[solved])
        return out

    def s(self, z0=50.0):
        """The scattering parameters S(f) = R^-1/2 (Z - R) (Z + R)^-1 R^1/2 with R = diag(z0), complex128 [F, P, P]:
        `z0` a positive finite reference resistance, one for every port or a [P] array.  ValueError for anything else.
        Frequencies with info > 0 stay NaN."""
        count = len(self.ports)
        try:
            r = np.asarray(z0, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("z0 must be a positive finite resistance or one per port") from None
        if r.ndim == 0:
            r = np.full(count, float(r))
        if r.shape != (count,) or not all(v > 0.0 and math.isfinite(v) for v in r.tolist()):
            raise ValueError("z0 must be a positive finite resistance or one per port")
        out = np.full(self.z.shape, np.nan + 1j * np.nan, dtype=np.complex128)
        solved = self._solved()
        if len(solved) and count:
            z, big = self.z[solved], np.diag(r)
            root = np.sqrt(r)
            # (Z - R) (Z + R)^-1 = ((Z + R)^T \ (Z - R)^T)^T, one batched solve
            core = np.linalg.solve(np.swapaxes(z + big, 1, 2), np.swapaxes(z - big, 1, 2))
            out[solved] = np.swapaxes(core, 1, 2) * root[None, None, :] / root[None, :, None]
        return out

    def peak_impedance(self):
        """(magnitude [P], frequency_index [P]): per port the largest |Z_pp| over the solved frequencies and the index
        of the first frequency that attains it; NaN and -1 when no frequency is solved."""
        count = len(self.ports)
        solved = self._solved()
        if not len(solved):
            return np.full(count, np.nan), np.full(count, -1, dtype=np.int64)
        mag = np.abs(self.driving_point()[solved])
        best = np.argmax(mag, axis=0)
        return mag[best, np.arange(count)], solved[best]
