"""One frequency that is singular by itself, in the middle of a sweep, through the four small-signal analyses
(nodal_ac_sweep, nodal_ac_noise, nodal_ac_ports, nodal_ac_gradient).  The convention -- that frequency alone gets
info = 1 and NaN in its rows, the ones after it are solved, a sum over the frequencies is void -- has one statement in
csrc/ac_sweep.h (AcLedger); every other singular test of the suite uses an island that is singular at every frequency.

The network: a source on a ladder of series resistors with a shunt at every node and one capacitor, and beside it an
island of two nodes joined by a resistor of 1 ohm, which touches the rest of the world only through C = 1 F and L = 1 H
from its node u1 to ground.  At omega = 1 their susceptances are w C = 1.0 and -1 / (w L) = -1.0 and add up to exactly
0.0, whatever the order: the doubled matrix there is that of a floating island, whose elimination meets 1 - 1 = 0 with
no rounding.  At omega = 0.5 and 2 the island is grounded through -1.5 S and +1.5 S.  omega goes to the handle as it is
(Circuit.ac would multiply a frequency by 2 pi).

Cases: 4 nodes (2n = 8: the dense panel on the sparse path) and 42 nodes (2n = 84: the sparse LU), each with an A source
(G symmetric: noise and the gradient's adjoint solve on h->ac) and with an E source (a branch row: they solve on the
transposed child, 2n = 10 and 86).

Bars: scaled_residual <= RESID_BAR = 1e-12 at the solved frequencies, the bar of tests/test_gpu_ac.py, test_gpu_noise.py,
test_gpu_ac_ports.py and test_gpu_ac_gradient.py.  The solved frequencies are also held against the same call without
the singular frequency: TOL = 1e-9, the project's normwise bar, times the largest magnitude of the array at hand (two
solves of one system with residuals under 1e-12; the factorisation after a failed one need not repeat the bits of one
after a good one, so equality is not asked for)."""
import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd.ac import resolve_amplitudes, resolve_reactive
from nodal_amd.ports import _as_pair, resolve_ports

pytestmark = pytest.mark.gpu

RESID_BAR = 1e-12
TOL = 1e-9
OMEGA = np.array([0.5, 1.0, 2.0])
SOLVED = [0, 2]
CASES = pytest.mark.parametrize("sections,source", [(2, "A"), (2, "E"), (40, "A"), (40, "E")],
                                ids=["panel-A", "panel-E", "lu-A", "lu-E"])


def network(sections, source):
    rows = []
    for k in range(sections):
        rows.append([f"rp{k}", "R", "2", f"n{k}", "g"])
        if k + 1 < sections:
            rows.append([f"rs{k}", "R", "1", f"n{k}", f"n{k + 1}"])
    rows.append(["ri", "R", "1", "u1", "u2"])
    rows.append(["s1", source, "1", "n0", "g"])
    caps = [("cd", 0.5, "n1", "g"), ("ci", 1.0, "u1", "g")]
    inds = [("li", 1.0, "u1", "g")]
    return rows, caps, inds


class Case:
    def __init__(self, sections, source, sparse=True):
        rows, caps, inds = network(sections, source)
        self.nl = n.Netlist.from_rows(rows)
        self.c = n.Circuit(self.nl, sparse=sparse)
        self.h = self.c._handle
        self.K = self.nl.nums["kcl"]
        assert self.K == sections + 2 and self.h.n == self.K + (source == "E")
        _, self.kind, self.value, self.ea, self.eb = resolve_reactive(self.nl, caps, inds)
        self.rows, self.amplitudes = resolve_amplitudes(self.nl, {"s1": 1.0 - 0.5j})
        pairs = [_as_pair(self.nl, p) for p in (f"n{sections - 1}", "u2", ("n0", "u1"))]
        self.pa, self.pb = resolve_ports(self.nl, pairs)
        self.cur = np.array([0, 1, 2], dtype=np.int32)
        self.cot = np.array([[1 + 2j, -1j, 0.5], [2, 1, 1j], [-1 + 1j, 0.25, 3]], dtype=np.complex128)

    def reactive(self):
        return self.kind, self.value, self.ea, self.eb

    def sweep(self, omega, dense=False):
        return self.h.ac_sweep(omega, *self.reactive(), self.rows, self.amplitudes, self.pa, self.pb, self.cur, dense=dense,
                               keep_every=1, peaks=True)

    def noise(self, omega, dense=False):
        return self.h.ac_noise(omega, *self.reactive(), 300.0, self.pa, self.pb, dense=dense, input_row=int(self.rows[0]),
                               weight=np.ones(len(omega)))

    def ports(self, omega, dense=False):
        return self.h.ac_ports(omega, *self.reactive(), self.pa, self.pb, dense=dense, peaks=True)

    def gradient(self, omega, dense=False):
        cot = self.cot if len(omega) == 3 else self.cot[SOLVED]
        return self.h.ac_gradient(omega, *self.reactive(), self.rows, self.amplitudes, self.pa, self.pb, cot, dense=dense,
                                  adjoints=True)


def check_ledger(tag, resid, info):
    """info and the residuals of a sweep over OMEGA"""
    print(tag, "info", info.tolist(), "scaled residuals", resid.tolist())
    assert info.tolist() == [0, 1, 0], tag
    assert np.isnan(resid[1]).all(), tag
    assert np.isfinite(resid[SOLVED]).all() and (resid[SOLVED] <= RESID_BAR).all(), tag


def check_rows(tag, got, clean):
    """a per-frequency output [3, ...] of the sweep over OMEGA: NaN exactly in the rows of frequency 1, in both parts of
    a complex array, and the rows of the solved frequencies finite and those of the call without frequency 1"""
    parts = got.view(np.float64) if np.iscomplexobj(got) else got
    assert got.shape[0] == 3 and np.isnan(parts[1]).all(), tag
    assert np.isfinite(parts[SOLVED]).all(), tag
    miss = float(np.max(np.abs(got[SOLVED] - clean), initial=0.0))
    scale = float(np.max(np.abs(clean), initial=0.0))
    print(tag, "largest miss against the clean call", miss, "over the bar", miss / (TOL * scale) if scale else miss)
    assert miss <= TOL * scale, tag


@CASES
def test_ac_sweep(sections, source):
    case = Case(sections, source)
    wave, cur, x, peak, resid, info = case.sweep(OMEGA)
    cwave, ccur, cx, cpeak, cresid, cinfo = case.sweep(OMEGA[SOLVED])
    assert (cinfo == 0).all() and (cresid <= RESID_BAR).all()
    check_ledger("ac sweep", resid, info)
    check_rows("ac sweep: phasors", wave, cwave)
    check_rows("ac sweep: currents", cur, ccur)
    check_rows("ac sweep: kept solutions", x, cx)
    # the peaks are those of the solved frequencies: the magnitudes of the clean call, attained at a solved frequency
    # (sqrt(re re + im im) against numpy's hypot: a few ulp of the largest magnitude; a node that an E source holds has
    # the same magnitude at every frequency up to rounding, so the index itself is not compared with the clean call's)
    assert np.isfinite(peak[0]).all() and np.abs(peak[0] - cpeak[0]).max() <= TOL * cpeak[0].max()
    assert set(peak[1].tolist()) <= set(SOLVED)
    magnitude = np.abs(x)[:, :case.K]
    assert np.abs(peak[0] - magnitude[SOLVED].max(axis=0)).max() <= 1e-14 * magnitude[SOLVED].max()
    assert np.abs(peak[0] - magnitude[peak[1], np.arange(case.K)]).max() <= 1e-14 * magnitude[SOLVED].max()


@CASES
def test_noise(sections, source):
    case = Case(sections, source)
    density, gain, contrib, resid, info = case.noise(OMEGA)
    cdensity, cgain, ccontrib, cresid, cinfo = case.noise(OMEGA[SOLVED])
    assert (cinfo == 0).all() and (cresid <= RESID_BAR).all() and np.isfinite(ccontrib).all()
    check_ledger("noise", resid, info)
    check_rows("noise: densities", density, cdensity)
    check_rows("noise: gains", gain, cgain)
    assert (density[SOLVED][:, 1] > 0.0).all()  # (the island's resistor is heard at u2)
    assert contrib.shape == ccontrib.shape and np.isnan(contrib).all()  # an integral over a list with a hole is none


@CASES
def test_ac_ports(sections, source):
    case = Case(sections, source)
    z, peak, resid, info, work = case.ports(OMEGA)
    cz, cpeak, cresid, cinfo, cwork = case.ports(OMEGA[SOLVED])
    assert (cinfo == 0).all() and (cresid <= RESID_BAR).all()
    check_ledger("ac ports", resid, info)
    check_rows("ac ports: z", z, cz)
    assert np.isfinite(peak[0]).all() and np.abs(peak[0] - cpeak[0]).max() <= TOL * cpeak[0].max()
    assert set(peak[2].tolist()) <= set(SOLVED) and ((peak[1] >= 0) & (peak[1] < len(case.pa))).all()
    assert work[0] == 3 and cwork[0] == 2  # one factorisation per frequency, the singular one's included


@CASES
def test_ac_gradient(sections, source):
    case = Case(sections, source)
    wave, grad, greact, gsrc, lam, resid, info, work = case.gradient(OMEGA)
    cwave, cgrad, cgreact, cgsrc, clam, cresid, cinfo, cwork = case.gradient(OMEGA[SOLVED])
    assert (cinfo == 0).all() and (cresid <= RESID_BAR).all() and np.isfinite(cgrad).all() and np.isfinite(cgreact).all()
    check_ledger("ac gradient", resid, info)
    check_rows("ac gradient: phasors", wave, cwave)
    check_rows("ac gradient: source terms", gsrc, cgsrc)
    check_rows("ac gradient: adjoints", lam, clam)
    # a sum over a list with a hole is none
    assert grad.shape == cgrad.shape and np.isnan(grad).all() and greact.shape == (3,) and np.isnan(greact).all()


@pytest.mark.parametrize("analysis", ["sweep", "noise", "ports", "gradient"])
@pytest.mark.parametrize("sections", [2, 40], ids=["panel", "forced"])
def test_dense_raises(sections, analysis):
    case = Case(sections, "A", sparse=False)
    with pytest.raises(_ffi.NodalHipError, match="singular matrix") as exc:
        getattr(case, analysis)(OMEGA, dense=True)
    assert exc.value.status == _ffi.E_SINGULAR
    # ... and the frequencies around it are solved by the same handle
    out = getattr(case, analysis)(OMEGA[SOLVED], dense=True)
    info = out[{"sweep": 5, "noise": 4, "ports": 3, "gradient": 6}[analysis]]
    assert (info == 0).all()
