"""AC analysis on the GPU (Circuit.ac / nodal_ac_sweep).  Every expected value comes from tests/ac_reference.py -- the
oracle's matrices and scipy's COMPLEX sparse LU, where the device solves the interleaved real system -- or from a closed
form, never from product code.

Bars: TOL = 1e-9, the project's normwise bar, per frequency: potentials against the largest potential of that frequency,
branch unknowns against the largest of theirs, element currents against the largest of theirs; 0 / 0 counts as 0.  The
two reference formulations agree to 5.4e-16 on the CPU (tests/test_ac_frontend.py), which leaves four decades.
scaled_residual <= RESID_BAR = 1e-12 per frequency, as in the transient suites."""
import math
import random
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd.circuit import MatrixRankWarning
from nodal_amd.lowering import lower
from tests import ac_reference as acr
from tests.ac_reference import TOL
from tests.test_gpu_branches import INPUTS, _island
from tests.test_gpu_transient_inductors import _grid_case, node_labels
from tests.transient_rl_reference import seeded_mix

pytestmark = pytest.mark.gpu

RESID_BAR = 1e-12
SPARSE = pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])


def ratio(miss, bar):
    return miss / bar if bar > 0 else (0.0 if miss == 0 else np.inf)


def worst_ratio(got, want):
    """per frequency (row) the largest miss over TOL times the largest expected magnitude of that row; the worst row"""
    worst = 0.0
    for g, w in zip(got, want):
        if len(w):
            worst = max(worst, ratio(np.abs(g - w).max(), TOL * np.abs(w).max()))
    return worst


def check_residuals(sw, tag):
    worst = float(np.max(sw.scaled_residual, initial=0.0))
    print(tag, "largest scaled residual", worst, "over the bar", worst / RESID_BAR)
    assert (sw.info == 0).all(), tag
    assert (sw.scaled_residual <= RESID_BAR).all(), tag


def full_sweep(c, freqs, caps, inds, amplitudes, **kw):
    """every node probed against ground in the order of its index, every element's current probed, every solution kept"""
    names = [e[0] for e in caps] + [e[0] for e in inds]
    return c.ac(freqs, caps, inds, sources=amplitudes, probes=node_labels(c.netlist), current_probes=names, keep_every=1, **kw)


def check_parity(r, sw, freqs, amplitudes, tag, X=None):
    X = r.sweep(freqs, amplitudes) if X is None else X
    K = r.K
    assert sw.solutions.shape == X.shape and sw.phasors.shape == (len(freqs), K)
    assert sw.solution_indices.tolist() == list(range(len(freqs)))
    assert np.array_equal(sw.solutions[:, :K], sw.phasors)
    pot = worst_ratio(sw.solutions[:, :K], X[:, :K])
    bra = worst_ratio(sw.solutions[:, K:], X[:, K:])
    cur = worst_ratio(sw.currents, r.currents(freqs, X))
    print(tag, "worst miss over the bar: potentials", pot, "branch unknowns", bra, "element currents", cur)
    assert pot <= 1.0 and bra <= 1.0 and cur <= 1.0, tag
    return X


def seeded_amplitudes(names, seed):
    rng = random.Random(seed)
    return {name: complex(rng.uniform(-2.0, 2.0), rng.uniform(-2.0, 2.0)) for name in names}


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_outputs(a, b):
    return all(same_bits(getattr(a, f), getattr(b, f)) for f in ("phasors", "currents", "solutions", "info", "scaled_residual"))


# ---- 1: the RC low-pass (2n = 6: the dense panel) ---------------------------------------------------------------------
@SPARSE
def test_rc_lowpass(sparse):
    R, C = 2.0, 0.25
    freqs = (1.0 / (2.0 * math.pi * R * C)) * np.logspace(-2, 2, 9)
    c = n.Circuit(n.Netlist.from_rows(acr.rc_lowpass_rows(R)), sparse=sparse)
    assert c._handle.n == 3
    sw = c.ac(freqs, [("c1", C, "out", "g")], sources={"e1": 1.0}, probes=["out", ("in", "out"), ("out", "out"), ("g", "g")],
              current_probes=["c1"])
    check_residuals(sw, "rc low-pass")
    v, i = acr.rc_lowpass_closed_form(freqs, R, C)
    print("rc low-pass: worst miss over the bar", worst_ratio(sw.phasors[:, :1], v[:, None]),
          worst_ratio(sw.currents, i[:, None]))
    assert worst_ratio(sw.phasors[:, :1], v[:, None]) <= 1.0
    assert worst_ratio(sw.phasors[:, 1:2], (1.0 - v)[:, None]) <= 1.0
    assert worst_ratio(sw.currents, i[:, None]) <= 1.0
    for col in (2, 3):  # a probe between a node and itself reads exactly +0.0
        assert same_bits(sw.phasors[:, col], np.zeros(len(freqs), dtype=np.complex128))
    assert abs(sw.magnitude_db()[4, 0] + 10.0 * math.log10(2.0)) <= 1e-8 and abs(sw.phase_deg()[4, 0] + 45.0) <= 1e-7
    assert np.array_equal(sw.omega, 2.0 * math.pi * freqs) and sw.solutions is None and sw.peaks is None


# ---- 2: the series RLC through resonance ------------------------------------------------------------------------------
@SPARSE
def test_series_rlc(sparse):
    R, L, C = 0.5, 2.0, 0.125
    f0 = 1.0 / (2.0 * math.pi * math.sqrt(L * C))
    freqs = f0 * np.array([0.1, 0.5, 0.9, 0.99, 1.0, 1.01, 1.1, 2.0, 10.0])
    c = n.Circuit(n.Netlist.from_rows(acr.series_rlc_rows(R)), sparse=sparse)
    caps = [("c1", C, "b", "g")]
    sw = c.ac(freqs, caps, [("l1", L, "in", "a")], sources={"e1": 1.0}, probes=["a", "b"], current_probes=["l1", "c1"])
    check_residuals(sw, "series rlc")
    va, vb, i = acr.series_rlc_closed_form(freqs, R, L, C)
    want = np.stack([va, vb], axis=1)
    print("series rlc: worst miss over the bar", worst_ratio(sw.phasors, want), worst_ratio(sw.currents, np.stack([i, i], axis=1)))
    assert worst_ratio(sw.phasors, want) <= 1.0
    assert worst_ratio(sw.currents, np.stack([i, i], axis=1)) <= 1.0
    # the sign convention: an element's current counts from lead a to lead b, so swapped leads negate it bit for bit
    swapped = c.ac(freqs, caps, [("l1", L, "a", "in")], sources={"e1": 1.0}, probes=["a", "b"], current_probes=["l1", "c1"])
    assert same_bits(swapped.phasors, sw.phasors) and same_bits(swapped.currents[:, 1], sw.currents[:, 1])
    assert same_bits(swapped.currents[:, 0], -sw.currents[:, 0])


# ---- 3: every input of the branches suite -----------------------------------------------------------------------------
def test_the_inputs_are_all_there():
    assert len(INPUTS) == 29


_REFERENCES = {}
INPUT_FREQS = [0.01, 0.3, 10.0]


def _reference_of(k):
    """the reference of input k with its seeded elements and amplitudes and its sweep, computed once for both paths"""
    if k not in _REFERENCES:
        name, rows = INPUTS[k]
        caps, inds = seeded_mix(rows, k)
        r = acr.ACReference(rows, caps, inds)
        amplitudes = seeded_amplitudes(r.source_names(), 1000 + k)
        _REFERENCES[k] = (name, rows, caps, inds, r, amplitudes, r.sweep(INPUT_FREQS, amplitudes))
    return _REFERENCES[k]


@SPARSE
@pytest.mark.parametrize("k", range(29))
def test_every_input(k, sparse):
    name, rows, caps, inds, r, amplitudes, X = _reference_of(k)
    freqs = INPUT_FREQS
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=sparse)
    with warnings.catch_warnings():
        warnings.simplefilter("error", MatrixRankWarning)
        sw = full_sweep(c, freqs, caps, inds, amplitudes)
    tag = f"{name} {'sparse' if sparse else 'dense'} (2n = {2 * r.n})"
    check_residuals(sw, tag)
    check_parity(r, sw, freqs, amplitudes, tag, X=X)
    # the route: only the sparse LU (sparse, 2n > 64) spends time in numeric factorisations of its own
    assert (sw.timings[1] > 0.0) == (sparse and 2 * r.n > 64), (tag, sw.timings)
    assert 2 * r.n <= 24 or 2 * r.n in (1194, 7198)


# ---- 4, 5: the sparse LU route with branch rows, and the peaks --------------------------------------------------------
GRID_FREQS = np.logspace(-4, 4, 17)
GRID_AMPLITUDES = {"e1": 1.0, "e2": 0.5 - 0.25j, "ld0": 2j, "ld1": -1.0 + 1j}


@pytest.fixture(scope="module")
def grid_case():
    rows, caps, inds = _grid_case(12, ["e1", "e2"], 5, seed=31)
    return rows, caps, inds, acr.ACReference(rows, caps, inds)


def test_sparse_lu_route(grid_case):
    rows, caps, inds, r = grid_case
    assert r.n == 145 and r.base.B == 2
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    sw = full_sweep(c, GRID_FREQS, caps, inds, GRID_AMPLITUDES)
    check_residuals(sw, "grid(12) sparse LU")
    check_parity(r, sw, GRID_FREQS, GRID_AMPLITUDES, "grid(12) sparse LU")
    # a sub-set of the nodes, in another order and against each other: the probes read the kept solutions
    labels = node_labels(c.netlist)
    picks = [labels[7], labels[100], (labels[3], labels[60])]
    some = c.ac(GRID_FREQS, caps, inds, sources=GRID_AMPLITUDES, probes=picks, keep_every=1)
    assert same_bits(some.solutions, sw.solutions)
    assert same_bits(some.phasors[:, 0], sw.solutions[:, 7]) and same_bits(some.phasors[:, 1], sw.solutions[:, 100])
    assert same_bits(some.phasors[:, 2], sw.solutions[:, 3] - sw.solutions[:, 60])
    every_other = c.ac(GRID_FREQS, caps, inds, sources=GRID_AMPLITUDES, keep_every=2)
    assert every_other.solution_indices.tolist() == list(range(1, 17, 2))
    assert same_bits(every_other.solutions, np.ascontiguousarray(sw.solutions[1::2]))


def test_peaks(grid_case):
    rows, caps, inds, r = grid_case
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    plain = full_sweep(c, GRID_FREQS, caps, inds, GRID_AMPLITUDES)
    sw = full_sweep(c, GRID_FREQS, caps, inds, GRID_AMPLITUDES, peaks=True)
    assert same_outputs(plain, sw) and plain.peaks is None
    K = r.K
    mag = np.abs(sw.solutions[:, :K])
    index = np.argmax(mag, axis=0)
    assert sw.peaks.frequency_index.dtype == np.int32 and sw.peaks.frequency_index.tolist() == index.tolist()
    want = mag[index, np.arange(K)]
    ulps = np.abs(sw.peaks.magnitude - want) / np.spacing(want)
    print("peaks: largest distance from numpy's |x| in ulp", ulps.max())
    assert (ulps <= 2.0).all()


# ---- 6: kept work and determinism -------------------------------------------------------------------------------------
def test_kept_work_and_determinism(grid_case):
    rows, caps, inds, r = grid_case
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    first = full_sweep(c, GRID_FREQS[:5], caps, inds, GRID_AMPLITUDES)
    assert first.timings[0] > 0.0 and first.timings[1] > 0.0 and first.timings[2] > 0.0
    again = full_sweep(c, GRID_FREQS[:5], caps, inds, GRID_AMPLITUDES)
    assert again.timings[0] == 0.0 and same_outputs(first, again)
    # other frequencies, amplitudes and element VALUES on the same leads: nothing of the analysis is repeated
    caps2 = [(name, 1.5 * value, a, b) for name, value, a, b in caps]
    inds2 = [(name, 0.5 * value, a, b) for name, value, a, b in inds]
    amp2 = {"e1": 2j, "ld1": 0.25}
    other = full_sweep(c, [0.02, 3.0, 70.0], caps2, inds2, amp2)
    assert other.timings[0] == 0.0
    check_residuals(other, "same leads, other values")
    check_parity(acr.ACReference(rows, caps2, inds2), other, [0.02, 3.0, 70.0], amp2, "same leads, other values")
    # another set of leads: the pattern and the analysis are new
    name, henries, a, b = inds[-1]
    assert caps[0][2] not in (a, b)
    moved = full_sweep(c, GRID_FREQS[:5], caps, inds[:-1] + [(name, henries, caps[0][2], b if a == "g" else a)], GRID_AMPLITUDES)
    assert moved.timings[0] > 0.0
    # the circuit is left as it was: solve() and a transient run give the bits of a circuit that never ran ac()
    fresh = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    assert same_bits(np.asarray(c.solve().result), np.asarray(fresh.solve().result))
    runs = [x.transient(caps[:7], 0.5, 4, probes=node_labels(nl)[:5], inductors=inds[:2], current_probes=[inds[0][0]], keep_every=1)
            for x in (c, fresh)]
    for f in ("waveforms", "solutions", "currents", "final_currents", "scaled_residual"):
        assert same_bits(getattr(runs[0], f), getattr(runs[1], f)), f
    after = full_sweep(c, GRID_FREQS[:5], caps, inds, GRID_AMPLITUDES)
    assert same_outputs(first, after)


# ---- 7: what the excitation means -------------------------------------------------------------------------------------
def test_excitation_semantics(grid_case):
    rows, caps, inds, r = grid_case
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    freqs = [0.05, 1.0, 20.0]
    # every source off: exactly zero, although the netlist's own sources are not
    assert np.abs(np.asarray(c.A)).max() > 0
    off = full_sweep(c, freqs, caps, inds, None, peaks=True)
    for arr in (off.phasors, off.currents, off.solutions):
        assert arr.size > 0 and (arr == 0).all()
    assert (off.info == 0).all() and (off.scaled_residual == 0).all()
    assert (off.peaks.magnitude == 0).all() and (off.peaks.frequency_index == 0).all()
    # linearity in the amplitudes
    alpha = 0.75 - 1.5j
    one = full_sweep(c, freqs, caps, inds, GRID_AMPLITUDES)
    scaled = full_sweep(c, freqs, caps, inds, {name: alpha * v for name, v in GRID_AMPLITUDES.items()})
    K = r.K
    lin = max(worst_ratio(scaled.solutions[:, :K], alpha * one.solutions[:, :K]),
              worst_ratio(scaled.solutions[:, K:], alpha * one.solutions[:, K:]),
              worst_ratio(scaled.currents, alpha * one.currents))
    print("linearity: worst miss over the bar", lin)
    assert lin <= 1.0
    # purely real amplitudes on a purely resistive network: imaginary parts exactly 0, real parts those of solve_sources
    real = {"e1": 1.5, "e2": -0.5, "ld0": 2.0}
    res = c.ac(freqs, sources=real, keep_every=1)
    assert (res.solutions.imag == 0).all() and (res.info == 0).all()
    assert set(real) < set(r.source_names())  # (the grid's own source among the ones left out: off in ac(), 0 here)
    dc = c.solve_sources({name: [real.get(name, 0.0)] for name in r.source_names()}).result[0]
    want = np.repeat(dc[None, :], len(freqs), axis=0)
    miss = max(worst_ratio(res.solutions.real[:, :K], want[:, :K]), worst_ratio(res.solutions.real[:, K:], want[:, K:]))
    print("resistive network against solve_sources: worst miss over the bar", miss)
    assert miss <= 1.0


# ---- 8: a singular network --------------------------------------------------------------------------------------------
def test_singular_dense_raises():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=False)
    with pytest.raises(type(c._singular())):
        c.solve_sources({"a1": [1.0]})
    with pytest.raises(type(c._singular())):
        c.ac([1.0, 2.0], sources={"a1": 1.0}, probes=node_labels(nl)[:1])


def test_singular_sparse_warns_once():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sw = c.ac([1.0, 2.0, 4.0], sources={"a1": 1.0, "fa": 1j}, probes=node_labels(nl)[:3], keep_every=1, peaks=True)
    assert sum(issubclass(i.category, MatrixRankWarning) for i in w) == 1
    assert (sw.info > 0).all() and np.isnan(sw.scaled_residual).all()
    assert np.isnan(sw.phasors).all() and np.isnan(sw.solutions).all()
    assert np.isnan(sw.peaks.magnitude).all() and (sw.peaks.frequency_index == -1).all()


# ---- 9: argument errors -----------------------------------------------------------------------------------------------
def test_argument_errors_through_the_circuit():
    rows = dict(INPUTS)["random0"]
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    a, b = node_labels(nl)[:2]
    source = acr.ACReference(rows).source_names()[0]
    resistor = next(r[0] for r in rows if r[1] == "R")
    with pytest.raises(ValueError, match="frequencies"):
        c.ac([0.0])
    with pytest.raises(ValueError, match="keep_every"):
        c.ac([1.0], keep_every=-1)
    with pytest.raises(ValueError, match="farads"):
        c.ac([1.0], [("c1", -1.0, a, b)])
    with pytest.raises(ValueError, match="given twice"):
        c.ac([1.0], [("x", 1.0, a, b)], [("x", 1.0, a, b)])
    with pytest.raises(KeyError):
        c.ac([1.0], [("c1", 1.0, a, "nowhere")])
    with pytest.raises(TypeError):
        c.ac([1.0], sources=[(source, 1.0)])
    with pytest.raises(KeyError):
        c.ac([1.0], sources={"no such source": 1.0})
    with pytest.raises(ValueError, match="independent sources"):
        c.ac([1.0], sources={resistor: 1.0})
    with pytest.raises(KeyError, match="current probe"):
        c.ac([1.0], [("c1", 1.0, a, b)], current_probes=["c2"])
    with pytest.raises(KeyError):
        c.ac([1.0], probes=["nowhere"])
    empty = c.ac([], [("c1", 1.0, a, b)], sources={source: 1.0}, probes=[a], current_probes=["c1"], keep_every=1, peaks=True)
    assert len(empty) == 0 and empty.phasors.shape == (0, 1) and empty.currents.shape == (0, 1)
    # two inductors in parallel: legal
    sw = c.ac([1.0], inductors=[("l1", 1.0, a, b), ("l2", 2.0, a, b)], sources={source: 1.0}, current_probes=["l1", "l2"])
    assert (sw.info == 0).all() and same_bits(sw.currents[:, 0], 2.0 * sw.currents[:, 1])


def test_abi_refuses_bad_arguments():
    table = lower(n.Netlist.from_rows(dict(INPUTS)["random0"]))
    K = table.K
    types = np.asarray(table.type)
    a_row, r_row = int(np.flatnonzero(types == 1)[0]), int(np.flatnonzero(types == 0)[0])
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    good = dict(omega=[1.0, 2.0], kind=[0, 1], value=[1.0, 2.0], lead_a=[0, -1], lead_b=[-1, 1], rows=[a_row], amplitudes=[1 + 1j],
                ia=[0], ib=[-1], cur_index=[1])

    def call(**kw):
        args = {**good, **kw}
        return h.ac_sweep(args["omega"], args["kind"], args["value"], args["lead_a"], args["lead_b"], args["rows"],
                          args["amplitudes"], args["ia"], args["ib"], args["cur_index"], dense=False)

    with pytest.raises(_ffi.NodalHipError, match="assemble_numeric") as exc:
        call()
    assert exc.value.status == _ffi.E_INVALID
    h.assemble_numeric(0)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(omega=[1.0, 0.0]), "angular frequency"), (dict(omega=[-1.0]), "angular frequency"),
             (dict(omega=[nan]), "angular frequency"), (dict(omega=[inf]), "angular frequency"),
             (dict(kind=[0, 2]), "kind"), (dict(value=[1.0, 0.0]), "value"), (dict(value=[nan, 1.0]), "value"),
             (dict(value=[1.0, inf]), "value"), (dict(lead_a=[K, -1]), "lead out of range"),
             (dict(lead_b=[-2, 1]), "lead out of range"), (dict(lead_a=[0, 1]), "both leads"),
             (dict(rows=[table.ncomp]), "source row out of range"), (dict(rows=[-1]), "source row out of range"),
             (dict(rows=[r_row]), "not an independent source"),
             (dict(rows=[a_row, a_row], amplitudes=[1.0, 2.0]), "named twice"),
             (dict(ia=[K]), "probe node out of range"), (dict(ib=[-2]), "probe node out of range"),
             (dict(cur_index=[2]), "current probe outside"), (dict(cur_index=[-1]), "current probe outside")]
    for kw, text in cases:
        with pytest.raises(_ffi.NodalHipError, match=text) as exc:
            call(**kw)
        assert exc.value.status == _ffi.E_INVALID, text
    # nfreq < 0 cannot be said through the wrapper
    status = h.lib.nodal_ac_sweep(h._h, 0, -1, None, 0, None, None, None, None, 0, None, None, None, 0, None, None, None, 0,
                                  None, None, 0, None, None, None, None, None)
    assert status == _ffi.E_INVALID and b"number of frequencies" in h.lib.nodal_last_error(h._h)
    # nfreq == 0 does nothing, and the good call is good
    none = call(omega=[])
    assert none[0].shape == (0, 1) and none[4].shape == (0,)
    wave, cur, x, peak, resid, info = call()
    assert wave.shape == (2, 1) and cur.shape == (2, 1) and x is None and peak is None and (info == 0).all()
    assert (resid <= RESID_BAR).all()
    h.close()
