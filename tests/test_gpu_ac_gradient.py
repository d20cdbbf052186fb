"""Gradients through frequency on the GPU (Circuit.ac_gradient / nodal_ac_gradient / autograd.ac).  Every expected value
comes from tests/ac_gradient_reference.py -- the oracle's matrices, scipy's complex LU of the TRANSPOSED system and the
per-row formulas restated in numpy, and central differences of the reference's own forward sweep -- or from a closed form,
never from product code.

Bars: the complex parity bars of the reference (TOL = 1e-9 in every entry of x and y carried through the formulas, plus 8 eps of
the formula's scale) against its adjoint formulation; DEVICE_END_TO_END = ten times the disagreement the reference's two
formulations have on the CPU (6.3e-12, measured there) against its central differences; scaled_residual <= 1e-12 in both
columns, as in the AC suite."""
import math
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd import generators as gen
from nodal_amd.circuit import MatrixRankWarning
from nodal_amd.lowering import lower
from tests import ac_gradient_reference as agr
from tests import ac_reference as acr
from tests.ac_gradient_reference import DEVICE_END_TO_END, TOL
from tests.noise_reference import two_outputs
from tests.sensitivity_reference import T_A, T_E
from tests.test_gpu_ac import worst_ratio
from tests.test_gpu_branches import INPUTS, _island
from tests.test_gpu_transient_inductors import _grid_case, node_labels
from tests.transient_rl_reference import seeded_mix

pytestmark = pytest.mark.gpu

RESID_BAR = 1e-12
SPARSE = pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
FIELDS = ("values", "capacitors", "inductors", "source_terms", "phasors", "info", "scaled_residual", "adjoints", "work")


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_outputs(a, b):
    return all((getattr(a, f) is None and getattr(b, f) is None) or same_bits(getattr(a, f), getattr(b, f)) for f in FIELDS) \
        and a.sources.keys() == b.sources.keys() and all(same_bits(np.array(a.sources[k]), np.array(b.sources[k])) for k in a.sources)


def ratio(miss, bar):
    return miss / bar if bar > 0 else (0.0 if miss == 0 else np.inf)


def over_bars(got, want, bars):
    """the worst |got - want| over its bar (0 / 0 counts as 0)"""
    got, want, bars = np.asarray(got).ravel(), np.asarray(want).ravel(), np.asarray(bars).ravel()
    return max((ratio(abs(g - w), b) for g, w, b in zip(got, want, bars)), default=0.0)


def ulp_miss(got, want):
    """the largest |got - want| in units of the spacing of want, the parts of a complex array taken apart"""
    got, want = (np.ascontiguousarray(v).view(np.float64) if np.iscomplexobj(v) else np.asarray(v, dtype=np.float64) for v in (got, want))
    return float(np.max(np.abs(got - want) / np.spacing(np.abs(want)), initial=0.0))


def run(c, case, **kw):
    args = dict(frequencies=case.frequencies, cotangents=case.cotangents, capacitors=case.capacitors, inductors=case.inductors,
                sources=case.sources, probes=case.probes)
    args.update(kw)
    return c.ac_gradient(**args)


def reactive(g):
    return np.concatenate([g.capacitors, g.inductors])


def check_residuals(g, tag):
    worst = float(np.max(g.scaled_residual, initial=0.0))
    print(tag, "largest scaled residual", worst, "over the bar", worst / RESID_BAR)
    assert (g.info == 0).all(), tag
    assert g.scaled_residual.shape == (len(g), 2) and (g.scaled_residual <= RESID_BAR).all(), tag


def check_parity(case, g, tag):
    """all four gradient arrays within the complex parity bars of the adjoint reference, the exact zeros, the phasors"""
    r = case.ref
    misses = dict(values=over_bars(g.values, case.values, case.bars[0]), reactive=over_bars(reactive(g), case.react, case.bars[1]),
                  source_terms=over_bars(g.source_terms, case.terms, case.bars[2]))
    bar_of = {k: sum(case.bars[2][:, j].sum() for j, i in enumerate(case.source_rows.tolist()) if r.keys[i] == k) for k in case.by_name}
    misses["sources"] = max((ratio(abs(g.sources[k] - case.by_name[k]), bar_of[k]) for k in case.by_name), default=0.0)
    misses["phasors"] = worst_ratio(g.phasors, case.W)
    print(tag, "worst miss over the bar:", misses)
    assert g.values.shape == (r.ncomp,) and len(g.capacitors) == r.ncap and len(g.capacitors) + len(g.inductors) == len(case.react)
    assert g.source_terms.shape == case.terms.shape and g.phasors.shape == case.W.shape and set(g.sources) == set(case.by_name)
    assert np.array_equal(g.source_rows, case.source_rows)
    assert all(m <= 1.0 for m in misses.values()), (tag, misses)
    at = np.flatnonzero((r.type == T_A) | (r.type == T_E))
    assert (g.values[at] == 0.0).all() and not np.signbit(g.values[at]).any(), tag
    assert g.capacitors_by_name == dict(zip([e[0] for e in case.capacitors], g.capacitors.tolist()))
    assert g.inductors_by_name == dict(zip([e[0] for e in case.inductors], g.inductors.tolist()))


def check_end_to_end(case, g, tag):
    """all four gradient arrays within DEVICE_END_TO_END of the central differences"""
    d = agr.disagreement(case, g.values, reactive(g), g.sources)
    print(tag, "|device - central differences|", d, "over the bar", d / DEVICE_END_TO_END)
    assert d <= DEVICE_END_TO_END, (tag, d)


# ---- 1: the RC low-pass driven by an E source (2n = 6: the dense panel; a branch row: the transposed child) -----------
@SPARSE
def test_rc_lowpass(sparse):
    R, C, alpha = 2.0e3, 0.25e-6, 0.8 - 0.3j
    freqs = (1.0 / (2.0 * math.pi * R * C)) * np.logspace(-2, 2, 9)
    c = n.Circuit(n.Netlist.from_rows(acr.rc_lowpass_rows(R)), sparse=sparse)
    assert c._handle.n == 3
    W = acr.rc_lowpass_closed_form(freqs, R, C, alpha)[0]
    g = c.ac_gradient(freqs, 2.0 * W[:, None], [("c1", C, "out", "g")], sources={"e1": alpha}, probes=["out"])  # L = sum |W|^2
    check_residuals(g, "rc low-pass")
    h2, dR, dC = agr.rc_lowpass_derivatives(freqs, R, C)
    a2, keys = abs(alpha) ** 2, list(c.netlist.component_keys)
    want = (a2 * dR.sum(), a2 * dC.sum(), 2.0 * alpha * h2.sum())
    got = (g.values[keys.index("r1")], g.capacitors[0], g.sources["e1"])
    print("rc low-pass: relative miss over TOL (dL/dR, dL/dC, dL/dalpha)", [abs(a - b) / (TOL * abs(b)) for a, b in zip(got, want)])
    assert all(abs(a - b) <= TOL * abs(b) for a, b in zip(got, want))
    assert (np.abs(g.source_terms[:, 0] - 2.0 * alpha * h2) <= TOL * np.abs(2.0 * alpha * h2).max()).all()
    assert (np.abs(g.phasors[:, 0] - W) <= TOL * np.abs(W).max()).all()
    assert g.values[keys.index("e1")] == 0.0 and not np.signbit(g.values[keys.index("e1")])
    assert g.timings[1] == 0.0 and g.capacitors_by_name == {"c1": g.capacitors[0]} and len(g.inductors) == 0


# ---- 2: the series RLC across its resonance ---------------------------------------------------------------------------
@SPARSE
def test_series_rlc(sparse):
    R, L, C = 5.0, 2.0e-3, 0.5e-6
    f0 = 1.0 / (2.0 * math.pi * math.sqrt(L * C))
    freqs = f0 * np.array([0.5, 0.9, 0.99, 1.0, 1.01, 1.1, 2.0])
    c = n.Circuit(n.Netlist.from_rows(acr.series_rlc_rows(R)), sparse=sparse)
    va, vb, _ = acr.series_rlc_closed_form(freqs, R, L, C)
    W = va - vb  # the voltage across the resistor; L = sum |W|^2
    g = c.ac_gradient(freqs, 2.0 * W[:, None], [("c1", C, "b", "g")], [("l1", L, "in", "a")], sources={"e1": 1.0}, probes=[("a", "b")])
    check_residuals(g, "series rlc")
    _, dR, dL, dC = agr.series_rlc_derivatives(freqs, R, L, C)
    keys = list(c.netlist.component_keys)
    # the terms change sign at the resonance: each is good to TOL of its own size, the sum to TOL of the sum of the sizes
    for name, got, terms in (("dL/dL", g.inductors[0], dL), ("dL/dC", g.capacitors[0], dC), ("dL/dR", g.values[keys.index("r1")], dR)):
        print("series rlc:", name, got, "closed form", terms.sum(), "miss over the bar", abs(got - terms.sum()) / (TOL * np.abs(terms).sum()))
        assert abs(got - terms.sum()) <= TOL * np.abs(terms).sum(), name


# ---- 3: every input of the branches suite -----------------------------------------------------------------------------
def test_the_inputs_are_all_there():
    assert len(INPUTS) == 29


_RESULTS = {}


def _result_of(k, sparse):
    """the device's gradient of input k, computed once per path for the two tests below"""
    if (k, sparse) not in _RESULTS:
        case = agr.input_case(k)
        c = n.Circuit(n.Netlist.from_rows(case.rows), sparse=sparse)
        with warnings.catch_warnings():
            warnings.simplefilter("error", MatrixRankWarning)
            _RESULTS[(k, sparse)] = run(c, case)
    return agr.input_case(k), _RESULTS[(k, sparse)]


@SPARSE
@pytest.mark.parametrize("k", range(29), ids=[name for name, _ in INPUTS])
def test_every_input(k, sparse):
    case, g = _result_of(k, sparse)
    tag = f"{case.name} {'sparse' if sparse else 'dense'} (2n = {2 * case.ref.n}, sources {case.sources})"
    check_residuals(g, tag)
    check_parity(case, g, tag)
    # the route: only the sparse LU (sparse, 2n > 64) spends time in numeric factorisations of its own
    assert (g.timings[1] > 0.0) == (sparse and 2 * case.ref.n > 64), (tag, g.timings)


@SPARSE
@pytest.mark.parametrize("k", range(29), ids=[name for name, _ in INPUTS])
def test_every_input_end_to_end(k, sparse):
    case, g = _result_of(k, sparse)
    check_end_to_end(case, g, f"{case.name} {'sparse' if sparse else 'dense'}")


# ---- 4: grid(12) with two E sources: two branch rows, the sparse LU on both children ----------------------------------
GRID_FREQS = np.logspace(-4, 4, 9)


@pytest.fixture(scope="module")
def grid_case():
    rows, caps, inds = _grid_case(12, ["e1", "e2"], 5, seed=31)
    labels = node_labels(n.Netlist.from_rows(rows))
    # two probes share node labels[7], one lies between a node and itself
    probes = [labels[7], (labels[100], labels[7]), (labels[30], labels[30]), ("g", labels[64]), (labels[-1], labels[0])]
    return agr.case_of(rows, caps, inds, GRID_FREQS, probes, {"ld0": 1.0 - 0.5j, "e1": 0.25 + 2.0j}, seed=31)


@SPARSE
def test_two_branch_rows_on_both_children(grid_case, sparse):
    case = grid_case
    assert case.ref.n == 145 and case.ref.ac.base.B == 2 and len(case.probes) == 5
    c = n.Circuit(n.Netlist.from_rows(case.rows), sparse=sparse)
    g = run(c, case, adjoints=True)
    tag = f"grid(12) with two E sources, {'sparse' if sparse else 'dense'}"
    check_residuals(g, tag)
    check_parity(case, g, tag)
    check_end_to_end(case, g, tag)
    assert worst_ratio(g.adjoints, case.Y) <= 1.0
    assert (g.phasors[:, 2] == 0).all() and not np.signbit(g.phasors[:, 2].real).any()
    if sparse:  # one factorisation per child and frequency, and no column redone alone
        print(tag, "work", g.work)
        assert g.work[0] == 2 * len(GRID_FREQS), g.work
    sweep = c.ac(case.frequencies, case.capacitors, case.inductors, sources=case.sources, probes=case.probes)
    print(tag, "phasors against Circuit.ac's, over the bar", worst_ratio(g.phasors, sweep.phasors))
    assert worst_ratio(g.phasors, sweep.phasors) <= 1.0


# ---- 5: a passive grid: A^T = A, one factorisation serves both solves; several workgroups and a partial one ------------
@pytest.fixture(scope="module")
def passive_case():
    rows = list(gen.grid_rows(24)) + [["ld0", "A", "1", "40", "g"], ["ld1", "A", "0.5", "300", "77"]]
    caps, inds = seeded_mix(rows, 24)
    nl = n.Netlist.from_rows(rows)
    probes = two_outputs(nl) + [node_labels(nl)[200]]
    return agr.case_of(rows, caps, inds, agr.CASE_FREQS, probes, {"ld0": 1.0 - 0.5j, "ld1": 0.5j}, seed=24)


@SPARSE
def test_passive_grid(passive_case, sparse):
    case = passive_case
    assert case.ref.ac.base.B == 0 and case.ref.ncomp % 256 != 0 and case.ref.ncomp > 1024
    c = n.Circuit(n.Netlist.from_rows(case.rows), sparse=sparse)
    g = run(c, case)
    tag = f"grid(24) with A sources, {'sparse' if sparse else 'dense'}"
    check_residuals(g, tag)
    check_parity(case, g, tag)
    check_end_to_end(case, g, tag)
    if sparse:  # ONE factorisation serves forward and adjoint: a condition, not a measurement
        print(tag, "work", g.work)
        assert g.work[0] == len(case.frequencies), g.work


def test_the_symmetric_child_is_shared_in_both_directions(passive_case):
    case = passive_case
    others = (lambda x: x.ac(case.frequencies, case.capacitors, case.inductors, sources=case.sources, probes=case.probes),
              lambda x: x.noise(case.frequencies, case.capacitors, case.inductors, outputs=case.probes),
              lambda x: x.ac_ports(case.frequencies, case.probes[:2], case.capacitors, case.inductors))
    c = n.Circuit(n.Netlist.from_rows(case.rows), sparse=True)
    first = run(c, case)
    assert first.timings[0] > 0.0 and first.timings[1] > 0.0
    for other in others:
        assert other(c).timings[0] == 0.0
    assert run(c, case).timings[0] == 0.0
    for other in others:  # and the other way round
        c2 = n.Circuit(n.Netlist.from_rows(case.rows), sparse=True)
        assert other(c2).timings[0] > 0.0
        g = run(c2, case)
        assert g.timings[0] == 0.0 and same_outputs(g, first)


# ---- 6: kept work and determinism -------------------------------------------------------------------------------------
def test_kept_work_and_determinism(grid_case):
    case = grid_case
    nl = n.Netlist.from_rows(case.rows)
    c = n.Circuit(nl, sparse=True)
    first = run(c, case, adjoints=True)
    assert first.timings[0] > 0.0 and first.timings[1] > 0.0 and first.timings[2] > 0.0
    again = run(c, case, adjoints=True)
    assert again.timings[0] == 0.0 and same_outputs(first, again)
    # other values, frequencies, probes and cotangents on the same leads: nothing of the analysis is repeated
    labels = node_labels(nl)
    caps2 = [(name, 1.5 * value, a, b) for name, value, a, b in case.capacitors]
    inds2 = [(name, 0.5 * value, a, b) for name, value, a, b in case.inductors]
    other = agr.case_of(case.rows, caps2, inds2, [0.02, 3.0, 70.0], [labels[5], (labels[9], labels[100])], {"e2": 2.0}, seed=77, fd=False)
    g2 = run(c, other)
    assert g2.timings[0] == 0.0
    check_residuals(g2, "same leads, other values")
    check_parity(other, g2, "same leads, other values")
    # twice the cotangent is twice the gradient, to the bit or nearly
    twice = run(c, case, cotangents=2.0 * case.cotangents)
    for f in ("values", "capacitors", "inductors", "source_terms"):
        ulps = ulp_miss(getattr(twice, f), 2.0 * getattr(first, f))
        print("twice the cotangent:", f, "ulp", ulps)
        assert ulps <= 4.0, f
    assert same_bits(twice.phasors, first.phasors)
    # the circuit is left as it was: solve(), a transient run and ac() give the bits of a circuit that never ran the gradient
    fresh = n.Circuit(n.Netlist.from_rows(case.rows), sparse=True)
    assert same_bits(np.asarray(c.solve().result), np.asarray(fresh.solve().result))
    runs = [x.transient(case.capacitors[:7], 0.5, 4, probes=labels[:5], inductors=case.inductors[:2],
                        current_probes=[case.inductors[0][0]], keep_every=1) for x in (c, fresh)]
    for f in ("waveforms", "solutions", "currents", "final_currents", "scaled_residual"):
        assert same_bits(getattr(runs[0], f), getattr(runs[1], f)), f
    sweeps = [x.ac(case.frequencies, case.capacitors, case.inductors, sources={"e1": 1.0}, probes=labels[:4], keep_every=1)
              for x in (c, fresh)]
    for f in ("phasors", "solutions", "scaled_residual"):
        assert same_bits(getattr(sweeps[0], f), getattr(sweeps[1], f)), f
    assert same_outputs(first, run(c, case, adjoints=True))


# ---- 7: a singular network --------------------------------------------------------------------------------------------
def _singular_call(c, nl, freqs):
    probes = node_labels(nl)[:2]
    return c.ac_gradient(freqs, np.ones((len(freqs), 2), dtype=np.complex128), sources={"fa": 1.0}, probes=probes)


def test_singular_dense_raises():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=False)
    with pytest.raises(type(c._singular())):
        _singular_call(c, nl, [1.0, 2.0])


def test_singular_sparse_warns_once():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        g = _singular_call(c, nl, [1.0, 2.0, 4.0])
    assert sum(issubclass(i.category, MatrixRankWarning) for i in w) == 1
    assert (g.info > 0).all() and np.isnan(g.scaled_residual).all() and np.isnan(g.phasors).all()
    assert np.isnan(g.values).all() and len(g.capacitors) == 0 and len(g.inductors) == 0
    assert np.isnan(g.source_terms).all() and np.isnan(g.sources["fa"])
    caps = [("c1", 1.0, node_labels(nl)[0], "g")]
    inds = [("l1", 1.0, node_labels(nl)[1], "g")]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", MatrixRankWarning)
        g = c.ac_gradient([1.0], np.ones((1, 1), dtype=np.complex128), caps, inds, sources={"fa": 1.0}, probes=node_labels(nl)[:1])
    assert np.isnan(g.values).all() and np.isnan(g.capacitors).all() and np.isnan(g.inductors).all() and np.isnan(g.source_terms).all()


# ---- 8: argument errors -----------------------------------------------------------------------------------------------
def test_argument_errors_through_the_circuit():
    rows = dict(INPUTS)["random0"]
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    a, b = node_labels(nl)[:2]
    source = agr.ACGradientReference(rows).first_source()
    resistor = next(r[0] for r in rows if r[1] == "R")
    one = np.ones((1, 1), dtype=np.complex128)
    with pytest.raises(ValueError, match="frequencies"):
        c.ac_gradient([0.0], one, probes=[a])
    with pytest.raises(ValueError, match="farads"):
        c.ac_gradient([1.0], one, [("c1", -1.0, a, b)], probes=[a])
    with pytest.raises(ValueError, match="henries"):
        c.ac_gradient([1.0], one, inductors=[("l1", 0.0, a, b)], probes=[a])
    with pytest.raises(KeyError):
        c.ac_gradient([1.0], one, probes=["nowhere"])
    with pytest.raises(KeyError):
        c.ac_gradient([1.0], one, sources={"no such source": 1.0}, probes=[a])
    with pytest.raises(ValueError, match="independent sources"):
        c.ac_gradient([1.0], one, sources={resistor: 1.0}, probes=[a])
    with pytest.raises(TypeError, match="complex"):
        c.ac_gradient([1.0], np.ones((1, 1)), probes=[a])
    with pytest.raises(ValueError, match="shape"):
        c.ac_gradient([1.0, 2.0], one, probes=[a])
    with pytest.raises(ValueError, match="finite"):
        c.ac_gradient([1.0], one * np.nan, probes=[a])
    ncomp = len(nl.component_keys)
    empty = c.ac_gradient([], np.zeros((0, 2), dtype=np.complex128), [("c1", 1.0, a, b)], sources={source: 1.0}, probes=[a, b])
    assert len(empty) == 0 and empty.phasors.shape == (0, 2) and empty.source_terms.shape == (0, 1)
    assert same_bits(empty.values, np.zeros(ncomp)) and same_bits(empty.capacitors, np.zeros(1)) and empty.sources == {source: 0j}
    none = c.ac_gradient([2.0, 1.0], np.zeros((2, 0), dtype=np.complex128), [("c1", 1.0, a, b)], sources={source: 1.0}, probes=[], adjoints=True)
    assert none.phasors.shape == (2, 0) and (none.info == 0).all() and same_bits(none.values, np.zeros(ncomp))
    assert same_bits(none.source_terms, np.zeros((2, 1), dtype=np.complex128)) and same_bits(none.adjoints, np.zeros((2, c._handle.n), dtype=np.complex128))


def test_abi_refuses_bad_arguments():
    table = lower(n.Netlist.from_rows(dict(INPUTS)["random0"]))
    K = table.K
    types = np.asarray(table.type)
    a_row, r_row = int(np.flatnonzero(types == 1)[0]), int(np.flatnonzero(types == 0)[0])
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    good = dict(omega=[1.0, 2.0], kind=[0, 1], value=[1.0, 2.0], lead_a=[0, -1], lead_b=[-1, 1], rows=[a_row], amplitudes=[1.0 + 1j],
                ia=[0, 1], ib=[-1, 0], cot=np.ones((2, 2), dtype=np.complex128))

    def call(**kw):
        args = {**good, **kw}
        return h.ac_gradient(args["omega"], args["kind"], args["value"], args["lead_a"], args["lead_b"], args["rows"],
                             args["amplitudes"], args["ia"], args["ib"], args["cot"], dense=False, adjoints=True)

    with pytest.raises(_ffi.NodalHipError, match="assemble_numeric") as exc:
        call()
    assert exc.value.status == _ffi.E_INVALID
    h.assemble_numeric(0)
    nan, inf = float("nan"), float("inf")
    bad_cot = np.ones((2, 2), dtype=np.complex128)
    bad_cot[1, 0] = 1j * inf
    cases = [(dict(omega=[1.0, 0.0]), "angular frequency"), (dict(omega=[nan, 1.0]), "angular frequency"),
             (dict(kind=[0, 2]), "kind"), (dict(value=[1.0, 0.0]), "value"), (dict(value=[1.0, inf]), "value"),
             (dict(lead_a=[K, -1]), "lead out of range"), (dict(lead_a=[0, 1]), "both leads"),
             (dict(ia=[K, 1]), "probe node out of range"), (dict(ib=[-2, 0]), "probe node out of range"),
             (dict(rows=[table.ncomp]), "source row out of range"), (dict(rows=[r_row]), "not an independent source"),
             (dict(rows=[a_row, a_row], amplitudes=[1.0, 1.0]), "named twice"), (dict(cot=bad_cot), "cotangent that is not finite"),
             (dict(cot=np.full((2, 2), complex(nan, 0.0))), "cotangent that is not finite")]
    for kw, text in cases:
        with pytest.raises(_ffi.NodalHipError, match=text) as exc:
            call(**kw)
        assert exc.value.status == _ffi.E_INVALID and "ac gradient: " in str(exc.value), text
    # no cotangents at all, nfreq < 0: not to be said through the wrapper
    import ctypes as C
    one = (C.c_double * 2)(1.0, 2.0)
    node = (C.c_int32 * 1)(0)
    ground = (C.c_int32 * 1)(-1)
    args = [0, None, None, None, None, 0, None, None, None, 1, node, ground]
    rest = [None] * 4 + [0] + [None] * 4
    status = h.lib.nodal_ac_gradient(h._h, 0, 2, one, *args, None, *rest)
    assert status == _ffi.E_INVALID and b"no cotangents" in h.lib.nodal_last_error(h._h)
    status = h.lib.nodal_ac_gradient(h._h, 0, -1, None, *args, None, *rest)
    assert status == _ffi.E_INVALID and b"number of frequencies" in h.lib.nodal_last_error(h._h)
    # every output may be NULL
    cot = (C.c_double * 4)(1.0, 0.0, 0.5, -0.5)
    assert h.lib.nodal_ac_gradient(h._h, 0, 2, one, *args, cot, *rest) == _ffi.OK
    # nfreq == 0 and nprobe == 0 give zeros, and the good call is good
    none = call(omega=[], cot=np.zeros((0, 2), dtype=np.complex128))
    assert none[0].shape == (0, 2) and same_bits(none[1], np.zeros(table.ncomp)) and same_bits(none[2], np.zeros(2))
    none = call(ia=[], ib=[], cot=np.zeros((2, 0), dtype=np.complex128))
    assert none[0].shape == (2, 0) and (none[6] == 0).all() and same_bits(none[1], np.zeros(table.ncomp))
    assert same_bits(none[3], np.zeros((2, 1), dtype=np.complex128)) and same_bits(none[4], np.zeros((2, h.n), dtype=np.complex128))
    wave, grad, greact, gsrc, lam, resid, info, work = call()
    assert wave.shape == (2, 2) and grad.shape == (table.ncomp,) and greact.shape == (2,) and gsrc.shape == (2, 1)
    assert lam.shape == (2, h.n) and (info == 0).all() and (resid <= RESID_BAR).all() and np.isfinite(grad).all()
    assert work[0] == 4 and work[2] == 0  # (branch rows: one factorisation per child and frequency)
    h.close()


# ---- 9: autograd ------------------------------------------------------------------------------------------------------
def test_autograd_ac():
    torch = pytest.importorskip("torch")
    from nodal_amd import autograd
    case = agr.input_case([name for name, _ in INPUTS].index("random0"))
    c = n.Circuit(n.Netlist.from_rows(case.rows), sparse=True)
    held = np.array(c.values, dtype=np.float64)
    names = sorted(case.sources)
    values = torch.tensor(held, dtype=torch.float64, requires_grad=True)
    farads = torch.tensor([e[1] for e in case.capacitors], dtype=torch.float64, requires_grad=True)
    henries = torch.tensor([e[1] for e in case.inductors], dtype=torch.float64, requires_grad=True)
    amps = torch.tensor([case.sources[k] for k in names], dtype=torch.complex128, requires_grad=True)
    caps = [(e[0], farads[q], e[2], e[3]) for q, e in enumerate(case.capacitors)]
    inds = [(e[0], henries[q], e[2], e[3]) for q, e in enumerate(case.inductors)]
    W = autograd.ac(c, values, caps, inds, case.frequencies, names, amps, case.probes)
    assert W.dtype == torch.complex128 and tuple(W.shape) == case.W.shape
    assert worst_ratio(W.detach().numpy(), case.W) <= 1.0
    loss = (torch.from_numpy(case.weights) * (W - torch.from_numpy(case.targets)).abs() ** 2).sum()
    loss.backward(retain_graph=True)
    # the direct call gets the cotangent backward() was handed: dL/dRe W + j dL/dIm W as torch's own backward of the loss forms it
    cot = _cotangent_torch_formed(torch, case, W)
    assert worst_ratio(cot, 2.0 * case.weights * (W.detach().numpy() - case.targets)) <= 1.0
    direct = c.ac_gradient(case.frequencies, cot, case.capacitors, case.inductors, sources=case.sources, probes=case.probes)
    got = (values.grad.numpy().copy(), farads.grad.numpy().copy(), henries.grad.numpy().copy(), amps.grad.numpy().copy())
    want = (direct.values, direct.capacitors, direct.inductors, np.array([direct.sources[k] for k in names], dtype=np.complex128))
    assert all(same_bits(a, np.asarray(b)) for a, b in zip(got, want))
    # a second backward after set_values with other values puts the saved ones back
    c.set_values(1.25 * held)
    for t in (values, farads, henries, amps):
        t.grad = None
    loss.backward()
    assert np.array_equal(np.asarray(c.values), held)
    again = (values.grad.numpy(), farads.grad.numpy(), henries.grad.numpy(), amps.grad.numpy())
    assert all(same_bits(a, b) for a, b in zip(again, got))


def _cotangent_torch_formed(torch, case, W):
    """dL/dRe W + j dL/dIm W as torch's own backward of the loss forms it"""
    leaf = W.detach().clone().requires_grad_(True)
    ((torch.from_numpy(case.weights) * (leaf - torch.from_numpy(case.targets)).abs() ** 2).sum()).backward()
    return leaf.grad.numpy()
