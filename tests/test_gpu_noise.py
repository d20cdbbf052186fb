"""Noise analysis on the GPU (Circuit.noise / nodal_ac_noise).  Every expected value comes from tests/noise_reference.py
-- the oracle's matrices and scipy's complex sparse LU of the TRANSPOSED system, where the device solves the interleaved
real one -- or from a closed form, never from product code.

Bars: TOL = 1e-9, the project's normwise bar, as tests/noise_reference.py states them: amplitude densities per frequency
against the largest expected one of that frequency's outputs, the contributions of a call against the call's largest,
gains against the largest |H| of the frequency; 0 / 0 counts as 0.  The reference's two formulations agree to 2.2e-15 /
5.4e-15 on the CPU (tests/test_noise_frontend.py), which leaves five decades.  scaled_residual <= RESID_BAR = 1e-12 for
every output of every frequency, as in the AC suite.

The AC suite has no network that is singular at one frequency only, so neither has this one."""
import math
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd import generators as gen
from nodal_amd.circuit import MatrixRankWarning
from nodal_amd.lowering import lower
from tests import noise_reference as nr
from tests.noise_reference import TOL
from tests.test_gpu_branches import INPUTS, _island
from tests.test_gpu_transient_inductors import _grid_case, node_labels
from tests.transient_rl_reference import seeded_mix

pytestmark = pytest.mark.gpu

RESID_BAR = 1e-12
T0 = 300.0
SPARSE = pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
INPUT_FREQS = [0.01, 0.3, 10.0]


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def same_outputs(a, b):
    fields = ("density", "gain", "input_density", "contributions", "info", "scaled_residual")
    return all((getattr(a, f) is None and getattr(b, f) is None) or same_bits(getattr(a, f), getattr(b, f)) for f in fields)


def check_residuals(sw, tag):
    worst = float(np.max(sw.scaled_residual, initial=0.0))
    print(tag, "largest scaled residual", worst, "over the bar", worst / RESID_BAR)
    assert (sw.info == 0).all(), tag
    assert sw.scaled_residual.shape == sw.density.shape and (sw.scaled_residual <= RESID_BAR).all(), tag


def single_source(r):
    """the first A / E source whose name the netlist defines once (the input of a gain), or None"""
    keys = list(r.nl.component_keys)
    return next((name for name in r.ac.source_names() if keys.count(name) == 1), None)


def check_parity(r, sw, freqs, want_c, want_gain, tag):
    """densities, integrated contributions, the exact zeros, gain and input-referred density against the reference"""
    want_density = nr.density(want_c)
    amp = nr.amplitude_miss(sw.density, want_density, TOL)
    con = nr.call_miss(sw.contributions, r.integrated_contributions(freqs, want_c), TOL)
    # (sqrt(S) to TOL of the largest sqrt(S) is S to 2 TOL of the largest S)
    integ = nr.call_miss(sw.integrated(), nr.trapezoid(freqs, want_density), 2.0 * TOL)
    print(tag, "worst miss over the bar: amplitude densities", amp, "contributions", con, "integrated", integ)
    assert sw.density.shape == want_density.shape and sw.contributions.shape == (want_density.shape[1], r.ncomp)
    assert amp <= 1.0 and con <= 1.0 and integ <= 1.0, tag
    quiet = np.setdiff1d(np.arange(r.ncomp), r.noisy)
    assert (sw.contributions[:, quiet] == 0.0).all() and not np.signbit(sw.contributions[:, quiet]).any(), tag
    assert (sw.density >= 0.0).all() and (sw.contributions >= 0.0).all(), tag
    if want_gain is None:
        assert sw.gain is None and sw.input_density is None
        return
    gm = nr.gain_miss(sw.gain, want_gain, TOL)
    print(tag, "worst miss over the bar: gains", gm)
    assert gm <= 1.0, tag
    with np.errstate(divide="ignore", invalid="ignore"):
        assert same_bits(sw.input_density, sw.density / (sw.gain.real * sw.gain.real + sw.gain.imag * sw.gain.imag))
    # the input-referred amplitude, where both factors are well above their bars: an output whose sqrt(S) and |H| are at
    # least a tenth of the frequency's largest has each to 10 TOL relative, the quotient to 20 TOL
    for f in range(len(freqs)):
        amp_w, h_w = np.sqrt(want_density[f]), np.abs(want_gain[f])
        for p in np.flatnonzero((amp_w >= 0.1 * amp_w.max()) & (h_w >= 0.1 * h_w.max()) & (h_w > 0)):
            want = amp_w[p] / h_w[p]
            assert abs(math.sqrt(sw.input_density[f, p]) - want) <= 20.0 * TOL * want, (tag, f, p)


# ---- 1: R parallel to C, no source (2n = 2: the dense panel) ----------------------------------------------------------
@SPARSE
def test_rc_parallel(sparse):
    R, C = 2.0e3, 0.25e-6
    freqs = (1.0 / (2.0 * math.pi * R * C)) * np.logspace(-2, 2, 9)
    c = n.Circuit(n.Netlist.from_rows(nr.rc_parallel_rows(R)), sparse=sparse)
    assert c._handle.n == 1
    sw = c.noise(freqs, [("c1", C, "out", "g")], outputs=["out"], temperature=T0, contributions=True)
    check_residuals(sw, "rc parallel")
    want = nr.rc_parallel_density(freqs, R, C, T0)
    print("rc parallel: worst relative miss over TOL", (np.abs(sw.density[:, 0] - want) / (TOL * want)).max())
    assert (np.abs(sw.density[:, 0] - want) <= TOL * want).all()
    # (over all frequencies the closed form integrates to k_B T / C; over these nine points only their trapezoid rule)
    total = nr.trapezoid(freqs, want[:, None])[0]
    assert abs(sw.integrated()[0] - total) <= TOL * total and abs(sw.rms()[0] - math.sqrt(total)) <= TOL * math.sqrt(total)
    assert abs(sw.contributions[0, 0] - total) <= TOL * total and sw.top(0, 3) == [("r1", sw.contributions[0, 0])]
    assert np.array_equal(sw.amplitude_density(), np.sqrt(sw.density)) and sw.gain is None and sw.input_density is None
    assert np.array_equal(sw.omega, 2.0 * math.pi * freqs) and len(sw) == 9
    # one resistor, one term in every sum: the density follows the temperature to the rounding of its three products
    cold = c.noise(freqs, [("c1", C, "out", "g")], outputs=["out"], temperature=77.0)
    ulps = np.abs(cold.density - sw.density * (77.0 / T0)) / np.spacing(cold.density)
    print("rc parallel: density at 77 K against 77 / 300 of the density at 300 K, ulp", ulps.max())
    assert (ulps <= 4.0).all()


# ---- 2: a divider driven by an E source (a branch row: the transposed child) ------------------------------------------
@SPARSE
def test_divider(sparse):
    R1, R2 = 3.0e3, 1.0e3
    freqs = [1.0, 10.0, 100.0, 1000.0]
    c = n.Circuit(n.Netlist.from_rows(nr.divider_rows(R1, R2)), sparse=sparse)
    assert c._handle.n == 3
    sw = c.noise(freqs, outputs=["out", ("out", "out")], input="e1", temperature=T0, contributions=True)
    check_residuals(sw, "divider")
    S, H, (c1, c2) = nr.divider_closed_form(R1, R2, T0)
    assert (np.abs(sw.density[:, 0] - S) <= TOL * S).all()
    assert (np.abs(sw.gain[:, 0] - H) <= TOL * H).all()
    assert (np.abs(sw.input_density[:, 0] - S / H ** 2) <= 3.0 * TOL * S / H ** 2).all()  # (S to TOL, |H|^2 to 2 TOL)
    band = freqs[-1] - freqs[0]
    keys = list(c.netlist.component_keys)
    got = sw.contributions[0]
    assert c2 > c1  # (the call's largest contribution is r2's)
    assert abs(got[keys.index("r1")] - c1 * band) <= TOL * c2 * band and abs(got[keys.index("r2")] - c2 * band) <= TOL * c2 * band
    assert got[keys.index("e1")] == 0.0 and abs(c1 / c2 - R2 / R1) < 1e-12  # (R2^2 : R1^2 once scaled by 4 k_B T / R)
    assert [name for name, _ in sw.top(0, 2)] == ["r2", "r1"]
    # an output between a node and itself: exactly +0.0 everywhere
    zero = np.zeros(len(freqs))
    assert same_bits(sw.density[:, 1], zero) and same_bits(sw.contributions[1], np.zeros(len(keys)))
    assert (sw.gain[:, 1] == 0).all() and same_bits(sw.integrated()[1:], np.zeros(1))


# ---- 3: every input of the branches suite -----------------------------------------------------------------------------
def test_the_inputs_are_all_there():
    assert len(INPUTS) == 29


_REFERENCES = {}


def _reference_of(k):
    """the reference of input k with its seeded elements, outputs and input, computed once for both paths"""
    if k not in _REFERENCES:
        name, rows = INPUTS[k]
        caps, inds = seeded_mix(rows, k)
        r = nr.NoiseReference(rows, caps, inds)
        outputs, source = nr.two_outputs(r.nl), single_source(r)
        _REFERENCES[k] = (name, rows, caps, inds, r, outputs, source) + r.adjoint(INPUT_FREQS, outputs, T0, input=source)
    return _REFERENCES[k]


@SPARSE
@pytest.mark.parametrize("k", range(29))
def test_every_input(k, sparse):
    name, rows, caps, inds, r, outputs, source, want_c, want_gain = _reference_of(k)
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=sparse)
    with warnings.catch_warnings():
        warnings.simplefilter("error", MatrixRankWarning)
        sw = c.noise(INPUT_FREQS, caps, inds, outputs=outputs, input=source, temperature=T0, contributions=True)
    tag = f"{name} {'sparse' if sparse else 'dense'} (2n = {2 * r.n}, input {source})"
    check_residuals(sw, tag)
    check_parity(r, sw, INPUT_FREQS, want_c, want_gain, tag)
    # the route: only the sparse LU (sparse, 2n > 64) spends time in numeric factorisations of its own
    assert (sw.timings[1] > 0.0) == (sparse and 2 * r.n > 64), (tag, sw.timings)


# ---- 4: the sparse LU on the transposed child, across a block of sixteen outputs --------------------------------------
GRID_FREQS = np.logspace(-4, 4, 9)


@pytest.fixture(scope="module")
def grid_case():
    rows, caps, inds = _grid_case(12, ["e1", "e2"], 5, seed=31)
    r = nr.NoiseReference(rows, caps, inds)
    labels = nr.node_labels(r.nl)
    outputs = [labels[8 * i] for i in range(15)] + [(labels[-1], labels[0]), (labels[3], labels[60])]
    return rows, caps, inds, r, outputs


@SPARSE
def test_seventeen_outputs_on_the_transposed_child(grid_case, sparse):
    rows, caps, inds, r, outputs = grid_case
    assert r.n == 145 and r.ac.base.B == 2 and len(outputs) == 17
    want_c, want_gain = r.adjoint(GRID_FREQS, outputs, T0, input="e1")
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=sparse)
    sw = c.noise(GRID_FREQS, caps, inds, outputs=outputs, input="e1", temperature=T0, contributions=True)
    tag = f"grid(12) with two E sources, 17 outputs, {'sparse' if sparse else 'dense'}"
    check_residuals(sw, tag)
    check_parity(r, sw, GRID_FREQS, want_c, want_gain, tag)
    # an output alone gives the bits it has inside a block (the sparse LU solves and the table pass keep the outputs apart)
    if not sparse:
        return
    alone = c.noise(GRID_FREQS, caps, inds, outputs=outputs[16:], input="e1", temperature=T0, contributions=True)
    assert same_bits(alone.density[:, 0], sw.density[:, 16]) and same_bits(alone.contributions[0], sw.contributions[16])
    assert same_bits(alone.gain[:, 0], sw.gain[:, 16])


# ---- 5: a passive grid: the child shared with ac(), several workgroups and a partial one -------------------------------
@pytest.fixture(scope="module")
def passive_case():
    rows = list(gen.grid_rows(24)) + [["ld0", "A", "1", "40", "g"], ["ld1", "A", "0.5", "300", "77"]]
    caps, inds = seeded_mix(rows, 24)
    r = nr.NoiseReference(rows, caps, inds)
    return rows, caps, inds, r, nr.two_outputs(r.nl) + [nr.node_labels(r.nl)[200]]


@SPARSE
def test_passive_grid(passive_case, sparse):
    rows, caps, inds, r, outputs = passive_case
    assert r.ac.base.B == 0 and len(r.noisy) == 1104 and r.ncomp > 1104 and r.ncomp % 256 != 0
    want_c, want_gain = r.adjoint(INPUT_FREQS, outputs, T0, input="ld1")
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=sparse)
    sw = c.noise(INPUT_FREQS, caps, inds, outputs=outputs, input="ld1", temperature=T0, contributions=True)
    tag = f"grid(24) with A sources, {'sparse' if sparse else 'dense'}"
    check_residuals(sw, tag)
    check_parity(r, sw, INPUT_FREQS, want_c, want_gain, tag)


# ---- 6: kept work and determinism -------------------------------------------------------------------------------------
def test_the_symmetric_child_is_shared_with_ac(passive_case):
    rows, caps, inds, r, outputs = passive_case
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    first = c.ac(INPUT_FREQS, caps, inds, sources={"ld0": 1.0}, probes=outputs)
    assert first.timings[0] > 0.0
    sw = c.noise(INPUT_FREQS, caps, inds, outputs=outputs)
    assert sw.timings[0] == 0.0 and sw.timings[1] > 0.0
    after = c.ac(INPUT_FREQS, caps, inds, sources={"ld0": 1.0}, probes=outputs)
    assert after.timings[0] == 0.0 and same_bits(after.phasors, first.phasors)
    # and the other way round
    c2 = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    sw2 = c2.noise(INPUT_FREQS, caps, inds, outputs=outputs)
    assert sw2.timings[0] > 0.0 and same_outputs(sw, sw2)
    second = c2.ac(INPUT_FREQS, caps, inds, sources={"ld0": 1.0}, probes=outputs)
    assert second.timings[0] == 0.0 and same_bits(second.phasors, first.phasors)


def test_kept_work_and_determinism(grid_case):
    rows, caps, inds, r, outputs = grid_case
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    freqs = GRID_FREQS[2:7]

    def run(x, **kw):
        args = dict(frequencies=freqs, capacitors=caps, inductors=inds, outputs=outputs, input="e2", temperature=T0,
                    contributions=True)
        args.update(kw)
        return x.noise(**args)

    first = run(c)
    assert first.timings[0] > 0.0 and first.timings[1] > 0.0 and first.timings[2] > 0.0
    again = run(c)
    assert again.timings[0] == 0.0 and same_outputs(first, again)
    # a network that is not symmetric has a child of its own: ac() keeps its own work and takes none of this one's
    labels = node_labels(nl)
    sweep = c.ac(freqs, caps, inds, sources={"e1": 1.0}, probes=labels[:4], keep_every=1)
    assert sweep.timings[0] > 0.0 and run(c).timings[0] == 0.0
    # other values, frequencies, outputs and temperature on the same leads: nothing of the analysis is repeated
    caps2 = [(name, 1.5 * value, a, b) for name, value, a, b in caps]
    inds2 = [(name, 0.5 * value, a, b) for name, value, a, b in inds]
    freqs2, outputs2 = [0.02, 3.0, 70.0], [labels[5], (labels[9], labels[100])]
    other = run(c, frequencies=freqs2, capacitors=caps2, inductors=inds2, outputs=outputs2, temperature=77.0)
    assert other.timings[0] == 0.0
    check_residuals(other, "same leads, other values")
    r2 = nr.NoiseReference(rows, caps2, inds2)
    check_parity(r2, other, freqs2, *r2.adjoint(freqs2, outputs2, 77.0, input="e2"), "same leads, other values")
    # twice the temperature is twice the density, to the bit or nearly
    hot = run(c, temperature=2.0 * T0)
    ulps = np.abs(hot.density - 2.0 * first.density) / np.spacing(hot.density)
    print("density at 600 K against twice the density at 300 K, ulp", ulps.max())
    assert (ulps <= 4.0).all() and same_bits(hot.gain, first.gain)
    # the circuit is left as it was: solve(), a transient run and ac() give the bits of a circuit that never ran noise()
    fresh = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    assert same_bits(np.asarray(c.solve().result), np.asarray(fresh.solve().result))
    runs = [x.transient(caps[:7], 0.5, 4, probes=labels[:5], inductors=inds[:2], current_probes=[inds[0][0]], keep_every=1)
            for x in (c, fresh)]
    for f in ("waveforms", "solutions", "currents", "final_currents", "scaled_residual"):
        assert same_bits(getattr(runs[0], f), getattr(runs[1], f)), f
    sweeps = [x.ac(freqs, caps, inds, sources={"e1": 1.0}, probes=labels[:4], keep_every=1) for x in (c, fresh)]
    for f in ("phasors", "solutions", "scaled_residual"):
        assert same_bits(getattr(sweeps[0], f), getattr(sweeps[1], f)) and same_bits(getattr(sweeps[0], f), getattr(sweep, f)), f
    assert same_outputs(first, run(c))


# ---- 7: a singular network --------------------------------------------------------------------------------------------
def test_singular_dense_raises():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=False)
    with pytest.raises(type(c._singular())):
        c.noise([1.0, 2.0], outputs=node_labels(nl)[:1])


def test_singular_sparse_warns_once():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sw = c.noise([1.0, 2.0, 4.0], outputs=node_labels(nl)[:3], input="a1", contributions=True)
    assert sum(issubclass(i.category, MatrixRankWarning) for i in w) == 1
    assert (sw.info > 0).all() and np.isnan(sw.scaled_residual).all()
    assert np.isnan(sw.density).all() and np.isnan(sw.gain).all() and np.isnan(sw.input_density).all()
    assert np.isnan(sw.contributions).all() and np.isnan(sw.integrated()).all() and np.isnan(sw.rms()).all()


# ---- 8: argument errors -----------------------------------------------------------------------------------------------
def test_argument_errors_through_the_circuit():
    rows = dict(INPUTS)["random0"]
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    a, b = node_labels(nl)[:2]
    source = nr.NoiseReference(rows).ac.source_names()[0]
    resistor = next(r[0] for r in rows if r[1] == "R")
    with pytest.raises(ValueError, match="frequencies"):
        c.noise([0.0], outputs=[a])
    with pytest.raises(ValueError, match="temperature"):
        c.noise([1.0], outputs=[a], temperature=0.0)
    with pytest.raises(ValueError, match="temperature"):
        c.noise([1.0], outputs=[a], temperature=float("inf"))
    with pytest.raises(ValueError, match="strictly increasing"):
        c.noise([2.0, 1.0], outputs=[a], contributions=True)
    with pytest.raises(ValueError, match="farads"):
        c.noise([1.0], [("c1", -1.0, a, b)], outputs=[a])
    with pytest.raises(KeyError):
        c.noise([1.0], outputs=["nowhere"])
    with pytest.raises(KeyError):
        c.noise([1.0], outputs=[a], input="no such source")
    with pytest.raises(ValueError, match="independent sources"):
        c.noise([1.0], outputs=[a], input=resistor)
    with pytest.raises(TypeError):
        c.noise([1.0], outputs=[a], input=[source])
    empty = c.noise([], [("c1", 1.0, a, b)], outputs=[a, b], input=source, contributions=True)
    assert len(empty) == 0 and empty.density.shape == (0, 2) and empty.gain.shape == (0, 2)
    assert same_bits(empty.contributions, np.zeros((2, len(nl.component_keys)))) and same_bits(empty.integrated(), np.zeros(2))
    none = c.noise([2.0, 1.0], outputs=[], input=source)  # (decreasing frequencies are legal without an integral)
    assert none.density.shape == (2, 0) and (none.info == 0).all()


def test_abi_refuses_bad_arguments():
    table = lower(n.Netlist.from_rows(dict(INPUTS)["random0"]))
    K = table.K
    types = np.asarray(table.type)
    a_row, r_row = int(np.flatnonzero(types == 1)[0]), int(np.flatnonzero(types == 0)[0])
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    good = dict(omega=[1.0, 2.0], kind=[0, 1], value=[1.0, 2.0], lead_a=[0, -1], lead_b=[-1, 1], temperature=300.0, oa=[0, 1],
                ob=[-1, 0], input_row=a_row, weight=[0.5, 0.5])

    def call(**kw):
        args = {**good, **kw}
        return h.ac_noise(args["omega"], args["kind"], args["value"], args["lead_a"], args["lead_b"], args["temperature"],
                          args["oa"], args["ob"], dense=False, input_row=args["input_row"], weight=args["weight"])

    with pytest.raises(_ffi.NodalHipError, match="assemble_numeric") as exc:
        call()
    assert exc.value.status == _ffi.E_INVALID
    h.assemble_numeric(0)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(omega=[1.0, 0.0]), "angular frequency"), (dict(omega=[nan, 1.0]), "angular frequency"),
             (dict(kind=[0, 2]), "kind"), (dict(value=[1.0, 0.0]), "value"), (dict(value=[1.0, inf]), "value"),
             (dict(lead_a=[K, -1]), "lead out of range"), (dict(lead_a=[0, 1]), "both leads"),
             (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
             (dict(temperature=nan), "temperature"), (dict(temperature=inf), "temperature"),
             (dict(oa=[K, 1]), "output node out of range"), (dict(ob=[-2, 0]), "output node out of range"),
             (dict(input_row=table.ncomp), "input: source row out of range"), (dict(input_row=-2), "input: source row out of range"),
             (dict(input_row=r_row), "not an independent source")]
    for kw, text in cases:
        with pytest.raises(_ffi.NodalHipError, match=text) as exc:
            call(**kw)
        assert exc.value.status == _ffi.E_INVALID and "noise: " in str(exc.value), text
    # gain_out without an input, contrib_out without weight, nfreq < 0: not to be said through the wrapper
    import ctypes as C
    one = (C.c_double * 2)(1.0, 2.0)
    node = (C.c_int32 * 1)(0)
    ground = (C.c_int32 * 1)(-1)
    out = (C.c_double * (2 * table.ncomp + 8))()
    info = (C.c_int32 * 2)()
    status = h.lib.nodal_ac_noise(h._h, 0, 2, one, 0, None, None, None, None, 300.0, 1, node, ground, -1, None, None, out, None,
                                  None, info)
    assert status == _ffi.E_INVALID and b"no input source" in h.lib.nodal_last_error(h._h)
    status = h.lib.nodal_ac_noise(h._h, 0, 2, one, 0, None, None, None, None, 300.0, 1, node, ground, -1, None, None, None, out,
                                  None, info)
    assert status == _ffi.E_INVALID and b"without weights" in h.lib.nodal_last_error(h._h)
    status = h.lib.nodal_ac_noise(h._h, 0, -1, None, 0, None, None, None, None, 300.0, 0, None, None, -1, None, None, None, None,
                                  None, None)
    assert status == _ffi.E_INVALID and b"number of frequencies" in h.lib.nodal_last_error(h._h)
    # nfreq == 0 and nout == 0 do nothing, and the good call is good
    none = call(omega=[], weight=[])
    assert none[0].shape == (0, 2) and none[3].shape == (0, 2)
    none = call(oa=[], ob=[])
    assert none[0].shape == (2, 0) and (none[4] == 0).all()
    density, gain, contrib, resid, info = call()
    assert density.shape == (2, 2) and gain.shape == (2, 2) and contrib.shape == (2, table.ncomp) and (info == 0).all()
    assert (resid <= RESID_BAR).all() and (density > 0).all()
    h.close()
