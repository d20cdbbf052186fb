"""AC port analysis on the GPU (Circuit.ac_ports / nodal_ac_ports).  Every expected value comes from
tests/ac_port_reference.py -- the oracle's matrices and scipy's COMPLEX sparse LU, factored once per frequency, where the
device solves the interleaved real system -- or from a closed form, never from product code.

Bars: TOL = 1e-9, the project's normwise bar.  Every entry of Z at a frequency is held against TOL times the largest
magnitude among all unknowns of the reference's P solutions at that frequency (on one input of the branches suite every
port voltage vanishes identically and only a branch current is left to scale by; on the others this scale is at most 487
times max|Z|, and the two reference formulations agree five decades below TOL: tests/test_ac_ports_frontend.py).
scaled_residual <= RESID_BAR = 1e-12 per column and info == 0, as in tests/test_gpu_ac.py."""
import math
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd.circuit import MatrixRankWarning
from nodal_amd.lowering import lower
from tests import ac_port_reference as apr
from tests.ac_port_reference import GRID_FREQS, INPUT_FREQS
from tests.ac_reference import ACReference
from tests.test_gpu_branches import INPUTS, _island
from tests.test_gpu_transient_inductors import _grid_case, node_labels
from tests.transient_rl_reference import seeded_mix

pytestmark = pytest.mark.gpu

RESID_BAR = 1e-12
SPARSE = pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])


def check_residuals(sw, tag):
    worst = float(np.max(sw.scaled_residual, initial=0.0))
    print(tag, "largest scaled residual", worst, "over the bar", worst / RESID_BAR)
    assert (sw.info == 0).all(), tag
    assert (sw.scaled_residual <= RESID_BAR).all(), tag


def check_parity(sw, X, Z, tag):
    """sw.z against the reference's Z [F, P, P], the bar scaled by its solutions X [F, n, P]"""
    assert sw.z.shape == Z.shape and sw.z.dtype == np.complex128, tag
    miss = apr.worst_ratio(sw.z, Z, X)
    print(tag, "worst miss of Z over the bar", miss)
    assert miss <= 1.0, tag


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_outputs(a, b):
    return all(same_bits(getattr(a, f), getattr(b, f)) for f in ("z", "info", "scaled_residual"))


# ---- 1: the T-network (2n = 6: the dense panel) -----------------------------------------------------------------------
@SPARSE
def test_t_network(sparse):
    R1, R2, C = 3.0, 5.0, 0.25
    freqs = np.logspace(-2, 2, 9)
    c = n.Circuit(n.Netlist.from_rows(apr.t_network_rows(R1, R2)), sparse=sparse)
    assert c._handle.n == 3
    caps = [("c1", C, "m", "g")]
    sw = c.ac_ports(freqs, ["a", "b", ("a", "b"), ("a", "a")], caps)
    check_residuals(sw, "t-network")
    assert sw.ports == [("a", "g"), ("b", "g"), ("a", "b"), ("a", "a")] and np.array_equal(sw.omega, 2.0 * math.pi * freqs)
    want = apr.t_network_closed_form(freqs, R1, R2, C)
    X, _ = apr.ACPortReference(ACReference(apr.t_network_rows(R1, R2), caps), ["a", "b"]).sweep(freqs)
    full = np.zeros((len(freqs), 4, 4), dtype=np.complex128)
    full[:, :2, :2] = want
    full[:, 2, :2] = want[:, 0, :] - want[:, 1, :]  # the difference port follows from the first two
    full[:, :2, 2] = want[:, :, 0] - want[:, :, 1]
    full[:, 2, 2] = want[:, 0, 0] - want[:, 0, 1] - want[:, 1, 0] + want[:, 1, 1]
    miss = apr.worst_ratio(sw.z, full, X)
    print("t-network: worst miss over the bar", miss)
    assert miss <= 1.0
    # a port between a node and itself: its row and its column are exactly +0.0 in both parts, bit for bit
    zeros = np.zeros((len(freqs), 4), dtype=np.complex128)
    assert same_bits(np.ascontiguousarray(sw.z[:, 3, :]), zeros) and same_bits(np.ascontiguousarray(sw.z[:, :, 3]), zeros)
    assert sw.work[1:] == (0, 0) and sw.peaks is None


# ---- 2: the parallel RLC tank through resonance -----------------------------------------------------------------------
@SPARSE
def test_rlc_tank(sparse):
    R, L, C = 40.0, 2.0, 0.125
    f0 = 1.0 / (2.0 * math.pi * math.sqrt(L * C))
    freqs = f0 * np.array([0.1, 0.5, 0.9, 0.99, 1.0, 1.01, 1.1, 2.0, 10.0])
    c = n.Circuit(n.Netlist.from_rows(apr.tank_rows(R)), sparse=sparse)
    caps, inds = [("c1", C, "t", "g")], [("l1", L, "t", "g")]
    sw = c.ac_ports(freqs, ["t"], caps, inds)
    check_residuals(sw, "rlc tank")
    want = apr.tank_closed_form(freqs, R, L, C)
    X, _ = apr.ACPortReference(ACReference(apr.tank_rows(R), caps, inds), ["t"]).sweep(freqs)
    miss = apr.worst_ratio(sw.z[:, 0, 0], want, X)
    print("rlc tank: worst miss over the bar", miss)
    assert miss <= 1.0
    mag, at = sw.peak_impedance()
    assert at.tolist() == [4] and abs(mag[0] - R) <= 1e-9 * R  # at resonance the tank is its resistor


# ---- 3: every input of the branches suite -----------------------------------------------------------------------------
_REFERENCES = {}


def _reference_of(k):
    """the reference of input k with its seeded elements and ports and its sweep, computed once for both paths"""
    if k not in _REFERENCES:
        name, rows = INPUTS[k]
        caps, inds = seeded_mix(rows, k)
        r = ACReference(rows, caps, inds)
        ports = apr.seeded_ports(r.nl, 5, 2000 + k)
        X, Z = apr.ACPortReference(r, ports).sweep(INPUT_FREQS)
        _REFERENCES[k] = (name, rows, caps, inds, r, ports, X, Z)
    return _REFERENCES[k]


@SPARSE
@pytest.mark.parametrize("k", range(29))
def test_every_input(k, sparse):
    assert len(INPUTS) == 29
    name, rows, caps, inds, r, ports, X, Z = _reference_of(k)
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=sparse)
    with warnings.catch_warnings():
        warnings.simplefilter("error", MatrixRankWarning)
        sw = c.ac_ports(INPUT_FREQS, ports, caps, inds)
    tag = f"{name} {'sparse' if sparse else 'dense'} (2n = {2 * r.n})"
    check_residuals(sw, tag)
    check_parity(sw, X, Z, tag)
    # the route: only the sparse LU (sparse, 2n > 64) spends time in numeric factorisations of its own
    lu = sparse and 2 * r.n > 64
    assert (sw.timings[1] > 0.0) == lu, (tag, sw.timings)
    if lu:
        assert sw.work == (3, 6, 0), (tag, sw.work)  # 2 applications x 3 frequencies x 1 block
    else:
        assert sw.work == (3, 0, 0), (tag, sw.work)  # one chunk per frequency


# ---- 4 .. 9: the sparse LU route on the grid case ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_case():
    rows, caps, inds = _grid_case(12, ["e1", "e2"], 5, seed=31)
    r = ACReference(rows, caps, inds)
    assert r.n == 145 and r.K == 143
    ports = apr.seeded_ports(r.nl, 33, 7)
    X, Z = apr.ACPortReference(r, ports).sweep(GRID_FREQS)
    return rows, caps, inds, r, ports, X, Z


def test_block_edges(grid_case):
    """a lone column, a full block, a block plus one column, two blocks plus one: a last block with one valid column is
    where stale columns of the block before it would show"""
    rows, caps, inds, r, ports, X, Z = grid_case
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    got = {}
    for P in (1, 16, 17, 33):
        sw = got[P] = c.ac_ports(GRID_FREQS, ports[:P], caps, inds)
        tag = f"grid(12), {P} ports"
        check_residuals(sw, tag)
        check_parity(sw, X[:, :, :P], Z[:, :P, :P], tag)
        assert sw.work == (17, 2 * 17 * math.ceil(P / 16), 0), (tag, sw.work)
    assert same_bits(np.ascontiguousarray(got[33].z[:, :16, :16]), got[16].z)
    # R, L, C and switched-off E sources: reciprocal.  Both of an entry pair are within the bar of the reference's
    rec = got[33].reciprocity()
    print("grid(12), 33 ports: largest reciprocity()", rec.max())
    top = np.abs(Z).max(axis=(1, 2))
    allowed = (2.0 * apr.TOL * apr.scales(X) + np.abs(Z - np.swapaxes(Z, 1, 2)).max(axis=(1, 2))) / (top - apr.TOL * apr.scales(X))
    assert rec.shape == (17,) and (rec <= allowed).all()


def test_redo_route(grid_case, monkeypatch):
    """NODAL_MULTI_BAR=-1: every column fails the bar and is redone alone; with the knob removed the call gives the bits
    of a call made before it was set"""
    rows, caps, inds, r, ports, X, Z = grid_case
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    freqs = GRID_FREQS[:5]
    before = c.ac_ports(freqs, ports[:17], caps, inds)
    monkeypatch.setenv("NODAL_MULTI_BAR", "-1")
    redone = c.ac_ports(freqs, ports[:17], caps, inds)
    monkeypatch.delenv("NODAL_MULTI_BAR")
    check_residuals(redone, "grid(12), every column redone")
    check_parity(redone, X[:5, :, :17], Z[:5, :17, :17], "grid(12), every column redone")
    assert redone.work[2] == 5 * 17 and before.work[2] == 0
    after = c.ac_ports(freqs, ports[:17], caps, inds)
    assert same_outputs(before, after) and after.work == before.work


def test_against_circuit_ac(grid_case):
    """the port across load ld0's nodes: a column of Z is what ac() gives for that source at 1 A (bits are not expected:
    single and block substitution differ)"""
    rows, caps, inds, r, ports, X, Z = grid_case
    a, b = next((row[3], row[4]) for row in rows if row[0] == "ld0")
    s = r.rhs({"ld0": 1.0}).real
    ia = apr._index(r.nl, a)
    assert abs(s[ia]) == 1.0 and np.count_nonzero(s) == 1 and b == r.nl.ground
    port = (a, b) if s[ia] > 0 else (b, a)  # the sign of the reference's right-hand side
    labels = node_labels(r.nl)
    others = [labels[7], (labels[100], labels[3]), (labels[60], labels[61])]
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    sw = c.ac_ports(GRID_FREQS, [port] + others, caps, inds)
    check_residuals(sw, "grid(12), the load's port")
    ac = c.ac(GRID_FREQS, caps, inds, sources={"ld0": 1.0}, probes=others)
    Xl = r.sweep(GRID_FREQS, {"ld0": 1.0})
    miss = apr.worst_ratio(sw.z[:, 1:, 0], ac.phasors, Xl[:, :, None])
    print("a column of Z against Circuit.ac: worst miss over the bar", miss)
    assert miss <= 1.0 and np.abs(ac.phasors).max() > 0


def test_no_reactive_elements(grid_case):
    rows, caps, inds, r, ports, X, Z = grid_case
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    freqs = [0.05, 1.0, 20.0]
    sw = c.ac_ports(freqs, ports[:17])
    check_residuals(sw, "grid(12), no reactive elements")
    dc = c.thevenin(ports[:17], sources=False)
    assert (dc.info == 0).all()
    Xr, _ = apr.ACPortReference(ACReference(rows), ports[:17]).sweep(freqs)
    want = np.repeat(dc.z[None, :, :], len(freqs), axis=0)
    re, im = apr.worst_ratio(sw.z.real, want, Xr), apr.worst_ratio(sw.z.imag, np.zeros_like(want), Xr)
    print("no reactive elements against thevenin: worst miss over the bar, real parts", re, "imaginary parts", im)
    assert re <= 1.0 and im <= 1.0


def test_node_peaks(grid_case):
    rows, caps, inds, r, ports, X, Z = grid_case
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    plain = c.ac_ports(GRID_FREQS, ports[:17], caps, inds)
    sw = c.ac_ports(GRID_FREQS, ports[:17], caps, inds, peaks=True)
    assert same_outputs(plain, sw) and plain.peaks is None and sw.work == plain.work
    K = r.K
    pk = sw.peaks
    assert pk.port.dtype == np.int32 and pk.frequency_index.dtype == np.int32
    assert pk.magnitude.shape == pk.port.shape == pk.frequency_index.shape == (K,)
    assert ((pk.port >= 0) & (pk.port < 17)).all() and ((pk.frequency_index >= 0) & (pk.frequency_index < 17)).all()
    mag = np.abs(X[:, :K, :17])  # [F, K, P]
    bar = apr.TOL * apr.scales(X[:, :, :17]).max()
    want = mag.max(axis=(0, 2))
    named = mag[pk.frequency_index, np.arange(K), pk.port]  # the reference at the (frequency, port) the device names
    print("node peaks: worst miss over the bar: magnitude", np.abs(pk.magnitude - want).max() / bar, "the named place",
          np.abs(named - want).max() / bar)
    assert (np.abs(pk.magnitude - want) <= bar).all()
    assert (np.abs(named - want) <= bar).all()  # (near ties may resolve either way, but the index is honest)


def test_kept_work_sharing_and_determinism(grid_case):
    rows, caps, inds, r, ports, X, Z = grid_case
    freqs = GRID_FREQS[:5]
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    first = c.ac_ports(freqs, ports[:17], caps, inds)
    assert first.timings[0] > 0.0 and first.timings[1] > 0.0 and first.timings[2] > 0.0
    again = c.ac_ports(freqs, ports[:17], caps, inds)
    assert again.timings[0] == 0.0 and same_outputs(first, again)
    # other values, frequencies and ports on the same leads: nothing of the analysis is repeated
    caps2 = [(name, 1.5 * value, a, b) for name, value, a, b in caps]
    inds2 = [(name, 0.5 * value, a, b) for name, value, a, b in inds]
    freqs2 = [0.02, 3.0, 70.0]
    other = c.ac_ports(freqs2, ports[20:29], caps2, inds2)
    assert other.timings[0] == 0.0
    check_residuals(other, "same leads, other values")
    X2, Z2 = apr.ACPortReference(ACReference(rows, caps2, inds2), ports[20:29]).sweep(freqs2)
    check_parity(other, X2, Z2, "same leads, other values")
    # pattern and analysis are shared with Circuit.ac in both directions
    probes = node_labels(r.nl)[:4]
    c1 = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    assert c1.ac(freqs, caps, inds, sources={"e1": 1.0}, probes=probes).timings[0] > 0.0
    shared = c1.ac_ports(freqs, ports[:17], caps, inds)
    assert shared.timings[0] == 0.0 and same_outputs(first, shared)
    c2 = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    assert c2.ac_ports(freqs, ports[:17], caps, inds).timings[0] > 0.0
    assert c2.ac(freqs, caps, inds, sources={"e1": 1.0}, probes=probes).timings[0] == 0.0
    # the circuit is left as it was: solve() and an ac() sweep give the bits of a circuit that never ran ac_ports()
    fresh = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    assert same_bits(np.asarray(c.solve().result), np.asarray(fresh.solve().result))
    sweeps = [x.ac(freqs, caps, inds, sources={"e1": 1.0, "ld0": 2j}, probes=probes, current_probes=[caps[0][0], inds[0][0]],
                   keep_every=1) for x in (c, fresh)]
    for f in ("phasors", "currents", "solutions", "info", "scaled_residual"):
        assert same_bits(getattr(sweeps[0], f), getattr(sweeps[1], f)), f
    assert same_outputs(first, c.ac_ports(freqs, ports[:17], caps, inds))


# ---- 10: singular networks --------------------------------------------------------------------------------------------
def test_singular_dense_raises():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=False)
    with pytest.raises(type(c._singular())):
        c.ac_ports([1.0, 2.0], node_labels(nl)[:2])


def test_singular_sparse_warns_once():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sw = c.ac_ports([1.0, 2.0, 4.0], node_labels(nl)[:3], peaks=True)
    assert sum(issubclass(i.category, MatrixRankWarning) for i in w) == 1
    assert (sw.info > 0).all() and np.isnan(sw.scaled_residual).all() and np.isnan(sw.z).all()
    assert np.isnan(sw.peaks.magnitude).all() and (sw.peaks.port == -1).all() and (sw.peaks.frequency_index == -1).all()
    assert np.isnan(sw.reciprocity()).all() and np.isnan(sw.y()).all()


# ---- 11: argument errors ----------------------------------------------------------------------------------------------
def test_argument_errors_through_the_circuit():
    rows = dict(INPUTS)["random0"]
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    a, b = node_labels(nl)[:2]
    with pytest.raises(ValueError, match="frequencies"):
        c.ac_ports([0.0], [a])
    with pytest.raises(ValueError, match="Port"):
        c.ac_ports([1.0], [(a, b, a)])
    with pytest.raises(KeyError):
        c.ac_ports([1.0], ["nowhere"])
    with pytest.raises(ValueError, match="farads"):
        c.ac_ports([1.0], [a], [("c1", -1.0, a, b)])
    with pytest.raises(ValueError, match="given twice"):
        c.ac_ports([1.0], [a], [("x", 1.0, a, b)], [("x", 1.0, a, b)])
    with pytest.raises(KeyError):
        c.ac_ports([1.0], [a], [("c1", 1.0, a, "nowhere")])
    with pytest.raises(TypeError):
        c.ac_ports([1.0])
    none = c.ac_ports([1.0, 2.0], [], [("c1", 1.0, a, b)], peaks=True)
    assert none.z.shape == (2, 0, 0) and none.scaled_residual.shape == (2, 0) and (none.info == 0).all()
    assert np.isnan(none.peaks.magnitude).all() and (none.peaks.port == -1).all() and none.work == (0, 0, 0)
    empty = c.ac_ports([], [a, (a, b)], [("c1", 1.0, a, b)])
    assert len(empty) == 0 and empty.z.shape == (0, 2, 2) and empty.scaled_residual.shape == (0, 2)
    # two identical ports are legal: four times the same driving-point impedance
    twice = c.ac_ports([1.0], [(a, b), (a, b)], [("c1", 1.0, a, b)])
    assert (twice.info == 0).all() and abs(twice.z[0, 0, 0]) > 0
    assert np.abs(twice.z[0] - twice.z[0, 0, 0]).max() <= 1e-9 * abs(twice.z[0, 0, 0])


def test_abi_refuses_bad_arguments():
    table = lower(n.Netlist.from_rows(dict(INPUTS)["random0"]))
    K = table.K
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    good = dict(omega=[1.0, 2.0], kind=[0, 1], value=[1.0, 2.0], lead_a=[0, -1], lead_b=[-1, 1], ia=[0, 1], ib=[-1, 0])

    def call(**kw):
        args = {**good, **kw}
        return h.ac_ports(args["omega"], args["kind"], args["value"], args["lead_a"], args["lead_b"], args["ia"], args["ib"],
                          dense=False, peaks=kw.get("peaks", False))

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
             (dict(ia=[K, 1]), "port node out of range"), (dict(ib=[-1, -2]), "port node out of range")]
    for kw, text in cases:
        with pytest.raises(_ffi.NodalHipError, match=text) as exc:
            call(**kw)
        assert exc.value.status == _ffi.E_INVALID, text
    # nfreq < 0 and nports < 0 cannot be said through the wrapper
    status = h.lib.nodal_ac_ports(h._h, 0, -1, None, 0, None, None, None, None, 0, None, None, None, None, None, None, None,
                                  None, None)
    assert status == _ffi.E_INVALID and b"number of frequencies" in h.lib.nodal_last_error(h._h)
    status = h.lib.nodal_ac_ports(h._h, 0, 0, None, 0, None, None, None, None, -1, None, None, None, None, None, None, None,
                                  None, None)
    assert status == _ffi.E_INVALID and b"number of ports" in h.lib.nodal_last_error(h._h)
    # nfreq == 0 and nports == 0 do nothing, and the good call is good
    z, peak, resid, info, work = call(omega=[])
    assert z.shape == (0, 2, 2) and resid.shape == (0, 2) and work.tolist() == [0, 0, 0]
    z, peak, resid, info, work = call(ia=[], ib=[], peaks=True)
    assert z.shape == (2, 0, 0) and (info == 0).all() and np.isnan(peak[0]).all() and work.tolist() == [0, 0, 0]
    z, peak, resid, info, work = call(peaks=True)
    assert z.shape == (2, 2, 2) and (info == 0).all() and (resid <= RESID_BAR).all() and np.isfinite(z).all()
    assert np.isfinite(peak[0]).all() and peak[1].dtype == peak[2].dtype == np.int32 and work[0] == 2
    h.close()
