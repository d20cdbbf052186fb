"""Gradients through time on the GPU (Circuit.transient_gradient / nodal_transient_gradient / autograd.transient).  Every
expected value comes from tests/transient_gradient_reference.py -- the oracle's matrices stepped backwards in numpy /
scipy, and central differences of its forward stepping -- never from product code.

Bars, all taken from the project:
  a  every backward step: info == 0 and scaled_residual <= 1e-12 (RESID_BAR of the forward tests);
  b  one step backwards: the reference steps the DEVICE's lambda_{k+1} back once and meets the device's lambda_k within
     2 TOL |lambda_k|_inf (check_one_step's rule);
  c  the accumulation alone: the formulas in numpy on the DEVICE's lambda and x, summed in the device's order, against
     grad (companion rows included), grad_sources and grad_x0.  Bar: rounding only, (steps + 4) EPS sum_k formulas_abs --
     `steps` roundings of the sum over the steps as in gradient_bars, and 4 for a term's own (two differences, the
     division, the product: the device forms D * (u / r^2), numpy D * u / r^2).  grad_sources: a difference of two
     entries of lambda, EPS |.|.  grad_x0: (terms + 3) EPS of its scale, `terms` the probes and capacitors on the node;
  d  end to end against the reference's OWN adjoint (its lambda, its x), passive networks only, per row
     steps (sum_k parity_bars + the rounding term): a passive network carries a step's error on without amplifying it;
  e  the public result against central differences of the reference on the small inputs: 10 x the disagreement of the
     two CPU formulations (tests/test_transient_gradient_frontend.py), relative to the largest entry of each array.
Seen on one MI355X (the worst over every test of this file): a 3.6e-15; b 4.2e-5 of its bar; c 0.11 of its bar for
grad, 0.0 for grad_sources (the same bits), 0.31 for grad_x0; d 1.0e-7 of its bar; e 7.1e-9 against the bar 7.2e-8 (the
central differences' own floor: the reference's adjoint misses them by the same 7.1e-9); the RC section 1.4e-15."""
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd import generators as gen
from nodal_amd.circuit import MatrixRankWarning
from nodal_amd.sweep import resolve_sources
from tests import transient_gradient_reference as tg
from tests import transient_reference as tref
from tests.test_gpu_branches import INPUTS
from tests.transient_gradient_reference import EPS, TOL, worst_ratio

pytestmark = pytest.mark.gpu

RESID_BAR = 1e-12


def device_run(rows, caps, dt, steps, sources, probes, sparse, initial=None):
    """(circuit, x_0, Transient with every solution kept): a recorded run"""
    c = n.Circuit(n.Netlist.from_rows([list(r) for r in rows]), sparse=sparse)
    x0 = np.array(c.solve().result) if initial is None else np.asarray(initial, dtype=np.float64)
    tr = c.transient(caps, dt, steps, sources=sources, probes=probes, initial=initial, keep_every=1, record=True)
    return c, x0, tr


def raw_gradient(c, cot, probes=None):
    """nodal_transient_gradient's own arrays for the recorded run: (grad with companion rows, grad_sources, grad_x0,
    adjoints, scaled residual, info)"""
    rec = c._transient_record
    pa, pb = (rec.pa, rec.pb) if probes is None else probes
    return rec.child._handle.transient_gradient(rec.steps, rec.nsrc, pa, pb, cot, dense=not c.sparse, adjoints=True)


def is_passive(r):
    t = r.r.table
    return t.B == 0 and bool((np.asarray(t.value)[np.asarray(t.type) == 0] > 0).all()) and bool((np.asarray(t.type) <= 1).all())


def check_device(r, x0, tr, raw, pairs, cot, table_rows, tag):
    """a, b and c for one recorded run and its raw gradient"""
    grad, gsrc, gx0, lam, resid, info = raw
    steps = len(cot) - 1
    # a
    print(tag, "largest backward scaled residual", float(np.max(resid, initial=0.0)))
    assert (info == 0).all() and (resid <= RESID_BAR).all(), tag
    # b
    want = r.one_step_back(lam, pairs, cot)
    worst = 0.0
    for k in range(1, steps + 1):
        bar = 2 * TOL * np.abs(lam[k - 1]).max()
        miss = np.abs(lam[k - 1] - want[k - 1]).max()
        worst = max(worst, miss / bar if bar > 0 else (0.0 if miss == 0 else np.inf))
    print(tag, "one step backwards, worst miss over the bar:", worst)
    assert worst <= 1.0, tag
    # c
    X = np.vstack([x0[None, :], tr.solutions]) if steps else x0[None, :]
    ratio = worst_ratio(grad, r.sums(lam, X), (steps + 4) * EPS * r.sums_abs(lam, X))
    ratio_s = worst_ratio(gsrc, r.sources(lam, table_rows), EPS * r.sources_abs(lam, table_rows))
    terms = np.zeros(r.n + 1)
    for a, b in list(pairs) + list(zip(r.r.ia, r.r.ib)):
        terms[a] += 1
        terms[b] += 1
    ratio_0 = worst_ratio(gx0, r.grad_x0(pairs, cot, lam), (terms[:r.n] + 3) * EPS * r.grad_x0_abs(pairs, cot, lam))
    print(tag, "formula parity, worst ratio grad / sources / x0:", ratio, ratio_s, ratio_0)
    assert max(ratio, ratio_s, ratio_0) <= 1.0, tag
    return ratio


def check_end_to_end(r, x0, sources, raw, pairs, cot, tag):
    """d: the reference's own forward and backward stepping"""
    grad = raw[0]
    steps = len(cot) - 1
    X = r.r.run(x0, r.r.rhs_steps(sources, steps))
    lam = r.adjoints(pairs, cot)
    bar = steps * (r.solution_bars(lam, X) + steps * EPS * r.sums_abs(lam, X))
    ratio = worst_ratio(grad, r.sums(lam, X), bar)
    print(tag, "end to end against the reference's own adjoint, worst ratio:", ratio)
    assert ratio <= 1.0, tag


def full_check(rows, caps, dt, steps, sources, probes, cot, sparse, tag, initial=None):
    r = tg.TransientGradientReference(rows, caps, dt)
    pairs = tg.probe_pairs(r.r.nl, probes)
    table_rows, _ = resolve_sources(r.r.nl, sources or {})
    with warnings.catch_warnings():
        warnings.simplefilter("error", MatrixRankWarning)
        c, x0, tr = device_run(rows, caps, dt, steps, sources, probes, sparse, initial)
        raw = raw_gradient(c, cot)
    check_device(r, x0, tr, raw, pairs, cot, table_rows, tag)
    if is_passive(r):
        check_end_to_end(r, x0, sources, raw, pairs, cot, tag)
    return c, r, raw


# ---- 1: every input of the branches suite, dense and sparse: every component type, the transposed child ------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("k", range(len(INPUTS)), ids=[i[0] for i in INPUTS])
def test_every_input(k, sparse):
    name, rows = INPUTS[k]
    caps, sources, probes, cot = tg.seeded_case(rows, 6, 7, k)
    full_check(rows, caps, 0.4, 6, sources, probes, cot, sparse, (name, sparse))


def test_the_inputs():
    assert len(INPUTS) == 29


# ---- 2: the sparse routes: one full block and a block of one / of two ---------------------------------------------------
@pytest.mark.parametrize("which", ["grid(12)", "cfg5(12)"])
def test_sparse_lu_routes(which):
    """grid(12) with two loads: 143 unknowns, passive -- the forward run's own factors serve the backward sweep;
    cfg5(12): 156 unknowns with branches -- the transposed child, factored once.  17 steps: blocks of 16 and 1."""
    rows = tg.small_grid_rows() if which == "grid(12)" else tg.cfg5_rows()
    caps, sources, probes, cot = tg.seeded_case(rows, 17, 7, 5)
    c, r, _ = full_check(rows, caps, 0.4, 17, sources, probes, cot, True, which)
    assert (r.n, is_passive(r)) == ((143, True) if which == "grid(12)" else (156, False))
    first = c._transient_record.child._handle.timings()[0]
    again = c.transient_gradient(2.0 * cot)
    print(which, "matrix work of the first backward sweep, ms:", first, "of the second:", again.timings[0])
    assert again.timings[0] == 0.0 and (first > 0.0) == (which == "cfg5(12)")


def test_multigrid_route():
    """grid(66): 4355 unknowns, passive, above the multigrid bound; a capacitor on every tenth node; 18 steps: blocks of
    16 and 2"""
    rows = list(gen.grid_rows(66))
    nl = n.Netlist.from_rows(rows)
    nodes = sorted(nl.nodenum, key=nl.nodenum.get)
    assert len(nodes) == 4355
    rng = np.random.default_rng(66)
    caps = [(f"cg{i}", float(rng.uniform(0.5, 2.0)), node, "g") for i, node in enumerate(nodes[::10])]
    _, sources, probes, cot = tg.seeded_case(rows, 18, 0, 66, caps=caps)
    c, r, _ = full_check(rows, caps, 0.4, 18, sources, probes, cot, True, "grid(66)")
    assert is_passive(r) and c.transient_gradient(cot).timings[0] == 0.0


# ---- 3: one RC section against the analytic derivatives ---------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("steps", [0, 1, 16])
def test_rc_section_analytic(steps, sparse):
    I, R, C, h = 0.7, 3.0, 0.02, 0.011
    rows, caps = tref.rc_rows(I, R), [("c1", C, "1", "g")]
    cot = np.random.default_rng(steps).uniform(-1.0, 1.0, size=(steps + 1, 1))
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=sparse)
    tr = c.transient(caps, h, steps, probes=["1"], initial=np.zeros(1), record=True)
    g = c.transient_gradient(cot)
    assert g.values.shape == (2,) and g.capacitors.shape == (1,) and g.initial.shape == (1,) and len(g) == steps
    assert g.source_values == {} and g.adjoints is None and tr.waveforms.shape == (steps + 1, 1)
    if steps == 0:
        assert not g.values.any() and not g.capacitors.any() and g.initial.tolist() == [cot[0, 0]]
        return
    dR, dC, dI = tg.rc_euler_derivatives(I, R, C, h, steps)
    want_v, want_c = np.array([cot[:, 0] @ dI, cot[:, 0] @ dR]), np.array([cot[:, 0] @ dC])
    miss = max(tg.relative_miss(g.values, want_v), tg.relative_miss(g.capacitors, want_c))
    print("RC section, steps", steps, "|device - closed form| / max:", miss, "bar", 2 * TOL * steps)
    assert miss <= 2 * TOL * steps  # (the forward tests' bar for the waveform at step k, through a bilinear formula)
    assert (g.info == 0).all() and (g.scaled_residual <= RESID_BAR).all()


# ---- 4: the public result against central differences, on the small inputs ------------------------------------------
def public_arrays(case, g, dc_start):
    values = np.array(g.values)
    swept = np.stack([g.source_values[name] for name in case.sources], axis=1) if case.sources else np.zeros((case.steps, 0))
    values[case.table_rows] -= swept.sum(axis=0)  # (no step uses the table value of a swept source)
    return values[case.subset], g.capacitors, swept, None if dc_start else g.initial[case.entries]


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("dc_start", [True, False], ids=["dc", "initial"])
@pytest.mark.parametrize("k", range(26))
def test_against_central_differences(k, dc_start, sparse):
    """e.  Case 23 is the edge network: two capacitors in parallel, one with its ground lead first, a node with
    capacitors and no probe and the reverse, probes to ground in either orientation, two probes on one node, a probe
    with a == b; dc_start False is `initial=` given (no DC chain, `initial` is an answer), True the DC start."""
    case = tg.small_case(k, dc_start)
    c = n.Circuit(n.Netlist.from_rows(case.rows), sparse=sparse)
    if dc_start:
        c.solve()
    c.transient(case.capacitors, tg.DT, case.steps, sources=case.sources, probes=case.probes, initial=case.initial, record=True)
    g = c.transient_gradient(case.cotangents)
    worst = tg.disagreement(public_arrays(case, g, dc_start), case.fd)
    print(case.name, "dc" if dc_start else "initial", sparse, "|device - central differences| / max:", worst,
          "the reference's own:", tg.disagreement(case.adjoint, case.fd))
    assert worst <= tg.DEVICE_END_TO_END, case.name


# ---- 5: edges of the lists and of the cotangents ------------------------------------------------------------------------
def _edge_run(sparse, initial):
    rows = tg.edge_rows()
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=sparse)
    x0 = np.array(c.solve().result)
    sources = {"a1": np.linspace(-1.0, 2.0, 5), "e1": np.linspace(0.5, 1.5, 5)}
    tr = c.transient(tg.EDGE_CAPACITORS, 0.4, 5, sources=sources, probes=tg.EDGE_PROBES, keep_every=1,
                     initial=x0 if initial else None, record=True)
    return c, x0, tr, sources


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_edges_formula_parity_and_special_cotangents(sparse):
    rows = tg.edge_rows()
    r = tg.TransientGradientReference(rows, tg.EDGE_CAPACITORS, 0.4)
    pairs = tg.probe_pairs(r.r.nl, tg.EDGE_PROBES)
    assert pairs[4][0] == pairs[4][1] and pairs[1][0] == -1 and pairs[0][1] == -1
    c, x0, tr, sources = _edge_run(sparse, True)
    table_rows, _ = resolve_sources(r.r.nl, sources)
    rng = np.random.default_rng(7)
    cot = rng.uniform(-1.0, 1.0, size=(6, len(pairs)))
    raw = raw_gradient(c, cot)
    check_device(r, x0, tr, raw, pairs, cot, table_rows, ("edges", sparse))
    # the cotangent of a probe between a node and itself changes nothing, bit for bit
    other = cot.copy()
    other[:, 4] = rng.uniform(-9.0, 9.0, size=6)
    for got, was in zip(raw_gradient(c, other)[:4], raw[:4]):
        assert np.array_equal(got, was)
    # zero except at row 0: no step has an adjoint to speak of -- dL/dx_0 = c_0 exactly, everything else exactly zero
    first = np.zeros_like(cot)
    first[0] = cot[0]
    g = c.transient_gradient(first)
    assert not g.values.any() and not g.capacitors.any() and not any(v.any() for v in g.source_values.values())
    assert np.array_equal(g.initial, r.seed(pairs, cot[0])) and g.initial.any()
    # zero except at the last step: every lambda_k is alive through the history alone
    last = np.zeros_like(cot)
    last[-1] = cot[-1]
    raw_last = raw_gradient(c, last)
    assert all(np.abs(l).max() > 0 for l in raw_last[3])
    check_device(r, x0, tr, raw_last, pairs, last, table_rows, ("edges, last step only", sparse))


def test_initial_given_against_the_dc_start():
    """the same x_0 handed over as `initial` and reached as the DC point: the same waveforms and adjoints, `initial` the
    same; `values` differ by exactly the DC chain, Circuit.gradient of dL/dx_0"""
    cot = np.random.default_rng(3).uniform(-1.0, 1.0, size=(6, len(tg.EDGE_PROBES)))
    c1, x0, tr1, _ = _edge_run(True, True)
    g1 = c1.transient_gradient(cot, adjoints=True)
    c2, _, tr2, _ = _edge_run(True, False)
    g2 = c2.transient_gradient(cot, adjoints=True)
    assert np.array_equal(tr1.waveforms, tr2.waveforms) and np.array_equal(g1.adjoints, g2.adjoints)
    assert np.array_equal(g1.initial, g2.initial) and np.array_equal(g1.capacitors, g2.capacitors)
    chain = c2.gradient(g2.initial, solutions=x0).values
    assert chain.any() and np.array_equal(g2.values, g1.values + chain)


# ---- 6: the contract ----------------------------------------------------------------------------------------------------
def test_contract_of_the_record():
    rows = tg.small_grid_rows()
    caps, sources, probes, cot = tg.seeded_case(rows, 17, 7, 5)
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    c.solve()
    kw = dict(sources=sources, probes=probes, keep_every=2, envelope=True)
    with pytest.raises(ValueError, match="no recorded transient"):
        c.transient_gradient(cot)
    plain = c.transient(caps, 0.4, 17, **kw)
    with pytest.raises(ValueError, match="no recorded transient: call transient\\(..., record=True\\) first"):
        c.transient_gradient(cot)
    # recording changes no bit of the forward results
    rec = c.transient(caps, 0.4, 17, record=True, **kw)
    assert np.array_equal(rec.waveforms, plain.waveforms) and np.array_equal(rec.solutions, plain.solutions)
    for key in ("potential_min", "potential_min_step", "potential_max", "potential_max_step"):
        assert np.array_equal(getattr(rec.envelope, key), getattr(plain.envelope, key))
    assert np.array_equal(rec.scaled_residual, plain.scaled_residual)
    # two calls give the same bits; a second call repeats no matrix work; the next forward run is unchanged
    g1 = c.transient_gradient(cot, adjoints=True)
    g2 = c.transient_gradient(cot, adjoints=True)
    for key in ("values", "capacitors", "initial", "adjoints", "scaled_residual"):
        assert np.array_equal(getattr(g1, key), getattr(g2, key)), key
    assert all(np.array_equal(g1.source_values[s], g2.source_values[s]) for s in sources)
    g3 = c.transient_gradient(-3.0 * cot)
    assert g3.timings[0] == 0.0 and not np.array_equal(g3.values, g1.values)
    with pytest.raises(ValueError, match="shape"):
        c.transient_gradient(cot[:-1])
    with pytest.raises(ValueError, match="shape"):
        c.transient_gradient(cot, probes=probes[:2])
    one = c.transient_gradient(cot[:, :2], probes=probes[:2])  # (other probes than the recorded call's)
    assert np.isfinite(one.values).all()
    after = c.transient(caps, 0.4, 17, **kw)
    assert np.array_equal(after.waveforms, plain.waveforms) and np.array_equal(after.solutions, plain.solutions)
    with pytest.raises(ValueError, match="no recorded transient"):  # (the call above did not record)
        c.transient_gradient(cot)
    # another dt replaces the record
    c.transient(caps, 0.4, 17, record=True, **kw)
    c.transient(caps, 0.2, 17, record=True, **kw)
    g4 = c.transient_gradient(cot)
    r = tg.TransientGradientReference(rows, caps, 0.2)
    pairs = tg.probe_pairs(r.r.nl, probes)
    check_end_to_end(r, np.array(c.solve().result), sources, raw_gradient(c, cot), pairs, cot, "dt replaced")
    assert not np.array_equal(g4.capacitors, g1.capacitors)
    # set_values() voids it
    c.set_values(np.array(c.values))
    with pytest.raises(ValueError, match="no recorded transient"):
        c.transient_gradient(cot)


def test_no_tape_on_the_handle_is_invalid():
    c = n.Circuit(n.Netlist.from_rows(tref.rc_rows(0.7, 3.0)), sparse=True)
    h = c._handle
    with pytest.raises(_ffi.NodalHipError) as exc:
        h.transient_gradient(0, 0, [0], [-1], np.zeros((1, 1)), dense=False)
    assert exc.value.status == _ffi.E_INVALID
    # a recorded run, then a new numeric assembly: void again; so is a probe out of range on a valid tape
    c.transient([("c1", 0.02, "1", "g")], 0.011, 3, probes=["1"], initial=np.zeros(1), record=True)
    ch = c._transient_record.child._handle
    with pytest.raises(_ffi.NodalHipError) as exc:
        ch.transient_gradient(3, 0, [1], [-1], np.zeros((4, 1)), dense=False)
    assert exc.value.status == _ffi.E_INVALID and "probe" in str(exc.value)
    assert ch.transient_gradient(3, 0, [0], [-1], np.ones((4, 1)), dense=False)[5].tolist() == [0, 0, 0]
    ch.assemble_numeric(0)
    with pytest.raises(_ffi.NodalHipError) as exc:
        ch.transient_gradient(3, 0, [0], [-1], np.ones((4, 1)), dense=False)
    assert exc.value.status == _ffi.E_INVALID and "no recorded transient" in str(exc.value)


# ---- 7: torch.autograd ------------------------------------------------------------------------------------------------
def test_autograd_transient():
    import torch
    from nodal_amd import autograd
    case = tg.small_case(23, True)  # the edge network from its DC start
    names = list(case.sources)
    c = n.Circuit(n.Netlist.from_rows(case.rows), sparse=True)
    values = torch.tensor(np.array(c.values), dtype=torch.float64, requires_grad=True)
    farads = torch.tensor([cap[1] for cap in case.capacitors], dtype=torch.float64, requires_grad=True)
    swept = torch.tensor(np.stack([case.sources[s] for s in names], axis=1), dtype=torch.float64, requires_grad=True)
    caps = [(cap[0], farads[j], cap[2], cap[3]) for j, cap in enumerate(case.capacitors)]
    wave = autograd.transient(c, values, caps, tg.DT, case.steps, names, swept, case.probes)
    assert wave.shape == (case.steps + 1, len(case.probes))
    cot = torch.tensor(case.cotangents)
    (wave * cot).sum().backward()
    g = c.transient_gradient(case.cotangents)
    want = np.array(g.values)
    want[case.table_rows] = g.start_values[case.table_rows]  # (a swept source's table value acts through the DC start alone)
    assert np.array_equal(values.grad.numpy(), want)
    assert np.array_equal(farads.grad.numpy(), g.capacitors)
    assert np.array_equal(swept.grad.numpy(), np.stack([g.source_values[s] for s in names], axis=1))
    # one composite loss, (wave[-1] - target)^2 summed over the probes, against central differences of the reference
    target = np.linspace(-0.5, 0.5, len(case.probes))
    for t in (values, farads, swept):
        t.grad = None
    wave = autograd.transient(c, values, caps, tg.DT, case.steps, names, swept, case.probes)
    ((wave[-1] - torch.tensor(target)) ** 2).sum().backward()
    fv, fc, fs, _ = tg.central_differences(lambda W: float(((W[-1] - target) ** 2).sum()), case.rows, case.capacitors, tg.DT,
                                           case.steps, case.sources, case.pairs, None)
    worst = max(tg.relative_miss(values.grad.numpy(), fv), tg.relative_miss(farads.grad.numpy(), fc),
                tg.relative_miss(swept.grad.numpy(), np.stack([fs[s] for s in names], axis=1)))
    print("autograd, composite loss, |device - central differences| / max:", worst)
    assert worst <= tg.DEVICE_END_TO_END
    # from `initial`, values.grad is zero at the swept rows: no step uses their table value
    values.grad = None
    x0 = np.array(c.solve().result)
    wave = autograd.transient(c, values, caps, tg.DT, case.steps, names, swept, case.probes, initial=x0)
    (wave * cot).sum().backward()
    assert not values.grad.numpy()[case.table_rows].any() and values.grad.numpy().any()
