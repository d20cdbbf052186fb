"""Transient analysis on the GPU (Circuit.transient / nodal_transient).  Every expected value comes from
tests/transient_reference.py -- the oracle's matrices stepped in numpy / scipy -- never from product code.

Bars: per step scaled_residual <= 1e-12 (the bar check_parity uses for the sweeps).  One-step parity: with keep_every=1
the reference advances the DEVICE's x_{k-1} by one step (trapezoidal: with the history rebuilt from the device's earlier
solutions) and must meet the device's x_k within 2 TOL |x_k|_inf -- errors cannot pile up.  Waveforms against the full
reference stepping on passive networks: within 2 TOL k max|x| at step k (each step's error is carried on by an operator
that does not amplify it for a passive network)."""
import random
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import generators as gen
from nodal_amd.circuit import MatrixRankWarning
from tests import transient_reference as ref
from tests.test_gpu_branches import INPUTS, _island
from tests.transient_reference import TOL

pytestmark = pytest.mark.gpu

RESID_BAR = 1e-12
METHODS = ["euler", "trapezoidal"]


def source_names(rows):
    return sorted({r[0] for r in rows if len(r) > 1 and r[1] in ("A", "E")})


def waveforms_of(names, steps, seed):
    rng = random.Random(seed)
    return {name: [rng.uniform(-5.0, 5.0) for _ in range(steps)] for name in names}


def check_residuals(tr, tag):
    worst = float(np.max(tr.scaled_residual, initial=0.0))
    print(tag, "largest scaled residual", worst, "over the bar", worst / RESID_BAR)
    assert (tr.info == 0).all(), tag
    assert (tr.scaled_residual <= RESID_BAR).all(), tag


def check_one_step(r, x0, tr, A_steps, tag):
    """the one-step parity of every step of a keep_every=1 run"""
    steps = len(A_steps)
    assert tr.solutions.shape == (steps, r.n) and tr.solution_steps.tolist() == list(range(1, steps + 1))
    X = np.vstack([np.asarray(x0, dtype=np.float64)[None, :], tr.solutions])
    want = r.one_step_from(X, A_steps)
    worst = 0.0
    for k in range(1, steps + 1):
        bar = 2 * TOL * np.abs(X[k]).max()
        miss = np.abs(X[k] - want[k - 1]).max()
        worst = max(worst, miss / bar if bar > 0 else (0.0 if miss == 0 else np.inf))
    print(tag, "one-step parity, worst miss over the bar:", worst)
    assert worst <= 1.0, tag
    check_residuals(tr, tag)
    return X


def check_waveforms(r, X_ref, tr, pairs, tag):
    """the waveforms against the full reference stepping: 2 TOL k max|x| at step k"""
    scale = np.abs(X_ref).max()
    xe = np.hstack([X_ref, np.zeros((len(X_ref), 1))])
    worst = 0.0
    for p, (a, b) in enumerate(pairs):
        want = xe[:, a] - xe[:, b]
        for k in range(1, len(X_ref)):
            worst = max(worst, abs(tr.waveforms[k, p] - want[k]) / (2 * TOL * k * scale))
    print(tag, "waveforms, worst miss over the bar:", worst)
    assert worst <= 1.0, tag


def device_run(rows, caps, dt, steps, method, sparse, sources=None, zero_start=False, **kw):
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    if zero_start:
        x0 = np.zeros(c._handle.n)
        tr = c.transient(caps, dt, steps, sources=sources, method=method, initial=x0, **kw)
    else:
        x0 = np.array(c.solve().result)
        tr = c.transient(caps, dt, steps, sources=sources, method=method, **kw)
    return c, x0, tr


# ---- 1: one RC section against the closed form (n = 1: the dense-per-step route) ----------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_rc_section_euler_closed_form(sparse):
    I, R, C, h, steps = 0.7, 3.0, 0.02, 0.011, 60
    _, _, tr = device_run(ref.rc_rows(I, R), [("c1", C, "1", "g")], h, steps, "euler", sparse, zero_start=True,
                          probes=["1"], keep_every=1)
    want = ref.rc_euler_closed_form(I, R, C, h, steps)
    assert tr.t.tolist() == (h * np.arange(steps + 1)).tolist() and tr.waveforms.shape == (steps + 1, 1)
    assert tr.waveforms[0, 0] == 0.0
    worst = np.max(np.abs(tr.waveforms[1:, 0] - want[1:]) / (2 * TOL * np.arange(1, steps + 1) * np.abs(want).max()))
    print("RC Euler against the closed form, worst miss over the bar:", worst)
    assert worst <= 1.0
    assert np.array_equal(tr.solutions[:, 0], tr.waveforms[1:, 0]) and (tr.iterations == 0).all()
    check_residuals(tr, "rc euler")


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_rc_section_trapezoidal_closed_form(sparse):
    I0, I1, R, C, h, steps = 0.7, -0.4, 3.0, 0.02, 0.011, 60
    _, x0, tr = device_run(ref.rc_rows(I0, R), [("c1", C, "1", "g")], h, steps, "trapezoidal", sparse,
                           sources={"a1": [I1] * steps}, probes=["1"])
    want = ref.rc_trapezoidal_closed_form(I0, I1, R, C, h, steps)
    assert tr.waveforms[0, 0] == x0[0] and tr.solutions is None
    worst = np.max(np.abs(tr.waveforms[1:, 0] - want[1:]) / (2 * TOL * np.arange(1, steps + 1) * np.abs(want).max()))
    print("RC trapezoidal against the closed form, worst miss over the bar:", worst)
    assert worst <= 1.0
    check_residuals(tr, "rc trapezoidal")


# ---- 2: every input of the branches suite, dense and sparse, both methods: one-step parity -----------------------
# the inputs that do not solve without a warning are left out by name, these and no others
LEFT_OUT = ()
SOLVABLE = [i for i in INPUTS if i[0] not in LEFT_OUT]


def test_the_inputs_left_out():
    assert len(LEFT_OUT) == 0 and len(SOLVABLE) == len(INPUTS) - len(LEFT_OUT) == 29


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("k", range(len(SOLVABLE)), ids=[i[0] for i in SOLVABLE])
def test_one_step_parity_on_every_input(k, sparse, method):
    name, rows = SOLVABLE[k]
    steps, dt = 20, 0.4
    caps = ref.seeded_capacitors(rows, 7, seed=k)
    sources = waveforms_of(source_names(rows), steps, seed=100 + k)
    with warnings.catch_warnings():
        warnings.simplefilter("error", MatrixRankWarning)  # (an input that warns belongs in LEFT_OUT)
        _, x0, tr = device_run(rows, caps, dt, steps, method, sparse, sources=sources, keep_every=1)
    r = ref.TransientReference(rows, caps, dt, method)
    check_one_step(r, x0, tr, r.rhs_steps(sources, steps), (name, sparse, method))


# ---- 3: steady state ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("which", ["grid(60)", "cfg5(24)"])
def test_steady_state(which, method):
    rows = dict(INPUTS)[which]
    caps = ref.seeded_capacitors(rows, 40, seed=9)
    _, x0, tr = device_run(rows, caps, 0.7, 12, method, True, keep_every=1)
    worst = np.abs(tr.solutions - x0).max() / (2 * TOL * np.abs(x0).max())
    print(which, method, "steady state, worst miss over the bar:", worst)
    assert worst <= 1.0
    check_residuals(tr, (which, method))


# ---- 4: no capacitors: every step is a DC solve -------------------------------------------------------------------
@pytest.mark.parametrize("which", ["random1", "grid(60)", "cfg5(24)"])
def test_no_capacitors_is_a_source_sweep(which):
    rows = dict(INPUTS)[which]
    steps = 9
    sources = waveforms_of(source_names(rows), steps, seed=4)
    c, _, tr = device_run(rows, [], 1.0, steps, "euler", True, sources=sources, keep_every=1)
    sw = c.solve_sources(sources)
    worst = max(np.abs(tr.solutions[m] - sw.result[m]).max() / (2 * TOL * np.abs(sw.result[m]).max()) for m in range(steps))
    print(which, "no capacitors against solve_sources, worst miss over the bar:", worst)
    assert worst <= 1.0
    check_residuals(tr, which)


# ---- 5: stiff limits on a small grid ------------------------------------------------------------------------------
def _small_grid():
    rows = list(gen.grid_rows(12)) + [["ld0", "A", "1", "40", "g"], ["ld1", "A", "1", "97", "g"]]
    nl = n.Netlist.from_rows(rows)
    rng = random.Random(2)
    caps = [(f"cg{i}", rng.uniform(0.5, 2.0), node, "g") for i, node in enumerate(sorted(nl.nodenum, key=nl.nodenum.get))]
    return rows, caps


def test_stiff_limit_long_steps():
    """dt six decades above every time constant: each Euler step is the DC solution of its sources.  From
    (G + C/h) x_k = A_k + C x_{k-1} / h:  x_k - G^-1 A_k = -G^-1 C (x_k - x_{k-1}) / h, so the step misses the DC solution
    by at most tau / h (|x_k| + |x_{k-1}|) with tau = |G^-1 C|_inf, the bound of every time constant of the network;
    the device adds its own 2 TOL |x_k|."""
    rows, caps = _small_grid()
    steps = 6
    r = ref.TransientReference(rows, caps, 1.0, "euler")
    tau = np.abs(np.linalg.solve(r.G.toarray(), r.capacitance().toarray())).sum(axis=1).max()
    dt = 1e6 * tau
    sources = waveforms_of(["a1", "ld0", "ld1"], steps, seed=8)
    _, x0, tr = device_run(rows, caps, dt, steps, "euler", True, sources=sources, keep_every=1)
    X = np.vstack([x0[None, :], tr.solutions])
    worst = 0.0
    for k, A_k in enumerate(r.rhs_steps(sources, steps), start=1):
        bar = 1e-6 * (np.abs(X[k]).max() + np.abs(X[k - 1]).max()) + 2 * TOL * np.abs(X[k]).max()
        worst = max(worst, np.abs(X[k] - r.dc(A_k)).max() / bar)
    print("long steps against the DC solutions, worst miss over the bar:", worst)
    assert worst <= 1.0
    check_residuals(tr, "long steps")


def test_stiff_limit_short_steps():
    """dt six decades below every node's own RC: the potentials hardly move.  x_k - x_{k-1} = (G + C/h)^-1 (A_k - G x_{k-1})
    and G + C/h is strictly diagonally dominant with a margin of at least min C / h (Varah), so a step moves no potential
    by more than h |A_k - G x_{k-1}|_inf / min C; the device adds its own 2 TOL |x_k|."""
    rows, caps = _small_grid()
    steps = 6
    r = ref.TransientReference(rows, caps, 1.0, "euler")
    cmin = min(c[1] for c in caps)
    dt = 1e-6 * cmin / r.G.diagonal().max()
    sources = waveforms_of(["a1", "ld0", "ld1"], steps, seed=8)
    _, x0, tr = device_run(rows, caps, dt, steps, "euler", True, sources=sources, keep_every=1)
    X = np.vstack([x0[None, :], tr.solutions])
    worst = 0.0
    for k, A_k in enumerate(r.rhs_steps(sources, steps), start=1):
        bar = dt * np.abs(A_k - r.G @ X[k - 1]).max() / cmin + 2 * TOL * np.abs(X[k]).max()
        worst = max(worst, np.abs(X[k] - X[k - 1]).max() / bar)
    print("short steps, the potentials' movement, worst over the bar:", worst)
    assert worst <= 1.0
    assert np.abs(X[-1] - x0).max() <= 1e-4 * np.abs(x0).max()  # (six steps of a millionth of an RC)
    rr = ref.TransientReference(rows, caps, dt, "euler")
    check_one_step(rr, x0, tr, rr.rhs_steps(sources, steps), "short steps")


# ---- 6: a star: more than sixteen capacitors on one node ----------------------------------------------------------
def test_star_of_forty_capacitors():
    rows, _ = _small_grid()
    rng = random.Random(6)
    others = [str(k) for k in rng.sample([k for k in range(1, 144) if k != 70], 36)]
    caps = [(f"cs{i}", rng.uniform(0.2, 3.0), "70", node) if i % 2 else (f"cs{i}", rng.uniform(0.2, 3.0), node, "70")
            for i, node in enumerate(others)]
    caps += [("par_a", 0.8, "70", others[0]), ("par_b", 1.3, "70", others[0]), ("gnd", 0.6, "70", "g"),
             ("rev", caps[3][1], caps[3][3], caps[3][2])]
    assert len(caps) == 40 and all("70" in (c[2], c[3]) for c in caps)
    steps, dt = 10, 0.3
    sources = waveforms_of(["a1", "ld0", "ld1"], steps, seed=12)
    for method in METHODS:
        c, x0, tr = device_run(rows, caps, dt, steps, method, True, sources=sources, keep_every=1, probes=["70"])
        r = ref.TransientReference(rows, caps, dt, method)
        check_one_step(r, x0, tr, r.rhs_steps(sources, steps), ("star", method))
        again = c.transient(caps, dt, steps, sources=sources, method=method, keep_every=1, probes=["70"])
        assert np.array_equal(again.solutions, tr.solutions) and np.array_equal(again.waveforms, tr.waveforms)
        assert np.array_equal(again.scaled_residual, tr.scaled_residual)


# ---- 7, 8: the multigrid route ------------------------------------------------------------------------------------
MG_STEPS = 33


@pytest.fixture(scope="module")
def grid100():
    N = 100
    rng = random.Random(5)
    rows = list(gen.grid_rows(N))
    picks = rng.sample(range(1, N * N - 1), 4)
    rows += [[f"ld{j}", "A", "1", str(k + 1), "g"] for j, k in enumerate(picks)]
    nl = n.Netlist.from_rows(rows)
    nodes = sorted(nl.nodenum, key=nl.nodenum.get)
    caps = [(f"cg{i}", rng.uniform(0.5, 2.0), node, "g") for i, node in enumerate(nodes)]
    caps += [(f"cc{i}", rng.uniform(0.5, 2.0), *rng.sample(nodes, 2)) for i in range(50)]
    sources = waveforms_of(["a1"] + [f"ld{j}" for j in range(4)], MG_STEPS, seed=21)
    out = {"rows": rows, "nl": nl, "caps": caps, "sources": sources, "dt": 1.0, "probes": ["1", ("5000", "77"), "9999"]}
    for method in METHODS:
        r = ref.TransientReference(rows, caps, out["dt"], method)
        A = r.rhs_steps(sources, MG_STEPS)
        out[method] = (r, A)
    return out


def _probe_pairs(nl, probes):
    from nodal_amd.ports import resolve_ports
    ia, ib = resolve_ports(nl, probes)
    return list(zip(ia.tolist(), ib.tolist()))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("steps", [1, 15, 16, 17, 33])
def test_multigrid_route(grid100, steps, method):
    g = grid100
    c = n.Circuit(g["nl"], sparse=True)
    assert c._handle.n == 9999
    x0 = np.array(c.solve().result)
    sources = {name: vals[:steps] for name, vals in g["sources"].items()}
    tr = c.transient(g["caps"], g["dt"], steps, sources=sources, method=method, keep_every=1, probes=g["probes"])
    assert (tr.iterations > 0).all(), tr.iterations
    r, A = g[method]
    check_one_step(r, x0, tr, A[:steps], ("grid(100)", steps, method))
    # (the full reference stepping starts where the device starts: from its DC point)
    check_waveforms(r, r.run(x0, A[:steps]), tr, _probe_pairs(g["nl"], g["probes"]), ("grid(100)", steps, method))
    # the second call with the child kept does no setup: the call's matrix work is reported as exactly 0.0
    assert tr.timings[0] > 0.0
    again = c.transient(g["caps"], g["dt"], steps, sources=sources, method=method, keep_every=1, probes=g["probes"])
    print("first call", tr.timings, "second call", again.timings)
    assert again.timings[0] == 0.0 and (again.iterations > 0).all()
    assert np.array_equal(again.solutions, tr.solutions)


def test_multigrid_gives_up(grid100, monkeypatch):
    g = grid100
    steps, method = 5, "euler"
    c = n.Circuit(g["nl"], sparse=True)
    x0 = np.array(c.solve().result)
    sources = {name: vals[:steps] for name, vals in g["sources"].items()}
    monkeypatch.setenv("NODAL_FCG_MAXIT", "3")
    tr = c.transient(g["caps"], g["dt"], steps, sources=sources, method=method, keep_every=1, probes=g["probes"])
    monkeypatch.delenv("NODAL_FCG_MAXIT")
    r, A = g[method]
    check_one_step(r, x0, tr, A[:steps], "grid(100), the iteration gives up")
    check_waveforms(r, r.run(x0, A[:steps]), tr, _probe_pairs(g["nl"], g["probes"]), "grid(100), the iteration gives up")


# ---- 9: the sparse LU route above the dense bounds ----------------------------------------------------------------
@pytest.fixture(scope="module")
def cfg5_95():
    rows = gen.cfg5_rows(95)
    caps = ref.seeded_capacitors(rows, 300, seed=17)
    steps = 17
    sources = waveforms_of(source_names(rows), steps, seed=18)
    r = ref.TransientReference(rows, caps, 0.5, "trapezoidal")
    return rows, caps, sources, steps, r, r.rhs_steps(sources, steps)


@pytest.mark.parametrize("redo", [False, True], ids=["refined", "every step redone"])
def test_sparse_lu_route(cfg5_95, redo, monkeypatch):
    rows, caps, sources, steps, r, A = cfg5_95
    if redo:
        monkeypatch.setenv("NODAL_MULTI_BAR", "-1")
    c, x0, tr = device_run(rows, caps, 0.5, steps, "trapezoidal", True, sources=sources, keep_every=1)
    if redo:
        monkeypatch.delenv("NODAL_MULTI_BAR")
    assert c._handle.n > 8192 and (tr.iterations >= 1).all()
    check_one_step(r, x0, tr, A, ("cfg5(95)", redo))


# ---- 10: probes ---------------------------------------------------------------------------------------------------
def test_probes():
    rows = dict(INPUTS)["random2"]
    caps = ref.seeded_capacitors(rows, 7, seed=1)
    steps = 8
    sources = waveforms_of(source_names(rows), steps, seed=2)
    probes = ["3", ("2", "5"), ("5", "2"), ("4", "4"), ("g", "g"), ("g", "6")]
    c, x0, tr = device_run(rows, caps, 0.4, steps, "euler", True, sources=sources, keep_every=1, probes=probes)
    num = c.netlist.nodenum
    X = np.vstack([x0[None, :], tr.solutions])
    assert tr.probes == [("3", c.netlist.ground), ("2", "5"), ("5", "2"), ("4", "4"), ("g", "g"), ("g", "6")]
    assert np.array_equal(tr.waveforms[:, 0], X[:, num["3"]])  # row 0 included: the initial state read at the probes
    assert np.array_equal(tr.waveforms[:, 1], X[:, num["2"]] - X[:, num["5"]])
    assert np.array_equal(tr.waveforms[:, 2], -tr.waveforms[:, 1])
    for p in (3, 4):
        assert (tr.waveforms[:, p] == 0.0).all() and not np.signbit(tr.waveforms[:, p]).any()
    assert np.array_equal(tr.waveforms[:, 5], 0.0 - X[:, num["6"]])


# ---- 11: the envelope ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["random3", "grid(60)"])
def test_envelope(which):
    rows = dict(INPUTS)[which]
    caps = ref.seeded_capacitors(rows, 9, seed=3)
    steps = 11
    sources = waveforms_of(source_names(rows), steps, seed=5)
    c, _, tr = device_run(rows, caps, 0.4, steps, "trapezoidal", True, sources=sources, keep_every=1, envelope=True)
    K = c.table.K
    P = tr.solutions[:, :K]
    env = tr.envelope
    assert np.array_equal(env.potential_min, P.min(axis=0)) and np.array_equal(env.potential_max, P.max(axis=0))
    assert np.array_equal(env.potential_min_step, 1 + P.argmin(axis=0))
    assert np.array_equal(env.potential_max_step, 1 + P.argmax(axis=0))
    assert env.potential_min_step.dtype == np.int32


def test_envelope_ties_take_the_lowest_step():
    """constant sources from the DC point: from some step on the solution repeats bit for bit, and among the steps
    that attain an extreme the lowest one is reported (numpy's argmin / argmax are the first occurrence too)"""
    rows = ref.rc_rows(0.7, 3.0)
    steps = 6
    _, x0, tr = device_run(rows, [], 1.0, steps, "euler", True, keep_every=1, envelope=True)
    assert (tr.solutions == tr.solutions[0]).all()  # (no capacitors, constant sources: the same solve six times)
    env = tr.envelope
    assert env.potential_min_step.tolist() == [1] and env.potential_max_step.tolist() == [1]
    assert env.potential_min[0] == tr.solutions[0, 0] == env.potential_max[0]


def test_envelope_of_a_floating_island_is_empty():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr = c.transient([("c1", 1.0, "5", "g")], 1.0, 3, initial=np.zeros(c._handle.n), envelope=True)
    env = tr.envelope
    assert np.isnan(env.potential_min).all() and np.isnan(env.potential_max).all()
    assert (env.potential_min_step == -1).all() and (env.potential_max_step == -1).all()


# ---- 12: keep_every -----------------------------------------------------------------------------------------------
def test_keep_every():
    rows = dict(INPUTS)["cfg5(24)"]
    caps = ref.seeded_capacitors(rows, 30, seed=4)
    steps = 19  # (more kept solutions than the staging ring holds, and a last block that does not fill it)
    sources = waveforms_of(source_names(rows), steps, seed=6)
    c, _, full = device_run(rows, caps, 0.4, steps, "euler", True, sources=sources, keep_every=1)
    assert full.solution_steps.tolist() == list(range(1, steps + 1))
    for s in (4, steps):
        tr = c.transient(caps, 0.4, steps, sources=sources, keep_every=s)
        assert tr.solution_steps.tolist() == list(range(s, steps + 1, s))
        assert np.array_equal(tr.solutions, full.solutions[s - 1::s])
    none = c.transient(caps, 0.4, steps, sources=sources)
    assert none.solutions is None and len(none.solution_steps) == 0
    assert np.array_equal(none.scaled_residual, full.scaled_residual)


# ---- 13: the circuit is left as found -----------------------------------------------------------------------------
def test_the_circuit_is_left_as_found():
    rows = dict(INPUTS)["random0"]
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    with pytest.raises(ValueError, match="no solution: call solve"):
        c.transient([], 1.0, 2)
    x = np.array(c.solve().result)
    before = c.branches()
    G, A, values = c.G.toarray().copy(), np.array(c.A), np.array(c.values)
    caps = ref.seeded_capacitors(rows, 5, seed=8)
    c.transient(caps, 0.3, 4, sources=waveforms_of(source_names(rows), 4, seed=1))
    after = c.branches()
    for name in ("voltage", "current", "power"):
        assert np.array_equal(np.asarray(getattr(before, name)), np.asarray(getattr(after, name))), name
    assert np.array_equal(np.asarray(c._handle.download_x()), x)
    assert np.array_equal(c.G.toarray(), G) and np.array_equal(np.array(c.A), A) and np.array_equal(c.values, values)
    child = c._transient_child[1]
    c.transient(caps, 0.3, 2)
    assert c._transient_child[1] is child  # (the same capacitors, dt and method: the child is kept)
    c.transient(caps, 0.3, 2, method="trapezoidal")
    assert c._transient_child[1] is not child
    c.set_values(values * 1.5)
    assert c._transient_child is None
    with pytest.raises(ValueError, match="no solution: call solve"):
        c.transient(caps, 0.3, 2)


def test_argument_errors_through_the_circuit():
    rows = dict(INPUTS)["random0"]
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    c.solve()
    with pytest.raises(KeyError):
        c.transient([("c1", 1.0, "1", "nowhere")], 1.0, 2)
    with pytest.raises(ValueError, match="farads"):
        c.transient([("c1", 0.0, "1", "g")], 1.0, 2)
    with pytest.raises(ValueError, match="dt"):
        c.transient([], 0.0, 2)
    with pytest.raises(ValueError, match="steps"):
        c.transient([], 1.0, -1)
    with pytest.raises(ValueError, match="euler"):
        c.transient([], 1.0, 2, method="trapezoidal", initial=np.zeros(c._handle.n))
    with pytest.raises(KeyError):
        c.transient([], 1.0, 2, sources={"nobody": [1.0, 2.0]})
    with pytest.raises(ValueError, match="one per step"):
        c.transient([], 1.0, 2, sources={"a0": [1.0, 2.0, 3.0]})
    empty = c.transient([], 1.0, 0, probes=["1"])
    assert empty.waveforms.shape == (1, 1) and len(empty) == 0 and empty.t.tolist() == [0.0]


# ---- 14: singular networks ----------------------------------------------------------------------------------------
def test_singular_sparse_gives_nan_steps_and_warns_once():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tr = c.transient([("c1", 1.0, "5", "g")], 1.0, 3, initial=np.zeros(c._handle.n), probes=["5"], keep_every=1)
    assert (tr.info > 0).all() and np.isnan(tr.solutions).all() and np.isnan(tr.waveforms[1:]).all()
    assert tr.waveforms[0, 0] == 0.0 and np.isnan(tr.scaled_residual).all()
    assert sum(issubclass(i.category, MatrixRankWarning) for i in w) == 1


def test_singular_dense_raises():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=False)
    with pytest.raises((np.linalg.LinAlgError, n.UnconnectedCircuitError)):
        c.transient([("c1", 1.0, "5", "g")], 1.0, 3, initial=np.zeros(c._handle.n))


# ---- the C ABI's own argument errors ------------------------------------------------------------------------------
def test_abi_refuses_bad_rows():
    from nodal_amd import _ffi
    from nodal_amd.lowering import lower
    rows = dict(INPUTS)["random0"]
    nl = n.Netlist.from_rows(rows)
    table = lower(nl)
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    none32, x0, values = np.zeros(0, dtype=np.int32), np.zeros(table.n), np.zeros((2, 0))

    def call(cap_rows, src_rows=(), vals=values, ia=none32, ib=none32):
        return h.transient(cap_rows, src_rows, vals, x0, ia, ib, dense=False)

    with pytest.raises(_ffi.NodalHipError, match="assemble_numeric") as exc:  # no numeric assembly yet
        call([])
    assert exc.value.status == _ffi.E_INVALID
    h.assemble_numeric(0)
    types = np.asarray(table.type)
    a_row, r_row = int(np.flatnonzero(types == 1)[0]), int(np.flatnonzero(types == 0)[0])
    for bad, text in (([table.ncomp], "out of range"), ([-1], "out of range"), ([a_row], "not a resistor")):
        with pytest.raises(_ffi.NodalHipError, match=text) as exc:
            call(bad)
        assert exc.value.status == _ffi.E_INVALID
    with pytest.raises(_ffi.NodalHipError, match="not an independent source") as exc:  # nodal_solve_sources' rule
        call([], src_rows=[r_row], vals=np.zeros((2, 1)))
    assert exc.value.status == _ffi.E_INVALID
    with pytest.raises(_ffi.NodalHipError, match="probe node out of range") as exc:
        call([], ia=np.array([table.K], dtype=np.int32), ib=np.array([-1], dtype=np.int32))
    assert exc.value.status == _ffi.E_INVALID
    wave, x, env, resid, info, iters = call([r_row])  # an R row of the table itself serves as a companion
    assert wave.shape == (3, 0) and x is None and env is None and (info == 0).all()
    h.close()
