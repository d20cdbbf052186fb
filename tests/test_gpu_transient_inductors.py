"""Transient analysis with inductors on the GPU (Circuit.transient(inductors=...) / nodal_transient_rlc).  Every expected
value comes from tests/transient_rl_reference.py -- the oracle's matrices stepped in numpy / scipy -- never from product
code.

Bars: per step scaled_residual <= 1e-12.  One-step parity: with keep_every=1 and every inductor probed the reference
advances the DEVICE's x_{k-1}, i_{k-1} by one step and must meet the device's x_k within 2 TOL |x_k|_inf and its i_k within
2 TOL (|i_k|_inf + max_j g_j |x_k|_inf): a current's error is the state's plus g times a voltage error.  Full runs on
passive networks: 2 TOL k scale at step k, scale = max|x| for potentials and max|i| + max g max|x| for currents.  The DC
start: the potentials within 2 TOL |x_0|_inf; the inductor currents are unknowns of the same DC system, so the normwise
bar over that system's whole solution applies to them, 2 TOL max(|x_0|_inf, |i_0|_inf)."""
import random
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import generators as gen
from nodal_amd.circuit import MatrixRankWarning
from tests import transient_rl_reference as rl
from tests.test_gpu_branches import INPUTS, _island
from tests.transient_rl_reference import TOL

pytestmark = pytest.mark.gpu

RESID_BAR = 1e-12
METHODS = ["euler", "trapezoidal"]


def source_names(rows):
    return sorted({r[0] for r in rows if len(r) > 1 and r[1] in ("A", "E")})


def waveforms_of(names, steps, seed):
    rng = random.Random(seed)
    return {name: [rng.uniform(-5.0, 5.0) for _ in range(steps)] for name in names}


def node_labels(nl):
    return sorted(nl.nodenum, key=nl.nodenum.get)


def check_residuals(tr, tag):
    worst = float(np.max(tr.scaled_residual, initial=0.0))
    print(tag, "largest scaled residual", worst, "over the bar", worst / RESID_BAR)
    assert (tr.info == 0).all(), tag
    assert (tr.scaled_residual <= RESID_BAR).all(), tag


def ratio(miss, bar):
    return miss / bar if bar > 0 else (0.0 if miss == 0 else np.inf)


def device_states(c, tr):
    """X [steps + 1, n], I [steps + 1, L] of a run with keep_every=1, every node probed against ground in the order of
    its index and every inductor probed in order: row 0 from the probes (its branch unknowns, which nothing reads, 0)"""
    K, steps = c.table.K, len(tr)
    assert tr.waveforms.shape == (steps + 1, K) and tr.solutions.shape == (steps, c.table.n)
    assert np.array_equal(tr.solutions[:, :K], tr.waveforms[1:])
    x0 = np.zeros(c.table.n)
    x0[:K] = tr.waveforms[0]
    return np.vstack([x0[None, :], tr.solutions]), tr.currents


def check_one_step(r, X, I, A_steps, tag):
    Xr, Ir = r.one_step_from(X, I, A_steps)
    gmax = r.g.max() if len(r.g) else 0.0
    worst_x = worst_i = 0.0
    for k in range(1, len(X)):
        xs = np.abs(X[k]).max()
        worst_x = max(worst_x, ratio(np.abs(X[k] - Xr[k - 1]).max(), 2 * TOL * xs))
        if I.shape[1]:
            worst_i = max(worst_i, ratio(np.abs(I[k] - Ir[k - 1]).max(), 2 * TOL * (np.abs(I[k]).max() + gmax * xs)))
    print(tag, "one-step parity, worst miss over the bar: potentials", worst_x, "currents", worst_i)
    assert worst_x <= 1.0 and worst_i <= 1.0, tag


def check_dc_start(r, X, I, tag):
    x0, i0 = r.dc_start()
    K = r.cap.K
    scale_x = np.abs(x0[:K]).max()
    scale = max(scale_x, np.abs(i0).max(initial=0.0))
    miss_x, miss_i = np.abs(X[0][:K] - x0[:K]).max(), np.abs(I[0] - i0).max(initial=0.0)
    print(tag, "DC start, miss over the bar: potentials", ratio(miss_x, 2 * TOL * scale_x), "currents",
          ratio(miss_i, 2 * TOL * scale))
    assert miss_x <= 2 * TOL * scale_x and miss_i <= 2 * TOL * scale, tag
    return x0, i0


def check_full_run(r, X, I, A_steps, tag):
    """the device's run against the reference stepping from the device's own start: 2 TOL k scale at step k"""
    Xr, Ir = r.run(X[0], I[0], A_steps)
    K = r.cap.K
    scale_x = np.abs(Xr).max()
    scale_i = np.abs(Ir).max() + r.g.max() * scale_x
    k = np.arange(1, len(X), dtype=np.float64)
    worst_x = (np.abs(X[1:, :K] - Xr[1:, :K]).max(axis=1) / (2 * TOL * k * scale_x)).max()
    worst_i = (np.abs(I[1:] - Ir[1:]).max(axis=1) / (2 * TOL * k * scale_i)).max()
    print(tag, "full run, worst miss over the bar: potentials", worst_x, "currents", worst_i)
    assert worst_x <= 1.0 and worst_i <= 1.0, tag


def run_all_probed(rows, caps, inds, dt, steps, method, sparse, sources=None, **kw):
    """a circuit on which solve() is never called, stepped from its DC start with every node and inductor probed"""
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    tr = c.transient(caps, dt, steps, sources=sources, method=method, keep_every=1, probes=node_labels(nl),
                     inductors=inds, current_probes=[i[0] for i in inds], **kw)
    return c, tr


# ---- 1: one RL section against the closed form (n = 1: the dense-per-step route) ----------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_rl_section_euler_closed_form(sparse):
    I, R, L, h, steps = 0.7, 3.0, 0.05, 0.011, 60
    c = n.Circuit(n.Netlist.from_rows(rl.rl_rows(I, R)), sparse=sparse)
    tr = c.transient([], h, steps, initial=np.array([I * R]), inductors=[("l1", L, "1", "g")], probes=["1"],
                     current_probes=["l1"], keep_every=1)
    v, i = rl.rl_euler_closed_form(I, R, L, h, steps)
    assert tr.waveforms.shape == (steps + 1, 1) and tr.currents.shape == (steps + 1, 1) and tr.current_probes == ["l1"]
    assert tr.waveforms[0, 0] == I * R and tr.currents[0, 0] == 0.0  # (initial= alone: the inductor starts at zero)
    k = np.arange(1, steps + 1)
    worst_v = np.max(np.abs(tr.waveforms[1:, 0] - v[1:]) / (2 * TOL * k * np.abs(v).max()))
    worst_i = np.max(np.abs(tr.currents[1:, 0] - i[1:]) / (2 * TOL * k * (np.abs(i).max() + h / L * np.abs(v).max())))
    print("RL Euler against the closed form, worst miss over the bar: voltage", worst_v, "current", worst_i)
    assert worst_v <= 1.0 and worst_i <= 1.0
    assert (tr.iterations == 0).all() and tr.final_currents.tolist() == [tr.currents[-1, 0]]
    check_residuals(tr, "rl euler")


# ---- 2: every input of the branches suite, dense and sparse, both methods: one-step parity -----------------------
def test_no_input_is_left_out():
    assert len(INPUTS) == 29


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("k", range(len(INPUTS)), ids=[i[0] for i in INPUTS])
def test_one_step_parity_on_every_input(k, sparse, method):
    name, rows = INPUTS[k]
    steps, dt = 20, 0.4
    caps, inds = rl.seeded_mix(rows, k)
    sources = waveforms_of(source_names(rows), steps, seed=100 + k)
    with warnings.catch_warnings():
        warnings.simplefilter("error", MatrixRankWarning)
        c, tr = run_all_probed(rows, caps, inds, dt, steps, method, sparse, sources=sources)
    r = rl.RLReference(rows, caps, inds, dt, method)
    X, I = device_states(c, tr)
    tag = (name, sparse, method)
    check_dc_start(r, X, I, tag)
    check_one_step(r, X, I, r.rhs_steps(sources, steps), tag)
    check_residuals(tr, tag)
    assert np.array_equal(tr.final_currents, I[-1])


# ---- 3: the DC start ----------------------------------------------------------------------------------------------
def _fed_through_an_inductor():
    """a regulator (E behind a resistor) that reaches a small loaded mesh through a package inductor ALONE: without
    the inductor the mesh hangs on current sources only and the parent's own system is singular"""
    rows = [["vreg", "E", "1.2", "reg", "g"], ["rreg", "R", "0.05", "reg", "pkg"],
            ["r12", "R", "1", "n1", "n2"], ["r23", "R", "2", "n2", "n3"], ["r34", "R", "1.5", "n3", "n4"],
            ["r41", "R", "0.5", "n4", "n1"], ["r13", "R", "3", "n1", "n3"],
            ["load3", "A", "0.4", "g", "n3"], ["load4", "A", "0.1", "g", "n4"]]
    caps = [("c1", 0.3, "n1", "g"), ("c3", 0.5, "n3", "g"), ("c4", 0.2, "g", "n4")]
    inds = [("lpkg", 0.4, "pkg", "n1")]
    return rows, caps, inds


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_dc_start_of_a_network_disconnected_without_its_inductor(sparse, method):
    rows, caps, inds = _fed_through_an_inductor()
    steps = 12
    sources = {"load3": [1.0] * steps, "vreg": [1.2] * steps}
    c, tr = run_all_probed(rows, caps, inds, 0.1, steps, method, sparse, sources=sources)
    r = rl.RLReference(rows, caps, inds, 0.1, method)
    assert np.linalg.matrix_rank(r.cap.G.toarray()) < r.n  # (the parent's own system: singular)
    X, I = device_states(c, tr)
    x0, i0 = check_dc_start(r, X, I, ("fed through an inductor", sparse, method))
    assert abs(i0[0] - 0.5) <= 1e-12  # (both loads come through the package: 0.4 + 0.1 A from pkg to n1)
    check_one_step(r, X, I, r.rhs_steps(sources, steps), ("fed through an inductor", sparse, method))
    check_residuals(tr, "fed through an inductor")
    # (solve() was never called, and the parent has no solution to offer)
    with pytest.raises(ValueError, match="no solution: call solve"):
        c.transient(caps, 0.1, 2, method=method)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_the_sign_of_the_current(sparse):
    rows, caps, inds = _fed_through_an_inductor()
    turned = [("lpkg", 0.4, "n1", "pkg")]
    steps = 6
    sources = {"load3": [1.0] * steps}
    _, fwd = run_all_probed(rows, caps, inds, 0.1, steps, "euler", sparse, sources=sources)
    _, bwd = run_all_probed(rows, caps, turned, 0.1, steps, "euler", sparse, sources=sources)
    assert (fwd.currents[:, 0] > 0.0).all()  # from the regulator's side into the mesh: positive as (pkg, n1)
    scale = np.abs(fwd.currents).max() + 0.1 / 0.4 * np.abs(fwd.waveforms).max()
    assert np.abs(fwd.currents + bwd.currents).max() <= 2 * TOL * steps * scale
    assert np.abs(fwd.waveforms - bwd.waveforms).max() <= 2 * TOL * steps * np.abs(fwd.waveforms).max()
    assert np.abs(fwd.final_currents + bwd.final_currents).max() <= 2 * TOL * steps * scale


# ---- 4: the routes above the dense bound --------------------------------------------------------------------------
def _grid_case(N, e_sources, ninductors, seed):
    """grid(N) with a capacitor on every node, `ninductors` inductors to ground on seeded nodes, E sources on others
    (an inductor on the node of an E source would be a loop without a DC solution) and two loads, each on a node next
    to an inductor's: with a capacitor on every node a disturbance dies out within a few nodes"""
    rng = random.Random(seed)
    rows = list(gen.grid_rows(N))
    last = N * N - 1
    picks = rng.sample(range(1, last), len(e_sources) + ninductors)
    at = picks[len(e_sources):]
    beside = [k + N if k + N < last else k - N for k in at[:2]]
    rows += [[f"ld{j}", "A", "1", str(k), "g"] for j, k in enumerate(beside)]
    rows += [[name, "E", "1.0", str(k), "g"] for name, k in zip(e_sources, picks)]
    nl = n.Netlist.from_rows(rows)
    caps = [(f"cg{i}", rng.uniform(0.5, 2.0), node, "g") for i, node in enumerate(node_labels(nl))]
    inds = [(f"lg{j}", rng.uniform(0.5, 3.0), str(k), "g") if j % 2 else (f"lg{j}", rng.uniform(0.5, 3.0), "g", str(k))
            for j, k in enumerate(at)]
    return rows, caps, inds


@pytest.mark.parametrize("method", METHODS)
def test_sparse_lu_route(method):
    rows, caps, inds = _grid_case(12, ["e1", "e2"], 5, seed=31)
    steps, dt = 16, 0.5
    sources = waveforms_of(["a1", "ld0", "ld1", "e1", "e2"], steps, seed=32)
    c, tr = run_all_probed(rows, caps, inds, dt, steps, method, True, sources=sources)
    assert c._handle.n == 145 and c.table.B == 2 and (tr.iterations == 1).all()  # 143 potentials and two branches
    r = rl.RLReference(rows, caps, inds, dt, method)
    X, I = device_states(c, tr)
    A = r.rhs_steps(sources, steps)
    check_dc_start(r, X, I, ("grid(12) with E", method))
    check_one_step(r, X, I, A, ("grid(12) with E", method))
    check_full_run(r, X, I, A, ("grid(12) with E", method))
    check_residuals(tr, ("grid(12) with E", method))


@pytest.fixture(scope="module")
def grid70():
    rows, caps, inds = _grid_case(70, [], 6, seed=41)
    steps = 10
    return rows, caps, inds, steps, waveforms_of(["a1", "ld0", "ld1"], steps, seed=42)


@pytest.mark.parametrize("method", METHODS)
def test_multigrid_route(grid70, method):
    rows, caps, inds, steps, sources = grid70
    dt = 1.0
    c, tr = run_all_probed(rows, caps, inds, dt, steps, method, True, sources=sources)
    assert c._handle.n == 4899 and c.table.B == 0
    assert (tr.iterations > 0).all(), tr.iterations
    r = rl.RLReference(rows, caps, inds, dt, method)
    X, I = device_states(c, tr)
    A = r.rhs_steps(sources, steps)
    check_dc_start(r, X, I, ("grid(70)", method))
    check_one_step(r, X, I, A, ("grid(70)", method))
    check_full_run(r, X, I, A, ("grid(70)", method))
    check_residuals(tr, ("grid(70)", method))


# ---- 5: continuation ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_continuation(sparse):
    rows, caps, inds = _grid_case(12, ["e1"], 4, seed=51)
    steps, dt = 20, 0.5
    names = ["a1", "ld0", "ld1", "e1"]
    sources = waveforms_of(names, steps, seed=52)
    c, whole = run_all_probed(rows, caps, inds, dt, steps, "euler", sparse, sources=sources)
    kw = dict(method="euler", keep_every=1, probes=whole.probes, inductors=inds, current_probes=[i[0] for i in inds])
    first = c.transient(caps, dt, 10, sources={k: v[:10] for k, v in sources.items()}, **kw)
    second = c.transient(caps, dt, 10, sources={k: v[10:] for k, v in sources.items()}, initial=first.solutions[-1],
                         initial_currents=first.final_currents, **kw)
    assert np.array_equal(second.waveforms[0], first.waveforms[-1]) and np.array_equal(second.currents[0], first.currents[-1])
    gmax = (dt / np.array([i[1] for i in inds])).max()
    X = np.vstack([first.solutions, second.solutions])
    C = np.vstack([first.currents[1:], second.currents[1:]])
    for k in range(steps):
        xs = np.abs(whole.solutions[k]).max()
        assert np.abs(X[k] - whole.solutions[k]).max() <= 2 * TOL * xs, k
        assert np.abs(C[k] - whole.currents[k + 1]).max() <= 2 * TOL * (np.abs(whole.currents[k + 1]).max() + gmax * xs), k
    assert np.abs(second.final_currents - whole.final_currents).max() <= 2 * TOL * (np.abs(whole.final_currents).max()
                                                                                    + gmax * np.abs(whole.solutions[-1]).max())


# ---- 6: the kept matrix work and a repeated call ------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_kept_matrix_work_and_a_repeated_call(method):
    rows, caps, inds = _grid_case(12, ["e1", "e2"], 5, seed=61)
    steps, dt = 9, 0.5
    names = ["a1", "ld0", "ld1", "e1", "e2"]
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    kw = dict(method=method, keep_every=1, envelope=True, inductors=inds)
    one = c.transient(caps, dt, steps, sources=waveforms_of(names, steps, seed=1), probes=["5", ("7", "100")],
                      current_probes=["lg0", "lg3"], **kw)
    assert one.timings[0] > 0.0
    child, dc = c._transient_child[1], c._transient_dc[1]
    two = c.transient(caps, dt, steps, sources=waveforms_of(names[:3], steps, seed=2), probes=["9"],
                      current_probes=["lg4", "lg1", "lg4"], **kw)
    print("first call", one.timings, "second call", two.timings)
    assert two.timings[0] == 0.0 and c._transient_child[1] is child and c._transient_dc[1] is dc
    assert two.currents.shape == (steps + 1, 3) and np.array_equal(two.currents[:, 0], two.currents[:, 2])
    again = c.transient(caps, dt, steps, sources=waveforms_of(names[:3], steps, seed=2), probes=["9"],
                        current_probes=["lg4", "lg1", "lg4"], **kw)
    for name in ("waveforms", "solutions", "currents", "final_currents", "scaled_residual", "info", "iterations"):
        assert np.array_equal(getattr(again, name), getattr(two, name)), name
    for name in ("potential_min", "potential_min_step", "potential_max", "potential_max_step"):
        assert np.array_equal(getattr(again.envelope, name), getattr(two.envelope, name)), name
    # other henries: another child, the same DC clone (it is keyed by the leads alone); set_values() drops both
    other = [(name, 2 * henries, a, b) for name, henries, a, b in inds]
    c.transient(caps, dt, 2, inductors=other, method=method)
    assert c._transient_child[1] is not child and c._transient_dc[1] is dc
    c.set_values(np.array(c.values) * 1.5)
    assert c._transient_child is None and c._transient_dc is None


# ---- 7: capacitors only -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["random2", "cfg5(24)"])
def test_capacitors_only_is_what_it_was(which):
    from tests.transient_reference import seeded_capacitors
    rows = dict(INPUTS)[which]
    caps = seeded_capacitors(rows, 7, seed=1)
    steps = 8
    sources = waveforms_of(source_names(rows), steps, seed=2)
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    c.solve()
    kw = dict(sources=sources, method="trapezoidal", keep_every=1, probes=node_labels(nl)[:3], envelope=True)
    plain = c.transient(caps, 0.4, steps, **kw)
    empty = c.transient(caps, 0.4, steps, inductors=(), **kw)
    for name in ("waveforms", "solutions", "scaled_residual", "info", "iterations"):
        assert np.array_equal(getattr(plain, name), getattr(empty, name)), name
    for name in ("potential_min", "potential_min_step", "potential_max", "potential_max_step"):
        assert np.array_equal(getattr(plain.envelope, name), getattr(empty.envelope, name)), name
    assert empty.currents.shape == (steps + 1, 0) and empty.final_currents.shape == (0,)
    assert plain.currents.shape == (steps + 1, 0)


# ---- 8: singular starts and dead steps ----------------------------------------------------------------------------
ACROSS_E = [["e1", "E", "1.5", "3", "g"], ["r1", "R", "2", "3", "2"], ["r2", "R", "5", "2", "g"], ["a1", "A", "1", "2", "g"]]


def test_an_inductor_across_an_e_source_dense_raises():
    c = n.Circuit(n.Netlist.from_rows(ACROSS_E), sparse=False)
    with pytest.raises(np.linalg.LinAlgError):
        c.transient([("c1", 1.0, "2", "g")], 0.1, 3, inductors=[("l1", 1.0, "3", "g")])


def test_an_inductor_across_an_e_source_sparse_warns_and_gives_nan():
    c = n.Circuit(n.Netlist.from_rows(ACROSS_E), sparse=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tr = c.transient([("c1", 1.0, "2", "g")], 0.1, 3, inductors=[("l1", 1.0, "3", "g")], probes=["2"],
                         current_probes=["l1"], keep_every=1)
    assert (tr.info > 0).all() and np.isnan(tr.waveforms).all() and np.isnan(tr.currents).all()
    assert tr.currents.shape == (4, 1) and np.isnan(tr.solutions).all() and np.isnan(tr.final_currents).all()
    assert sum(issubclass(i.category, MatrixRankWarning) for i in w) == 1


def test_dead_steps_leave_nan_currents():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr = c.transient([("c1", 1.0, "5", "g")], 1.0, 3, initial=np.zeros(c._handle.n), inductors=[("l1", 1.0, "7", "g")],
                         initial_currents=[0.25], current_probes=["l1"])
    assert (tr.info > 0).all() and tr.currents[0, 0] == 0.25 and np.isnan(tr.currents[1:]).all()
    assert np.isnan(tr.final_currents).all()


# ---- 9: argument errors through the circuit -----------------------------------------------------------------------
def test_argument_errors_through_the_circuit():
    rows = dict(INPUTS)["random0"]
    nl = n.Netlist.from_rows(rows)
    a, b, d = node_labels(nl)[:3]
    c = n.Circuit(nl, sparse=True)
    inds = [("l1", 1.0, a, b)]
    with pytest.raises(ValueError, match="record=True with inductors"):
        c.transient([], 1.0, 2, inductors=inds, record=True)
    with pytest.raises(KeyError):
        c.transient([], 1.0, 2, inductors=inds, current_probes=["l2"])
    with pytest.raises(KeyError):
        c.transient([], 1.0, 2, inductors=[("l1", 1.0, a, "nowhere")])
    with pytest.raises(ValueError, match="henries"):
        c.transient([], 1.0, 2, inductors=[("l1", 0.0, a, b)])
    with pytest.raises(ValueError, match="loop of inductors"):
        c.transient([], 1.0, 2, inductors=inds + [("l2", 1.0, b, d), ("l3", 2.0, d, a)])
    with pytest.raises(ValueError, match="initial_currents needs"):
        c.transient([], 1.0, 2, inductors=inds, initial_currents=[0.0])
    with pytest.raises(ValueError, match="shape"):
        c.transient([], 1.0, 2, inductors=inds, initial=np.zeros(c._handle.n), initial_currents=[0.0, 1.0])
    with pytest.raises(ValueError, match="euler"):
        c.transient([], 1.0, 2, inductors=inds, method="trapezoidal", initial=np.zeros(c._handle.n))
    empty = c.transient([], 1.0, 0, inductors=inds, current_probes=["l1"], initial=np.zeros(c._handle.n),
                        initial_currents=[0.5])
    assert empty.currents.tolist() == [[0.5]] and empty.final_currents.tolist() == [0.5] and len(empty) == 0


def test_abi_refuses_bad_inductor_rows():
    from nodal_amd import _ffi
    from nodal_amd.lowering import lower
    table = lower(n.Netlist.from_rows(dict(INPUTS)["random0"]))
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    h.assemble_numeric(0)
    none32, x0, values = np.zeros(0, dtype=np.int32), np.zeros(table.n), np.zeros((2, 0))
    types = np.asarray(table.type)
    a_row, r_row = int(np.flatnonzero(types == 1)[0]), int(np.flatnonzero(types == 0)[0])

    def call(ind_rows, cur_index=none32):
        return h.transient_rlc([], ind_rows, [], values, x0, np.zeros(len(ind_rows)), none32, none32, cur_index, dense=False)

    for bad, text in (([table.ncomp], "inductor row out of range"), ([-1], "inductor row out of range"),
                      ([a_row], "inductor row that is not a resistor")):
        with pytest.raises(_ffi.NodalHipError, match=text) as exc:
            call(bad)
        assert exc.value.status == _ffi.E_INVALID
    for bad in ([1], [-1]):
        with pytest.raises(_ffi.NodalHipError, match="current probe outside") as exc:
            call([r_row], cur_index=np.array(bad, dtype=np.int32))
        assert exc.value.status == _ffi.E_INVALID
    out = call([r_row], cur_index=np.array([0], dtype=np.int32))  # an R row of the table itself serves as a companion
    assert out[6].shape == (3, 1) and out[7].shape == (1,) and (out[4] == 0).all()
    h.close()
