"""Loss gradients on the GPU (Circuit.gradient / nodal_gradient, Circuit.set_values, nodal_amd.autograd).  Every
expected value comes from tests/sensitivity_reference.py through the sums of tests/gradient_reference.py (the oracle's G,
an LU of G and of G^T, the per-row formulas), never from product code; the bars are those stated there."""
import types
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd import generators as gen
from nodal_amd.circuit import MatrixRankWarning
from tests import gradient_reference as gref
from tests import sensitivity_reference as ref
from tests.sensitivity_reference import TOL
from tests.test_gpu_branches import INPUTS, _island
from tests.test_gpu_sensitivity import DESTROYED_BITS, MOVED, SMALL, _ladder_rows, _state
from tests.test_gpu_sweep import _grid_with_loads, _random_rows

pytestmark = pytest.mark.gpu


def _cotangents(M, size, seed):
    return np.random.default_rng(seed).standard_normal((M, size))


def _check_residuals(sr, grad, cotangents, tag):
    """the adjoint solves themselves: G^T lam_m = c_m to 1e-12, scaled, on the host and as the device reports it"""
    for m, c in enumerate(cotangents):
        res = sr.r.adjoint_residual(np.asarray(grad.adjoints[m]), c)
        assert res <= 1e-12, (tag, m, res)
        assert float(grad.scaled_residual[m]) <= 1e-12, (tag, m, float(grad.scaled_residual[m]))


# ---- the single solve ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("k", range(len(INPUTS)), ids=[i[0] for i in INPUTS])
def test_single_solve_parity(k, sparse):
    name, rows = INPUTS[k]
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    c.solve()
    size = c._handle.n
    sr = gref.SweepReference(rows, sparse=size > SMALL)
    cot = _cotangents(1, size, 300 + k)
    grad = c.gradient(cot[0], adjoints=True)
    assert grad.adjoints.shape == (1, size) and grad.names == list(nl.component_keys) and grad.source_values == {}
    gref.check_gradient(sr, grad, cot, [sr.r.x], None, (name, sparse))
    if name not in DESTROYED_BITS:
        _check_residuals(sr, grad, cot, (name, sparse))
    # a solution the caller kept serves as well as the one on the device
    kept = c.gradient(cot[0], solutions=np.array(c._handle.download_x()))
    assert np.array_equal(kept.values, grad.values)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("k", range(len(INPUTS)), ids=[i[0] for i in INPUTS])
def test_a_unit_cotangent_gives_the_sensitivity_row(k, sparse):
    """One output c^T x as a loss: the gradient with cotangent c and the sensitivity of that output share the row
    formulas (csrc/table_rows.h), the right-hand side and the route, so they agree bit for bit.  A voltage output: the
    explicit term of a current output belongs to the sensitivity alone.  One column: with more the gradient is a fused
    chain over the members and the sensitivity is not."""
    name, rows = INPUTS[k]
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    c.solve()
    table = ref.table_of(nl)
    # (the sample's voltage between two nodes, or -- where it drew one node twice -- its node potential)
    found = [(s, ref.output_vector(nl, table, s)) for s in ref.sample_outputs(nl, table, 3, 700 + k) if s[0] != "i"]
    spec, (cvec, row) = max(found, key=lambda f: np.count_nonzero(f[1][0]))
    assert row is None and cvec.any()
    sens = c.sensitivities([spec], adjoints=True)
    grad = c.gradient(cvec, adjoints=True)
    assert np.array_equal(np.asarray(grad.adjoints)[0], np.asarray(sens.adjoints)[0]), (name, sparse, spec)
    assert np.array_equal(np.asarray(grad.values), np.asarray(sens.values)[0]), (name, sparse, spec)


# ---- every route of the driver, at its smallest shape ---------------------------------------------------------------
class Case:
    """a network, its reference, one sweep of M members and what the device made of it"""

    def __init__(self, rows, sparse, ref_sparse=True, nsrc=3):
        self.rows = rows
        self.sr = gref.SweepReference(rows, sparse=ref_sparse)
        self.names = gref.source_names(rows, nsrc)
        self.sparse = sparse

    def run(self, M, seed, tag, adjoints=True, env=None, monkeypatch=None):
        sr = self.sr
        c = n.Circuit(sr.nl, sparse=self.sparse)
        sources = gref.sweep_values(self.names, M, seed)
        sw = c.solve_sources(sources)
        assert (sw.info == 0).all()
        cot = _cotangents(M, c._handle.n, seed + 1)
        for key, value in (env or {}).items():
            monkeypatch.setenv(key, value)
        grad = c.gradient(cot, sources=sources, solutions=sw.result, adjoints=adjoints)
        for key in env or {}:
            monkeypatch.delenv(key)
        xs = sr.members(sources)
        # (the solutions handed to the device are the device's own; they are the reference's within the project's bar)
        assert np.abs(np.asarray(sw.result) - xs).max() <= TOL * np.abs(xs).max()
        worst, lams = gref.check_gradient(sr, grad, cot, xs, sources, tag)
        if adjoints:
            _check_residuals(sr, grad, cot, tag)
        return types.SimpleNamespace(c=c, grad=grad, cot=cot, xs=xs, lams=lams, sources=sources, sw=sw)


@pytest.fixture(scope="module")
def grid80():
    return Case(_grid_with_loads(80, 3, 80)[0], sparse=True, nsrc=4)


@pytest.fixture(scope="module")
def cfg5_95():
    return Case(gen.cfg5_rows(95), sparse=True)  # 9025 grid nodes plus branches: above 8192 unknowns, not passive


@pytest.mark.parametrize("M", [1, 2, 16, 17, 33])
def test_block_multigrid_route(grid80, M):
    assert len(grid80.sr.r.A) > 4096 and len(grid80.names) == 4
    grid80.run(M, 10 * M, ("grid(80) with loads", M))


def test_block_failure_falls_back(grid80, monkeypatch):
    grid80.run(20, 7, ("grid(80) with loads, block iteration capped", 20), env={"NODAL_FCG_MAXIT": "3"},
               monkeypatch=monkeypatch)


def test_sparse_lu_of_the_transposed_child(cfg5_95):
    assert len(cfg5_95.sr.r.A) > 8192
    out = cfg5_95.run(18, 18, ("cfg5(95)", 18))
    assert (out.grad.scaled_residual <= 1e-14).all(), out.grad.scaled_residual.max()


@pytest.mark.parametrize("adjoints", [True, False], ids=["adjoints", "plain"])
def test_redo_branch_of_the_sparse_lu_route(cfg5_95, monkeypatch, adjoints):
    out = cfg5_95.run(18, 19, ("cfg5(95), redo", adjoints), adjoints=adjoints, env={"NODAL_MULTI_BAR": "-1"},
                      monkeypatch=monkeypatch)
    assert (out.grad.scaled_residual <= 1e-12).all(), out.grad.scaled_residual.max()


@pytest.mark.parametrize("which", ["random0", "grid(6)"])
def test_dense_chunk_edge(which):
    """513 members on the dense route -- one full chunk of 512 and a chunk of one -- on the transposed child (random0)
    and on the handle itself (a passive grid)"""
    rows = _random_rows(0) if which == "random0" else list(gen.grid_rows(6))
    Case(rows, sparse=False, ref_sparse=False).run(513, 5, (which, 513))


def test_low_degree_elimination():
    case = Case(_ladder_rows(20000), sparse=True)
    assert len(case.sr.r.A) > 4096 and case.names == ["a1"]
    case.run(18, 3, ("ladder(20000)", 18))


# ---- the transpose is really taken ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["random0", "cfg5(24)"])
def test_the_transpose_is_really_taken(which):
    rows = _random_rows(0) if which == "random0" else gen.cfg5_rows(24)
    wrong = gref.SweepReference(rows, sparse=which != "random0", transposed=False)
    c = n.Circuit(wrong.nl, sparse=True)
    c.solve()
    cot = _cotangents(1, c._handle.n, 5)
    grad = c.gradient(cot[0])
    lams = wrong.adjoints(cot)
    want, _ = gref.gradient_sum(wrong.table, lams, [wrong.r.x])
    bar, _ = gref.gradient_bars(wrong.table, lams, [wrong.r.x])
    miss = gref.worst_ratio(grad.values, want, np.where(bar > 0, bar, np.inf))
    print(which, "with G in place of G^T the bar is missed by a factor", miss)
    assert miss > 100.0


# ---- members are really paired -------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["grid(80) with loads", "cfg5(95)"])
def test_members_are_really_paired(which, grid80, cfg5_95):
    case = grid80 if which.startswith("grid") else cfg5_95
    out = case.run(17, 41, (which, "pairing"))
    table = case.sr.table
    bar, _ = gref.gradient_bars(table, out.lams, out.xs)
    # every member with x_0; the cotangents rotated by one member: each wrong pairing must miss the bar somewhere
    same_x, _ = gref.gradient_sum(table, out.lams, [out.xs[0]] * 17)
    rotated, per = gref.gradient_sum(table, np.roll(out.lams, 1, axis=0), out.xs)
    miss_x = gref.worst_ratio(out.grad.values, same_x, np.where(bar > 0, bar, np.inf))
    miss_rot = gref.worst_ratio(out.grad.values, rotated, np.where(bar > 0, bar, np.inf))
    print(which, "x_0 for every member misses by", miss_x, "rotated cotangents by", miss_rot)
    assert miss_x > 1.0 and miss_rot > 1.0
    # the members' own source derivatives: rotated they miss as well
    _, per_bar = gref.gradient_bars(table, out.lams, out.xs)
    name = case.names[0]
    j = list(case.sr.nl.component_keys).index(name)
    assert gref.worst_ratio(out.grad.source_values[name], per[:, j], per_bar[:, j]) > 1.0


# ---- linearity against the library itself ---------------------------------------------------------------------------
@pytest.mark.parametrize("which,sparse", [("random1", False), ("random1", True), ("cfg5(24)", True),
                                          ("grid(12) with loads", True)])
def test_linearity_against_sensitivities(which, sparse):
    rows = {"random1": lambda: _random_rows(1), "cfg5(24)": lambda: gen.cfg5_rows(24),
            "grid(12) with loads": lambda: _grid_with_loads(12, 3, 12)[0]}[which]()
    sr = gref.SweepReference(rows, sparse=which != "random1")
    nl, table = sr.nl, sr.table
    c = n.Circuit(nl, sparse=sparse)
    c.solve()
    specs = [s for s in ref.sample_outputs(nl, table, 30, 9) if s[0] in ("e", "v")]
    assert len(specs) == 20
    sens = c.sensitivities(specs)
    w = np.random.default_rng(2).uniform(-2.0, 2.0, size=len(specs))
    vectors = np.array([ref.output_vector(nl, table, spec)[0] for spec in specs])
    cot = (w[:, None] * vectors).sum(axis=0)
    grad = c.gradient(cot)
    bar = ref.parity_bars(table, sr.r.adjoint(cot), sr.r.x, None)
    for q, spec in enumerate(specs):
        bar = bar + abs(w[q]) * ref.parity_bars(table, sr.r.adjoint(vectors[q]), sr.r.x, None)
    want = (w[:, None] * np.asarray(sens.values)).sum(axis=0)
    worst = gref.worst_ratio(grad.values, want, bar)
    print(which, sparse, "worst |gradient - sum w sens| / summed bars:", worst)
    assert worst <= 1.0


# ---- independent of the formulas: central differences through set_values + solve() -------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("seed", range(4))
def test_central_differences(seed, sparse):
    nl = n.Netlist.from_rows(_random_rows(seed))
    c = n.Circuit(nl, sparse=sparse)
    c.solve()
    cot = _cotangents(1, c._handle.n, 60 + seed)[0]
    grad = np.array(c.gradient(cot).values)
    base = np.array(c.values, dtype=np.float64)
    fd = np.zeros(len(base))
    for i in range(len(base)):
        step = 1e-5 * abs(base[i])
        assert step > 0
        loss = []
        for sign in (1.0, -1.0):
            moved = base.copy()
            moved[i] += sign * step
            c.set_values(moved)
            loss.append(float(cot @ np.asarray(c.solve().result)))
        fd[i] = (loss[0] - loss[1]) / (2.0 * step)
    scale = np.abs(grad).max()
    print("random%d" % seed, sparse, "worst |grad - central difference| / max|grad|:", np.abs(grad - fd).max() / scale)
    assert np.abs(grad - fd).max() <= 1e-6 * scale


# ---- nothing else moved ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,sparse", MOVED, ids=[f"{w}-{'sparse' if s else 'dense'}" for w, s in MOVED])
def test_nothing_else_moved(which, sparse):
    rows = {"grid(12) with loads": lambda: _grid_with_loads(12, 3, 12)[0], "random2": lambda: _random_rows(2),
            "grid(80) with loads": lambda: _grid_with_loads(80, 3, 80)[0], "cfg5(24)": lambda: gen.cfg5_rows(24),
            "cfg5(95)": lambda: gen.cfg5_rows(95)}[which]()
    nl = n.Netlist.from_rows(rows)
    sources = gref.sweep_values(gref.source_names(rows, 2), 19, 8)
    sw = n.Circuit(nl, sparse=sparse).solve_sources(sources)  # (on a circuit of its own: a sweep drops the solution)
    c = n.Circuit(nl, sparse=sparse)
    before = _state(c)
    cot = _cotangents(19, c._handle.n, 8)
    one = c.gradient(cot[0], adjoints=True)
    # the solution is still there: what reads it gives the same bits without a new solve
    br = c.branches()
    assert np.array_equal(np.array(br.current), before[1]) and br.dissipated == before[3]
    assert c.scaled_residual() == before[4]
    assert np.array_equal(np.array(c._handle.download_x()), before[0])
    swept = c.gradient(cot, sources=sources, solutions=sw.result, adjoints=True)
    assert np.array_equal(np.array(c._handle.download_x()), before[0])
    two = c.gradient(cot[0], adjoints=True)
    again = c.gradient(cot, sources=sources, solutions=sw.result, adjoints=True)
    for first, second in ((one, two), (swept, again)):
        for name in ("values", "adjoints", "scaled_residual", "info"):
            assert np.array_equal(getattr(first, name), getattr(second, name)), name
        assert first.source_values.keys() == second.source_values.keys()
        for name in first.source_values:
            assert np.array_equal(first.source_values[name], second.source_values[name]), name
    after = _state(c)
    for b, a in zip(before, after):
        assert np.array_equal(b, a)


# ---- set_values ------------------------------------------------------------------------------------------------------
def _rows_with(rows, values):
    return [[r[0], r[1], repr(float(v)), *r[3:]] for r, v in zip(rows, values)]


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("which", ["random3", "cfg5(24)", "grid(12) with loads"])
def test_set_values(which, sparse):
    rows = {"random3": lambda: _random_rows(3), "cfg5(24)": lambda: gen.cfg5_rows(24),
            "grid(12) with loads": lambda: _grid_with_loads(12, 3, 12)[0]}[which]()
    nl = n.Netlist.from_rows(rows)
    assert list(nl.component_keys) == [r[0] for r in rows]
    c = n.Circuit(nl, sparse=sparse)
    old = np.array(c.values, dtype=np.float64)
    c.solve()
    new = old * np.random.default_rng(4).uniform(0.5, 2.0, size=len(old))
    c.set_values(new)
    assert np.array_equal(c.values, new) and np.array_equal(c.table.value, new)
    with pytest.raises(ValueError, match="no solution"):
        c.gradient(np.zeros(c._handle.n))
    x = np.array(c.solve().result)
    fresh_rows = _rows_with(rows, new)
    fresh = np.array(n.Circuit(n.Netlist.from_rows(fresh_rows), sparse=sparse).solve().result)
    print(which, sparse, "set_values against a fresh Circuit: bit-identical" if np.array_equal(x, fresh)
          else "set_values against a fresh Circuit: max difference %g" % np.abs(x - fresh).max())
    assert np.abs(x - fresh).max() <= TOL * np.abs(fresh).max()
    # the gradient after set_values: the bar with the new values, a miss with the old ones
    sr = gref.SweepReference(fresh_rows, sparse=which != "random3")
    cot = _cotangents(1, c._handle.n, 12)
    grad = c.gradient(cot[0])
    gref.check_gradient(sr, grad, cot, [sr.r.x], None, (which, sparse, "new values"))
    assert np.array_equal(grad.component_values, new)
    stale = gref.SweepReference(rows, sparse=which != "random3")
    lams = stale.adjoints(cot)
    want, _ = gref.gradient_sum(stale.table, lams, [stale.r.x])
    bar, _ = gref.gradient_bars(stale.table, lams, [stale.r.x])
    assert gref.worst_ratio(grad.values, want, np.where(bar > 0, bar, np.inf)) > 1.0
    # the netlist is not touched
    assert [float(nl.components[r[0]].value) for r in rows[:3]] == [float(r[2]) for r in rows[:3]]


def test_set_values_failures_leave_the_circuit_usable():
    rows = _random_rows(1)
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    x = np.array(c.solve().result)
    old = np.array(c.values, dtype=np.float64)
    bad = old.copy()
    bad[[r[0] for r in rows].index("r2")] = 0.0
    with pytest.raises(ValueError, match="null resistance"):
        c.set_values(bad)
    assert np.array_equal(c.values, old)
    assert np.array_equal(np.array(c.solve().result), x)
    with pytest.raises(ValueError, match="shape"):
        c.set_values(old[:-1])
    assert np.array_equal(np.array(c.solve().result), x)
    # a driving resistor of value 0: what lowering raises
    driven = [["r1", "R", "2", "1", "g"], ["r2", "R", "3", "1", "2"], ["r3", "R", "1", "2", "g"],
              ["h1", "CCVS", "0.5", "3", "g", "1", "2", "r2"], ["r4", "R", "1", "3", "g"], ["a1", "A", "1", "1", "g"]]
    cd = n.Circuit(n.Netlist.from_rows(driven), sparse=False)
    xd = np.array(cd.solve().result)
    zero = np.array(cd.values, dtype=np.float64)
    zero[1] = 0.0
    with pytest.raises(ZeroDivisionError):
        cd.set_values(zero)
    assert np.array_equal(np.array(cd.solve().result), xd)


# ---- errors and edges ------------------------------------------------------------------------------------------------
def test_call_order_shapes_and_empty():
    rows = _random_rows(1)
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    size = c._handle.n
    with pytest.raises(ValueError, match="no solution"):
        c.gradient(np.zeros(size))
    c.solve()
    first = c.gradient(np.ones(size))
    with pytest.raises(ValueError, match="shape"):
        c.gradient(np.ones(size + 1))
    with pytest.raises(ValueError, match="shape"):
        c.gradient(np.ones((2, size)))
    sources = {"a0": [1.0, 2.0, -3.0]}
    sw = n.Circuit(nl, sparse=True).solve_sources(sources)
    with pytest.raises(ValueError, match="shape"):
        c.gradient(np.ones((2, size)), sources=sources, solutions=sw.result)
    with pytest.raises(ValueError, match="shape"):
        c.gradient(np.ones((3, size)), sources=sources, solutions=sw.result[:2])
    with pytest.raises(ValueError):
        c.gradient(np.ones((3, size)), sources=sources)
    with pytest.raises(ValueError):
        c.gradient(np.ones((3, size)), sources={"r0": [1.0, 2.0, 3.0]}, solutions=sw.result)
    # count == 0: zeros
    empty = c.gradient(np.zeros((0, size)), sources={"a0": []}, solutions=np.zeros((0, size)))
    assert np.array_equal(empty.values, np.zeros(len(rows))) and len(empty) == 0
    assert empty.source_values["a0"].shape == (0,)
    # the library refuses what the front end refuses: a resistor among the swept rows, a repeated row, a row out of
    # range, the handle's solution for more than one member or with swept rows
    h = c._handle
    keys = list(nl.component_keys)
    a0, r0 = keys.index("a0"), keys.index("r0")
    cot, x = np.ones((2, size)), np.asarray(sw.result)[:2]
    for kw in (dict(rows=[r0], solutions=x), dict(rows=[a0, a0], solutions=x), dict(rows=[len(keys)], solutions=x),
               dict(rows=[-1], solutions=x), dict(rows=None, solutions=None), dict(rows=[a0], solutions=None)):
        with pytest.raises(_ffi.NodalHipError) as exc:
            h.gradient(cot if kw["solutions"] is not None or kw["rows"] is None else cot[:1], dense=False, **kw)
        assert exc.value.status == _ffi.E_INVALID, kw
    assert np.array_equal(c.gradient(np.ones(size)).values, first.values)
    # no numeric assembly: a fresh handle with a table alone
    h2 = _ffi.Handle(0)
    try:
        h2.upload(c.table)
        h2.assemble_symbolic()
        with pytest.raises(_ffi.NodalHipError) as exc:
            h2.gradient(np.ones((1, h2.n)), dense=False, solutions=np.ones((1, h2.n)))
        assert exc.value.status == _ffi.E_INVALID
    finally:
        h2.close()


def test_floating_island():
    rows = _island()
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c.solve()
    size = c._handle.n
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        grad = c.gradient(np.ones(size), adjoints=True)
    assert (grad.info > 0).all() and np.isnan(grad.values).all() and np.isnan(grad.adjoints).all()
    assert sum(issubclass(i.category, MatrixRankWarning) for i in w) == 1
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sources = {"a1": [1.0, 2.0, 3.0], "fa": [0.5, 0.0, 1.0]}
        grad = c.gradient(np.ones((3, size)), sources=sources, solutions=np.ones((3, size)))
    assert (grad.info > 0).all() and np.isnan(grad.values).all()
    assert all(np.isnan(v).all() for v in grad.source_values.values())
    assert sum(issubclass(i.category, MatrixRankWarning) for i in w) == 1
    small = list(gen.grid_rows(6)) + rows[-41:]  # a small version for the dense path
    cd = n.Circuit(n.Netlist.from_rows(small), sparse=False)
    with pytest.raises((np.linalg.LinAlgError, n.UnconnectedCircuitError)):
        cd.gradient(np.ones(cd._handle.n), solutions=np.ones(cd._handle.n))


def test_every_lead_is_ground():
    nl = n.Netlist.from_rows([["r1", "R", "2", "g", "g"], ["a1", "A", "1", "g", "g"]])
    for sparse in (False, True):
        c = n.Circuit(nl, sparse=sparse)
        assert c._handle.n == 0
        c.solve()
        grad = c.gradient(np.zeros(0))
        assert np.array_equal(grad.values, np.zeros(2)) and np.array_equal(grad.info, np.zeros(1, dtype=np.int32))
        swept = c.gradient(np.zeros((2, 0)), sources={"a1": [1.0, 2.0]}, solutions=np.zeros((2, 0)))
        assert np.array_equal(swept.values, np.zeros(2)) and np.array_equal(swept.source_values["a1"], np.zeros(2))
        assert np.array_equal(swept.info, np.zeros(2, dtype=np.int32))


# ---- torch -----------------------------------------------------------------------------------------------------------
def _power_loss(torch, x, values, a, b, i, extra):
    return (x[..., a] - x[..., b]).pow(2).sum() / values[i] + (x * extra).sum()


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_autograd_solve(sparse):
    import torch
    from nodal_amd import autograd
    rows = _random_rows(2)
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    i = [r[0] for r in rows].index("r3")
    a, b = int(c.table.a[i]), int(c.table.b[i])
    assert a >= 0 and b >= 0
    base = np.array(c.values, dtype=np.float64)
    extra = torch.from_numpy(_cotangents(1, c._handle.n, 70)[0])
    values = torch.tensor(base, dtype=torch.float64, requires_grad=True)
    x = autograd.solve(c, values)
    x.retain_grad()
    loss = _power_loss(torch, x, values, a, b, i, extra)
    loss.backward()
    # exactly the arrays Circuit.gradient returns for the same cotangent, plus the loss's own partial derivative
    cot = x.grad.numpy()
    c.solve()
    direct = np.array(c.gradient(cot).values)
    explicit = np.zeros(len(base))
    xd = x.detach().numpy()
    explicit[i] = -float((xd[a] - xd[b]) ** 2) / base[i] ** 2
    assert np.array_equal(values.grad.numpy(), direct + explicit)

    def loss_at(v):
        c.set_values(v)
        xs = torch.from_numpy(np.array(c.solve().result))
        return float(_power_loss(torch, xs, torch.from_numpy(v), a, b, i, extra))

    fd = np.zeros(len(base))
    for j in range(len(base)):
        step = 1e-5 * abs(base[j])
        up, down = base.copy(), base.copy()
        up[j] += step
        down[j] -= step
        fd[j] = (loss_at(up) - loss_at(down)) / (2.0 * step)
    got = values.grad.numpy()
    assert np.abs(got - fd).max() <= 1e-6 * np.abs(got).max()


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_autograd_solve_sources(sparse):
    import torch
    from nodal_amd import autograd
    rows = _random_rows(3)
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    keys = [r[0] for r in rows]
    i = keys.index("r3")
    a, b = int(c.table.a[i]), int(c.table.b[i])
    assert a >= 0 and b >= 0
    base = np.array(c.values, dtype=np.float64)
    names = ["a1", "e0"]
    M = 5
    swept0 = np.random.default_rng(6).uniform(-5.0, 5.0, size=(M, 2))
    extra = torch.from_numpy(_cotangents(M, c._handle.n, 71))
    values = torch.tensor(base, dtype=torch.float64, requires_grad=True)
    swept = torch.tensor(swept0, dtype=torch.float64, requires_grad=True)
    x = autograd.solve_sources(c, values, names, swept)
    x.retain_grad()
    loss = _power_loss(torch, x, values, a, b, i, extra)
    loss.backward()
    cot = x.grad.numpy()
    sources = {name: swept0[:, j] for j, name in enumerate(names)}
    direct = c.gradient(cot, sources=sources, solutions=x.detach().numpy())
    want = np.array(direct.values)
    want[[keys.index(name) for name in names]] = 0.0
    xd = x.detach().numpy()
    want[i] += -float(((xd[:, a] - xd[:, b]) ** 2).sum()) / base[i] ** 2
    assert np.array_equal(values.grad.numpy(), want)
    assert np.array_equal(swept.grad.numpy(), np.stack([direct.source_values[name] for name in names], axis=1))

    def loss_at(v, s):
        c.set_values(v)
        xs = torch.from_numpy(np.array(c.solve_sources({name: s[:, j] for j, name in enumerate(names)}).result))
        return float(_power_loss(torch, xs, torch.from_numpy(v), a, b, i, extra))

    fd = np.zeros(len(base))
    for j in range(len(base)):
        step = 1e-5 * abs(base[j])
        up, down = base.copy(), base.copy()
        up[j] += step
        down[j] -= step
        fd[j] = (loss_at(up, swept0) - loss_at(down, swept0)) / (2.0 * step)
    got = values.grad.numpy()
    assert np.abs(got - fd).max() <= 1e-6 * np.abs(got).max()
    fds = np.zeros_like(swept0)
    for m in range(M):
        for j in range(2):
            step = 1e-5 * abs(swept0[m, j])
            up, down = swept0.copy(), swept0.copy()
            up[m, j] += step
            down[m, j] -= step
            fds[m, j] = (loss_at(base, up) - loss_at(base, down)) / (2.0 * step)
    gots = swept.grad.numpy()
    assert np.abs(gots - fds).max() <= 1e-6 * np.abs(gots).max()
