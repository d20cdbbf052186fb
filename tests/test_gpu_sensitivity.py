"""Adjoint sensitivities on the GPU (Circuit.sensitivities / nodal_sensitivities).  Every expected value comes from the
numpy restatement of tests/sensitivity_reference.py (the oracle's G, an LU of G^T, the per-row formulas), never from
product code; every bar is a multiple of the formulas' own scale F^abs (see that module)."""
import math
import types
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd import generators as gen
from nodal_amd.circuit import MatrixRankWarning
from oracle import nodal_oracle as oracle
from tests import sensitivity_reference as ref
from tests.sensitivity_reference import EPS, TOL
from tests.test_gpu_branches import INPUTS, _island
from tests.test_gpu_sweep import _grid_with_loads, _random_rows

pytestmark = pytest.mark.gpu

# the input whose 1e-17 ohm self-loop destroys the low bits of G (left out of the Kirchhoff checks of
# tests/test_gpu_branches.py for that reason): the oracle's G is not the matrix the device solved with
DESTROYED_BITS = ("edge/self_loop_r_bits",)
SMALL = 60  # unknowns up to which every unknown and every admissible current is an output


def test_the_inputs_are_the_ones_the_checks_were_sized_for():
    assert len(INPUTS) == 29 and sum(1 for name, _ in INPUTS if "/" in name) == 23
    assert all(name in [i[0] for i in INPUTS] for name in DESTROYED_BITS)


def check_against_reference(c, nl, r, specs, sens, tag, residual_check=True):
    """the bars of test 4 on every output and table row; returns the worst |got - want| / bar"""
    table = r.table
    x_scale = np.abs(r.x).max(initial=0.0)
    assert sens.values.shape == (len(specs), table.ncomp) and sens.adjoints.shape == (len(specs), table.K + table.B)
    assert (sens.info == 0).all(), tag
    worst = worst_resid = 0.0
    for q, spec in enumerate(specs):
        y, cvec, row, lam, want = r.output(spec)
        bar = ref.parity_bars(table, lam, r.x, row)
        off = np.abs(np.asarray(sens.values[q]) - want)
        with np.errstate(all="ignore"):
            ratio = np.where(bar > 0, off / bar, np.where(off > 0, np.inf, 0.0))
        worst = max(worst, float(ratio.max(initial=0.0)))
        assert (off <= bar).all(), (tag, spec, int(np.argmax(ratio)), float(ratio.max()))
        assert abs(sens.output_values[q] - y) <= TOL * np.abs(cvec).sum() * x_scale, (tag, spec)
        if residual_check:
            got_lam = np.asarray(sens.adjoints[q])
            res = r.adjoint_residual(got_lam, cvec)
            worst_resid = max(worst_resid, res)
            assert res <= 1e-12, (tag, spec, res)
            # The returned residual is the same quantity evaluated on the device (fused multiply-adds, its own G).  Each
            # evaluation of a row of G^T lam - c carries a rounding error of up to (entries of that row + 2) eps of the
            # denominator: neither resolves the residual below that floor, and a factor between two numbers that are
            # both rounding noise (one of them often exactly 0) says nothing.  Within a factor 2 up to that floor.
            G = r.G
            per_row = int(np.diff(G.tocsc().indptr).max()) if r.sparse else int((G != 0).sum(axis=0).max())
            floor = (per_row + 2) * EPS
            dev = float(sens.scaled_residual[q])
            assert dev <= 1e-12, (tag, spec, dev)
            if max(dev, res) > floor:
                assert 0.5 * res - floor <= dev <= 2.0 * res + floor, (tag, spec, dev, res)
    print(tag, "outputs", len(specs), "worst |got - want| / bar:", worst, "worst adjoint residual:", worst_resid)
    return worst


# ---- 4: parity with the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("k", range(len(INPUTS)), ids=[i[0] for i in INPUTS])
def test_parity_with_the_restatement(k, sparse):
    name, rows = INPUTS[k]
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    c.solve()
    table = ref.table_of(nl)
    small = table.K + table.B <= SMALL
    specs = ref.all_outputs(nl, table) if small else ref.sample_outputs(nl, table, 33, 100 + k)
    if not small:
        assert {s[0] for s in specs} == {"e", "v", "i"} and len(specs) == 33
    sens = c.sensitivities(specs, adjoints=True)
    r = ref.Reference(nl, sparse=not small)
    check_against_reference(c, nl, r, specs, sens, (name, sparse), residual_check=name not in DESTROYED_BITS)
    assert sens.outputs == specs and sens.names == list(nl.component_keys)


# ---- 5: the transpose is really taken ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["random0", "cfg5(24)"])
def test_the_transpose_is_really_taken(which):
    rows = _random_rows(0) if which == "random0" else gen.cfg5_rows(24)
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    c.solve()
    table = ref.table_of(nl)
    specs = ref.all_outputs(nl, table) if which == "random0" else ref.sample_outputs(nl, table, 33, 5)
    sens = c.sensitivities(specs)
    wrong = ref.Reference(nl, sparse=which != "random0", transposed=False)
    miss = 0.0
    for q, spec in enumerate(specs):
        _, _, row, lam, want = wrong.output(spec)
        bar = ref.parity_bars(table, lam, wrong.x, row)
        off = np.abs(np.asarray(sens.values[q]) - want)
        with np.errstate(all="ignore"):
            miss = max(miss, float(np.where(bar > 0, off / bar, 0.0).max()))
    print(which, "with G in place of G^T the bar is missed by a factor", miss)
    assert miss > 100.0


# ---- 6: every route ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid300():
    rows, _ = _grid_with_loads(300, 6, 3)
    nl = n.Netlist.from_rows(rows)
    return rows, nl, ref.Reference(nl, sparse=True)


@pytest.fixture(scope="module")
def cfg5_95():
    rows = gen.cfg5_rows(95)  # 9025 grid nodes plus branches: above 8192 unknowns, not passive
    nl = n.Netlist.from_rows(rows)
    return rows, nl, ref.Reference(nl, sparse=True)


def _with_ground(nl, table, M, seed):
    specs = ref.sample_outputs(nl, table, M, seed)
    specs[M // 2] = ("e", nl.ground)  # an all-zero column
    return specs


@pytest.mark.parametrize("M", [1, 2, 16, 17, 33])
def test_block_multigrid_route(grid300, M):
    rows, nl, r = grid300
    c = n.Circuit(nl, sparse=True)
    c.solve()
    specs = _with_ground(nl, r.table, M, M)
    sens = c.sensitivities(specs, adjoints=True)
    check_against_reference(c, nl, r, specs, sens, ("grid300", M))
    assert np.array_equal(sens.values[M // 2], np.zeros(r.table.ncomp)) and sens.output_values[M // 2] == 0.0


def test_block_failure_falls_back(grid300, monkeypatch):
    rows, nl, r = grid300
    c = n.Circuit(nl, sparse=True)
    c.solve()
    specs = _with_ground(nl, r.table, 20, 11)
    monkeypatch.setenv("NODAL_FCG_MAXIT", "3")
    sens = c.sensitivities(specs, adjoints=True)
    monkeypatch.delenv("NODAL_FCG_MAXIT")
    check_against_reference(c, nl, r, specs, sens, ("grid300, block iteration capped", 20))


def test_sparse_lu_of_the_transposed_child(cfg5_95):
    rows, nl, r = cfg5_95
    c = n.Circuit(nl, sparse=True)
    assert c._handle.n > 8192
    c.solve()
    specs = ref.sample_outputs(nl, r.table, 18, 18)
    sens = c.sensitivities(specs, adjoints=True)
    check_against_reference(c, nl, r, specs, sens, ("cfg5(95)", 18))
    assert (sens.scaled_residual <= 1e-14).all(), sens.scaled_residual.max()


def test_dense_switch_on_a_grid():
    nl = n.Netlist.from_rows(list(gen.grid_rows(40)))
    c = n.Circuit(nl, sparse=False)
    c.solve()
    r = ref.Reference(nl, sparse=True)
    specs = _with_ground(nl, r.table, 19, 40)
    sens = c.sensitivities(specs, adjoints=True)
    check_against_reference(c, nl, r, specs, sens, ("grid(40) dense", 19))


@pytest.mark.parametrize("adjoints", [True, False], ids=["adjoints", "plain"])
def test_redo_branch_of_the_sparse_lu_route(cfg5_95, monkeypatch, adjoints):
    """NODAL_MULTI_BAR=-1: every column fails the bar, is redone alone on the child and the factors are made anew; then
    the same call with the switch off, on the same Circuit, meets the refinement's own bar again"""
    rows, nl, r = cfg5_95
    c = n.Circuit(nl, sparse=True)
    assert c._handle.n > 8192
    c.solve()
    specs = ref.sample_outputs(nl, r.table, 18, 18)
    monkeypatch.setenv("NODAL_MULTI_BAR", "-1")
    redone = c.sensitivities(specs, adjoints=adjoints)
    monkeypatch.delenv("NODAL_MULTI_BAR")
    again = c.sensitivities(specs, adjoints=adjoints)
    for sens, bar in ((redone, 1e-12), (again, 1e-14)):
        # (without the adjoints the reference check reads their shape alone)
        lam = sens.adjoints if adjoints else np.empty((18, r.table.K + r.table.B))
        part = types.SimpleNamespace(values=sens.values, adjoints=lam, info=sens.info, output_values=sens.output_values,
                                     scaled_residual=sens.scaled_residual)
        check_against_reference(c, nl, r, specs, part, ("cfg5(95), redo", bar), residual_check=adjoints)
        assert (sens.scaled_residual <= bar).all(), sens.scaled_residual.max()


@pytest.mark.parametrize("which", ["random0", "grid(6)"])
def test_dense_chunk_edge(which):
    """513 outputs on the dense route -- one full chunk of 512 and a chunk of one -- on the transposed child (random0)
    and on the handle itself (a passive grid)"""
    rows = _random_rows(0) if which == "random0" else list(gen.grid_rows(6))
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=False)
    c.solve()
    r = ref.Reference(nl, sparse=False)
    outputs = ref.all_outputs(nl, r.table)
    specs = [outputs[q % len(outputs)] for q in range(513)]
    sens = c.sensitivities(specs, adjoints=True)
    assert sens.values.shape == (513, r.table.ncomp) and (sens.info == 0).all()
    for lo, hi in ((0, 33), (496, 513)):
        part = types.SimpleNamespace(values=sens.values[lo:hi], adjoints=sens.adjoints[lo:hi], info=sens.info[lo:hi],
                                     output_values=sens.output_values[lo:hi], scaled_residual=sens.scaled_residual[lo:hi])
        check_against_reference(c, nl, r, specs[lo:hi], part, (which, lo, hi))
    for q in range(len(outputs), 513):
        assert np.array_equal(sens.values[q], sens.values[q % len(outputs)]), q


def _ladder_rows(sections):
    """resistors in series, a shunt to ground at every tenth node, 1 A into the first node (the shape of
    generators.ladder_table)"""
    rng = np.random.default_rng(1)
    rows = [[f"s{k}", "R", repr(float(rng.uniform(0.5, 2.0))), f"n{k}", f"n{k + 1}"] for k in range(sections)]
    rows += [[f"t{k}", "R", repr(float(rng.uniform(0.5e4, 2e4))), f"n{k}", "g"] for k in range(0, sections + 1, 10)]
    return rows + [["a1", "A", "1", "n0", "g"]]


def test_no_hierarchy_after_the_low_degree_elimination():
    nl = n.Netlist.from_rows(_ladder_rows(20000))
    c = n.Circuit(nl, sparse=True)
    assert c._handle.n > 4096
    c.solve()
    r = ref.Reference(nl, sparse=True)
    specs = _with_ground(nl, r.table, 18, 7)
    sens = c.sensitivities(specs, adjoints=True)
    check_against_reference(c, nl, r, specs, sens, ("ladder(20000)", 18))


# ---- 7: identities that need no reference --------------------------------------------------------------------------
def check_identities(table, value, kinds, explicit_rows, y, S, lam, x, tag):
    """sum over the A and E rows of v s = y (the output is linear in the independent sources); sum over R + sum over
    CCVS - sum over A of v s = 0 for potentials and voltages, = -y for currents (scale every resistance and
    transresistance by t and every source current by 1 / t).  Bar TOL (sum |v| F^abs(lam, x) + |y|)."""
    ty = np.asarray(table.type)
    value = np.asarray(value, dtype=np.float64)
    src = (ty == ref.T_A) | (ty == ref.T_E)
    worst = 0.0
    for q in range(len(y)):
        vs = value * np.asarray(S[q], dtype=np.float64)
        bar = TOL * (math.fsum(np.abs(value) * ref.formulas_abs(table, lam[q], x, value, explicit_rows[q])) + abs(y[q]))
        first = math.fsum(vs[src]) - y[q]
        second = math.fsum(vs[ty == ref.T_R]) + math.fsum(vs[ty == ref.T_CCVS]) - math.fsum(vs[ty == ref.T_A])
        second += y[q] if kinds[q] == 1 else 0.0
        worst = max(worst, abs(first) / bar if bar > 0 else 0.0, abs(second) / bar if bar > 0 else 0.0)
        assert abs(first) <= bar, (tag, q, first, bar)
        assert abs(second) <= bar, (tag, q, second, bar)
    print(tag, "outputs", len(y), "worst identity defect / bar:", worst)


def _identities_of_a_circuit(nl, specs, tag):
    c = n.Circuit(nl, sparse=True)
    x = np.array(c.solve().result)
    sens = c.sensitivities(specs, adjoints=True)
    assert (sens.info == 0).all()
    table = ref.table_of(nl)
    rows = [ref.output_vector(nl, table, spec)[1] for spec in specs]
    kinds = [1 if spec[0] == "i" else 0 for spec in specs]
    check_identities(table, table.value, kinds, rows, sens.output_values, sens.values, sens.adjoints, x, tag)


def test_identities_grid300(grid300):
    rows, nl, r = grid300
    _identities_of_a_circuit(nl, ref.sample_outputs(nl, r.table, 20, 1), "grid300")


def test_identities_cfg5(cfg5_95):
    rows, nl, r = cfg5_95
    _identities_of_a_circuit(nl, ref.sample_outputs(nl, r.table, 20, 2), "cfg5(95)")


def test_identities_full_size_grid1000():
    table = gen.grid_table(1000)
    rng = np.random.default_rng(3)
    res = np.flatnonzero(np.asarray(table.type) == ref.T_R)
    kind = np.array([0, 0, 1, 0] * 4, dtype=np.int32)
    p = np.where(kind == 1, rng.choice(res, 16), rng.integers(table.K, size=16)).astype(np.int32)
    q2 = np.where(kind == 1, -1, np.where(np.arange(16) % 2 == 1, rng.integers(table.K, size=16), -1)).astype(np.int32)
    h = _ffi.Handle(0)
    try:
        h.upload(table)
        assert h.run(False) == 0
        x = np.array(h.download_x())
        S, y, lam, resid, info = h.sensitivities(kind, p, q2, dense=False, adjoints=True)
    finally:
        h.close()
    assert (info == 0).all() and (resid <= 1e-12).all(), resid.max()
    rows = [int(p[q]) if kind[q] == 1 else None for q in range(16)]
    check_identities(table, table.value, kind, rows, y, S, lam, x, "grid(1000)")


# ---- 8: nothing else moved -----------------------------------------------------------------------------------------
def _state(c):
    x = np.array(c.solve().result)
    br = c.branches()
    c._G = c._A = None  # (exported anew)
    G = c.G
    parts = (G.indptr.copy(), G.indices.copy(), G.data.copy()) if hasattr(G, "indptr") else (np.array(G),)
    return (x, np.array(br.current), np.array(br.power), br.dissipated, c.scaled_residual(), np.array(c.A)) + parts


# passive and not, each on both switches; then the two sparse routes that work on the handle's own buffers or on the
# child: the multigrid (grid(80): above 4096 unknowns) and the sparse LU of the transposed child (cfg5(95))
MOVED = [("grid(12) with loads", False), ("grid(12) with loads", True), ("random2", False), ("random2", True),
         ("cfg5(24)", False), ("cfg5(24)", True), ("grid(80) with loads", True), ("cfg5(95)", True)]


@pytest.mark.parametrize("which,sparse", MOVED, ids=[f"{w}-{'sparse' if s else 'dense'}" for w, s in MOVED])
def test_nothing_else_moved(which, sparse):
    rows = {"grid(12) with loads": lambda: _grid_with_loads(12, 3, 12)[0], "random2": lambda: _random_rows(2),
            "grid(80) with loads": lambda: _grid_with_loads(80, 3, 80)[0], "cfg5(24)": lambda: gen.cfg5_rows(24),
            "cfg5(95)": lambda: gen.cfg5_rows(95)}[which]()
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    before = _state(c)
    specs = ref.sample_outputs(nl, ref.table_of(nl), 19, 8)
    one = c.sensitivities(specs, adjoints=True)
    # the solution is still there: what reads it gives the same bits without a new solve
    br = c.branches()
    assert np.array_equal(np.array(br.current), before[1]) and br.dissipated == before[3]
    assert c.scaled_residual() == before[4]
    assert np.array_equal(np.array(c._handle.download_x()), before[0])
    two = c.sensitivities(specs, adjoints=True)
    for name in ("values", "output_values", "adjoints", "scaled_residual", "info"):
        assert np.array_equal(getattr(one, name), getattr(two, name)), name
    after = _state(c)
    for b, a in zip(before, after):
        assert np.array_equal(b, a)


def test_value_table_member():
    table = gen.grid_table(60)
    vals = np.ones((3, table.ncomp))
    for b in range(3):
        vals[b, :-1] = gen.cfg4_values(b, 60)
    rng = np.random.default_rng(4)
    kind = np.array([0, 1, 0, 1, 0], dtype=np.int32)
    p = np.where(kind == 1, rng.integers(table.ncomp - 1, size=5), rng.integers(table.K, size=5)).astype(np.int32)
    q2 = np.array([-1, -1, 7, -1, 11], dtype=np.int32)
    h = _ffi.Handle(0)
    try:
        h.upload(table)
        h.upload_values(vals)
        assert h.run(False, member=2) == 0
        S, y, lam, resid, info = h.sensitivities(kind, p, q2, dense=False, adjoints=True)
    finally:
        h.close()
    assert (info == 0).all()
    G, A = oracle.assemble_fast(gen.grid_table(60, vals[2, :-1]))
    G = np.asarray(G.toarray() if hasattr(G, "toarray") else G, dtype=np.float64)
    x = np.linalg.solve(G, np.asarray(A, dtype=np.float64).ravel())
    a, b = np.asarray(table.a), np.asarray(table.b)
    moved = False
    for q in range(5):
        c = np.zeros(len(x))
        row = None
        if kind[q] == 0:
            c[p[q]] += 1.0
            if q2[q] >= 0:
                c[q2[q]] -= 1.0
        else:
            row = int(p[q])
            if a[row] >= 0:
                c[a[row]] += 1.0 / vals[2, row]
            if b[row] >= 0:
                c[b[row]] -= 1.0 / vals[2, row]
        lam_ref = np.linalg.solve(G.T, c)
        want = ref.formulas(table, lam_ref, x, vals[2], row)
        bar = ref.parity_bars(table, lam_ref, x, row, vals[2])
        assert (np.abs(S[q] - want) <= bar).all(), q
        moved = moved or (np.abs(S[q] - ref.formulas(table, lam_ref, x, vals[0], row)) > bar).any()
    assert moved, "member 0's values would have passed as well"


# ---- 9: errors -----------------------------------------------------------------------------------------------------
def test_call_order_and_empty():
    rows = _random_rows(1)
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    with pytest.raises(ValueError, match="no solution"):
        c.sensitivities([("e", "1")])
    c.solve()
    first = c.sensitivities([("e", "1"), ("i", "rs0")])
    empty = c.sensitivities([])
    assert len(empty) == 0 and empty.values.shape == (0, len(nl.component_keys)) and empty.output_values.shape == (0,)
    c.solve_sources({"a0": [1.0, 2.0]})
    with pytest.raises(_ffi.NodalHipError) as exc:
        c._handle.sensitivities([0], [0], [-1], dense=False)
    assert exc.value.status == _ffi.E_INVALID
    with pytest.raises(ValueError, match="no solution"):
        c.sensitivities([("e", "1")])
    c.solve()
    again = c.sensitivities([("e", "1"), ("i", "rs0")])
    assert np.array_equal(first.values, again.values)
    # the library refuses what resolve_outputs refuses: the current of a current source, indices out of range
    src = list(nl.component_keys).index("a0")
    for kind, p, q2 in [([1], [src], [-1]), ([0], [c._handle.n + 5], [-1]), ([1], [len(rows) + 3], [-1]), ([2], [0], [0])]:
        with pytest.raises(_ffi.NodalHipError) as exc:
            c._handle.sensitivities(kind, p, q2, dense=False)
        assert exc.value.status == _ffi.E_INVALID
    assert np.array_equal(c.sensitivities([("e", "1"), ("i", "rs0")]).values, first.values)


def test_floating_island():
    rows = _island()
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c.solve()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sens = c.sensitivities([("e", "1"), ("i", "f3"), ("v", "x3", "x17")])
    assert (sens.info > 0).all() and np.isnan(sens.values).all()
    assert sum(issubclass(i.category, MatrixRankWarning) for i in w) == 1
    small = list(gen.grid_rows(6)) + rows[-41:]  # a small version for the dense path
    cd = n.Circuit(n.Netlist.from_rows(small), sparse=False)
    with pytest.raises((np.linalg.LinAlgError, n.UnconnectedCircuitError)):
        cd.solve()
    with pytest.raises(ValueError, match="no solution"):
        cd.sensitivities([("e", "1")])
