"""The presolve (nodal_amd/csrc/presolve.hip) and the scan under its renumbering (nodal_amd/csrc/scan.hip) piece by piece
against tests/presolve_reference.py: the elimination stated as linear algebra on the original assembled system.  A whole
solve hides this stage better than any other: presolve_solve accepts its answer only on the original system's residual
and otherwise hands the system, without a word, to the full-system FGMRES or the pivoted LU -- a wrong rewritten row, a
stale stamping list or a current recovered one level too early gives a correct number by a path many times slower.
Here nothing is behind the pieces: nodal_debug_presolve_build runs plan, rewrite and the reduced assembly as a solve does
and exports them, nodal_debug_presolve_recover runs the recovery kernels on any y, nodal_debug_scan_u32 runs the scan.

Bars.  Exact, or the reference's a-priori first-order bound per value (its docstring) times BAR = 2, the project's bar
(tests/test_gpu_fgmres.py).  The reduced system is built from the DEVICE's own export_csr and its own exported plan,
after the reference's identities have held for that plan: a wrong expression fails by name.  A structurally zero entry
has bound 0: the device holds an exact 0 there or nothing.

Cases.  The families of presolve_reference.families() (6 x 6 grids, 35 to 38 nodes; `combined` 8 x 8), whose plans are
written by hand there; _stubborn_sources(12, kind) of tests/test_gpu_parity.py (161 / 162 nodes, 33 / 34 branches);
cfg5_table(32): 2020 components, nc + 1 = 2021, one scan tile; cfg5_table(33): 2152, two tiles; _grid_with_sources(46):
K + 1 = 2132 nodes, two tiles of the node scan (4188 components); cfg5_table(730): 1082893 components > 4096 * 256 =
1048576, every grid-stride loop takes a second trip (540829 nodes, 10622 branches), reference in float64 scipy sparse.

MEASURED on MI355X (worst device error / bound per case and quantity, as each test prints it; the bar is 2).  R, r: the
reduced matrix and right-hand side; pot: recovered pivot potentials; cur: recovered currents; any y: branch rows and
pivots' KCL rows of the original system for two random y; y*: every row of G x - b at the reference's reduced solution.

  case                   R      r       pot    cur    any y  y*
  e_ground               0.11   0.032   0      0.038  0.015  0.044
  e_floating             0.12   0.082   0.17   0.13   0.034  0.061
  stack3                 0      0.047   0      0.085  0.032  0.057
  shared_base            0.028  0.031   0      0.044  0.019  0.038
  e_zero                 0.11   0       0      0.039  0.016  0.048
  parallel_r             0.10   0.073   0.11   0.14   0.052  0.027
  a_on_pivot             0.10   0.073   0.11   0.019  0.022  0.048
  vcvs_surviving         0.023  0       0.22   0.052  0.040  0.051
  vcvs_pivot_control     0.11   0.032   0.13   0.14   0.041  0.036
  vcvs_one_base          0.11   0.032   0      0.15   0.055  0.031
  ccvs                   0.035  0       0.091  0.075  0.033  0.057
  cccs_driver_on_pivot   0.11   0.060   0      0.071  0.027  0.047
  cccs_output_pivot      0.10   0.030   0      0.084  0.032  0.051
  stubborn_cascade       0.11   0.032   0      0.074  0.029  0.043
  stubborn_feedback      0.11   0.032   0      0.035  0.014  0.059
  stubborn_stacked       0.11   0.032   0      0.074  0.029  0.10
  vcvs_c_eq_d            0      0       0      0.086  0.029  0.052
  combined               0.11   0.086   0.23   0.10   0.040  0.046
  cascade (12 x 12)      0.064  0.0088  0.17   0.22   0.075  0.12
  feedback               0.064  0.0088  0.21   0.21   0.050  0.072
  stacked                0.069  0.0096  0.30   0.22   0.075  0.059
  cfg5_32, cfg5_33       0      0       0             0.026         (unit resistors: every sum is exact)
  grid_with_sources_46   0      0       0.20          0.078
  cfg5_730               0      0       0.31          0.10
  sweep, members 0 .. 7  <= 0.14  <= 0.082
  A pivot potential with bound 0 (a constant alone, or a base plus zero) is met exactly.  No ratio is above 0.5.
  The hooks found no defect in the kernels.  Times: the whole file 3.4 s; the child under NODAL_PRESOLVE_KEEP=0 0.8 s,
  cfg5_730 0.44 s, each of the two largest scans 0.21 s, every other case under 0.25 s.

PLANTED by hand in a scratch copy of the library, each run against this file (and, where safe, against the whole-solve
presolve tests of test_gpu_parity.py / test_gpu_kernels.py, which passed but for the trace assertion of
test_presolve_resolves_chains_of_sources):
  recover_currents in descending level order    test_recovery[stack3, cccs_output_pivot, combined]: NaN left
  the sign of the sy.g term in rewrite_hits     test_reduced_system[vcvs_surviving, ccvs, combined]
  the CCVS gain without its minus               test_plan[ccvs, stubborn_stacked], I1 in test_reduced_system and
                                                test_recovery[ccvs, stubborn_stacked, cascade, feedback, stacked],
                                                test_shapes[grid_with_sources_46]
  place_extras not renumbering c                test_reduced_system[cccs_output_pivot] (plan and reduced tests of the
                                                small families only: an unrenumbered column stays inside their buffers)
  the fingerprint not mixing nx                 NOTHING, and rightly: the rewritten rows themselves are mixed and the
                                                component count is compared next to the key.  Not mixing the rows
                                                fails test_value_sweep (members 2 and 3: as many rows, other nodes)
  scan_tiles_direct dropping the last tile      test_scan_is_cumsum[2049, 4097, 16777216, 16777217] (scan tests only:
                                                every assembly scans)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd import generators as gen
from nodal_amd.lowering import lower
from tests import presolve_reference as ref
from tests.test_gpu_parity import _grid_with_sources, _stubborn_sources

pytestmark = pytest.mark.gpu

LD = ref.LD
U = ref.U
BAR = 2.0  # over the first-order bound, for the second-order terms
FAMILIES = ref.families()
OK = [name for name, (_, plan) in FAMILIES.items() if plan["ok"]]
STUBBORN = ("cascade", "feedback", "stacked")
_runs = {}


@pytest.fixture(scope="module", autouse=True)
def close_cached_handles():
    yield
    for case in list(_runs):
        _runs.pop(case)[0].close()


def open_handle(table):
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    return h


def exported(h):
    indptr, indices, data, rhs = h.export_csr()
    G = sp.csr_matrix((data, indices, indptr), shape=(h.n, h.n))
    G.sort_indices()
    return G, rhs


def reduced_csr(out):
    nn = out["n"]
    A = sp.csr_matrix((out["r_data"], out["r_indices"], out["r_indptr"]), shape=(nn, nn))
    A.sort_indices()
    return A


def table_of(case):
    if case in FAMILIES:
        return FAMILIES[case][0].table()
    if case in STUBBORN:
        return lower(n.Netlist.from_rows(_stubborn_sources(12, case)))
    if case == "grid_with_sources_46":
        return lower(n.Netlist.from_rows(_grid_with_sources(46, 3)))
    return gen.cfg5_table(int(case.split("_")[1]))


def run(case):
    """One build on a fresh handle (cached, the handle stays open for the recovery tests): (h, table, out, G, b)."""
    if case not in _runs:
        table = table_of(case)
        h = open_handle(table)
        out = h.debug_presolve_build()
        G, b = exported(h)
        _runs[case] = (h, table, out, G, b)
    return _runs[case]


def ratio(err, bound):
    """The worst err / bound; an error where the bound is 0 counts as inf."""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0.0))
    return float(np.max(r))


# ---- 4.1 the plan, family by family -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FAMILIES))
def test_plan_is_the_hand_written_one(name):
    net, plan = FAMILIES[name]
    h, table, out, G, b = run(name)
    K, B = table.K, table.B
    assert (out["K"], out["B"]) == (K, B)
    assert bool(out["ok"]) == plan["ok"], name
    if not plan["ok"]:
        assert not out["built"]
        return
    dev = ref.plan_from_export(out)
    assert out["built"] == 1
    assert list(out["pivots"]) == sorted(plan["exprs"]) == sorted(dev["exprs"])
    assert out["Kr"] == K - len(plan["exprs"]) and out["npivots"] == len(plan["exprs"])
    sources = sum(abs(r[1]) for r in net.rows if r[0] == ref.T_E)
    gains = max([abs(e[4]) for e in plan["exprs"].values()] + [1.0])
    for p, (q, cst, c, d, g) in plan["exprs"].items():
        dq, dcst, dc, dd, dg = dev["exprs"][p]
        assert (dq, dc, dd) == (q, c, d), (name, p, dev["exprs"][p])
        assert abs(dcst - cst) <= BAR * 3 * U * sources * gains, (name, p, dcst, cst)  # (two or three operations)
        assert abs(dg - g) <= BAR * 2 * U * abs(g), (name, p, dg, g)
    assert len(dev["kept"]) == len(plan["kept"]) == out["nkept"]
    for got, want in zip(dev["kept"], plan["kept"]):
        assert got[:2] + got[3:] == want[:2] + want[3:], (name, got, want)
        assert abs(got[2] - want[2]) <= BAR * 2 * U * abs(want[2])
    assert dev["level_of"] == plan["level_of"], name
    assert out["max_level"] == max(plan["level_of"])
    Gd = G.toarray()
    for kk, (row, level) in enumerate(zip(out["row_of"], out["level_of"])):
        if level >= 1:  # the pivot whose KCL row holds this branch's current
            assert row in plan["exprs"] and Gd[row, K + kk] != 0
        else:
            assert row == K + kk
    assert out["n"] == out["Kr"] + out["nkept"]
    if plan["kept"]:
        assert out["nkept"] > 0 and out["n"] > out["Kr"]  # B' > 0, and the rest of the network is still eliminated
        assert out["npivots"] == B - out["nkept"]


def test_an_e_of_value_zero_emits_no_current_source_and_a_parallel_resistor_is_dropped():
    for name, kind, change in (("e_zero", ref.T_A, 0), ("parallel_r", ref.T_R, -2)):
        net = FAMILIES[name][0]
        out = run(name)[2]
        before = sum(1 for r in net.rows if r[0] == kind)
        assert np.count_nonzero(out["r_type"] == kind) == before + change, name


@pytest.mark.parametrize("kind", STUBBORN)
def test_stubborn_sources_stay_and_the_rest_is_eliminated(kind):
    h, table, out, G, b = run(kind)
    assert out["ok"] and out["built"]
    assert out["nkept"] > 0 and out["n"] == out["Kr"] + out["nkept"] > out["Kr"]
    ncccs = int(np.count_nonzero(np.asarray(table.type) == ref.T_CCCS))
    assert out["npivots"] == table.B - out["nkept"] - ncccs > 0
    assert set(out["level_of"][out["kept_kk"]]) == {-1}
    assert not out["passive"]


def test_without_keep_a_stubborn_source_ends_the_plan():
    """NODAL_PRESOLVE_KEEP is read once per process: tests/presolve_child.py builds the three kinds under 0."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "presolve_child.py")],
                       env=dict(os.environ, NODAL_PRESOLVE_KEEP="0"), cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "presolve child" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = json.loads(r.stdout.split("presolve child", 1)[1])
    assert got == {k: {"ok": 0, "built": 0} for k in STUBBORN + tuple("stubborn_" + k for k in STUBBORN)}, got


# ---- 4.2 the reduced system ---------------------------------------------------------------------------------------

def check_reduced_dense(case, h, table, out, G, b, values=None):
    """Identities for the device's plan, then its reduced CSR, right-hand side, newidx and kept table rows."""
    plan = ref.plan_from_export(out)
    red = ref.Reduction(G, b, table.K, plan, ref.stamps_per_node(table))
    assert red.identities(BAR) == [], case
    assert out["Kr"] == red.Kr and out["n"] == red.Kr + len(red.kept)
    Gd = reduced_csr(out).toarray()
    rG = ratio(np.abs(Gd - red.Gr), red.gGr)
    rb = ratio(np.abs(out["r_rhs"] - red.br), red.gbr)
    print(f"{case}: reduced matrix {rG:.2g} of its bound, right-hand side {rb:.2g}")
    assert rG <= BAR and rb <= BAR, (case, rG, rb)
    new, cols = ref.host_compaction(table, plan, values)
    assert np.array_equal(out["newidx"], new)
    nkeep = len(cols["type"])
    for name in ("type", "value", "a", "b", "c", "d", "k"):
        assert np.array_equal(out["r_" + name][:nkeep], cols[name]), (case, name)
    rest = slice(nkeep, None)
    for name in ("a", "b", "c", "d"):
        assert np.all((out["r_" + name][rest] >= -1) & (out["r_" + name][rest] < red.Kr)), (case, name)
    assert list(out["r_k"][rest][out["r_k"][rest] >= 0]) == list(range(len(red.kept)))
    kinds = out["r_type"]
    assert set(kinds) <= {ref.T_R, ref.T_A, ref.T_GM, ref.T_E, ref.T_VCVS}
    passive = len(red.kept) == 0 and not np.any(kinds == ref.T_GM) and bool(np.all(out["r_value"][kinds == ref.T_R] > 0))
    assert bool(out["passive"]) == passive, case
    return red


@pytest.mark.parametrize("case", OK + list(STUBBORN))
def test_reduced_system_is_the_reference(case):
    h, table, out, G, b = run(case)
    check_reduced_dense(case, h, table, out, G, b)


# ---- 4.3 recovery -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", OK + list(STUBBORN))
def test_recovery_of_any_y_and_of_the_reference_solution(case):
    h, table, out, G, b = run(case)
    K = table.K
    red = ref.Reduction(G, b, K, ref.plan_from_export(out), ref.stamps_per_node(table))
    Kr, kept = red.Kr, red.kept
    rng = np.random.default_rng(11)
    worst = {}

    def note(name, value):
        worst[name] = max(worst.get(name, 0.0), value)
    for trial in range(3):  # (a) two random y, (b) the reference's own solution of its reduced system
        solved = trial == 2
        y = (red.solve_reduced() if solved else rng.standard_normal(Kr + len(kept))).astype(np.float64)
        x = h.debug_presolve_recover(y)
        assert not np.isnan(x).any(), case
        xr, e = red.recover(y)
        surv = np.flatnonzero(red.newidx >= 0)
        assert np.array_equal(x[surv], y[red.newidx[surv]])
        assert np.array_equal(x[K + kept], y[Kr:])
        note("pivot potentials", ratio(np.abs(x[red.pivots] - xr[red.pivots]), e[red.pivots]))
        cur = K + np.concatenate([red.elim, red.cccs]).astype(np.int64)
        note("currents", ratio(np.abs(x[cur] - xr[cur]), e[cur]))
        bound = red.residual_bounds(x, e, y, solved)
        hold = np.isfinite(bound)
        assert hold.sum() == (red.n if solved else len(red.pivots) + len(red.elim) + len(red.cccs))
        r = np.abs(red.G @ x.astype(LD) - red.b)
        note("rows of G x - b at y*" if solved else "branch and pivot rows, any y", ratio(r[hold], bound[hold]))
    print(f"{case}: " + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))
    assert max(worst.values()) <= BAR, (case, worst)


# ---- 4.4 shapes where the kernels' bookkeeping turns over -----------------------------------------------------------

def check_reduced_sparse(case, h, table, out, G, b):
    plan = ref.plan_from_export(out)
    s = ref.sparse_reduction(G, b, table.K, plan, ref.stamps_per_node(table))
    assert s["bad"] == [], case
    assert out["Kr"] == s["Kr"] == out["n"]
    A = reduced_csr(out)
    diff = abs(A - s["Gr"]).tocsr()
    diff.eliminate_zeros()
    rG = 0.0
    if diff.nnz:  # (an entry outside the reference's structural pattern meets the bound 0)
        d = diff.tocoo()
        rG = ratio(d.data, np.asarray(s["gGr"][d.row, d.col]).ravel())
    rb = ratio(np.abs(out["r_rhs"] - s["br"]), s["gbr"])
    print(f"{case}: reduced matrix {rG:.2g} of its bound, right-hand side {rb:.2g}")
    assert rG <= BAR and rb <= BAR, (case, rG, rb)
    new, cols = ref.host_compaction(table, plan)
    assert np.array_equal(out["newidx"], new)
    nkeep = len(cols["type"])
    for name in ("type", "value", "a", "b", "c", "d", "k"):
        assert np.array_equal(out["r_" + name][:nkeep], cols[name]), (case, name)
    return s


def check_recovery_sparse(case, h, table, out, G, b, s):
    """T y + t0 on the nodes, no NaN, and the rows that hold whatever y is: eliminated branch rows, the pivots' KCL rows
    (the device's own current closes each), CCCS rows."""
    K, Kr = table.K, s["Kr"]
    y = np.random.default_rng(5).standard_normal(Kr)
    x = h.debug_presolve_recover(y)
    assert not np.isnan(x).any()
    want = s["T"] @ y + s["t0"]
    e = np.zeros(h.n)
    e[s["pivots"]] = 2 * 4 * U * (abs(s["T"]) @ np.abs(y) + np.abs(s["t0"]))[s["pivots"]]
    surv = np.flatnonzero(s["newidx"] >= 0)
    assert np.array_equal(x[surv], y[s["newidx"][surv]])
    rp = ratio(np.abs(x[:K] - want)[s["pivots"]], e[s["pivots"]])
    aG = abs(G).tocsr()
    entries = np.diff(G.indptr)
    own = 2 * U * (entries + 2) * (aG @ np.abs(x) + np.abs(b)) + aG @ e
    through = abs(s["T"]) @ np.abs(y) + np.abs(s["t0"])
    rows_el = K + s["elim"]
    own[rows_el] = 2 * U * (entries[rows_el] + 6) * (aG[rows_el][:, :K] @ through + np.abs(b[rows_el])) + aG[rows_el][:, :K] @ e[:K]
    hold = np.concatenate([s["pivots"], rows_el, K + s["cccs"]])
    r = np.abs(G @ x - b)
    rr = ratio(r[hold], own[hold])
    print(f"{case}: pivot potentials {rp:.2g}, branch and pivot rows {rr:.2g}")
    assert rp <= BAR and rr <= BAR, (case, rp, rr)


@pytest.mark.parametrize("case", ["cfg5_32", "cfg5_33", "grid_with_sources_46", "cfg5_730"])
def test_shapes_where_the_bookkeeping_turns_over(case):
    h, table, out, G, b = run(case)
    assert out["ok"] and out["built"] and out["nkept"] == 0
    tiles = lambda items: -(-items // 2048)  # noqa: E731
    want = {"cfg5_32": (1, 1), "cfg5_33": (2, 1), "grid_with_sources_46": (3, 2), "cfg5_730": (529, 265)}[case]
    assert (tiles(table.ncomp + 1), tiles(table.K + 1)) == want
    if case == "cfg5_730":
        assert table.ncomp > 4096 * 256
    s = check_reduced_sparse(case, h, table, out, G, b)
    check_recovery_sparse(case, h, table, out, G, b, s)
    if case == "cfg5_730":  # (the only handle of this size: not kept)
        _runs.pop(case)[0].close()


# ---- 4.5 a value sweep on one handle --------------------------------------------------------------------------------

def test_value_sweep_reuses_the_reduced_symbolic_assembly_only_for_the_same_rows():
    """upload_values + assemble_numeric(m) on one handle.  The reduced context's stamping lists may stand only while the
    emitted rows do: members 2 and 3 emit the SAME NUMBER of rows on different nodes (one of two E at exactly 0 each),
    which the counts cannot tell apart -- only the fingerprint's mixing of the rows does."""
    net = ref.Net(6)
    v = net.node()
    e1 = net.E(7, -1, 2.5)
    e2 = net.E(8, 20, 1.25)
    e3 = net.E(27, -1, 1.75)
    w = net.VCVS(v, -1, 3, 16, 0.4)
    net.R(v, 10, 1.1)
    net.R(7, 20, 1.9)  # between two pivots on different bases: its current source carries the difference of their constants
    table = net.table()
    base = np.asarray(table.value, dtype=np.float64).copy()
    rng = np.random.default_rng(2)
    other = base * rng.uniform(0.5, 2.0, len(base))  # every value moves, no emitted row does
    zero_e1, zero_e3, zero_gain, equal_cst = other.copy(), other.copy(), other.copy(), other.copy()
    zero_e1[e1] = 0.0                  # one E at exactly 0: the current sources of its four resistors are not emitted
    zero_e3[e3] = 0.0                  # ... the other one: as many rows as before, elsewhere
    zero_gain[w] = 0.0                 # the gain gone: the control term and its transconductance row vanish
    equal_cst[e2] = -equal_cst[e1]     # e_20 = e_8 + E1: the two constants cancel in the resistor between the pivots
    members = np.stack([base, other, zero_e1, zero_e3, zero_gain, equal_cst, base, other])
    reused = [0, 1, 0, 0, 0, 0, 0, 1]
    h = _ffi.Handle(0)
    h.upload(table)
    h.upload_values(members)
    h.assemble_symbolic()
    counts = []
    for m, want in enumerate(reused):
        assert h.assemble_numeric(m)[0] == _ffi.OK
        out = h.debug_presolve_build()
        assert out["ok"] and out["built"]
        assert out["same_topology"] == want, (m, out["same_topology"])
        counts.append(out["ncomp"])
        G, b = exported(h)
        check_reduced_dense(f"sweep member {m}", h, table.with_values(members[m]), out, G, b, members[m])
    assert counts[0] == counts[1] == counts[6] == counts[7]
    assert counts[2] == counts[3] == counts[0] - 4 and counts[4] == counts[5] == counts[0] - 1, counts
    h.close()


# ---- 4.6 the scan ---------------------------------------------------------------------------------------------------

SCAN_SIZES = [1, 255, 256, 2047, 2048, 2049, 4097, 2048 * 8192, 2048 * 8192 + 1]


@pytest.fixture(scope="module")
def scan_handle():
    h = _ffi.Handle(0)
    yield h
    h.close()


@pytest.mark.parametrize("size", SCAN_SIZES)
def test_scan_is_cumsum(scan_handle, size):
    """One tile, up to 8192 tiles with the offsets summed in place (2048 * 8192 is the last such size), the recursive
    scan above that (2048 * 8192 + 1 the first): 0 / 1 flags and counts 0 .. 4, totals below 2^32."""
    rng = np.random.default_rng(size)
    for high in (2, 5):
        values = rng.integers(0, high, size, dtype=np.uint32)
        want = np.zeros(size, dtype=np.uint64)
        np.cumsum(values[:-1], out=want[1:], dtype=np.uint64)
        total = int(want[-1]) + int(values[-1])
        assert total < 2 ** 32
        want = want.astype(np.uint32)
        combos = [(False, True), (True, True), (False, False), (True, False)]
        if size > 10 ** 6:  # (67 MB each way per call: two calls per kind of input)
            combos = combos[:2] if high == 2 else combos[2:][::-1] + combos[1:2]
        for in_place, with_total in combos:
            got, tot = scan_handle.debug_scan_u32(values, in_place=in_place, total=with_total)
            assert np.array_equal(got, want), (size, high, in_place, with_total)
            assert tot == (total if with_total else None)


# ---- 4.7 the hooks displace nothing ----------------------------------------------------------------------------------

def test_a_solve_after_the_hooks_returns_the_bits_of_a_fresh_solve(monkeypatch, capfd):
    monkeypatch.setenv("NODAL_TRACE", "1")
    table = gen.cfg5_table(40)
    fresh = open_handle(table)
    x0, info0, it0, _ = fresh.solve_sparse(method=_ffi.SPARSE_LU)
    fresh.close()
    assert info0 == 0
    h = open_handle(table)
    out = h.debug_presolve_build()
    assert out["ok"] and out["built"] and not out["same_topology"]
    y = np.random.default_rng(1).standard_normal(out["n"])
    h.debug_presolve_recover(y)
    assert h.debug_presolve_build()["same_topology"] == 1
    capfd.readouterr()
    x1, info1, it1, _ = h.solve_sparse(method=_ffi.SPARSE_LU)
    err = capfd.readouterr().err
    assert "[presolve] accepted" in err, err[-600:]
    assert info1 == 0 and it1 == it0
    assert np.array_equal(np.asarray(x1).view(np.uint64), np.asarray(x0).view(np.uint64))
    # ... and with a solution on the handle the recovery hook puts it back
    h.debug_presolve_build()
    x = h.debug_presolve_recover(y)
    assert not np.isnan(x).any()
    assert np.array_equal(h.download_x().view(np.uint64), np.asarray(x0).view(np.uint64))
    x2 = h.solve_sparse(method=_ffi.SPARSE_LU)[0]
    assert np.array_equal(np.asarray(x2).view(np.uint64), np.asarray(x0).view(np.uint64))
    h.close()
