"""The rounds of the exact low-degree elimination (nodal_amd/csrc/lowdeg.hip) taken apart, each against
tests/lowdeg_reference.py: exact rational arithmetic on the round's own parent as the DEVICE holds it.  The whole-solve
tests (test_gpu_kernels.py::test_sparse_low_degree_elimination*, test_gpu_parity.py, test_gpu_direct.py) look at
|x - x_SuperLU| <= 1e-9 after up to 48 rounds and a dense, multigrid or direct solve: a round's matrix can be far off
rounding and pass, and the documented invariants of S (bitwise symmetric, M-matrix signs, order kept, exact pattern) --
on which block_elim.hip's symmetric elimination relies for every child -- were asserted nowhere.

Handle.debug_lowdeg exports what the last solve left, round by round; ld_state and the round count come from there, not
from stderr.  NODAL_LOWDEG_SHARE=64 keeps later rounds going on every case (a knob, read per call); every network has
more than 32 unknowns, the gate of the route.

Bars.  Integers, flags and the pattern: exact.  Every double: |device - exact| <= (m + 3) u T, u = 2^-53, derived in
lowdeg_reference.py's docstring (m terms of absolute sum T); kept nodes of the recovery and S(i,k) against S(k,i): the
same bits.  Each test prints the worst error / bound per round before it asserts.

The pair sweep.  nodal_solve_pairs hands a sweep to lowdeg_solve_pairs only above 1024 unknowns (api.hip), so the
600-node ladder never reaches it: the pair test runs the same ladder with 1200 nodes; the 600-node one is among the
round cases.

MEASURED on MI355X.  Worst error / bound over every round of every case (the bar is 1): S 0.44, b_C 0.25, x_F 0.36; the
fifteen small graphs of small_floating_check agree with union-find; the whole file takes 3 s, no test above 0.3 s.
The one defect found is in test_schur_complement_is_bitwise_symmetric_on_the_bypass_motif's docstring.
"""
import numpy as np
import pytest

from nodal_amd import _ffi
from nodal_amd import generators as gen
from tests import lowdeg_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def later_rounds_keep_going(monkeypatch):
    monkeypatch.setenv("NODAL_LOWDEG_SHARE", "64")


# ---- the networks: (a, b, ohms, source node, ground); ids 0 .. ground - 1 are the unknowns ---------------------------
# generators.passive_table numbers the nodes by first appearance as a lead.  _ordered lists the resistors so that this IS
# the numbering written here (each as (smaller, larger) id, by the larger id: a node then shows up right after the one
# before it); table_of asserts it.  The permuted chain alone is listed in a shuffled order, and its numbering is whatever
# first appearance makes of that.

def _ordered(a, b, vals):
    a, b, vals = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(vals, dtype=np.float64)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.lexsort((lo, hi))  # stable: parallel resistors keep their order
    return lo[order], hi[order], vals[order]


def _chain(n, shuffled=False, seed=1):
    rng = np.random.default_rng(seed)
    k = np.arange(n - 1)
    a, b, vals = np.append(k, 0), np.append(k + 1, n), rng.uniform(0.5, 2.0, n)
    if shuffled:
        order = rng.permutation(n)
        return a[order], b[order], vals[order], n - 1, n
    return _ordered(a, b, vals) + (n - 1, n)


def _ladder(n, every=5, seed=2, extra=()):
    """n nodes in series, a shunt to ground at every fifth; extra: resistors (a, b) on ids n .. (floating islands)"""
    rng = np.random.default_rng(seed)
    ground = 1 + max(max(e) for e in extra) if extra else n
    k = np.arange(n - 1)
    taps = np.arange(0, n, every)
    a = np.concatenate([k, taps, [e[0] for e in extra]])
    b = np.concatenate([k + 1, np.full(len(taps), ground), [e[1] for e in extra]])
    vals = np.concatenate([rng.uniform(0.5, 2.0, n - 1), rng.uniform(50.0, 200.0, len(taps)), rng.uniform(0.5, 2.0, len(extra))])
    return _ordered(a, b, vals) + (n - 1, ground)


def _tree(n=511, seed=3):
    rng = np.random.default_rng(seed)
    child = np.arange(1, n)
    return _ordered(np.append(child, 0), np.append((child - 1) // 2, n), rng.uniform(0.5, 2.0, n)) + (n - 1, n)


def _motifs(kind, repeats, seed=4):
    """Disjoint copies of lowdeg_reference's small motifs, each tied to ground; values over six decades (bypass)."""
    rng = np.random.default_rng(seed)
    size = 4 if kind == "bypass" else 5
    ground = size * repeats
    a, b, v = [], [], []
    for m in range(repeats):
        if kind == "bypass":
            res = ref.bypass_motif("outside" if m % 2 == 0 else "inside", 10.0 ** rng.uniform(-3.0, 3.0, 7))
        else:  # 0 - 1 - 2 with a direct 0 - 2 (the fill lands on it), a parallel pair 2 = 3, and ties that keep 0, 2, 4 busy
            r = rng.uniform(0.5, 2.0, 10)
            res = [(0, 1, r[0]), (1, 2, r[1]), (0, 2, r[2]), (2, 3, r[3]), (2, 3, r[4]), (0, 5, r[5]), (3, 4, r[6]), (4, 5, r[7]),
                   (0, 4, r[8]), (2, 4, r[9])]
        for p, q, ohms in res:
            a.append(size * m + p if p < size else ground)
            b.append(size * m + q if q < size else ground)
            v.append(ohms)
    return _ordered(a, b, v) + (1, ground)


def _grid_with_wires(side=20, wires=6, length=40, seed=5):
    rng = np.random.default_rng(seed)
    idx = np.arange(side * side).reshape(side, side)
    a = [idx[:, :-1].ravel(), idx[:-1, :].ravel(), [0]]
    b = [idx[:, 1:].ravel(), idx[1:, :].ravel(), [-1]]
    n = side * side
    for w in range(wires):
        nodes = np.arange(n, n + length)
        start = int(idx[3 * w + 1, 2 * w + 1])
        a += [[start], nodes[:-1]]
        b += [[nodes[0]], nodes[1:]]
        if w % 2:  # every other wire comes back to the grid; the others dangle
            a.append([nodes[-1]])
            b.append([int(idx[side - 2 - w, side - 3])])
        n += length
    a, b = np.concatenate(a).astype(np.int64), np.concatenate(b).astype(np.int64)
    b[b < 0] = n
    return _ordered(a, b, rng.uniform(0.5, 2.0, len(a))) + (n - 1, n)


REGULAR = {
    "chain33": lambda: _chain(33),
    "chain257": lambda: _chain(257),
    "chain300_permuted": lambda: _chain(300, shuffled=True, seed=7),
    "ladder600": lambda: _ladder(600),
    "tree511": lambda: _tree(511),
    "bypass100": lambda: _motifs("bypass", 100),
    "fill_and_parallel": lambda: _motifs("fill", 10),
    "grid20_wires40": lambda: _grid_with_wires(),
}
FLOATING = {
    "floating_chain2": lambda: _ladder(64, extra=[(64, 65)]),
    "floating_chain3": lambda: _ladder(64, extra=[(64, 65), (65, 66)]),
    "floating_ring3": lambda: _ladder(64, extra=[(64, 65), (65, 66), (66, 64)]),
    "floating_chain40": lambda: _ladder(1200, extra=[(1200 + k, 1201 + k) for k in range(39)]),
}
CONSECUTIVE = ("chain33", "chain257")
_runs = {}


@pytest.fixture(scope="module", autouse=True)
def close_cached_handles():
    yield
    for case in list(_runs):
        _runs.pop(case)["h"].close()


def as_table(a, b, vals, src, ground, numbered_as_written=True):
    table = gen.passive_table(a, b, vals, src, ground)
    same = np.array_equal(table.a[:-1], np.where(a == ground, -1, a)) and np.array_equal(table.b[:-1], np.where(b == ground, -1, b))
    assert same == numbered_as_written and table.K == ground
    return table


def table_of(case, values=None):
    a, b, vals, src, ground = {**REGULAR, **FLOATING}[case]()
    return as_table(a, b, vals if values is None else values, src, ground, case != "chain300_permuted")


def open_handle(table):
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    return h


def solve_and_export(h):
    x, info, _, _ = h.solve_sparse()
    indptr, indices, data, rhs = h.export_csr()
    return dict(h=h, x=np.array(x), info=info, rounds=h.debug_lowdeg(), indptr=indptr, indices=indices, data=data, rhs=rhs)


def run(case):
    """One solve on a fresh handle and what the hook exports after it (cached; the reference never changes it)."""
    if case not in _runs:
        _runs[case] = solve_and_export(open_handle(table_of(case)))
    return _runs[case]


def parents(out):
    """(indptr, indices, data) of every round's parent: the handle's matrix, then the child of the round before."""
    yield out["indptr"], out["indices"], out["data"]
    for rd in out["rounds"][:-1]:
        yield rd["indptr"], rd["indices"], rd["data"]


def check_rounds(out, consecutive=False, label=""):
    bad = []
    for r, (rd, (indptr, indices, data)) in enumerate(zip(out["rounds"], parents(out))):
        ratios = {}
        found = ref.check_round(indptr, indices, data, rd, consecutive_chain=consecutive, ratios=ratios)
        print("%s round %d: %d -> %d unknowns, error / bound %s" % (
            label, r, rd["n"], rd["child_n"], " ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))
        bad += ["round %d: %s" % (r, f) for f in found]
    return bad


def same_exports(one, two):
    assert len(one) == len(two)
    for r, (p, q) in enumerate(zip(one, two)):
        for name in _ffi.LOWDEG_INFO:
            assert p[name] == q[name], (r, name)
        for name, _ in _ffi.LOWDEG_ARRAYS:
            assert p[name].tobytes() == q[name].tobytes(), (r, name)


# ---- the route, the chain of rounds ------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(REGULAR))
def test_the_solve_takes_the_route_and_the_rounds_hang_together(case):
    out = run(case)
    rounds = out["rounds"]
    assert out["info"] == 0 and len(rounds) >= 1
    assert rounds[0]["n"] == len(out["rhs"]) > 32 and rounds[0]["nnz"] == len(out["data"])
    assert rounds[0]["p_rhs"].tobytes() == out["rhs"].tobytes()
    assert rounds[0]["p_x"].tobytes() == out["x"].tobytes()
    for r, rd in enumerate(rounds):
        assert rd["ld_state"] == 2 and rd["ld_rounds"] == r + 1
        assert rd["child_n"] < rd["n"] and len(rd["indptr"]) == rd["child_n"] + 1 and len(rd["data"]) == rd["child_nnz"]
        assert len(rd["contrib"]) == rd["ncontrib"] and len(rd["p_x"]) == rd["n"] and len(rd["x"]) == rd["child_n"]
        if r:
            up = rounds[r - 1]
            assert (rd["n"], rd["nnz"]) == (up["child_n"], up["child_nnz"])
            for mine, theirs in (("p_rhs", "rhs"), ("p_grounded", "grounded"), ("p_x", "x")):
                assert rd[mine].tobytes() == up[theirs].tobytes(), (r, mine)
    if case in CONSECUTIVE:  # half of a consecutively numbered chain per round, down to the gate of 32 unknowns
        assert [rd["child_n"] for rd in rounds] == [n for n in (129, 65, 33, 17, 9) if n < rounds[0]["n"]][:len(rounds)]
        assert rounds[-1]["child_n"] <= 32


@pytest.mark.parametrize("case", list(REGULAR))
def test_every_round_against_the_exact_reference(case):
    """Selection, renumbering, pattern, lists, values, signs, symmetry, right-hand side, flags and recovery of every
    exported round (lowdeg_reference.check_round names what fails)."""
    assert check_rounds(run(case), case in CONSECUTIVE, case) == []


def test_schur_complement_is_bitwise_symmetric_on_the_bypass_motif():
    """i < f1 < f2 < k (and f1 < i < k < f2) with a direct resistor i - k and two bypasses taken in ONE round: S(i,k) sums
    the pass-through entry and the two products in an order that must not depend on the row.

    FOUND on MI355X before the fix of schur_values (contributions summed in list order, ascending column of the source
    entry): round 0 of this case, 7 of the 50 motifs with i < f1 < f2 < k differed in the last bit, none of the other
    order -- first S(4,5) = -0x1.64ec25c0b475ep-8 against S(5,4) = -0x1.64ec25c0b475fp-8 (parent nodes 8 and 11), then
    S(32,33) = -0x1.62a662ab96f91p-3 against S(33,32) = ...92p-3 and S(92,93) = -0x1.3ec49a3d88074p-1 against ...75p-1.
    The reference's fp64 replay of that order (float_values("contrib")) names the same 7 pairs.  schur_values now adds
    the pass-through entry first and the eliminated neighbours in their stored order, the same sequence in both rows."""
    out = run("bypass100")
    rd = out["rounds"][0]
    assert rd["n"] == 400 and rd["child_n"] == 200  # both bypass nodes of every motif go in the first round
    dense = np.zeros((200, 200))
    rows = np.repeat(np.arange(200), np.diff(rd["indptr"]))
    dense[rows, rd["indices"]] = rd["data"]
    differ = np.argwhere(dense.view(np.uint64) != dense.T.copy().view(np.uint64))
    print("asymmetric entries:", [(int(r), int(c), float(dense[r, c]).hex(), float(dense[c, r]).hex()) for r, c in differ[:6]],
          len(differ) // 2, "pairs")
    assert len(differ) == 0


# ---- floating sub-networks ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(FLOATING))
def test_floating_leftover_is_found_in_the_round_the_reference_predicts(case):
    out = run(case)
    rounds = out["rounds"]
    assert out["info"] > 0 and np.isnan(out["x"]).all()
    # the reference alone, from the handle's matrix and flags: rounds until a row of at most one entry is not grounded
    indptr, indices, data, grounded = out["indptr"], out["indices"], out["data"], rounds[0]["p_grounded"]
    assert ref.floating_component(indptr, indices, grounded) == 1
    for predicted in range(_ffi.LOWDEG_MAX_ROUNDS):
        rd = ref.Round(indptr, indices, data)
        ip, ix, _ = rd.pattern()
        gc = rd.flags(grounded)
        if ref.leftover(ip, gc):
            break
        indptr, indices, data, grounded = ip, ix, rd.float_values(), gc
    assert [rd["ld_state"] for rd in rounds] == [2] * predicted + [3]
    # (a chain of 2 loses a node at once; the middle of 64 - 65 - 66 goes first and leaves the pair 64 - 66; a ring of 3
    # loses one node per round; 40 nodes halve down to a handful first)
    assert predicted in {"floating_chain2": (0,), "floating_chain3": (1,), "floating_ring3": (1,), "floating_chain40": (4, 5)}[case]
    # ... and round by round on the device's own parents: the verdict is the leftover rule, the rest as ever
    for rd in rounds:
        assert (3 if ref.leftover(rd["indptr"], rd["grounded"]) else 2) == rd["ld_state"]
        assert len(rd["x"]) == 0 or rd["ld_state"] == 2
    assert check_rounds(out, False, case) == []


def test_no_leftover_verdict_on_the_regular_cases():
    for case in REGULAR:
        out = run(case)
        for rd in out["rounds"]:
            assert not ref.leftover(rd["indptr"], rd["grounded"]), case
        last = out["rounds"][-1]
        assert ref.floating_component(last["indptr"], last["indices"], last["grounded"]) == 0, case


# ---- reuse of the kept lists -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["ladder600", "grid20_wires40", "bypass100"])
def test_repeated_solve_on_kept_lists_exports_the_bits_of_a_fresh_build(case):
    a, b, vals, src, ground = REGULAR[case]()
    new = vals * np.random.default_rng(17).uniform(0.5, 2.0, len(vals))
    h = open_handle(table_of(case))
    first = solve_and_export(h)
    h.upload_values(np.append(new, 1.0)[None, :])
    assert h.assemble_numeric(0)[0] == _ffi.OK
    again = solve_and_export(h)  # ld_state 2 stands: values, right-hand side and recovery on the kept lists
    fresh = solve_and_export(open_handle(table_of(case, new)))
    try:
        assert again["data"].tobytes() == fresh["data"].tobytes() != first["data"].tobytes()
        same_exports(again["rounds"], fresh["rounds"])
        assert again["x"].tobytes() == fresh["x"].tobytes()
        assert check_rounds(again, False, case + " (kept lists)") == []
    finally:
        h.close()
        fresh["h"].close()


def test_nothing_of_the_old_rounds_survives_another_topology():
    h = open_handle(table_of("chain300_permuted"))
    assert len(solve_and_export(h)["rounds"]) >= 3
    other = as_table(*_chain(300, shuffled=True, seed=9), numbered_as_written=False)
    h.upload(other)
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    assert h.debug_lowdeg() == []  # the cached decision belonged to the old pattern
    again = solve_and_export(h)
    fresh = solve_and_export(open_handle(other))
    try:
        same_exports(again["rounds"], fresh["rounds"])
        assert again["x"].tobytes() == fresh["x"].tobytes()
        assert check_rounds(again, False, "second topology") == []
    finally:
        h.close()
        fresh["h"].close()


# ---- the pair sweep ----------------------------------------------------------------------------------------------------

def test_pair_sweep_goes_through_the_rounds_and_leaves_the_last_pair():
    from oracle import nodal_oracle as oracle
    import scipy.sparse.linalg as spla
    table = as_table(*_ladder(1200))
    G, _ = oracle.assemble_fast(table)
    lu = spla.splu(G.tocsc())
    ia, ib = np.array([0, 10, 3]), np.array([1199, 600, 700])
    want = []
    for p, q in zip(ia, ib):
        e = np.zeros(1200)
        e[p], e[q] = 1.0, -1.0
        want.append(e @ lu.solve(e))
    h = open_handle(table)
    try:
        got, info = h.solve_pairs(ia, ib, False)
        print("pairs", got, want)
        assert info == 0 and np.all(np.abs(got - want) <= 1e-9 * np.abs(want))
        indptr, indices, data, _ = h.export_csr()
        rounds = h.debug_lowdeg()
        assert len(rounds) >= 4 and all(rd["ld_state"] == 2 for rd in rounds)
        e = np.zeros(1200)
        e[3], e[700] = 1.0, -1.0
        assert rounds[0]["p_rhs"].tobytes() == e.tobytes()
        x = rounds[0]["p_x"]
        assert x[3] - x[700] == got[2]
        out = dict(rounds=rounds, indptr=indptr, indices=indices, data=data)
        assert check_rounds(out, False, "pairs") == []
    finally:
        h.close()


# ---- the hook leaves no trace --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["ladder600", "grid20_wires40"])
def test_a_solve_after_the_hook_returns_the_bits_of_a_solve_without_it(case):
    table = table_of(case)
    h1, h2 = open_handle(table), open_handle(table)
    try:
        x1 = np.array(h1.solve_sparse()[0])
        assert len(h1.debug_lowdeg()) >= 1
        assert h1.debug_floating_small([0, 1], [0], [1]) == 0
        y1 = np.array(h1.solve_sparse()[0])
        x2 = np.array(h2.solve_sparse()[0])
        y2 = np.array(h2.solve_sparse()[0])
        assert x1.tobytes() == x2.tobytes() and y1.tobytes() == y2.tobytes()
    finally:
        h1.close()
        h2.close()


def test_the_hook_refuses_what_is_not_there():
    import ctypes as C
    h = open_handle(table_of("chain33"))
    try:
        assert h.debug_lowdeg() == []  # nothing solved yet
        h.solve_sparse()
        rounds = h.debug_lowdeg()
        assert len(rounds) == 1
        size, buf = C.c_int64(-1), np.zeros(64)
        call = h.lib.nodal_debug_lowdeg_array
        assert call(h._h, 0, 7, None, 0, C.byref(size)) == _ffi.OK and size.value == rounds[0]["child_nnz"] * 8
        for rnd, which, cap in ((1, 7, 512), (-1, 7, 512), (0, 13, 512), (0, -1, 512), (0, 7, 8)):
            assert call(h._h, rnd, which, C.c_void_p(buf.ctypes.data), cap, C.byref(size)) == _ffi.E_INVALID, (rnd, which, cap)
        assert not buf.any()
        same_exports(h.debug_lowdeg(), rounds)
    finally:
        h.close()


# ---- small_floating_check: one workgroup, labels in LDS ------------------------------------------------------------------

def _graph(n, edges):
    """CSR with the diagonal present, as a matrix has it; columns ascending"""
    rows = [{i} for i in range(n)]
    for p, q in edges:
        rows[p].add(q)
        rows[q].add(p)
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    return indptr, np.array([j for r in rows for j in sorted(r)], dtype=np.int32)


def _path(labels):
    return [(int(labels[k]), int(labels[k + 1])) for k in range(len(labels) - 1)]


def _bit_reversal(bits):
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(1 << bits)])


def _flags(n, *on):
    g = np.zeros(n, dtype=np.uint8)
    g[list(on)] = 1
    return g


def _small_graphs():
    n = 4096
    seq, rev, bitrev = np.arange(n), np.arange(n)[::-1], _bit_reversal(12)
    pairs = [(2 * k, 2 * k + 1) for k in range(2048)]
    star = [(0, k) for k in range(1, n)]
    two = _path(np.arange(10)) + _path(np.arange(10, 20))
    p1025 = np.random.default_rng(3).permutation(1025)
    return {
        "one_grounded": (1, [], _flags(1, 0), 0),
        "one_not_grounded": (1, [], _flags(1), 1),
        "path4096_grounded_at_the_largest_label": (n, _path(seq), _flags(n, 4095), 0),
        "path4096_not_grounded": (n, _path(seq), _flags(n), 1),
        "path4096_reversed": (n, _path(rev), _flags(n, 0), 0),
        "path4096_bit_reversal": (n, _path(bitrev), _flags(n, int(bitrev[-1])), 0),
        "path4096_bit_reversal_not_grounded": (n, _path(bitrev), _flags(n), 1),
        "pairs2048_one_ungrounded": (n, pairs, _flags(n, *[2 * k + (k % 2) for k in range(2048) if k != 1371]), 1),
        "pairs2048_all_grounded": (n, pairs, _flags(n, *[2 * k + (k % 2) for k in range(2048)]), 0),
        "star4096_leaf_grounded": (n, star, _flags(n, 4095), 0),
        "star4096_not_grounded": (n, star, _flags(n), 1),
        "grounded_node_has_the_largest_label": (20, two, _flags(20, 9, 19), 0),
        "second_component_not_grounded": (20, two, _flags(20, 9), 1),
        "path1025_permuted": (1025, _path(p1025), _flags(1025, 1024), 0),
        "path1025_in_two_pieces": (1025, _path(p1025[:512]) + _path(p1025[512:]), _flags(1025, int(p1025[0])), 1),
    }


SMALL = _small_graphs()


@pytest.fixture(scope="module")
def bare_handle():
    h = _ffi.Handle(0)
    yield h
    h.close()


@pytest.mark.parametrize("name", list(SMALL))
def test_small_floating_check_against_union_find(name, bare_handle):
    n, edges, grounded, expected = SMALL[name]
    indptr, indices = _graph(n, edges)
    want = ref.floating_component(indptr, indices, grounded)
    assert want == expected
    assert bare_handle.debug_floating_small(indptr, indices, grounded) == want  # asked once


def test_small_floating_check_refuses_4097_nodes(bare_handle):
    indptr, indices = _graph(4097, _path(np.arange(4097)))
    with pytest.raises(_ffi.NodalHipError) as err:
        bare_handle.debug_floating_small(indptr, indices, _flags(4097, 0))
    assert err.value.status == _ffi.E_INVALID
    bad = indices.copy()
    bad[5] = 4096  # an index outside the graph never reaches the device either
    with pytest.raises(_ffi.NodalHipError) as err:
        bare_handle.debug_floating_small(indptr[:4097], bad[:indptr[4096]], _flags(4096, 0))
    assert err.value.status == _ffi.E_INVALID
    assert bare_handle.debug_floating_small([0, 1], [0], [1]) == 0  # the handle is as good as before
