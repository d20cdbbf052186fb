"""tests/lowdeg_reference.py pinned down without a GPU.  On hand-written networks the exact round composed with an exact
solve of S reproduces the exact solve of A; what a faultless device would export (the reference's own fp64 replay)
passes check_round; and each planted defect -- a dropped contribution, a non-independent pair, a flag not propagated, a
swapped renumbering, the asymmetric summation order -- fails its check BY NAME.  tests/test_gpu_lowdeg.py holds the
device's rounds to the same check_round."""
import numpy as np
import pytest

from tests import lowdeg_reference as ref


def _chain(n, seed=3):
    r = np.random.default_rng(seed).uniform(0.5, 2.0, n + 1)
    return n, [(k, k + 1, r[k]) for k in range(n - 1)] + [(0, n, r[n - 1]), (n - 1, n, r[n])]


def _tree(n=7, seed=4):
    r = np.random.default_rng(seed).uniform(0.5, 2.0, n)
    return n, [(0, n, r[0])] + [(c, (c - 1) // 2, r[c]) for c in range(1, n)]


def _bypass(order="outside", seed=5):
    return 4, ref.bypass_motif(order, np.random.default_rng(seed).uniform(1.0, 1000.0, 7))


def _fill_on_existing(seed=6):
    """0 - 1 - 2 with a direct 0 - 2: eliminating 1 lands on the existing entry (0, 2); 3 hangs on 2 with a parallel pair"""
    r = np.random.default_rng(seed).uniform(0.5, 2.0, 7)
    return 5, [(0, 1, r[0]), (1, 2, r[1]), (0, 2, r[2]), (2, 3, r[3]), (2, 3, r[4]), (0, 5, r[5]), (3, 4, r[6]), (4, 5, 1.5),
               (0, 4, 0.75), (2, 4, 1.25)]


NETWORKS = {"chain9": _chain(9), "tree7": _tree(), "bypass_outside": _bypass("outside"), "bypass_inside": _bypass("inside"),
            "fill": _fill_on_existing()}


def _system(name):
    n, res = NETWORKS[name]
    b = np.random.default_rng(11).uniform(-1.0, 1.0, n)
    return ref.assemble(n, res, b)


def test_priority_with_uint64_is_the_integer_formula():
    idx = np.array([0, 1, 2, 3, 255, 256, 257, 4095, 65537, 2 ** 31 - 1, 2 ** 32 - 1])
    assert [int(v) for v in ref.node_priority(idx)] == [ref._priority_int(int(i)) for i in idx]
    pri = ref.node_priority(np.arange(4096))
    assert len(set(int(p) for p in pri)) == 4096
    assert pri[1::2].min() > pri[0::2].max()  # bit 63: every odd index beats every even one


@pytest.mark.parametrize("name", list(NETWORKS))
def test_exact_round_and_exact_solve_of_S_is_the_exact_solve_of_A(name):
    indptr, indices, data, b, grounded = _system(name)
    n = len(b)
    rd = ref.Round(indptr, indices, data)
    assert rd.F.any() and not rd.adjacent_in_F() and np.all(rd.cand[rd.F])
    full = ref.exact_solve({(i, int(indices[e])): float(data[e]) for i in range(n) for e in range(indptr[i], indptr[i + 1])}, b, n)
    keys = sorted(rd.lists())
    S = {key: v for key, (v, _, _) in zip(keys, rd.exact_values())}
    bc = [v for v, _, _ in rd.exact_rhs(b)]
    xc = ref.exact_solve(S, bc, rd.nk)
    rec = rd.exact_recovery(b, xc)
    x = [xc[rd.newidx[i]] if not rd.F[i] else rec[i][0] for i in range(n)]
    assert x == full
    # the pattern: columns ascending, the diagonal found, S symmetric as a set
    ip, ix, dp = rd.pattern()
    for r in range(rd.nk):
        cols = list(ix[ip[r]:ip[r + 1]])
        assert cols == sorted(set(cols)) and ix[dp[r]] == r
    assert all((c, r) in S and S[(c, r)] == S[(r, c)] for r, c in S)


@pytest.mark.parametrize("name", list(NETWORKS))
def test_a_faultless_replay_passes_every_check(name):
    indptr, indices, data, b, grounded = _system(name)
    rd = ref.Round(indptr, indices, data)
    dev = rd.emulate(b, grounded)
    xc = np.random.default_rng(2).uniform(-1.0, 1.0, rd.nk)
    dev["x"], dev["p_x"] = xc, rd.float_recovery(b, xc)
    ratios = {}
    assert ref.check_round(indptr, indices, data, dev, ratios=ratios) == []
    assert set(ratios) == {"S", "b", "x"} and max(ratios.values()) <= 1.0


def test_fill_lands_on_an_existing_entry_and_parallel_resistors_add():
    indptr, indices, data, b, grounded = _system("fill")
    rd = ref.Round(indptr, indices, data)
    assert rd.F[1] and not rd.F[0] and not rd.F[2]
    items = rd.lists()[(int(rd.newidx[0]), int(rd.newidx[2]))]
    assert sorted(slot for _, slot, _ in items) == [0, 2]  # the direct resistor and the path through node 1
    dense = np.zeros((5, 5))
    for i in range(5):
        dense[i, indices[indptr[i]:indptr[i + 1]]] = data[indptr[i]:indptr[i + 1]]
    n, res = NETWORKS["fill"]
    assert dense[2, 3] == -(1.0 / res[3][2] + 1.0 / res[4][2]) and dense[2, 3] == dense[3, 2]


def _differing_bypass():
    """The first bypass motif (conductances 1 / U(1, 1000)) whose two summation orders give different bits."""
    for seed in range(200):
        n, res = _bypass("outside", seed)
        indptr, indices, data, b, grounded = ref.assemble(n, res, np.ones(n))
        rd = ref.Round(indptr, indices, data)
        assert list(rd.F) == [False, True, True, False]
        v = rd.float_values("contrib")
        pos = {key: p for p, key in enumerate(sorted(rd.lists()))}
        if v[pos[(0, 1)]] != v[pos[(1, 0)]]:
            return indptr, indices, data, b, grounded, rd
    raise AssertionError("no draw shows the asymmetry")


def test_planted_defects_fail_by_name():
    failed = {}

    def names(indptr, indices, data, dev):
        return sorted(set(f.split(":")[0] for f in ref.check_round(indptr, indices, data, dev)))

    indptr, indices, data, b, grounded = _system("chain9")
    rd = ref.Round(indptr, indices, data)
    # a dropped contribution: one term of one diagonal entry left out
    dev = rd.emulate(b, grounded)
    pos = next(p for p, (_, _, m) in enumerate(rd.exact_values()) if m >= 2)
    dev["data"] = dev["data"].copy()
    dev["data"][pos] = float(rd.exact_values(drop=(pos, 1))[pos][0])
    failed["dropped contribution"] = names(indptr, indices, data, dev)
    assert "values.bound" in failed["dropped contribution"]
    # a non-independent pair: a neighbour of a node of F taken too
    F = rd.F.copy()
    i = int(np.nonzero(F)[0][0])
    F[i + 1] = True
    dev = rd.emulate(b, grounded)
    dev["p_newidx"] = ref.renumber(F)
    failed["non-independent pair"] = names(indptr, indices, data, dev)
    assert "selection.independent" in failed["non-independent pair"]
    # a flag not propagated: only an eliminated node touches ground, and its kept neighbours do not hear of it
    g = np.zeros(9, dtype=np.uint8)
    g[i] = 1
    dev = rd.emulate(b, g)
    assert dev["grounded"].sum() == 2  # both kept neighbours inherit it
    dev["grounded"] = np.zeros_like(dev["grounded"])
    failed["flag not propagated"] = names(indptr, indices, data, dev)
    assert failed["flag not propagated"] == ["flags"]
    # a swapped renumbering: two kept nodes exchange their ranks
    dev = rd.emulate(b, grounded)
    kept = np.nonzero(~rd.F)[0]
    dev["p_newidx"] = dev["p_newidx"].copy()
    dev["p_newidx"][kept[0]], dev["p_newidx"][kept[1]] = dev["p_newidx"][kept[1]], dev["p_newidx"][kept[0]]
    failed["swapped renumbering"] = names(indptr, indices, data, dev)
    assert failed["swapped renumbering"] == ["renumbering"]
    # the asymmetric summation order: within the bound, yet S(i, k) != S(k, i)
    indptr, indices, data, b, grounded, rd = _differing_bypass()
    failed["asymmetric order"] = names(indptr, indices, data, rd.emulate(b, grounded, order="contrib"))
    assert failed["asymmetric order"] == ["values.symmetry"]
    assert names(indptr, indices, data, rd.emulate(b, grounded, order="fixed")) == []
    assert all(failed.values()), failed


def test_leftover_rule_and_union_find():
    assert ref.leftover(np.array([0, 1, 3, 5]), np.array([0, 1, 1])) and not ref.leftover(np.array([0, 1, 3, 5]), np.array([1, 0, 0]))
    assert ref.leftover(np.array([0, 0]), np.array([0]))
    # two components: {0, 1, 2} and {3, 4}
    indptr, indices = np.array([0, 2, 5, 7, 9, 11]), np.array([0, 1, 0, 1, 2, 1, 2, 3, 4, 3, 4])
    assert ref.floating_component(indptr, indices, [0, 0, 1, 0, 0]) == 1
    assert ref.floating_component(indptr, indices, [0, 0, 1, 0, 1]) == 0
    assert ref.floating_component(indptr, indices, [0, 0, 0, 0, 0]) == 1
    assert ref.floating_component(np.array([0, 0]), np.array([], dtype=int), [1]) == 0
    assert ref.floating_component(np.array([0, 0]), np.array([], dtype=int), [0]) == 1


def test_floating_chain_collapses_to_a_leftover_in_the_predicted_round():
    """A floating chain of 3 next to a grounded chain: rounds on the reference alone until the leftover shows."""
    n = 12
    res = [(k, k + 1, 1.0 + 0.1 * k) for k in range(8)] + [(0, n, 1.0), (8, n, 2.0), (9, 10, 1.0), (10, 11, 3.0)]
    indptr, indices, data, b, grounded = ref.assemble(n, res, np.ones(n))
    assert ref.floating_component(indptr, indices, grounded) == 1
    for r in range(6):
        rd = ref.Round(indptr, indices, data)
        assert rd.F.any()
        ip, ix, dp = rd.pattern()
        gc = rd.flags(grounded)
        if ref.leftover(ip, gc):
            break
        indptr, indices, data, grounded = ip, ix, rd.float_values(), gc
    else:
        raise AssertionError("no leftover")
    assert r <= 2
    lone = np.nonzero((np.diff(ip) <= 1) & (gc == 0))[0]
    # its diagonal cancels but for the rounding of the rounds before (the parent is the fp64 S of the last round): the
    # entry stays in the pattern, and the verdict is structural
    v, T, _ = rd.exact_values()[dp[lone[0]]]
    assert len(lone) == 1 and T > 0 and abs(v) <= 4 * ref.U * T
