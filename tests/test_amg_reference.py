"""tests/amg_reference.py against a hierarchy built on the host (no GPU): the clean one passes, every planted defect is
caught.

The hierarchy is a greedy pairing of a graded 24 x 24 grid (conductances 10^U(-2, 2), off-diagonals perturbed by a few
percent so that the matrix is NOT symmetric -- the general route's node block, the case the transposed block inverses
exist for) plus one isolated grounded node, whose unit vector makes the second inner step of a K-cycle vanish (the rho2
guard).  It is laid out exactly as Handle.debug_amg() exports the device's: blocks, coarse_inv, a tail image packed by the
layout rule of build_tail.  A setup defect is caught when check_amg raises; a cycle defect when it moves z by at least
1000 E, E the spread of the three fp64 orderings around the extended-precision result (amg_reference.cycle_bar)."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

from tests import amg_reference as ar

SIDE = 24
BLOCK_MAX = 32
BUDGET = 150 * 1024


def graded_matrix(seed=7):
    rng = np.random.default_rng(seed)
    n = SIDE * SIDE + 1  # (the last node is isolated: one resistor to ground)
    idx = np.arange(SIDE * SIDE).reshape(SIDE, SIDE)
    pairs = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1),
                            np.stack([idx[:-1, :].ravel(), idx[1:, :].ravel()], 1)])
    g = 10.0 ** rng.uniform(-2, 2, len(pairs))
    i, j = pairs[:, 0], pairs[:, 1]
    diag = np.zeros(n)
    np.add.at(diag, i, g)
    np.add.at(diag, j, g)
    diag[rng.choice(SIDE * SIDE, 12, replace=False)] += 10.0 ** rng.uniform(-1, 1, 12)
    diag[n - 1] = 2.0
    A = sp.coo_matrix((np.concatenate([-g, -g, diag]), (np.concatenate([i, j, np.arange(n)]),
                                                         np.concatenate([j, i, np.arange(n)]))), shape=(n, n)).tocsr()
    # rows scaled by a few percent: entry (i, j) and entry (j, i) differ, every Galerkin diagonal stays positive
    scale = 1 + 0.05 * rng.uniform(-1, 1, n)
    scale[n - 1] = 1.0
    A = (sp.diags(scale) @ A).tocsr()
    A.sort_indices()
    return A


def greedy_pairing(A, merge=None):
    """Pairs over the strongest free link in node order, leftovers join their strongest neighbour's aggregate;
    merge: two nodes whose aggregates are joined afterwards (a planted defect)."""
    n = A.shape[0]
    agg = np.full(n, -1, dtype=np.int64)
    nagg = 0
    for i in range(n):
        if agg[i] >= 0:
            continue
        cols, vals = A.indices[A.indptr[i]:A.indptr[i + 1]], -A.data[A.indptr[i]:A.indptr[i + 1]]
        free = (cols != i) & (agg[cols] < 0) & (vals > 0)
        if free.any():
            j = cols[free][np.argmax(vals[free])]
            agg[i] = agg[j] = nagg
            nagg += 1
    for i in np.nonzero(agg < 0)[0]:
        cols, vals = A.indices[A.indptr[i]:A.indptr[i + 1]], -A.data[A.indptr[i]:A.indptr[i + 1]]
        taken = (cols != i) & (agg[cols] >= 0) & (vals > 0)
        if taken.any():
            agg[i] = agg[cols[taken][np.argmax(vals[taken])]]
        else:
            agg[i] = nagg
            nagg += 1
    if merge is not None:
        a, b = agg[merge[0]], agg[merge[1]]
        agg[agg == b] = a
    return np.unique(agg, return_inverse=True)[1]


def up16(x):
    return (x + 15) & ~15


def pack_tail(levels, tail, coarse_inv):
    """The descriptor and the image by build_tail's rule: per level data, dinv, indptr, memptr, indices, agg, mem (the
    last level: nothing), coarse_inv, then the vectors."""
    nt = len(levels) - tail
    td = {"nlev": nt, "lv": []}
    off = 0
    for k in range(nt):
        lv = levels[tail + k]
        t = {name: 0 for name in ("o_data", "o_dinv", "o_indptr", "o_memptr", "o_indices", "o_agg", "o_mem", "o_B", "o_X", "o_E", "o_R")}
        t.update(n=lv["n"], nnz=lv["nnz"], nc=lv["nc"])
        if k < nt - 1:
            for name, nb in (("o_data", t["nnz"] * 8), ("o_dinv", t["n"] * 8), ("o_indptr", (t["n"] + 1) * 4),
                             ("o_memptr", (t["nc"] + 1) * 4), ("o_indices", t["nnz"] * 2), ("o_agg", t["n"] * 2),
                             ("o_mem", t["n"] * 2)):
                t[name] = off
                off = up16(off + nb)
        td["lv"].append(t)
    td["o_inv"] = off
    off = up16(off + coarse_inv.nbytes)
    td["image_bytes"] = off
    for t in td["lv"]:
        for name in ("o_B", "o_X", "o_E", "o_R"):
            t[name] = off
            off = up16(off + t["n"] * 8)
    for name in ("o_C1", "o_V1"):
        td[name] = off
        off = up16(off + td["lv"][0]["n"] * 8)
    td["total_bytes"] = off
    img = np.zeros(td["image_bytes"], dtype=np.uint8)

    def put(at, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8)
        img[at:at + len(raw)] = raw

    for k, t in enumerate(td["lv"][:-1]):
        lv = levels[tail + k]
        put(t["o_data"], lv["data"]); put(t["o_dinv"], lv["dinv"]); put(t["o_indptr"], lv["indptr"])
        put(t["o_memptr"], lv["memptr"]); put(t["o_indices"], lv["indices"].astype(np.uint16))
        put(t["o_agg"], lv["agg"].astype(np.uint16)); put(t["o_mem"], lv["mem"].astype(np.uint16))
    put(td["o_inv"], coarse_inv)
    return td, img


def build(block=True, sweeps0=2, tail=2, kmax=1, merge=None):
    A = graded_matrix()
    levels = []
    while True:
        n = A.shape[0]
        lv = {"n": n, "nnz": A.nnz, "nc": 0, "block": 0, "in_tail": 0, "indptr": A.indptr.astype(np.int32),
              "indices": A.indices.astype(np.int32), "data": A.data.copy(), "dinv": 1.0 / A.diagonal(),
              "agg": np.empty(0, np.int32), "memptr": np.empty(0, np.int32), "mem": np.empty(0, np.int32),
              "boff": np.empty(0, np.uint32), "binv": np.empty(0)}
        levels.append(lv)
        if n <= 64:
            break
        agg = greedy_pairing(A, merge if len(levels) == 1 else None)
        nc = int(agg.max()) + 1
        lv.update(nc=nc, agg=agg.astype(np.int32), mem=np.argsort(agg, kind="stable").astype(np.int32),
                  memptr=np.concatenate([[0], np.cumsum(np.bincount(agg, minlength=nc))]).astype(np.int32))
        P = ar.prolongator(lv)
        pattern = (P.T @ ar._ones(A) @ P).tocsr()
        pattern.sort_indices()
        A = sp.csr_matrix((ar._on_pattern(P.T @ A @ P, pattern), pattern.indices, pattern.indptr), shape=(nc, nc))
    nlev = len(levels)
    assert nlev >= 4, [lv["n"] for lv in levels]
    for l, lv in enumerate(levels):
        lv["in_tail"] = int(tail >= 0 and l >= tail)
        if block and l < (tail if tail >= 0 else nlev - 1):
            m, sq = ar.block_sizes(lv, BLOCK_MAX)
            lv["block"] = 1
            lv["boff"] = np.concatenate([[0], np.cumsum(sq)]).astype(np.uint32)
            binv = np.zeros(int(lv["boff"][-1]))
            for size in np.unique(m):
                which = np.nonzero(m == size)[0]
                inv = np.linalg.inv(ar.dense_blocks(lv, which))
                idx = lv["boff"][which].astype(np.int64)[:, None] + np.arange(size * size)[None, :]
                binv[idx] = inv.transpose(0, 2, 1).reshape(len(which), -1)  # stored transposed
            lv["binv"] = binv
    coarse_inv = np.linalg.inv(ar.csr_of_level(levels[-1]).toarray()).ravel()
    info = {"tail": tail, "kmax": kmax, "coarse_direct": 1, "block_smoother": int(block), "sweeps0": sweeps0,
            "BLOCK_MAX": BLOCK_MAX, "COARSEST_MAX": 64, "K_MIN_ROWS": 32768, "SPLIT_PROLONG_MIN": 200000, "DOT_BLOCKS": 128,
            "TAIL_LDS_BUDGET": BUDGET, "STREAM_CAP": 3072, "LONG_PART": 96, "TAIL_MAX_LEVELS": 8, "theta": 0.1 if block else 0.0,
            "OMEGA": 0.85, "coarse_inv": coarse_inv, "tail_image": np.empty(0, np.uint8), "tdesc": None}
    if tail >= 0:
        info["tdesc"], info["tail_image"] = pack_tail(levels, tail, coarse_inv)
    return levels, info


@pytest.fixture(scope="module")
def clean():
    return build()


@pytest.fixture(scope="module")
def point():
    return build(block=False)


def test_the_clean_hierarchy_passes(clean, point):
    levels, info = clean
    A0 = graded_matrix()
    stats = ar.check_amg(levels, info, csr0=(A0.indptr, A0.indices, A0.data))
    print([lv["n"] for lv in levels], stats)
    assert abs(A0 - A0.T).max() > 0  # (not symmetric: the transposition of binv shows)
    assert set(stats) == {"galerkin", "binv", "coarse_inv"} and max(stats.values()) <= 1.0
    assert levels[0]["block"] and levels[1]["block"] and not levels[2]["block"] and info["tdesc"]["nlev"] == len(levels) - 2
    ar.check_amg(*point)
    ar.check_amg(*build(tail=-1, kmax=2))


def plant_untransposed_binv(levels, info):
    lv = levels[0]
    m, _ = ar.block_sizes(lv, BLOCK_MAX)
    for I in np.nonzero(m >= 2)[0]:
        a, k = int(lv["boff"][I]), int(m[I])
        lv["binv"][a:a + k * k] = lv["binv"][a:a + k * k].reshape(k, k).T.ravel()


def plant_dropped_contribution(levels, info):
    fine, coarse = levels[0], levels[1]
    e = int(fine["indptr"][5])  # the first entry of row 5
    I, J = fine["agg"][5], fine["agg"][fine["indices"][e]]
    row = slice(coarse["indptr"][I], coarse["indptr"][I + 1])
    coarse["data"][row.start + int(np.searchsorted(coarse["indices"][row], J))] -= fine["data"][e]


def plant_stale_dinv(levels, info):
    levels[1]["dinv"][3] = np.nextafter(levels[1]["dinv"][3], np.inf)


def plant_swapped_image_sections(levels, info):
    t = info["tdesc"]["lv"][0]
    img, nb = info["tail_image"], t["n"] * 2
    a, b = img[t["o_agg"]:t["o_agg"] + nb].copy(), img[t["o_mem"]:t["o_mem"] + nb].copy()
    img[t["o_agg"]:t["o_agg"] + nb], img[t["o_mem"]:t["o_mem"] + nb] = b, a


@pytest.mark.parametrize("plant, quantity", [
    (plant_untransposed_binv, "binv"), (plant_dropped_contribution, "galerkin values"), (plant_stale_dinv, "dinv"),
    (plant_swapped_image_sections, "tail image")], ids=lambda p: getattr(p, "__name__", p))
def test_a_planted_setup_defect_is_caught(clean, plant, quantity):
    levels, info = copy.deepcopy(clean)
    plant(levels, info)
    with pytest.raises(ar.AmgMismatch) as caught:
        ar.check_amg(levels, info)
    assert caught.value.quantity == quantity, str(caught.value)


def test_an_aggregate_split_across_two_components_is_caught():
    """Two aggregates of opposite corners of the grid joined into one: every other identity still holds (the coarse
    levels are built from that partition), the aggregate is not connected."""
    levels, info = build(merge=(0, SIDE * SIDE - 1))
    with pytest.raises(ar.AmgMismatch, match="not connected") as caught:
        ar.check_amg(levels, info)
    assert caught.value.quantity == "partition" and caught.value.level == 0


def vectors(levels):
    n = levels[0]["n"]
    rng = np.random.default_rng(11)
    unit = np.zeros(n)
    unit[n - 1] = 1.0  # the isolated node
    return {"random": rng.standard_normal(n), "isolated": unit}


@pytest.mark.parametrize("which", ["clean", "point"])
def test_the_orderings_agree_and_zero_gives_zero(clean, point, which):
    levels, info = clean if which == "clean" else point
    ref = ar.Reference(levels, info)
    for level in range(info["tail"]):
        n = levels[level]["n"]
        r = np.random.default_rng(3 + level).standard_normal(n)
        z, E = ar.cycle_bar(levels, info, level, r, ref=ref)
        print(which, level, E)
        assert 0 < E < 1e-12
        for o in ar.ORDERINGS + ("ext",):
            assert not ar.reference_cycle(levels, info, level, np.zeros(n), o, ref=ref).any()
    # the cycle reduces the error of A z = r: it is an approximate inverse, not just a consistent formula
    r = vectors(levels)["random"]
    z = np.asarray(ar.reference_cycle(levels, info, 0, r, "asc", ref=ref), dtype=np.float64)
    A0 = ar.csr_of_level(levels[0])
    assert np.linalg.norm(r - A0 @ z) < 0.9 * np.linalg.norm(r)


@pytest.mark.parametrize("defect, which, vector", [
    ("gamma_beta", "clean", "random"), ("no_s2", "clean", "random"), ("no_rho2_guard", "clean", "isolated"),
    ("one_sweep", "point", "random"), ("block_post_b", "clean", "random")])
def test_a_planted_cycle_defect_is_caught(clean, point, defect, which, vector):
    levels, info = clean if which == "clean" else point
    ref = ar.Reference(levels, info)
    r = vectors(levels)[vector]
    z, E = ar.cycle_bar(levels, info, 0, r, ref=ref)
    moved = min(ar.distance(ar.reference_cycle(levels, info, 0, r, o, defect=defect, ref=ref), z) for o in ar.ORDERINGS)
    print(defect, "E", E, "moved", moved)
    assert moved >= 1000 * max(E, ar.U), (moved, E)


def test_the_k_cycle_runs_on_a_global_level_and_in_the_tail(clean):
    """(what the cycle defects above rely on: level 0 hands over through two steps at level 1, level 1 through the tail)"""
    levels, info = clean
    assert info["kmax"] >= 1 and info["tail"] == 2 and len(levels) >= 4
    levels2, info2 = build(tail=-1, kmax=2)
    r = vectors(levels2)["random"]
    z, E = ar.cycle_bar(levels2, info2, 0, r)
    assert ar.distance(ar.reference_cycle(levels2, info2, 0, r, "asc", defect="no_s2"), z) >= 1000 * E
