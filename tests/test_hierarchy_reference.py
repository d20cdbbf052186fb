"""tests/hierarchy_reference.py is itself shown to bite (no GPU): a small correct hierarchy built on the host and
encoded into the raw device layouts with their padding passes check_hierarchy; one planted defect at a time -- the
defects a rewrite of a setup kernel of csrc/sagg.hip could introduce without moving the solution -- is reported at the
right level and quantity.

The hierarchy: a random-valued 30 x 30 grid (resistances uniform in [1, 3], the rim tied to ground) with 3 x 3 block
aggregates (900 -> 100 rows), 1 x 2 strips of those (100 -> 50: a nine-point row meets six of them, so rows lump), a
dense inverse at the bottom; P by build_P's rule,
R = P^T, A_c = R (A P) summed in fp64 in the kernels' order of association (the checker multiplies (R A) P), W in f32."""
import copy

import numpy as np
import pytest
import scipy.sparse as sp

from tests import hierarchy_reference as ref
from tests.hierarchy_reference import APAD, PW, HierarchyMismatch, check_hierarchy

OMEGA_P, OMEGA_P_COARSE, OMEGA = 0.70, 0.85, 0.85
GARBAGE = -12345


def pad64(n):
    return (n + 63) & ~63


def grid_matrix(N, rng):
    k = np.arange(N * N).reshape(N, N)
    a = np.concatenate([k[:, :-1].ravel(), k[:-1, :].ravel()])
    b = np.concatenate([k[:, 1:].ravel(), k[1:, :].ravel()])
    g = 1.0 / rng.uniform(1.0, 3.0, size=len(a))
    rim = np.unique(np.concatenate([k[0], k[-1], k[:, 0], k[:, -1]]))
    d = np.bincount(a, g, N * N) + np.bincount(b, g, N * N)
    d[rim] += 1.0 / rng.uniform(1.0, 3.0, size=len(rim))
    n = N * N
    A = sp.csr_matrix((np.concatenate([-g, -g, d]), (np.concatenate([a, b, np.arange(n)]),
                                                     np.concatenate([b, a, np.arange(n)]))), shape=(n, n))
    A.sort_indices()
    return A


def block_aggregates(side, bi, bj):
    i, j = np.divmod(np.arange(side * side), side)
    per = (side + bj - 1) // bj
    return ((i // bi) * per + j // bj).astype(np.int32)


def encode_level(l, A, width, wfix):
    """CSR -> the level's raw buffers: column-major ELL, padding up to wfix (level 0) / APAD, garbage behind it."""
    n = A.shape[0]
    ld = pad64(n)
    alen = np.diff(A.indptr).astype(np.int32)
    acol = np.full((width, ld), GARBAGE, dtype=np.int32)
    aval = np.full((width, ld), np.nan)
    pad_to = wfix if l == 0 else APAD
    rows = np.arange(n)
    for s in range(width):
        has = s < alen
        e = A.indptr[:-1][has] + s
        acol[s, rows[has]] = A.indices[e]
        aval[s, rows[has]] = A.data[e]
        pad = ~has & (s < pad_to)
        acol[s, rows[pad]] = rows[pad]
        aval[s, rows[pad]] = 0.0
    lv = {"n": n, "ld": ld, "nc": 0, "width": width, "maxlen": int(alen.max()), "wfix": wfix, "nnz": int(alen.sum()),
          "rld": 0, "rcap": 0, "wslots": 0, "fold_want": 0, "fold": 0, "d16": int(l == 0), "in_tail": int(l > 0),
          "refreshed": 0, "dense_coarsest": 1, "omega_p": OMEGA_P if l == 0 else OMEGA_P_COARSE, "omega": OMEGA,
          "acol": acol.ravel(), "aval": aval.ravel(), "avalf": aval.astype(np.float32).ravel(), "alen": alen,
          "dinv": 1.0 / A.diagonal()}
    dcol = np.where(acol == GARBAGE, 0, acol - np.arange(ld)[None, :])
    lv["adcol"] = dcol.astype(np.int16).ravel() if l == 0 else np.empty(0, dtype=np.int16)
    for name, dtype in (("agg", np.int32), ("pcol", np.int32), ("pval", np.float64), ("pvalf", np.float32),
                        ("rcol", np.int32), ("rval", np.float64), ("rvalf", np.float32), ("rlen", np.int32),
                        ("wcol", np.int32), ("wval", np.float32), ("wlen", np.int32)):
        lv[name] = np.empty(0, dtype=dtype)
    return lv


def add_transfer(lv, A, agg, fold):
    """P by the slot rule (row by row: independent of reference_P's vectorised form), R = P^T blocked by eights, W in
    f32; returns the coarse matrix R (A P)."""
    n, ld = lv["n"], lv["ld"]
    nc = int(agg.max()) + 1
    pcol = np.full((PW, ld), GARBAGE, dtype=np.int32)
    pval = np.full((PW, ld), np.nan)
    for i in range(n):
        c, v = [-1] * PW, [0.0] * PW
        c[0], v[0] = int(agg[i]), 1.0
        wd = lv["omega_p"] * lv["dinv"][i]
        for e in range(A.indptr[i], A.indptr[i + 1]):
            J, t = int(agg[A.indices[e]]), -wd * A.data[e]
            if J in c:
                v[c.index(J)] += t
            elif -1 in c[1:]:
                k = c.index(-1)
                c[k], v[k] = J, t
            else:
                v[0] += t
        pcol[:, i], pval[:, i] = c, v
    lv.update(nc=nc, agg=agg.copy(), pcol=pcol.ravel(), pval=pval.ravel(), pvalf=pval.astype(np.float32).ravel())
    k, i = np.nonzero(pcol[:, :n] >= 0)
    P = sp.csr_matrix((pval[k, i], (i, pcol[k, i])), shape=(n, nc))
    P.sort_indices()
    R = P.T.tocsr()
    R.sort_indices()
    rld, rcap = pad64(nc), 512
    rlen = np.diff(R.indptr).astype(np.int32)
    rcol = np.zeros((rcap, rld), dtype=np.int32)
    rval = np.zeros((rcap, rld))
    for I in range(nc):
        rcol[:rlen[I], I] = R.indices[R.indptr[I]:R.indptr[I + 1]]
        rval[:rlen[I], I] = R.data[R.indptr[I]:R.indptr[I + 1]]
    blocked = lambda x: np.ascontiguousarray(x.reshape(rcap // 8, 8, rld).transpose(0, 2, 1)).ravel()  # noqa: E731
    lv.update(rld=rld, rcap=rcap, rlen=rlen, rcol=blocked(rcol), rval=blocked(rval),
              rvalf=blocked(rval.astype(np.float32)))
    AP = (A @ P).tocsr()
    AP.sort_indices()
    if fold:
        wslots = 16 if lv["maxlen"] <= 6 else 64
        wlen = np.diff(AP.indptr).astype(np.int32)
        assert wlen.max() <= wslots
        wcol = np.full((wslots, ld), GARBAGE, dtype=np.int32)
        wval = np.full((wslots, ld), np.nan, dtype=np.float32)
        Pd = P.toarray()
        for i in range(n):
            cols = AP.indices[AP.indptr[i]:AP.indptr[i + 1]][::-1]  # (any slot order will do: descending here)
            vals = AP.data[AP.indptr[i]:AP.indptr[i + 1]][::-1]
            wcol[:len(cols), i] = cols
            wval[:len(cols), i] = (Pd[i, cols] - OMEGA * lv["dinv"][i] * vals).astype(np.float32)
        lv.update(wslots=wslots, fold_want=1, fold=1, wcol=wcol.ravel(), wval=wval.ravel(), wlen=wlen)
    C = (R @ AP).tocsr()
    C.sort_indices()
    return C, (R, A, P)


@pytest.fixture(scope="module")
def built():
    rng = np.random.default_rng(3)
    A0 = grid_matrix(30, rng)
    l0 = encode_level(0, A0, 5, 5)
    A1, ops0 = add_transfer(l0, A0, block_aggregates(30, 3, 3), True)
    l1 = encode_level(1, A1, 64, 12)
    A2, _ = add_transfer(l1, A1, block_aggregates(10, 1, 2), True)
    l2 = encode_level(2, A2, 64, 32)
    l2["coarse_inv"] = np.linalg.inv(A2.toarray()).ravel()
    assert (A0.shape[0], A1.shape[0], A2.shape[0]) == (900, 100, 50)
    return [l0, l1, l2], ops0


@pytest.fixture
def levels(built):
    return copy.deepcopy(built[0])


def slot(lv, s, i):
    return s * lv["ld"] + i


def r_at(lv, t, I):
    return ((t >> 3) * lv["rld"] + I) * 8 + (t & 7)


def test_a_correct_hierarchy_passes(levels):
    stats = check_hierarchy(levels)
    print(stats)
    assert set(stats) == {"P", "galerkin", "W", "coarse_inv"}
    assert all(0.0 <= v <= 1.0 for v in stats.values()), stats
    seen, sizes = ref.coverage(levels)
    assert sizes.startswith("900/5/100 100/9/50 50/"), sizes
    assert {"ap_rows (16 slots)", "ap_rows_lds (64 slots)", "lumping fine row", "r_sort_short"} <= seen, seen


def expect(levels, level, quantity, row=None):
    with pytest.raises(HierarchyMismatch) as exc:
        check_hierarchy(levels)
    e = exc.value
    assert (e.level, e.quantity) == (level, quantity), str(e)
    if row is not None:
        assert e.row == row, str(e)


def test_a_product_left_out_of_a_coarse_entry(levels, built):
    R, A, P = built[1]
    I = 37
    i = R.indices[R.indptr[I] + 2]          # a member of the aggregate,
    k = A.indices[A.indptr[i] + 1]          # one entry of its row,
    J = P.indices[P.indptr[k]]              # one entry of P's row there
    product = R[I, i] * A[i, k] * P[k, J]
    assert product != 0.0
    l1 = levels[1]
    s = int(np.nonzero(l1["acol"].reshape(64, -1)[:l1["alen"][I], I] == J)[0][0])
    l1["aval"][slot(l1, s, I)] -= product
    l1["avalf"][slot(l1, s, I)] = np.float32(l1["aval"][slot(l1, s, I)])
    if J == I:
        l1["dinv"][I] = 1.0 / l1["aval"][slot(l1, s, I)]
    expect(levels, 1, "Galerkin values", I)


def test_a_stale_coarse_value(levels):
    l1 = levels[1]
    at = slot(l1, 1, 11)  # (slot 1 of row 11: an off-diagonal, so that dinv stays consistent)
    assert l1["acol"][at] != 11
    l1["aval"][at] *= 1.5
    l1["avalf"][at] = np.float32(l1["aval"][at])
    expect(levels, 1, "Galerkin values", 11)


def test_two_R_values_swapped_within_a_row(levels):
    l0 = levels[0]
    a, b = r_at(l0, 0, 5), r_at(l0, 3, 5)
    for name in ("rval", "rvalf"):
        l0[name][a], l0[name][b] = l0[name][b], l0[name][a]
    expect(levels, 0, "R values", 5)


def test_an_R_row_in_descending_order(levels):
    l0 = levels[0]
    I, n = 9, int(l0["rlen"][9])
    at = [r_at(l0, t, I) for t in range(n)]
    for name in ("rcol", "rval", "rvalf"):
        l0[name][at] = l0[name][at][::-1]
    expect(levels, 0, "R order", I)


@pytest.mark.parametrize("level", [0, 1])
def test_a_nonzero_padding_value_in_A(levels, level):
    lv = levels[level]
    i = int(np.argmin(lv["alen"]))
    s = int(lv["alen"][i])
    assert s < (lv["wfix"] if level == 0 else APAD)
    lv["aval"][slot(lv, s, i)] = 1e-30
    expect(levels, level, "A padding", i)
    lv["aval"][slot(lv, s, i)] = 0.0
    lv["avalf"][slot(lv, s, i)] = 1e-30
    expect(levels, level, "A padding", i)


@pytest.mark.parametrize("level", [0, 1])
def test_a_padding_column_that_is_not_the_rows_own_index(levels, level):
    lv = levels[level]
    i = int(np.argmin(lv["alen"]))
    s = (lv["wfix"] if level == 0 else APAD) - 1
    lv["acol"][slot(lv, s, i)] = i + 1
    expect(levels, level, "A padding", i)


@pytest.mark.parametrize("name,quantity,level", [("avalf", "avalf", 1), ("pvalf", "pvalf", 0), ("rvalf", "rvalf", 1)])
def test_an_f32_copy_off_by_one_ulp(levels, name, quantity, level):
    lv = levels[level]
    at = r_at(lv, 1, 3) if name == "rvalf" else slot(lv, 1, 3)
    lv[name][at] = np.nextafter(lv[name][at], np.float32(np.inf))
    expect(levels, level, quantity, 3)


def test_dinv_off_by_one_ulp(levels):
    levels[1]["dinv"][42] = np.nextafter(levels[1]["dinv"][42], np.inf)
    expect(levels, 1, "dinv", 42)


def test_a_P_entry_in_the_wrong_slot(levels):
    l0 = levels[0]
    n = l0["n"]
    pcol = l0["pcol"].reshape(PW, -1)
    i = int(np.nonzero((pcol[1, :n] >= 0) & (pcol[2, :n] >= 0))[0][0])
    for name in ("pcol", "pval", "pvalf"):
        a, b = slot(l0, 1, i), slot(l0, 2, i)
        l0[name][a], l0[name][b] = l0[name][b], l0[name][a]
    expect(levels, 0, "pcol", i)


def test_a_W_row_missing_a_column(levels):
    l0 = levels[0]
    i = 444
    last = int(l0["wlen"][i]) - 1
    own = set(l0["pcol"].reshape(PW, -1)[:, i].tolist())
    wcol = l0["wcol"].reshape(16, -1)
    s = [q for q in range(last + 1) if int(wcol[q, i]) not in own][0]  # (a column of A P beside the row's P entries)
    for name in ("wcol", "wval"):
        l0[name][slot(l0, s, i)] = l0[name][slot(l0, last, i)]
    l0["wlen"][i] = last
    expect(levels, 0, "W pattern", i)


def test_a_W_row_missing_a_column_of_its_own_P_entries(levels):
    l0 = levels[0]
    i = 444
    own = int(l0["agg"][i])
    wcol = l0["wcol"].reshape(16, -1)
    s = int(np.nonzero(wcol[:l0["wlen"][i], i] == own)[0][0])
    last = int(l0["wlen"][i]) - 1
    for name in ("wcol", "wval"):
        l0[name][slot(l0, s, i)] = l0[name][slot(l0, last, i)]
    l0["wlen"][i] = last
    expect(levels, 0, "W pattern", i)


def test_a_W_value_off_by_four_f32_ulps(levels):
    l1 = levels[1]
    at = slot(l1, 2, 17)
    x = l1["wval"][at]
    for _ in range(4):
        x = np.nextafter(x, np.float32(np.inf))
    l1["wval"][at] = x
    expect(levels, 1, "W values", 17)


def test_a_coarse_inverse_entry_off_by_1e_6(levels):
    levels[2]["coarse_inv"][3 * 50 + 7] *= 1.0 + 1e-6
    expect(levels, 2, "coarse_inv", 3)


def test_an_empty_aggregate_and_an_unassigned_node(levels):
    bad = copy.deepcopy(levels)
    bad[0]["agg"][17] = bad[0]["nc"]
    expect(bad, 0, "agg", 17)
    levels[1]["agg"][levels[1]["agg"] == 24] = 23
    expect(levels, 1, "agg", 24)


def test_an_entry_that_cancels_exactly_stays_in_the_pattern():
    """scipy's product leaves out an entry whose products sum to exactly zero; the kernels keep it (their patterns are
    structural), and so does the reference: values are read onto the pattern of the all-ones product."""
    A = sp.csr_matrix(np.array([[1.0, -1.0], [0.0, 1.0]]))
    B = sp.csr_matrix(np.array([[1.0, 0.0], [1.0, 1.0]]))
    pattern = ref._sorted(ref._ones(A) @ ref._ones(B))
    assert pattern.nnz == 4
    assert np.array_equal(ref._on_pattern(A @ B, pattern), [0.0, -1.0, 1.0, 1.0])
