"""An fp64 host reference of the smoothed-aggregation setup (csrc/sagg.hip), level by level.

The setup has a closed algebraic specification, which its kernels state in their comments:

    P       = (I - w_p D^-1 A) P_tent, cut to four entries per row, the rest lumped into the row's own aggregate
    R       = P^T
    A_{l+1} = R A_l P
    dinv    = 1 / diag(A_l)                  f32 copies are casts of the f64 values
    W       = P - w D^-1 (A_l P)             (levels that fold their first post-smoothing sweep)
    coarse_inv = A_last^-1                   (dense, n <= 64)

check_hierarchy() takes what Handle.debug_hierarchy() exports -- per level the info words and the device buffers as
flat arrays in the kernels' own layouts -- decodes the layouts HERE (they, their padding included, are part of what is
checked) and raises HierarchyMismatch naming level, quantity and row on the first violation.  numpy / scipy only: no
GPU, nothing of the library.

Layouts: A, P and W are column-major ELL, slot s of row i at [s * ld + i]; R is blocked by eights, entry t of coarse
row I at [((t >> 3) * rld + I) * 8 + (t & 7)]; adcol is an int16 holding column - row.

Bounds (u = 2^-52; every one is taken against sums of ABSOLUTE values, so a cancelled entry does not loosen it):
  pval      (m + 2) u sum|terms|, m the entry's number of terms: the reference does the same operations in the same
            order, so this covers the contraction of a multiply-add and nothing else
  Galerkin  (N_ij + 3) u (|R| |A| |P|)_ij against scipy's R @ A @ P, N_ij = (1_R 1_A 1_P)_ij the number of elementary
            products of the entry: the standard bound of a sum of N products, whatever the order of summation
  wval      2^-23 |W_ref| (one f32 rounding) + (k + 3) u (|P| + w dinv |A| |P|)_ij, k the entry's products in A P
  coarse_inv  64 u cond_2(A_last) max|inv_ref| against numpy.linalg.inv: the first-order perturbation bound of an
            inverse with n <= 64; A_last coarse_inv - I the same times max|A_last|
Everything else (patterns, paddings, R against P^T, dinv, the f32 casts) is compared bit for bit."""
import numpy as np
import scipy.sparse as sp

PW = 4      # prolongation entries per fine row
APAD = 32   # every coarse row is zero-padded up to this many slots
U = 2.0 ** -52


class HierarchyMismatch(AssertionError):
    def __init__(self, level, quantity, row, detail=""):
        super().__init__(f"level {level}: {quantity}: row {row}: {detail}")
        self.level, self.quantity, self.row, self.detail = level, quantity, row, detail


def _fail_where(bad, level, quantity, detail=""):
    """bad: a boolean array whose LAST axis is the row; raises on the first row with a violation."""
    bad = np.asarray(bad)
    if bad.any():
        rows = bad.reshape(-1, bad.shape[-1]).any(axis=0)
        raise HierarchyMismatch(level, quantity, int(np.argmax(rows)), detail)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


# ---- decoders ---------------------------------------------------------------------------------------------------------
def ell(flat, ld, slots, n):
    """column-major ELL -> [slots, n]"""
    return flat[:slots * ld].reshape(slots, ld)[:, :n]


def r_blocked(flat, rld, slots, nc):
    """R's blocks of eight -> [slots, nc] (slots a multiple of 8)"""
    return flat[:slots * rld].reshape(slots // 8, rld, 8).transpose(0, 2, 1).reshape(slots, rld)[:, :nc]


def csr_of_level(lv):
    """The level's matrix as scipy CSR (slots below the row's length, in slot order)."""
    n, ld, w = lv["n"], lv["ld"], lv["maxlen"]
    alen = lv["alen"][:n]
    col, val = ell(lv["acol"], ld, w, n), ell(lv["aval"], ld, w, n)
    valid = np.arange(w)[:, None] < alen[None, :]
    rows = np.broadcast_to(np.arange(n), (w, n))
    # (row-major order of the transposed mask = by row, then by slot)
    vt = valid.T
    return _csr(rows.T[vt], col.T[vt], val.T[vt], (n, n), alen)


def _csr(rows, cols, vals, shape, counts=None):
    """CSR from entries already ordered by row (no duplicate merging, no pruning of zeros)."""
    if counts is None:
        counts = np.bincount(rows, minlength=shape[0])
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return sp.csr_matrix((np.asarray(vals, dtype=np.float64), np.asarray(cols, dtype=np.int64), indptr), shape=shape)


def _ones(M):
    return sp.csr_matrix((np.ones_like(M.data), M.indices, M.indptr), shape=M.shape)


def _sorted(M):
    M = M.tocsr()
    M.sort_indices()
    return M


def _on_pattern(M, pattern):
    """M's values on the entries of `pattern` (a sorted CSR whose pattern contains M's; zeros elsewhere): scipy's
    product leaves out entries whose sum is exactly zero, the structural pattern -- the product of all-ones copies --
    keeps them, and so do the kernels."""
    M = _sorted(M)
    width = pattern.shape[1]
    key = np.repeat(np.arange(pattern.shape[0], dtype=np.int64), np.diff(pattern.indptr)) * width + pattern.indices
    mkey = np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr)) * width + M.indices
    pos = np.searchsorted(key, mkey)
    assert (pos < len(key)).all() and np.array_equal(key[pos], mkey)
    out = np.zeros(len(key))
    out[pos] = M.data
    return out


# ---- the checks of one level --------------------------------------------------------------------------------------------
def check_matrix(l, lv):
    """Structure of A_l, its padding, adcol, dinv and the f32 copy."""
    n, ld, width, maxlen, wfix = lv["n"], lv["ld"], lv["width"], lv["maxlen"], lv["wfix"]
    alen = lv["alen"][:n]
    if not (1 <= maxlen <= width and ld >= n and len(lv["acol"]) >= width * ld):
        raise HierarchyMismatch(l, "A structure", 0, f"maxlen {maxlen} width {width} ld {ld} n {n}")
    _fail_where((alen < 1) | (alen > maxlen), l, "A structure", "row length outside [1, maxlen]")
    if int(alen.max()) != maxlen:
        raise HierarchyMismatch(l, "A structure", int(np.argmax(alen)), f"maxlen {maxlen} but the longest row has {alen.max()}")
    if int(alen.sum()) != lv["nnz"]:
        raise HierarchyMismatch(l, "A structure", 0, f"nnz {lv['nnz']} but the lengths sum to {alen.sum()}")
    pad_to = wfix if l == 0 else APAD
    slots = max(maxlen, min(pad_to, width))
    col, val, valf = (ell(lv[k], ld, slots, n) for k in ("acol", "aval", "avalf"))
    s = np.arange(slots)[:, None]
    rows = np.arange(n)[None, :]
    valid = s < alen[None, :]
    _fail_where(valid & ((col < 0) | (col >= n)), l, "A structure", "column outside [0, n)")
    _fail_where(valid[1:] & (col[1:] <= col[:-1]), l, "A structure", "columns not ascending and distinct")
    isdiag = valid & (col == rows)
    _fail_where(~isdiag.any(axis=0), l, "A structure", "no stored diagonal")
    pad = ~valid & (s < pad_to)
    _fail_where(pad & (col != rows), l, "A padding", "a padding slot's column is not the row's own index")
    _fail_where(pad & ((val != 0.0) | (valf != 0.0)), l, "A padding", "a padding slot's value is not zero")
    written = valid | pad
    if lv["d16"]:
        dcol = ell(lv["adcol"], ld, slots, n)
        _fail_where(written & (dcol.astype(np.int64) != col.astype(np.int64) - rows), l, "adcol", "not column - row")
    elif len(lv["adcol"]):
        raise HierarchyMismatch(l, "adcol", 0, "exported without d16")
    diag = np.where(isdiag, val, 0.0).sum(axis=0)  # (one stored diagonal per row: columns are distinct)
    _fail_where(_bits(lv["dinv"][:n]) != _bits(1.0 / diag), l, "dinv", "not 1 / diag bit for bit")
    _fail_where(written & (_bits(valf) != _bits(val.astype(np.float32))), l, "avalf", "not the cast of aval")


def reference_P(lv):
    """P of the level by build_P's rule from the exported A, agg, dinv and omega_p: columns [PW, n] (-1 empty),
    values, and per entry the sum of |terms| and the number of terms."""
    n, ld, maxlen = lv["n"], lv["ld"], lv["maxlen"]
    alen, agg = lv["alen"][:n], lv["agg"][:n]
    col, val = ell(lv["acol"], ld, maxlen, n), ell(lv["aval"], ld, maxlen, n)
    c = np.full((PW, n), -1, dtype=np.int32)
    v = np.zeros((PW, n))
    S = np.zeros((PW, n))
    m = np.zeros((PW, n), dtype=np.int64)
    c[0], v[0], S[0], m[0] = agg, 1.0, 1.0, 1
    wd = lv["omega_p"] * lv["dinv"][:n]
    lumped = np.zeros(n, dtype=bool)
    for s in range(maxlen):
        act = s < alen
        J = agg[np.where(act, col[s], 0)]
        t = -wd * val[s]
        placed = ~act
        for k in range(PW):
            hit = ~placed & (c[k] == J)
            v[k] = np.where(hit, v[k] + t, v[k])
            S[k] += np.where(hit, np.abs(t), 0.0)
            m[k] += hit
            placed |= hit
        for k in range(1, PW):
            free = ~placed & (c[k] < 0)
            c[k] = np.where(free, J, c[k])
            v[k] = np.where(free, t, v[k])
            S[k] += np.where(free, np.abs(t), 0.0)
            m[k] += free
            placed |= free
        rest = ~placed
        v[0] = np.where(rest, v[0] + t, v[0])
        S[0] += np.where(rest, np.abs(t), 0.0)
        m[0] += rest
        lumped |= rest
    return c, v, S, m, lumped


def check_aggregates(l, lv):
    n, nc = lv["n"], lv["nc"]
    agg = lv["agg"][:n]
    if nc < 1 or len(lv["agg"]) < n:
        raise HierarchyMismatch(l, "agg", 0, f"nc {nc}, {len(lv['agg'])} entries for {n} rows")
    _fail_where((agg < 0) | (agg >= nc), l, "agg", "aggregate outside [0, nc)")
    _fail_where(np.bincount(agg, minlength=nc) == 0, l, "agg", "an aggregate without a member (row = the aggregate)")


def check_P(l, lv, stats):
    n, ld = lv["n"], lv["ld"]
    c, v, S, m, _ = reference_P(lv)
    pcol, pval, pvalf = (ell(lv[k], ld, PW, n) for k in ("pcol", "pval", "pvalf"))
    _fail_where(pcol != c, l, "pcol", "not build_P's slot rule")
    bound = (m + 2) * U * S
    err = np.abs(pval - v)
    _fail_where(err > bound, l, "pval", f"worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    stats["P"] = max(stats.get("P", 0.0), float(np.max(err[c >= 0] / np.maximum(bound[c >= 0], 1e-300))))
    _fail_where(_bits(pvalf) != _bits(pval.astype(np.float32)), l, "pvalf", "not the cast of pval")
    # row sums are kept: sum_k p_ik = 1 - w dinv_i sum_s a_is (the reference side in extended precision)
    L = np.longdouble
    maxlen, alen = lv["maxlen"], lv["alen"][:n]
    val = ell(lv["aval"], ld, maxlen, n)
    valid = np.arange(maxlen)[:, None] < alen[None, :]
    wd = (lv["omega_p"] * lv["dinv"][:n]).astype(L)
    ref = L(1) - wd * np.where(valid, val, 0.0).astype(L).sum(axis=0)
    dev = pval.astype(L).sum(axis=0)
    rbound = (alen + 1 + 2) * U * S.sum(axis=0)
    _fail_where(np.abs(dev - ref) > rbound, l, "P row sum", "not 1 - w dinv (row sum of A)")


def p_entries(lv):
    """P's entries (fine row, coarse column, value, slot) in (coarse column, fine row, slot) order: R's own order."""
    n, ld = lv["n"], lv["ld"]
    pcol, pval = ell(lv["pcol"], ld, PW, n), ell(lv["pval"], ld, PW, n)
    k, i = np.nonzero(pcol >= 0)
    J, x = pcol[k, i], pval[k, i]
    order = np.lexsort((k, i, J))
    return i[order], J[order], x[order], k[order]


def check_R(l, lv):
    """R decoded to CSR is P^T bit for bit; returns it."""
    n, nc, rld, rcap = lv["n"], lv["nc"], lv["rld"], lv["rcap"]
    rlen = lv["rlen"][:nc]
    if rld < nc or rcap % 8 or len(lv["rcol"]) < rcap * rld:
        raise HierarchyMismatch(l, "rlen", 0, f"rld {rld} nc {nc} rcap {rcap}")
    _fail_where((rlen < 0) | (rlen > rcap), l, "rlen", "row length outside [0, rcap]")
    upto = np.full(nc, rcap) if nc <= 4096 else (rlen + 7) & ~7
    T = int(upto.max())
    rcol, rval, rvalf = (r_blocked(lv[k], rld, T, nc) for k in ("rcol", "rval", "rvalf"))
    t = np.arange(T)[:, None]
    valid = t < rlen[None, :]
    pad = ~valid & (t < upto[None, :])
    _fail_where(pad & ((rcol != 0) | (rval != 0.0) | (rvalf != 0.0)), l, "R padding", "not column 0 / value 0")
    _fail_where(valid & ((rcol < 0) | (rcol >= n)), l, "R pattern", "fine row outside [0, n)")
    _fail_where(valid[1:] & (rcol[1:] <= rcol[:-1]), l, "R order", "entries not ascending by fine row")
    _fail_where(valid & (_bits(rvalf) != _bits(rval.astype(np.float32))), l, "rvalf", "not the cast of rval")
    i, J, x, _ = p_entries(lv)
    want = np.bincount(J, minlength=nc)
    _fail_where(rlen != want, l, "R pattern", "row length is not the column count of P")
    vt = valid.T  # (by coarse row, then by entry)
    if not np.array_equal(rcol.T[vt], i):
        bad = np.zeros(nc, dtype=bool)
        bad[J[rcol.T[vt] != i]] = True
        _fail_where(bad, l, "R pattern", "fine rows are not those of P's column")
    if not np.array_equal(_bits(rval.T[vt]), _bits(x)):
        bad = np.zeros(nc, dtype=bool)
        bad[J[_bits(rval.T[vt]) != _bits(x)]] = True
        _fail_where(bad, l, "R values", "an entry is not the value of P it is paired with")
    return _csr(J, i, x, (nc, n), rlen)


def p_csr(lv):
    i, J, x, _ = p_entries(lv)
    return _sorted(sp.csr_matrix((x, (i, J)), shape=(lv["n"], lv["nc"])))


def check_galerkin(l, lv, nxt, R, A, P, stats):
    """A_{l+1} against R A_l P: the structural pattern (from all-ones copies) and the values.  Reported at level l + 1."""
    nc = lv["nc"]
    cnt = _sorted(_ones(R) @ _ones(A) @ _ones(P))
    ref, absb = _on_pattern(R @ A @ P, cnt), _on_pattern(abs(R) @ abs(A) @ abs(P), cnt)
    if nxt["n"] != nc:
        raise HierarchyMismatch(l + 1, "Galerkin pattern", 0, f"{nxt['n']} rows for {nc} aggregates")
    C = csr_of_level(nxt)
    want = np.diff(cnt.indptr)
    _fail_where(nxt["alen"][:nc] != want, l + 1, "Galerkin pattern", "row length is not that of R A P")
    same = C.indices == cnt.indices
    if not same.all():
        bad = np.zeros(nc, dtype=bool)
        bad[np.repeat(np.arange(nc), want)[~same]] = True
        _fail_where(bad, l + 1, "Galerkin pattern", "columns are not those of R A P")
    bound = (cnt.data + 3) * U * absb
    err = np.abs(C.data - ref)
    ratio = err / np.maximum(bound, 1e-300)
    stats["galerkin"] = max(stats.get("galerkin", 0.0), float(ratio.max()))
    if (err > bound).any():
        bad = np.zeros(nc, dtype=bool)
        bad[np.repeat(np.arange(nc), want)[err > bound]] = True
        _fail_where(bad, l + 1, "Galerkin values", f"worst error / bound {ratio.max():.3g}")
    return cnt


def check_W(l, lv, A, P, stats):
    """W = P - w D^-1 (A P): the row's column set is the pattern of A P in any slot order."""
    n, nc, ld, wslots = lv["n"], lv["nc"], lv["ld"], lv["wslots"]
    if len(lv["wcol"]) < wslots * ld or len(lv["wlen"]) < n:
        raise HierarchyMismatch(l, "W pattern", 0, "the level folds but exports no W")
    k = _sorted(_ones(A) @ _ones(P))
    AP, absAP = _on_pattern(A @ P, k), _on_pattern(abs(A) @ abs(P), k)
    want = np.diff(k.indptr)
    rows_ref = np.repeat(np.arange(n), want)
    key_ref = rows_ref * nc + k.indices
    wlen = lv["wlen"][:n]
    _fail_where((wlen < 0) | (wlen > wslots), l, "W pattern", "row length outside [0, wslots]")
    wcol, wval = ell(lv["wcol"], ld, wslots, n), ell(lv["wval"], ld, wslots, n)
    vt = (np.arange(wslots)[:, None] < wlen[None, :]).T
    rows_dev = np.broadcast_to(np.arange(n), (wslots, n)).T[vt]
    cols_dev = wcol.T[vt].astype(np.int64)
    _bad = np.zeros(n, dtype=bool)
    _bad[rows_dev[(cols_dev < 0) | (cols_dev >= nc)]] = True
    _fail_where(_bad, l, "W pattern", "column outside [0, nc)")
    # every column of the row's own P entries, and exactly the columns of A P
    Pc = P.tocoo()
    have = np.isin(Pc.row * nc + Pc.col, rows_dev * nc + cols_dev)
    _bad[Pc.row[~have]] = True
    _fail_where(_bad, l, "W pattern", "a column of the row's own P entries is missing")
    _fail_where(wlen != want, l, "W pattern", "row length is not that of A P")
    order = np.argsort(rows_dev * nc + cols_dev, kind="stable")
    key_dev = (rows_dev * nc + cols_dev)[order]
    _bad[rows_ref[key_dev != key_ref]] = True
    _fail_where(_bad, l, "W pattern", "columns are not those of A P")
    p_at = np.zeros(len(key_ref))
    p_at[np.searchsorted(key_ref, Pc.row * nc + Pc.col)] = Pc.data
    wd = (lv["omega"] * lv["dinv"][:n])[rows_ref]
    ref = p_at - wd * AP
    bound = 2.0 ** -23 * np.abs(ref) + (k.data + 3) * U * (np.abs(p_at) + wd * absAP)
    err = np.abs(wval.T[vt][order].astype(np.float64) - ref)
    ratio = err / np.maximum(bound, 1e-300)
    stats["W"] = max(stats.get("W", 0.0), float(ratio.max()))
    _bad[rows_ref[err > bound]] = True
    _fail_where(_bad, l, "W values", f"worst error / bound {ratio.max():.3g}")


def check_coarsest(l, lv, stats):
    n = lv["n"]
    inv = lv.get("coarse_inv", np.empty(0))
    if len(inv) != n * n or n > 64:
        raise HierarchyMismatch(l, "coarse_inv", 0, f"{len(inv)} values for a last level of {n} rows")
    inv = inv.reshape(n, n)
    Ad = csr_of_level(lv).toarray()
    ref = np.linalg.inv(Ad)
    bound = 64 * U * np.linalg.cond(Ad, 2) * np.abs(ref).max()
    err = np.abs(inv - ref)
    stats["coarse_inv"] = max(stats.get("coarse_inv", 0.0), float(err.max() / bound))
    _fail_where(err.T > bound, l, "coarse_inv", f"worst error / bound {err.max() / bound:.3g}")
    res = np.abs(Ad @ inv - np.eye(n))
    _fail_where(res.T > bound * np.abs(Ad).max(), l, "coarse_inv", "A coarse_inv - I beyond the bound")


def check_hierarchy(levels):
    """Every identity of the module's docstring on an exported hierarchy; raises HierarchyMismatch on the first
    violation.  Returns the largest observed error / bound per bounded quantity ("P", "galerkin", "W", "coarse_inv")."""
    stats = {}
    nlev = len(levels)
    for l, lv in enumerate(levels):
        check_matrix(l, lv)
        if l + 1 == nlev:
            break
        check_aggregates(l, lv)
        check_P(l, lv, stats)
        R = check_R(l, lv)
        A, P = csr_of_level(lv), p_csr(lv)
        check_matrix(l + 1, levels[l + 1])  # (its lengths and columns are decoded next)
        check_galerkin(l, lv, levels[l + 1], R, A, P, stats)
        if lv["fold"]:
            check_W(l, lv, A, P, stats)
    if levels[-1]["dense_coarsest"]:
        check_coarsest(nlev - 1, levels[-1], stats)
    return stats


# ---- what the tests ask of the exported data beside its correctness -----------------------------------------------------
def coverage(levels):
    """Which paths of the setup kernels this hierarchy went through (tests/test_gpu_hierarchy.py asserts that its
    shapes together reach every one): a set of names, and a line of level sizes."""
    seen = set()
    sizes = []
    for l, lv in enumerate(levels):
        sizes.append(f"{lv['n']}/{lv['maxlen']}/{lv['nc']}")
        if l + 1 == len(levels):
            break
        apw = 16 if lv["maxlen"] <= 6 else 64
        seen.add("ap_rows (16 slots)" if apw == 16 else "ap_rows_lds (64 slots)")
        if l >= 1 and lv["n"] > 1024 and lv["fold"]:
            seen.add("folded level >= 1 above 1024 rows")
        rlen = lv["rlen"][:lv["nc"]]
        if (rlen > (40 if apw == 16 else 16)).any():
            seen.add("second Galerkin group")
        seen.add("r_sort_short" if (rlen <= 32).any() else "")
        if (rlen > 32).any():
            seen.add("r_sort_medium")
        clen = levels[l + 1]["alen"][:lv["nc"]]
        for name, hit in (("coarse row <= 16", clen <= 16), ("coarse row 17-32", (clen > 16) & (clen <= 32)),
                          ("coarse row > 32", clen > 32)):
            if hit.any():
                seen.add(name)
        if reference_P(lv)[4].any():
            seen.add("lumping fine row")
    seen.discard("")
    return seen, " ".join(sizes)


COVERAGE = {"ap_rows (16 slots)", "ap_rows_lds (64 slots)", "folded level >= 1 above 1024 rows", "second Galerkin group",
            "r_sort_short", "r_sort_medium", "coarse row <= 16", "coarse row 17-32", "coarse row > 32", "lumping fine row"}
