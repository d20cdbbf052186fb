"""A host reference of the plain-aggregation multigrid (csrc/amg.hip): its setup, level by level, and one cycle.

It works from what Handle.debug_amg() exports -- per level the info words and the raw device buffers, for the hierarchy
the words of nodal_debug_amg_info, coarse_inv, the packed tail image and its descriptor -- decodes the layouts HERE and
imports nothing of the library.  numpy / scipy only, no GPU.

Setup (check_amg; raises AmgMismatch naming level, quantity and row / aggregate on the first violation):

    agg       maps the n nodes onto [0, nc) with no empty aggregate; memptr / mem list every aggregate's members in
              ascending order and agree with agg; every aggregate is connected in the graph of A_l (the structural
              singularity check relies on aggregation never joining two components)
    A_{l+1}   = P^T A_l P, P piecewise constant from agg: row starts, sorted columns and the structural pattern (explicit
              zeros kept) exact; values within (N + 3) u sum|contributions| of scipy's product, N the entry's number
              of contributions (the Galerkin bound of tests/hierarchy_reference.py); level 0 the bytes of export_csr()
    dinv      1 / diag(A_l), bit for bit
    boff      the exclusive scan of m^2 (m for an aggregate above BLOCK_MAX members); `block` set on exactly the levels
              above the tail (all but the last without one) when the block smoother is on
    binv      per aggregate the inverse of A_l restricted to it, in member order, TRANSPOSED: against numpy.linalg.inv
              within m u cond_2(B) max|inv_ref| per entry and the same times max|B| for B X - I (the dense-inverse bound
              of hierarchy_reference.py with the block in the last level's place); above BLOCK_MAX: 1 / diag, bit for bit
    coarse_inv  64 u cond_2(A_last) max|inv_ref|, and A_last coarse_inv - I within the same times max|A_last|
    tail image  decoded from the descriptor: every section the bits of the level array it was packed from (u16 casts for
              indices, agg and mem; coarse_inv at o_inv), offsets 16-byte aligned and not overlapping, total_bytes
              within the budget

Cycle (reference_cycle): the visit as cycle() and amg_tail_kernel perform it.  At level l with right-hand side b, w the
smoother's weight:

    x  = w Binv b (block levels)  or  w dinv b (point levels);  r = b - A x
    point mode, level 0, sweeps0 == 2:  x += w dinv r;  r = b - A x
    rc = sum of r over each aggregate's members
    coarse solve, one of
      the level below is the tail's first: two flexible-CG steps (below) over the tail's own V-cycle -- point Jacobi
        from zero, restriction, ..., dense inverse at the bottom, correction and one point sweep on the way up
      the level below is the last one, or lies below kmax: c1 = cycle(l + 1, rc), s1 = 1, s2 = 0
      otherwise the same two steps over cycle(l + 1, .)
    two steps:  c1 = M rc, v1 = A_c c1, rho1 = c1.v1, alpha1 = c1.rc, r2 = rc - (rho1 > 0 ? alpha1 / rho1 : 0) v1,
      c2 = M r2, v2 = A_c c2, gamma = c2.v1, beta = c2.v2, alpha2 = c2.r2, and kcycle_coefficients' guards:
      rho1 <= 0: (0, 0);  rho2 = beta - gamma^2 / rho1 <= 0: (alpha1 / rho1, 0);
      else (alpha1 / rho1 - gamma alpha2 / (rho1 rho2), alpha2 / rho2)
    xp = x + P (s1 c1 + s2 c2)
    z  = xp + w Binv (b - A xp)  or  xp + w dinv (b - A xp), the point sweep twice where the pre-smoothing ran twice
    the last level: coarse_inv b, or dinv b where there is none (the one-level hierarchy)

Everything on the device is fp64, so the bar comes from the arithmetic itself (cycle_bar): the cycle is evaluated in
extended precision (np.longdouble) and three more times in fp64 that differ only in the order of additions -- row
entries ascending, descending, and ascending with every dot product as 128 partial sums instead of one pairwise sum.
E is the largest relative distance (max norm) of those three from the extended result; the device, a fourth ordering
(256-row blocks, per-workgroup partials), is held to 4 E per vector, the margin for an ordering effect the host sampled
three times only.  `defect` states a wrong cycle for tests/test_amg_reference.py and is never used against the device."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

U = 2.0 ** -52
ORDERINGS = ("asc", "desc", "dots128")
DEFECTS = ("gamma_beta", "no_s2", "no_rho2_guard", "one_sweep", "block_post_b")


class AmgMismatch(AssertionError):
    def __init__(self, level, quantity, where, detail=""):
        super().__init__(f"level {level}: {quantity}: {where}: {detail}")
        self.level, self.quantity, self.where, self.detail = level, quantity, where, detail


def _first(bad):
    return int(np.argmax(np.asarray(bad).reshape(-1)))


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def csr_of_level(lv):
    n = lv["n"]
    return sp.csr_matrix((lv["data"], lv["indices"], lv["indptr"]), shape=(n, n))


def _ones(M):
    return sp.csr_matrix((np.ones_like(M.data), M.indices, M.indptr), shape=M.shape)


def _abs(M):
    return sp.csr_matrix((np.abs(M.data), M.indices, M.indptr), shape=M.shape)


def _on_pattern(M, pattern):
    """M's values on the entries of the sorted CSR `pattern`, which contains M's pattern (zeros elsewhere)."""
    M = M.tocsr()
    M.sort_indices()
    width = pattern.shape[1]
    key = np.repeat(np.arange(pattern.shape[0], dtype=np.int64), np.diff(pattern.indptr)) * width + pattern.indices
    mkey = np.repeat(np.arange(M.shape[0], dtype=np.int64), np.diff(M.indptr)) * width + M.indices
    pos = np.searchsorted(key, mkey)
    assert (pos < len(key)).all() and np.array_equal(key[pos], mkey)
    out = np.zeros(len(key))
    out[pos] = M.data
    return out


def prolongator(lv):
    n, nc = lv["n"], lv["nc"]
    return sp.csr_matrix((np.ones(n), lv["agg"].astype(np.int64), np.arange(n + 1)), shape=(n, nc))


# ---- setup ---------------------------------------------------------------------------------------------------------------
def check_matrix(l, lv):
    n, nnz = lv["n"], lv["nnz"]
    ip, ix, da = lv["indptr"], lv["indices"], lv["data"]
    if not (len(ip) == n + 1 and len(ix) == nnz and len(da) == nnz and n >= 1):
        raise AmgMismatch(l, "A structure", 0, f"n {n} nnz {nnz}: {len(ip)} row starts, {len(ix)} columns, {len(da)} values")
    if ip[0] != 0 or ip[-1] != nnz or (np.diff(ip) < 0).any():
        raise AmgMismatch(l, "A structure", _first(np.diff(ip) < 0), "row starts do not ascend from 0 to nnz")
    if nnz and (ix.min() < 0 or ix.max() >= n):
        raise AmgMismatch(l, "A structure", 0, "column outside [0, n)")
    rows = np.repeat(np.arange(n), np.diff(ip))
    inner = np.ones(nnz, dtype=bool)
    inner[ip[:-1][np.diff(ip) > 0]] = False  # the first entry of each row
    bad = inner & (np.diff(ix, prepend=-1) <= 0)
    if bad.any():
        raise AmgMismatch(l, "A structure", int(rows[_first(bad)]), "columns of a row not strictly ascending")


def check_dinv(l, lv):
    A = csr_of_level(lv)
    diag = A.diagonal()
    if len(lv["dinv"]) != lv["n"] or not (diag > 0).all():
        raise AmgMismatch(l, "dinv", _first(~(diag > 0)), "missing or a diagonal entry that is not positive")
    bad = _bits(lv["dinv"]) != _bits(1.0 / diag)
    if bad.any():
        raise AmgMismatch(l, "dinv", _first(bad), "not the bits of 1 / diag")


def check_partition(l, lv, n_next):
    n, nc = lv["n"], lv["nc"]
    agg, memptr, mem = lv["agg"], lv["memptr"], lv["mem"]
    if nc != n_next or nc < 1 or len(agg) != n or len(memptr) != nc + 1 or len(mem) != n:
        raise AmgMismatch(l, "partition", 0, f"nc {nc}, next level {n_next}: {len(agg)} / {len(memptr)} / {len(mem)} items")
    if agg.min() < 0 or agg.max() >= nc:
        raise AmgMismatch(l, "partition", _first((agg < 0) | (agg >= nc)), "aggregate outside [0, nc)")
    counts = np.bincount(agg, minlength=nc)
    if (counts == 0).any():
        raise AmgMismatch(l, "partition", _first(counts == 0), "empty aggregate")
    ref_ptr = np.concatenate([[0], np.cumsum(counts)])
    if not np.array_equal(memptr, ref_ptr):
        raise AmgMismatch(l, "partition", _first(memptr != ref_ptr), "memptr is not the scan of the aggregates' sizes")
    ref_mem = np.argsort(agg, kind="stable")  # by aggregate, members ascending
    if not np.array_equal(mem, ref_mem):
        raise AmgMismatch(l, "partition", int(agg[ref_mem[_first(mem != ref_mem)]]), "mem: members not ascending / not agg's")
    # connected: the edges of A_l inside aggregates leave exactly nc components
    A = csr_of_level(lv).tocoo()
    keep = (agg[A.row] == agg[A.col]) & (A.data != 0.0) & (A.row != A.col)
    G = sp.csr_matrix((np.ones(int(keep.sum())), (A.row[keep], A.col[keep])), shape=(n, n))
    ncomp, label = connected_components(G, directed=False)
    if ncomp != nc:
        per = np.zeros(nc, dtype=np.int64)
        np.add.at(per, agg[np.unique(label, return_index=True)[1]], 1)
        raise AmgMismatch(l, "partition", _first(per > 1), f"aggregate not connected in A ({ncomp} pieces for {nc} aggregates)")


def check_galerkin(l, lv, nxt, stats):
    A, P = csr_of_level(lv), prolongator(lv)
    pattern = (P.T @ _ones(A) @ P).tocsr()
    pattern.sort_indices()
    nc = lv["nc"]
    if nxt["nnz"] != pattern.nnz or not np.array_equal(nxt["indptr"], pattern.indptr):
        raise AmgMismatch(l, "galerkin pattern", _first(np.asarray(nxt["indptr"][:nc + 1]) != pattern.indptr[:len(nxt["indptr"])]),
                          f"{nxt['nnz']} entries, P^T A P has {pattern.nnz}")
    rows = np.repeat(np.arange(nc), np.diff(pattern.indptr))
    if not np.array_equal(nxt["indices"], pattern.indices):
        raise AmgMismatch(l, "galerkin pattern", int(rows[_first(nxt["indices"] != pattern.indices)]), "columns differ")
    ref = _on_pattern(P.T @ A @ P, pattern)
    bound = (pattern.data + 3.0) * U * _on_pattern(P.T @ _abs(A) @ P, pattern)
    err = np.abs(nxt["data"] - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    stats["galerkin"] = max(stats.get("galerkin", 0.0), float(ratio.max()))
    if (err > bound).any():
        raise AmgMismatch(l, "galerkin values", int(rows[_first(err > bound)]), f"worst error / bound {ratio.max():.3g}")


def block_sizes(lv, block_max):
    m = np.diff(lv["memptr"]).astype(np.int64)
    return m, np.where(m <= block_max, m * m, m)


def dense_blocks(lv, which):
    """A_l restricted to the aggregates `which` (all of one size m), in member order: [len(which), m, m]."""
    memptr, mem, agg = lv["memptr"], lv["mem"], lv["agg"]
    n = lv["n"]
    m = int(memptr[which[0] + 1] - memptr[which[0]])
    pos = np.empty(n, dtype=np.int64)
    pos[mem] = np.arange(n) - np.repeat(memptr[:-1], np.diff(memptr))
    slot = np.full(lv["nc"], -1, dtype=np.int64)
    slot[which] = np.arange(len(which))
    A = csr_of_level(lv).tocoo()
    keep = (agg[A.row] == agg[A.col]) & (slot[agg[A.row]] >= 0)
    out = np.zeros((len(which), m, m))
    out[slot[agg[A.row[keep]]], pos[A.row[keep]], pos[A.col[keep]]] = A.data[keep]
    return out


def stored_blocks(lv, which, m):
    """The level's binv blocks of the aggregates `which` as stored, [len(which), m, m] row-major."""
    idx = lv["boff"][which].astype(np.int64)[:, None] + np.arange(m * m)[None, :]
    return lv["binv"][idx].reshape(len(which), m, m)


def check_blocks(l, lv, block_max, stats):
    nc = lv["nc"]
    m, sq = block_sizes(lv, block_max)
    ref_off = np.concatenate([[0], np.cumsum(sq)])
    if len(lv["boff"]) != nc + 1 or not np.array_equal(lv["boff"].astype(np.int64), ref_off):
        raise AmgMismatch(l, "boff", 0, "not the exclusive scan of m^2 (m above BLOCK_MAX)")
    if len(lv["binv"]) != ref_off[-1]:
        raise AmgMismatch(l, "binv", 0, f"{len(lv['binv'])} doubles, the blocks take {ref_off[-1]}")
    diag = csr_of_level(lv).diagonal()
    for size in np.unique(m):
        which = np.nonzero(m == size)[0]
        size = int(size)
        if size > block_max:
            for I in which:
                members = lv["mem"][lv["memptr"][I]:lv["memptr"][I + 1]]
                got = lv["binv"][ref_off[I]:ref_off[I] + size]
                if not _same_bits(got, 1.0 / diag[members]):
                    raise AmgMismatch(l, "binv", int(I), "an aggregate above BLOCK_MAX does not hold the bits of 1 / diag")
            continue
        B = dense_blocks(lv, which)
        X = stored_blocks(lv, which, size).transpose(0, 2, 1)  # stored transposed
        ref = np.linalg.inv(B)
        cond = np.linalg.cond(B, 2)
        bound = size * U * cond * np.abs(ref).max(axis=(1, 2))
        err = np.abs(X - ref).max(axis=(1, 2))
        res = np.abs(B @ X - np.eye(size)).max(axis=(1, 2))
        stats["binv"] = max(stats.get("binv", 0.0), float((err / bound).max()))
        bad = (err > bound) | (res > bound * np.abs(B).max(axis=(1, 2))) | ~np.isfinite(err)
        if bad.any():
            k = _first(bad)
            raise AmgMismatch(l, "binv", int(which[k]), f"{size} members: error / bound {err[k] / bound[k]:.3g}, "
                              f"|B X - I| / bound {res[k] / (bound[k] * np.abs(B[k]).max()):.3g}")


def check_coarse_inv(l, lv, inv, stats):
    n = lv["n"]
    if len(inv) != n * n or n > 64:
        raise AmgMismatch(l, "coarse_inv", 0, f"{len(inv)} values for a last level of {n} rows")
    inv = inv.reshape(n, n)
    Ad = csr_of_level(lv).toarray()
    ref = np.linalg.inv(Ad)
    bound = 64 * U * np.linalg.cond(Ad, 2) * np.abs(ref).max()
    err = np.abs(inv - ref)
    stats["coarse_inv"] = max(stats.get("coarse_inv", 0.0), float(err.max() / bound))
    if (err > bound).any() or not np.isfinite(err).all():
        raise AmgMismatch(l, "coarse_inv", _first((err > bound).any(axis=1)), f"worst error / bound {err.max() / bound:.3g}")
    res = np.abs(Ad @ inv - np.eye(n))
    if (res > bound * np.abs(Ad).max()).any():
        raise AmgMismatch(l, "coarse_inv", _first((res > bound * np.abs(Ad).max()).any(axis=1)), "A coarse_inv - I beyond the bound")


def check_tail(levels, info):
    tail, td, img = info["tail"], info["tdesc"], info["tail_image"]
    nlev = len(levels)
    if tail < 0:
        if td is not None or len(img):
            raise AmgMismatch(-1, "tail", 0, "an image without a tail")
        return
    if not (1 <= tail < nlev - 1) or not info["coarse_direct"]:
        raise AmgMismatch(tail, "tail", 0, f"tail {tail} of {nlev} levels (level 0 and the last alone never form one)")
    nt = td["nlev"]
    if nt != nlev - tail or nt > info["TAIL_MAX_LEVELS"] or len(td["lv"]) != nt:
        raise AmgMismatch(tail, "tail", 0, f"{nt} levels in the descriptor, {nlev - tail} below the tail's first")
    if len(img) != td["image_bytes"] or td["image_bytes"] > td["total_bytes"] or td["total_bytes"] > info["TAIL_LDS_BUDGET"]:
        raise AmgMismatch(tail, "tail", 0, f"image {len(img)} / {td['image_bytes']} bytes, total {td['total_bytes']}, "
                          f"budget {info['TAIL_LDS_BUDGET']}")
    spans = []  # (offset, bytes, name, inside the image)
    for k, t in enumerate(td["lv"]):
        lv = levels[tail + k]
        want = (lv["n"], lv["nnz"], lv["nc"])
        if (t["n"], t["nnz"], t["nc"]) != want:
            raise AmgMismatch(tail + k, "tail", 0, f"descriptor sizes {(t['n'], t['nnz'], t['nc'])}, level {want}")
        if k < nt - 1:
            sections = (("o_data", lv["data"]), ("o_dinv", lv["dinv"]), ("o_indptr", lv["indptr"]), ("o_memptr", lv["memptr"]),
                        ("o_indices", lv["indices"].astype(np.uint16)), ("o_agg", lv["agg"].astype(np.uint16)),
                        ("o_mem", lv["mem"].astype(np.uint16)))
            if lv["n"] > 65535:
                raise AmgMismatch(tail + k, "tail", 0, "a level of more than 65535 rows inside the tail")
            for name, src in sections:
                off, nb = t[name], src.nbytes
                spans.append((off, nb, f"{name}[{k}]", True))
                if off < 0 or off + nb > len(img) or not np.array_equal(img[off:off + nb], np.ascontiguousarray(src).view(np.uint8)):
                    raise AmgMismatch(tail + k, "tail image", name, "not the bits of the level's array")
        for name in ("o_B", "o_X", "o_E", "o_R"):
            spans.append((t[name], lv["n"] * 8, f"{name}[{k}]", False))
    inv = info["coarse_inv"]
    spans.append((td["o_inv"], inv.nbytes, "o_inv", True))
    off = td["o_inv"]
    if off < 0 or off + inv.nbytes > len(img) or not np.array_equal(img[off:off + inv.nbytes], inv.view(np.uint8)):
        raise AmgMismatch(nlev - 1, "tail image", "o_inv", "not the bits of coarse_inv")
    for name in ("o_C1", "o_V1"):
        spans.append((td[name], levels[tail]["n"] * 8, name, False))
    spans.sort()
    end = 0
    for off, nb, name, inside in spans:
        limit = td["image_bytes"] if inside else td["total_bytes"]
        if off % 16 or off < end or off + nb > limit or (not inside and off < td["image_bytes"]):
            raise AmgMismatch(tail, "tail layout", name, f"offset {off} (+{nb}) after {end}, limit {limit}")
        end = off + nb


def check_amg(levels, info, csr0=None):
    """Every identity of the module's docstring on an exported hierarchy; raises AmgMismatch on the first violation.
    csr0: (indptr, indices, data) of the matrix level 0 aliases, compared byte for byte.  Returns the largest observed
    error / bound per bounded quantity ("galerkin", "binv", "coarse_inv")."""
    stats = {}
    nlev = len(levels)
    tail = info["tail"]
    if csr0 is not None:
        for name, ref in zip(("indptr", "indices", "data"), csr0):
            ref = np.ascontiguousarray(ref)
            if levels[0][name].tobytes() != ref.astype(levels[0][name].dtype).tobytes():
                raise AmgMismatch(0, "level 0", name, "not the bytes of the context's CSR matrix")
    upto = tail if tail >= 0 else nlev - 1
    for l, lv in enumerate(levels):
        check_matrix(l, lv)
        check_dinv(l, lv)
        want_block = bool(info["block_smoother"]) and l < upto
        if bool(lv["block"]) != want_block or lv["in_tail"] != int(tail >= 0 and l >= tail):
            raise AmgMismatch(l, "flags", 0, f"block {lv['block']} (expected {int(want_block)}), in_tail {lv['in_tail']}")
        if l + 1 == nlev:
            if lv["nc"] != 0 or len(lv["agg"]) or len(lv["mem"]) or len(lv["memptr"]):
                raise AmgMismatch(l, "partition", 0, "the last level exports aggregates")
            break
        check_matrix(l + 1, levels[l + 1])
        check_partition(l, lv, levels[l + 1]["n"])
        check_galerkin(l, lv, levels[l + 1], stats)
        if want_block:
            check_blocks(l, lv, info["BLOCK_MAX"], stats)
        elif len(lv["boff"]) or len(lv["binv"]):
            raise AmgMismatch(l, "binv", 0, "blocks on a level without the block smoother")
    last = levels[-1]
    if bool(info["coarse_direct"]) != (nlev > 1 and last["n"] <= info["COARSEST_MAX"]):
        raise AmgMismatch(nlev - 1, "coarse_inv", 0, f"coarse_direct {info['coarse_direct']} with a last level of {last['n']} rows")
    if info["coarse_direct"]:
        check_coarse_inv(nlev - 1, last, info["coarse_inv"], stats)
    elif len(info["coarse_inv"]):
        raise AmgMismatch(nlev - 1, "coarse_inv", 0, "an inverse without a direct coarsest solve")
    check_tail(levels, info)
    return stats


# ---- cycle ----------------------------------------------------------------------------------------------------------------
LONG_ROW = 64  # rows above this many entries are summed one by one (np.cumsum: sequential), the others slot by slot


class _Sums:
    """Sequential sums of consecutive runs (rows of a CSR matrix, member lists), ascending or descending."""

    def __init__(self, ptr):
        self.ptr = np.asarray(ptr, dtype=np.int64)
        self.lens = np.diff(self.ptr)
        self.long = np.nonzero(self.lens > LONG_ROW)[0]
        short = np.nonzero((self.lens <= LONG_ROW) & (self.lens > 0))[0]
        short = short[np.argsort(-self.lens[short], kind="stable")]  # longest first: the active rows are a prefix
        self.short = short
        slens = self.lens[short]
        width = int(slens.max()) if len(short) else 0
        self.active = [int(np.searchsorted(-slens, -k, side="right")) for k in range(1, width + 1)]  # rows with len >= k

    def __call__(self, values, descending):
        out = np.zeros(len(self.lens), dtype=values.dtype)
        ptr, short = self.ptr, self.short
        for k, cnt in enumerate(self.active):
            rows = short[:cnt]
            out[rows] += values[(ptr[rows + 1] - 1 - k) if descending else (ptr[rows] + k)]
        for i in self.long:
            seg = values[ptr[i]:ptr[i + 1]]
            out[i] = np.cumsum(seg[::-1] if descending else seg)[-1]
        return out


class Reference:
    """The decoded hierarchy with what the four evaluations of reference_cycle share."""

    def __init__(self, levels, info):
        self.levels, self.info = levels, info
        self.nlev = len(levels)
        self.row_sums = [_Sums(lv["indptr"]) for lv in levels]
        self.mem_sums = [_Sums(lv["memptr"]) if l + 1 < self.nlev else None for l, lv in enumerate(levels)]
        self.blocks = {}

    def level_blocks(self, l):
        """per size m: (aggregates, members [k, m], inverse [k, m, m] with [g, r, c] = entry (r, c) of the inverse)"""
        if l not in self.blocks:
            lv = self.levels[l]
            m, _ = block_sizes(lv, self.info["BLOCK_MAX"])
            groups = []
            for size in np.unique(m):
                which = np.nonzero(m == size)[0]
                size = int(size)
                members = lv["mem"][lv["memptr"][which].astype(np.int64)[:, None] + np.arange(size)[None, :]]
                if size > self.info["BLOCK_MAX"]:
                    idx = lv["boff"][which].astype(np.int64)[:, None] + np.arange(size)[None, :]
                    groups.append((size, members, lv["binv"][idx], True))
                else:
                    groups.append((size, members, stored_blocks(lv, which, size).transpose(0, 2, 1), False))
            self.blocks[l] = groups
        return self.blocks[l]


class _Arith:
    def __init__(self, ref, ordering, defect):
        assert ordering in ORDERINGS + ("ext",) and defect in DEFECTS + (None,)
        self.ref, self.defect = ref, defect
        self.dt = np.longdouble if ordering == "ext" else np.float64
        self.desc = ordering == "desc"
        self.partials = ordering == "dots128"
        self.w = self.dt(ref.info["OMEGA"])

    def c(self, a):
        return np.asarray(a, dtype=self.dt)

    def spmv(self, l, x):
        lv = self.ref.levels[l]
        return self.ref.row_sums[l](self.c(lv["data"]) * x[lv["indices"]], self.desc)

    def restrict(self, l, r):
        return self.ref.mem_sums[l](r[self.ref.levels[l]["mem"]], self.desc)

    def dot(self, a, b):
        p = a * b
        if self.partials:
            s = self.dt(0)
            for piece in np.array_split(p, 128):
                s = s + piece.sum(dtype=self.dt)
            return s
        return p.sum(dtype=self.dt)

    def dense(self, inv, b):
        n = len(b)
        M = self.c(inv).reshape(n, n)
        out = np.zeros(n, dtype=self.dt)
        for j in (range(n - 1, -1, -1) if self.desc else range(n)):
            out += M[:, j] * b[j]
        return out

    def block_apply(self, l, v):
        out = np.zeros(len(v), dtype=self.dt)
        for size, members, inv, diagonal in self.ref.level_blocks(l):
            vm = v[members]
            if diagonal:
                out[members] = self.c(inv) * vm
                continue
            s = np.zeros(members.shape, dtype=self.dt)
            inv = self.c(inv)
            for c in (range(size - 1, -1, -1) if self.desc else range(size)):
                s += inv[:, :, c] * vm[:, c][:, None]
            out[members] = s
        return out

    # -- the algebra --
    def coefficients(self, rho1, alpha1, gamma, beta, alpha2):
        if self.defect == "gamma_beta":
            gamma, beta = beta, gamma
        if not rho1 > 0:
            return self.dt(0), self.dt(0)
        rho2 = beta - gamma * gamma / rho1
        if not rho2 > 0 and self.defect != "no_rho2_guard":
            return alpha1 / rho1, self.dt(0)
        with np.errstate(divide="ignore", invalid="ignore"):
            return alpha1 / rho1 - gamma * alpha2 / (rho1 * rho2), alpha2 / rho2

    def two_steps(self, l, rc, solve):
        """two flexible-CG steps on A_l c = rc preconditioned by `solve`: c1, c2, (s1, s2)"""
        c1 = solve(rc)
        v1 = self.spmv(l, c1)
        rho1, alpha1 = self.dot(c1, v1), self.dot(c1, rc)
        t = alpha1 / rho1 if rho1 > 0 else self.dt(0)
        r2 = rc - t * v1
        c2 = solve(r2)
        v2 = self.spmv(l, c2)
        s1, s2 = self.coefficients(rho1, alpha1, self.dot(c2, v1), self.dot(c2, v2), self.dot(c2, r2))
        if self.defect == "no_s2":
            s2 = self.dt(0)
        return c1, c2, s1, s2

    def tail_vcycle(self, b):
        ref, w = self.ref, self.w
        first, last = ref.info["tail"], ref.nlev - 1
        B, X = {first: b}, {}
        for l in range(first, last):
            dinv = self.c(ref.levels[l]["dinv"])
            X[l] = w * dinv * B[l]
            B[l + 1] = self.restrict(l, B[l] - self.spmv(l, X[l]))
        E = self.dense(ref.info["coarse_inv"], B[last])
        for l in range(last - 1, first - 1, -1):
            lv = ref.levels[l]
            xp = X[l] + E[lv["agg"]]
            E = xp + w * self.c(lv["dinv"]) * (B[l] - self.spmv(l, xp))
        return E

    def cycle(self, l, b):
        ref, w, info = self.ref, self.w, self.ref.info
        lv = ref.levels[l]
        if l == ref.nlev - 1:
            return self.dense(info["coarse_inv"], b) if info["coarse_direct"] else self.c(lv["dinv"]) * b
        dinv = self.c(lv["dinv"])
        block = bool(lv["block"])
        x = w * self.block_apply(l, b) if block else w * dinv * b
        r = b - self.spmv(l, x)
        two = (not block) and l == 0 and info["sweeps0"] == 2
        if two and self.defect != "one_sweep":
            x = x + w * dinv * r
            r = b - self.spmv(l, x)
        rc = self.restrict(l, r)
        if l + 1 == info["tail"]:
            c1, c2, s1, s2 = self.two_steps(l + 1, rc, self.tail_vcycle)
        elif l + 1 == ref.nlev - 1 or l + 1 > info["kmax"]:
            c1, c2, s1, s2 = self.cycle(l + 1, rc), None, self.dt(1), self.dt(0)
        else:
            c1, c2, s1, s2 = self.two_steps(l + 1, rc, lambda v: self.cycle(l + 1, v))
        agg = lv["agg"]
        xp = x + s1 * c1[agg]
        if c2 is not None:
            xp = xp + s2 * c2[agg]
        if block:
            r2 = b if self.defect == "block_post_b" else b - self.spmv(l, xp)
            return xp + w * self.block_apply(l, r2)
        out = xp + w * dinv * (b - self.spmv(l, xp))
        if two and self.defect != "one_sweep":
            out = out + w * dinv * (b - self.spmv(l, out))
        return out


def reference_cycle(levels, info, level, r, ordering="ext", defect=None, ref=None):
    """One cycle at `level` (outside the tail) applied to r in the arithmetic `ordering` ("ext": np.longdouble; "asc" /
    "desc" / "dots128": fp64, see the module's docstring).  ref: a Reference of (levels, info) to share."""
    ref = ref or Reference(levels, info)
    assert 0 <= level < ref.nlev and not (info["tail"] >= 0 and level >= info["tail"])
    a = _Arith(ref, ordering, defect)
    with np.errstate(over="ignore", invalid="ignore"):
        return a.cycle(level, a.c(r))


def distance(z, z_ext):
    """max-norm distance of z from the extended result relative to it (inf where z is not finite; 0 for 0 against 0)."""
    z_ext = np.asarray(z_ext, dtype=np.longdouble)
    z = np.asarray(z, dtype=np.longdouble)
    if not np.isfinite(z).all():
        return float("inf")
    scale = np.abs(z_ext).max()
    d = np.abs(z - z_ext).max()
    return float(d / scale) if scale > 0 else (0.0 if d == 0 else float("inf"))


def cycle_bar(levels, info, level, r, ref=None):
    """(z_ext, E): the cycle in extended precision and the largest distance of the three fp64 orderings from it."""
    ref = ref or Reference(levels, info)
    z_ext = reference_cycle(levels, info, level, r, "ext", ref=ref)
    E = max(distance(reference_cycle(levels, info, level, r, o, ref=ref), z_ext) for o in ORDERINGS)
    return z_ext, E
