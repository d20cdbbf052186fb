"""One round of the exact low-degree elimination (nodal_amd/csrc/lowdeg.hip) restated on the host in exact rational
arithmetic, for tests/test_gpu_lowdeg.py (the device's rounds, exported by Handle.debug_lowdeg) and
tests/test_lowdeg_reference.py (this file against itself, no GPU).

A round takes the parent's CSR matrix A (a symmetric M-matrix: positive diagonal, off-diagonals <= 0), removes an
independent set F of nodes with one or two neighbours and leaves, on the kept nodes C in their old order,

    S   = A_CC - A_CF D_F^-1 A_FC        b_C = b_C - A_CF D_F^-1 b_F        x_F = D_F^-1 (b_F - A_FC x_C).

Everything is stated on the parent the DEVICE holds (its doubles, read as rationals): a round is judged alone, errors
of earlier rounds do not leak in.

The bound.  Every device value is a sum of m terms; a term is an entry of A as it stands (no rounding) or a product
v w / d (two roundings, relative error <= 2u + u^2), and the running sum of m terms rounds m - 1 times (the first
addition, to 0.0 or to b_i, is exact).  To first order |device - exact| <= (m - 1 + 2) u T with T = sum |term|; the
bar is (m + 3) u T, u = 2^-53: two more units of u T for everything of second order.  The recovery's terms a x / d
carry the product's rounding and the final division's: the same form.  T = 0 demands the exact value.  Nothing here
was tuned against the device.
"""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
_M64 = (1 << 64) - 1


def node_priority(i):
    """lowdeg.hip's node_priority with numpy.uint64 (wrapping products): odd indices first, a hash among equals."""
    i = np.asarray(i, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = i * np.uint64(0x9E3779B97F4A7C15)
        h = h ^ (h >> np.uint64(31))
        h = h * np.uint64(0xBF58476D1CE4E5B9)
        h = h ^ (h >> np.uint64(29))
        return ((i & np.uint64(1)) << np.uint64(63)) | ((h >> np.uint64(1)) & np.uint64(0x7FFFFFFF00000000)) | i


def _priority_int(i):
    """The same with Python integers: node_priority is held against it in the self-test."""
    h = (i * 0x9E3779B97F4A7C15) & _M64
    h ^= h >> 31
    h = (h * 0xBF58476D1CE4E5B9) & _M64
    h ^= h >> 29
    return ((i & 1) << 63) | ((h >> 1) & 0x7FFFFFFF00000000) | i


def diag_positions(indptr, indices):
    """Position of each row's diagonal entry in the CSR arrays, -1 where there is none."""
    n = len(indptr) - 1
    dp = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        for e in range(indptr[i], indptr[i + 1]):
            if indices[e] == i:
                dp[i] = e
    return dp


def candidates(indptr, indices, data):
    """1 or 2 off-diagonal entries and a positive diagonal."""
    dp = diag_positions(indptr, indices)
    off = np.diff(indptr) - 1
    cand = (dp >= 0) & (off >= 1) & (off <= 2)
    cand[cand] = np.asarray(data)[dp[cand]] > 0.0
    return cand


def select(indptr, indices, data):
    """F as a bool array: a candidate is taken if no candidate neighbour has a higher priority."""
    n = len(indptr) - 1
    cand = candidates(indptr, indices, data)
    pri = node_priority(np.arange(n))
    take = cand.copy()
    for i in np.nonzero(cand)[0]:
        for e in range(indptr[i], indptr[i + 1]):
            j = indices[e]
            if j != i and cand[j] and pri[j] > pri[i]:
                take[i] = False
    return take


def renumber(F):
    """newidx: the rank among the kept nodes, -1 for a node of F."""
    F = np.asarray(F, dtype=bool)
    return np.where(F, -1, np.cumsum(~F) - 1).astype(np.int32)


def floating_component(indptr, indices, grounded):
    """Union-find verdict: 1 if some connected component of the graph holds no grounded node."""
    n = len(indptr) - 1
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i in range(n):
        for e in range(indptr[i], indptr[i + 1]):
            a, b = find(i), find(int(indices[e]))
            if a != b:
                parent[max(a, b)] = min(a, b)
    ok = set(find(i) for i in range(n) if grounded[i])
    return int(any(find(i) not in ok for i in range(n)))


class Round:
    """One round on the parent (indptr, indices, data); F defaults to the selection rule's set."""

    def __init__(self, indptr, indices, data, F=None):
        self.indptr = np.asarray(indptr, dtype=np.int64)
        self.indices = np.asarray(indices, dtype=np.int64)
        self.data = np.asarray(data, dtype=np.float64)
        self.n = len(self.indptr) - 1
        self.diag = diag_positions(self.indptr, self.indices)
        self.cand = candidates(self.indptr, self.indices, self.data)
        self.rule = select(self.indptr, self.indices, self.data)
        self.F = self.rule.copy() if F is None else np.asarray(F, dtype=bool).copy()
        self.newidx = renumber(self.F)
        self.nk = int((~self.F).sum())
        self._lists = None
        self._exact = None

    def row(self, i):
        return range(self.indptr[i], self.indptr[i + 1])

    def adjacent_in_F(self):
        """Pairs (i, j), i < j, of adjacent nodes that are both in F: must be empty."""
        return [(i, int(self.indices[e])) for i in np.nonzero(self.F)[0] for e in self.row(i)
                if self.indices[e] > i and self.F[self.indices[e]]]

    def lists(self):
        """{(row, col) of S: [(e, slot, q)]} in the device's contrib order, ascending (e, slot): slot 0 passes A's
        entry e through (q = -1); slot 1 + t multiplies entry e = (i, f) with entry q = (f, k), k the t-th off-diagonal
        entry of row f."""
        if self._lists is None:
            assert not self.adjacent_in_F(), "F is not an independent set"
            out = {}
            for i in np.nonzero(~self.F)[0]:
                ni = int(self.newidx[i])
                for e in self.row(i):
                    j = int(self.indices[e])
                    if not self.F[j]:
                        out.setdefault((ni, int(self.newidx[j])), []).append((e, 0, -1))
                        continue
                    t = 0
                    for q in self.row(j):
                        k = int(self.indices[q])
                        if k == j:
                            continue
                        out.setdefault((ni, int(self.newidx[k])), []).append((e, 1 + t, q))
                        t += 1
            self._lists = {key: sorted(v) for key, v in out.items()}
        return self._lists

    def pattern(self):
        """(indptr, indices, diag_pos) of S: kept-kept entries united with (i, k) for every neighbour k of an eliminated
        neighbour of i (k == i included), columns ascending; an entry whose value cancels stays."""
        keys = sorted(self.lists())
        indptr = np.zeros(self.nk + 1, dtype=np.int32)
        for r, _ in keys:
            indptr[r + 1] += 1
        indptr = np.cumsum(indptr).astype(np.int32)
        indices = np.array([c for _, c in keys], dtype=np.int32)
        diag_pos = np.full(self.nk, -1, dtype=np.int32)
        for pos, (r, c) in enumerate(keys):
            if r == c:
                diag_pos[r] = pos
        return indptr, indices, diag_pos

    def contrib(self):
        """(cptr, contrib) as group.h lays them out for this pattern: e << 3 | slot, ascending per entry."""
        keys = sorted(self.lists())
        cptr, con = [0], []
        for key in keys:
            con += [(e << 3) | slot for e, slot, _ in self.lists()[key]]
            cptr.append(len(con))
        return np.array(cptr, dtype=np.int32), np.array(con, dtype=np.uint32)

    def _term(self, e, q):
        a = Fraction(float(self.data[e]))
        if q < 0:
            return a
        f = int(self.indices[e])
        return -a * Fraction(float(self.data[q])) / Fraction(float(self.data[self.diag[f]]))

    def exact_values(self, drop=None):
        """Per entry of S in pattern order: (value, T = sum |term|, m = terms), Fractions.  drop = (entry, k) leaves the
        k-th term of one entry out (the self-test's planted defect)."""
        if self._exact is None or drop is not None:
            out = []
            for pos, key in enumerate(sorted(self.lists())):
                terms = [self._term(e, q) for e, _, q in self.lists()[key]]
                if drop is not None and drop[0] == pos:
                    terms.pop(drop[1])
                out.append((sum(terms, Fraction(0)), sum((abs(t) for t in terms), Fraction(0)), len(terms)))
            if drop is not None:
                return out
            self._exact = out
        return self._exact

    def float_values(self, order="fixed"):
        """S in fp64 as the device sums it.  order "fixed": the pass-through entry first, then the eliminated
        neighbours in their stored (ascending) order -- the same sequence in S(i, k) and S(k, i); "contrib": ascending
        (e, slot) as the lists stand, which puts the pass-through entry where its column falls among the others."""
        out = []
        for key in sorted(self.lists()):
            items = self.lists()[key]
            if order == "fixed":
                items = [it for it in items if it[1] == 0] + [it for it in items if it[1] != 0]
            s = 0.0
            for e, slot, q in items:
                v = float(self.data[e])
                if slot == 0:
                    s += v
                else:
                    s -= v * float(self.data[q]) / float(self.data[self.diag[int(self.indices[e])]])
            out.append(s)
        return np.array(out, dtype=np.float64)

    def exact_rhs(self, b):
        """b_C per kept node: (value, T, m)."""
        out = []
        for i in np.nonzero(~self.F)[0]:
            terms = [Fraction(float(b[i]))]
            for e in self.row(i):
                f = int(self.indices[e])
                if self.F[f]:
                    terms.append(-Fraction(float(self.data[e])) * Fraction(float(b[f])) / Fraction(float(self.data[self.diag[f]])))
            out.append((sum(terms, Fraction(0)), sum((abs(t) for t in terms), Fraction(0)), len(terms)))
        return out

    def float_rhs(self, b):
        out = []
        for i in np.nonzero(~self.F)[0]:
            s = float(b[i])
            for e in self.row(i):
                f = int(self.indices[e])
                if self.F[f]:
                    s -= float(self.data[e]) * float(b[f]) / float(self.data[self.diag[f]])
            out.append(s)
        return np.array(out, dtype=np.float64)

    def exact_recovery(self, b, xc):
        """{eliminated node: (value, T, m)} of x_F at the given x_C (doubles or Fractions)."""
        out = {}
        for i in np.nonzero(self.F)[0]:
            d = Fraction(float(self.data[self.diag[i]]))
            terms = [Fraction(float(b[i])) / d]
            for e in self.row(i):
                k = int(self.indices[e])
                if k != i:
                    terms.append(-Fraction(float(self.data[e])) * Fraction(xc[self.newidx[k]]) / d)
            out[int(i)] = (sum(terms, Fraction(0)), sum((abs(t) for t in terms), Fraction(0)), len(terms))
        return out

    def float_recovery(self, b, xc):
        x = np.empty(self.n, dtype=np.float64)
        for i in range(self.n):
            if not self.F[i]:
                x[i] = xc[self.newidx[i]]
                continue
            s = float(b[i])
            for e in self.row(i):
                k = int(self.indices[e])
                if k != i:
                    s -= float(self.data[e]) * float(xc[self.newidx[k]])
            x[i] = s / float(self.data[self.diag[i]])
        return x

    def flags(self, grounded):
        """The child's "touches ground" flags: a kept node's own flag OR those of its eliminated neighbours."""
        out = []
        for i in np.nonzero(~self.F)[0]:
            g = int(grounded[i])
            for e in self.row(i):
                if self.F[self.indices[e]]:
                    g |= int(grounded[self.indices[e]])
            out.append(g)
        return np.array(out, dtype=np.uint8)

    def emulate(self, b, grounded, order="fixed"):
        """What a faultless device exports for this round, the child's side: a dict with the names of
        _ffi.LOWDEG_ARRAYS (no solutions)."""
        indptr, indices, diag_pos = self.pattern()
        cptr, con = self.contrib()
        return dict(p_newidx=self.newidx.copy(), p_rhs=np.asarray(b, dtype=np.float64), p_grounded=np.asarray(grounded, dtype=np.uint8),
                    indptr=indptr, indices=indices, diag_pos=diag_pos, data=self.float_values(order),
                    rhs=self.float_rhs(b), grounded=self.flags(grounded), cptr=cptr, contrib=con,
                    p_x=np.empty(0), x=np.empty(0), child_n=self.nk, child_nnz=len(indices))


def leftover(indptr, grounded):
    """The structural verdict of ld_state 3: a row of at most one entry that is not grounded."""
    return bool(np.any((np.diff(indptr) <= 1) & (np.asarray(grounded) == 0)))


def _outside(dev, exact):
    """Indices where a device double misses its (value, T, m) by more than (m + 3) u T; the worst error / bound."""
    bad, worst = [], 0.0
    for pos, (val, T, m) in enumerate(exact):
        d = float(dev[pos])
        if not np.isfinite(d):
            bad.append(pos)
            worst = float("inf")
            continue
        err, bound = abs(Fraction(d) - val), (m + 3) * U * T
        if err > bound:
            bad.append(pos)
        if err:
            worst = max(worst, float(err / bound) if bound else float("inf"))
    return bad, worst


def check_round(indptr, indices, data, dev, consecutive_chain=False, ratios=None):
    """Everything a round's export (a dict as Handle.debug_lowdeg returns per round) must satisfy against the parent
    (indptr, indices, data), as a list of failures BY NAME -- empty when all is well.  ratios (a dict) receives the
    worst error / bound of the values, the right-hand side and the recovery."""
    bad = []
    newidx = np.asarray(dev["p_newidx"])
    rule = Round(indptr, indices, data)
    F = newidx < 0
    if np.any(F & ~rule.cand):
        bad.append("selection.candidate: %s" % np.nonzero(F & ~rule.cand)[0][:4])
    rd = Round(indptr, indices, data, F)
    if rd.adjacent_in_F():
        return bad + ["selection.independent: %s" % rd.adjacent_in_F()[:4]]
    if not np.array_equal(F, rule.F):
        bad.append("selection.rule: %s" % np.nonzero(F != rule.F)[0][:4])
    if consecutive_chain and np.any(rule.cand[1::2] & ~F[1::2]):
        bad.append("selection.odd: an odd-indexed candidate was left")
    if not np.array_equal(newidx, rd.newidx) or dev["child_n"] != rd.nk:
        bad.append("renumbering")
        return bad  # (every index below goes through newidx)
    ip, ix, dp = rd.pattern()
    if not (np.array_equal(dev["indptr"], ip) and np.array_equal(dev["indices"], ix) and np.array_equal(dev["diag_pos"], dp)):
        return bad + ["pattern"]
    cptr, con = rd.contrib()
    if not (np.array_equal(dev["cptr"], cptr) and np.array_equal(dev["contrib"], con)):
        bad.append("lists")
    val = np.asarray(dev["data"])
    exact = rd.exact_values()
    out, worst = _outside(val, exact)
    if ratios is not None:
        ratios["S"] = worst
    if out:
        r, c = sorted(rd.lists())[out[0]]
        bad.append("values.bound: %d entries, first S(%d,%d) = %r, exact %r" % (len(out), r, c, float(val[out[0]]), float(exact[out[0]][0])))
    where = {key: pos for pos, key in enumerate(sorted(rd.lists()))}
    for (r, c), pos in where.items():
        if r < c:
            t = where.get((c, r))
            if t is None or val[pos].tobytes() != val[t].tobytes():
                bad.append("values.symmetry: S(%d,%d) = %s, S(%d,%d) = %s" % (
                    r, c, float(val[pos]).hex(), c, r, float(val[t]).hex() if t is not None else "absent"))
                break
    for (r, c), pos in where.items():
        if r != c and not val[pos] <= 0.0:
            bad.append("values.sign: S(%d,%d) = %r" % (r, c, float(val[pos])))
            break
        if r == c and exact[pos][0] > 0 and not val[pos] > 0.0:
            bad.append("values.sign: S(%d,%d) = %r" % (r, c, float(val[pos])))
            break
    b = np.asarray(dev["p_rhs"])
    out, worst = _outside(dev["rhs"], rd.exact_rhs(b))
    if ratios is not None:
        ratios["b"] = worst
    if out:
        bad.append("rhs.bound: %d rows, first %d" % (len(out), out[0]))
    if not np.array_equal(dev["grounded"], rd.flags(dev["p_grounded"])):
        bad.append("flags")
    if len(dev["p_x"]) and len(dev["x"]) and np.all(np.isfinite(dev["x"])):
        x, xc = np.asarray(dev["p_x"]), np.asarray(dev["x"])
        kept = np.nonzero(~F)[0]
        if x[kept].tobytes() != xc.tobytes():
            bad.append("recover.copy")
        rec = rd.exact_recovery(b, [float(v) for v in xc])
        nodes = sorted(rec)
        out, worst = _outside(x[nodes], [rec[i] for i in nodes])
        if ratios is not None:
            ratios["x"] = worst
        if out:
            bad.append("recover.bound: %d nodes, first %d" % (len(out), nodes[out[0]]))
    return bad


# ---- small networks for the self-test and the device tests -----------------------------------------------------------

def assemble(n, resistors, rhs=None):
    """The conductance matrix of resistors [(a, b, ohms)] on unknowns 0 .. n - 1 (a node id >= n is the ground) as sorted
    CSR with every diagonal present, fp64, bitwise symmetric (parallel resistors are summed in list order on both
    sides); grounded[i] = 1 where a resistor joins i to ground."""
    rows = [dict() for _ in range(n)]
    grounded = np.zeros(n, dtype=np.uint8)
    for a, b, ohms in resistors:
        g = 1.0 / float(ohms)
        for p, q in ((a, b), (b, a)):
            if p < n:
                rows[p][p] = rows[p].get(p, 0.0) + g
                if q < n:
                    rows[p][q] = rows[p].get(q, 0.0) - g
                else:
                    grounded[p] = 1
    indptr, indices, data = [0], [], []
    for i in range(n):
        rows[i].setdefault(i, 0.0)
        for j in sorted(rows[i]):
            indices.append(j)
            data.append(rows[i][j])
        indptr.append(len(indices))
    b = np.zeros(n) if rhs is None else np.asarray(rhs, dtype=np.float64)
    return np.array(indptr, dtype=np.int32), np.array(indices, dtype=np.int32), np.array(data), b, grounded


def exact_solve(entries, b, n):
    """Gaussian elimination in Fractions: entries {(i, j): value}, b [n]; None when a pivot is exactly zero."""
    M = [[Fraction(0)] * n + [Fraction(b[i])] for i in range(n)]
    for (i, j), v in entries.items():
        M[i][j] += Fraction(v)
    for c in range(n):
        p = next((r for r in range(c, n) if M[r][c] != 0), None)
        if p is None:
            return None
        M[c], M[p] = M[p], M[c]
        for r in range(n):
            if r != c and M[r][c] != 0:
                f = M[r][c] / M[c][c]
                M[r] = [x - f * y for x, y in zip(M[r], M[c])]
    return [M[i][n] / M[i][i] for i in range(n)]


def bypass_motif(order, values):
    """Four nodes i, f1, f2, k with a direct resistor i - k, the bypasses i - f1 - k and i - f2 - k, and i and k tied
    to ground: (resistor list on ids 0 .. 3, ground 4).  order "outside": i < f1 < f2 < k; "inside": f1 < i < k < f2.
    values: the seven resistances (direct, i-f1, f1-k, i-f2, f2-k, i-ground, k-ground)."""
    i, f1, f2, k = (0, 1, 2, 3) if order == "outside" else (1, 0, 3, 2)
    r = list(values)
    return [(i, k, r[0]), (i, f1, r[1]), (f1, k, r[2]), (i, f2, r[3]), (f2, k, r[4]), (i, 4, r[5]), (k, 4, r[6])]
