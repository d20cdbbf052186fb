"""The identity behind the folded post-smoothing sweep (csrc/sagg.hip ap_rows / ap_rows_lds, csrc/sagg_cycle.h
k_prolong_post), restated in numpy.  With xp = x + P e and r = b - A x,

    xp + w D^-1 (b - A xp) = (x + w D^-1 r) + W e,     W = P - w D^-1 (A P),

and W has the pattern of the row of A P the setup merges anyway.  No symmetry is used.  Everything here is fp64 (the
device stores W in f32; what that costs is the subject of tests/test_gpu_fold_post.py)."""
import numpy as np
import pytest

OMEGA = 0.85  # csrc/sagg.hip, NODAL_SA_OMEGA
PW = 4        # prolongation entries per fine row


def ell_of(dense_rows):
    """[(columns, values)] per row, in slot order."""
    return [(np.asarray(c, dtype=np.int64), np.asarray(v, dtype=np.float64)) for c, v in dense_rows]


def grid_matrix(N):
    """5-point grid with a resistor to ground on every boundary node; slots in ascending column order, as csr_to_ell
    leaves them."""
    rows = []
    for i in range(N):
        for j in range(N):
            k = i * N + j
            ent = {}
            deg = 0.0
            for di, dj in ((-1, 0), (0, -1), (0, 1), (1, 0)):
                a, b = i + di, j + dj
                if 0 <= a < N and 0 <= b < N:
                    g = 1.0 + 0.25 * ((k + a * N + b) % 3)
                    ent[a * N + b] = -g
                    deg += g
                else:
                    deg += 0.5
            ent[k] = deg
            cols = sorted(ent)
            rows.append((cols, [ent[c] for c in cols]))
    return ell_of(rows)


def random_matrix(n, rng, drop_diagonal_of=()):
    """Non-symmetric, 3-9 entries per row in random slot order, a positive diagonal (left out for the rows named)."""
    rows = []
    for i in range(n):
        m = int(rng.integers(2, 9))
        cols = [int(c) for c in rng.choice(n, size=m, replace=False) if c != i]
        vals = [float(v) for v in rng.uniform(-1.0, 1.0, size=len(cols))]
        if i not in drop_diagonal_of:
            at = int(rng.integers(0, len(cols) + 1))
            cols.insert(at, i)
            vals.insert(at, float(rng.uniform(2.0, 4.0)))
        rows.append((cols, vals))
    return ell_of(rows)


def prolongation(n, nc, rng, own=None):
    """Rows of at most PW entries, distinct columns, -1 = an empty slot.  own[i]: a column row i must have."""
    pcol = -np.ones((n, PW), dtype=np.int64)
    pval = np.zeros((n, PW))
    for i in range(n):
        m = int(rng.integers(1, PW + 1))
        cols = list(rng.choice(nc, size=m, replace=False))
        if own is not None and own[i] not in cols:
            cols[0] = own[i]
        slots = rng.permutation(PW)[:m]
        pcol[i, slots] = cols
        pval[i, slots] = rng.uniform(-1.0, 1.0, size=m)
    return pcol, pval


def ap_row(A, pcol, pval, i):
    """Row i of A P merged as ap_rows does it: products in (A slot, P slot) order, a new column takes the next slot."""
    c, v = [], []
    cols, vals = A[i]
    for k, a in zip(cols, vals):
        for sp in range(PW):
            J = pcol[k, sp]
            if J < 0:
                continue
            t = a * pval[k, sp]
            if J in c:
                v[c.index(J)] += t
            else:
                c.append(J)
                v.append(t)
    return c, v


def w_rows(A, dinv, pcol, pval):
    """(W rows as [(columns, values)], the A P rows, miss): slot q of W under column c[q] of the A P row,
    (P[i, c[q]] if present, else 0) - OMEGA dinv[i] v[q].  miss: some column of a row of P is not in its A P row -- the
    level must not be folded."""
    W, AP, miss = [], [], False
    for i in range(len(A)):
        c, v = ap_row(A, pcol, pval, i)
        AP.append((c, v))
        own = {int(pcol[i, sp]): pval[i, sp] for sp in range(PW) if pcol[i, sp] >= 0}
        if not set(own) <= set(c):
            miss = True
        W.append((list(c), [own.get(int(J), 0.0) - OMEGA * dinv[i] * t for J, t in zip(c, v)]))
    return W, AP, miss


def p_times(pcol, pval, e):
    out = np.zeros(pcol.shape[0])
    for sp in range(PW):
        ok = pcol[:, sp] >= 0
        out[ok] += pval[ok, sp] * e[pcol[ok, sp]]
    return out


def a_times(A, x):
    return np.array([float(np.dot(v, x[c])) for c, v in A])


def both_forms(A, dinv, pcol, pval, W, x, b, e):
    xp = x + p_times(pcol, pval, e)
    two = xp + OMEGA * dinv * (b - a_times(A, xp))
    r = b - a_times(A, x)
    fused = x + OMEGA * dinv * r + np.array([float(np.dot(v, e[np.asarray(c, dtype=np.int64)])) if c else 0.0 for c, v in W])
    return two, fused


def row_bound(A, dinv, pcol, pval, x, b, e):
    """gamma_n sum |terms| per row.  The terms of either form are x_i, b_i, the row's P entries times e, the row's
    a_ij x_j and its a_ij P_js e_s; each is a chain of at most four products (a, p, e, w dinv: four roundings) and goes
    through at most n additions, n = their number: (1 + u)^(n + 4) per term, for each of the two forms."""
    u = 2.0 ** -53
    pe = np.zeros(len(A))
    for sp in range(PW):
        ok = pcol[:, sp] >= 0
        pe[ok] += np.abs(pval[ok, sp] * e[pcol[ok, sp]])
    out = np.zeros(len(A))
    for i, (c, v) in enumerate(A):
        n = 2 + PW + len(c) * (1 + PW)
        s = abs(x[i]) + pe[i] + OMEGA * dinv[i] * (abs(b[i]) + float(np.dot(np.abs(v), np.abs(x[c]) + pe[c])))
        g = (n + 4) * u / (1.0 - (n + 4) * u)
        out[i] = 2.0 * g * s
    return out


def diagonal_inverse(A):
    d = np.zeros(len(A))
    for i, (c, v) in enumerate(A):
        hit = np.nonzero(c == i)[0]
        d[i] = 1.0 / v[hit[0]] if len(hit) else 1.0
    return d


CASES = {
    "grid12": lambda rng: (grid_matrix(12), 30),
    "random_nonsymmetric": lambda rng: (random_matrix(200, rng), 37),
}


@pytest.mark.parametrize("case", list(CASES))
def test_fused_form_equals_prolongation_then_sweep(case):
    rng = np.random.default_rng(5)
    A, nc = CASES[case](rng)
    n = len(A)
    dinv = diagonal_inverse(A)
    pcol, pval = prolongation(n, nc, rng)
    W, AP, miss = w_rows(A, dinv, pcol, pval)
    assert not miss  # (every row stores its diagonal)
    for (wc, _), (ac, _) in zip(W, AP):  # the pattern of W is that of A P, slot for slot
        assert wc == ac
        assert len(set(wc)) == len(wc)
    worst = 0.0
    for trial in range(3):
        x, b, e = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, nc)
        two, fused = both_forms(A, dinv, pcol, pval, W, x, b, e)
        bound = row_bound(A, dinv, pcol, pval, x, b, e)
        diff = np.abs(two - fused)
        worst = max(worst, float((diff / bound).max()))
        assert (diff <= bound).all(), (case, float((diff / bound).max()))
    print(case, "largest difference over its bound", worst)


def test_row_without_a_stored_diagonal_is_reported_not_folded():
    """Row 7 stores no diagonal and none of its neighbours' P rows names its own aggregate: the A P row lacks a column
    of P's row.  The setup must say so (ST_FOLDMISS) and leave the level unfolded -- dropping the entry would lose
    P[7, own] e from the result."""
    rng = np.random.default_rng(11)
    n, nc = 40, 9
    A = random_matrix(n, rng, drop_diagonal_of=(7,))
    own = [int(i % (nc - 1)) for i in range(n)]  # aggregate nc - 1 belongs to row 7 alone
    own[7] = nc - 1
    pcol, pval = prolongation(n, nc - 1, rng, own=own)
    pcol[7, :] = -1
    pcol[7, 0] = nc - 1
    pval[7, 0] = 0.75
    dinv = diagonal_inverse(A)
    W, AP, miss = w_rows(A, dinv, pcol, pval)
    assert nc - 1 not in AP[7][0]
    assert miss
    # what folding regardless would cost: the fused form without that entry is off by P[7, own] e
    x, b, e = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, nc)
    two, fused = both_forms(A, dinv, pcol, pval, W, x, b, e)
    assert abs((two - fused)[7] - 0.75 * e[nc - 1]) <= 1e-12
    # with the diagonal stored the same row folds
    A[7] = (np.append(A[7][0], 7), np.append(A[7][1], 3.0))
    dinv = diagonal_inverse(A)
    W, AP, miss = w_rows(A, dinv, pcol, pval)
    assert not miss and nc - 1 in AP[7][0]
    two, fused = both_forms(A, dinv, pcol, pval, W, x, b, e)
    assert (np.abs(two - fused) <= row_bound(A, dinv, pcol, pval, x, b, e)).all()
