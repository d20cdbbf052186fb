"""The identities behind the three-launch visit of the level directly above the dense tail (csrc/sagg_cycle.h:
k_visit_first / k_visit_second / k_visit_last; csrc/sagg.hip: p2_rows_wave, d2_scatter), restated in numpy / scipy, fp64.

With G = I - w D^-1 A, sweep(x) = G x + w D^-1 b, x0 = w D^-1 b, W = G P, R = P^T and T the tail's operator, the six
launches of a visit with two sweeps per side

    x1 = sweep(x0);  r = b - A x1;  rc = R r;  c = T rc;  xp = x1 + w D^-1 r + W c;  out = sweep(xp)

become, with P2 = G W,

    rc = P2^T b                      (r = (I - A w D^-1)^2 b, and R (I - A w D^-1)^2 = (G^2 P)^T needs A = A^T, R = P^T)
    out = sweep(sweep(x1)) + P2 c    (no symmetry needed)

The operators are the ones tests/hierarchy_reference.py builds from a level's exported arrays (reference_P: build_P's
rule); the level here is a random-valued grid written in the export's layout by hand, so no GPU is involved."""
import numpy as np
import scipy.sparse as sp

from tests import hierarchy_reference as ref

OMEGA = 0.85  # csrc/sagg.hip, NODAL_SA_OMEGA


def grid_level(N, rng, block=3, skew=0.0):
    """A level in the layout of Handle.debug_hierarchy(): the 5-point grid with random conductances (1 / uniform[1, 3]
    ohm), a resistor to ground on every boundary node, aggregates of block x block nodes.  skew > 0: every off-diagonal
    entry is scaled by its own factor in [1 - skew, 1 + skew] -- the same pattern, A != A^T."""
    n = N * N
    idx = np.arange(n).reshape(N, N)
    a = np.concatenate([idx[:-1].ravel(), idx[:, :-1].ravel()])
    b = np.concatenate([idx[1:].ravel(), idx[:, 1:].ravel()])
    g = 1.0 / rng.uniform(1.0, 3.0, size=len(a))
    off = sp.coo_matrix((np.concatenate([-g, -g]), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n)).tocsr()
    deg = -np.asarray(off.sum(axis=1)).ravel()
    edge = np.zeros((N, N))
    edge[0] += 0.5
    edge[-1] += 0.5
    edge[:, 0] += 0.5
    edge[:, -1] += 0.5
    if skew:
        off.data *= rng.uniform(1.0 - skew, 1.0 + skew, size=len(off.data))
    A = (off + sp.diags(deg + edge.ravel())).tocsr()
    A.sort_indices()
    alen = np.diff(A.indptr).astype(np.int32)
    maxlen, ld = int(alen.max()), (n + 63) // 64 * 64
    acol = np.zeros((maxlen, ld), dtype=np.int32)
    aval = np.zeros((maxlen, ld))
    for i in range(n):
        s, e = A.indptr[i], A.indptr[i + 1]
        acol[:e - s, i] = A.indices[s:e]
        aval[:e - s, i] = A.data[s:e]
    nb = (N + block - 1) // block
    agg = ((idx // N) // block * nb + (idx % N) // block).ravel().astype(np.int32)
    lv = {"n": n, "ld": ld, "maxlen": maxlen, "alen": alen, "agg": agg, "acol": acol.ravel(), "aval": aval.ravel(),
          "dinv": 1.0 / A.diagonal(), "omega_p": 0.85, "nc": nb * nb}
    return lv, A


def operators(lv, A):
    n, nc = lv["n"], lv["nc"]
    c, v, _, _, _ = ref.reference_P(lv)
    rows = np.broadcast_to(np.arange(n), c.shape)
    P = sp.csr_matrix((v[c >= 0], (rows[c >= 0], c[c >= 0])), shape=(n, nc))
    wd = sp.diags(OMEGA * lv["dinv"])
    G = sp.identity(n) - wd @ A
    W = (G @ P).tocsr()
    P2 = (G @ W).tocsr()
    # the tail as one fixed operator: here the exact inverse of the Galerkin matrix of the symmetric part
    As = 0.5 * (A + A.T)
    T = np.linalg.inv((P.T @ As @ P).toarray())
    return P, G, W, P2, T


def six_launches(A, dinv, P, W, T, b):
    w = OMEGA * dinv
    x0 = w * b
    x1 = x0 + w * (b - A @ x0)
    r = b - A @ x1
    rc = P.T @ r
    c = T @ rc
    xp = x1 + w * r + W @ c
    return xp + w * (b - A @ xp), rc


def three_launches(A, dinv, P2, T, b):
    w = OMEGA * dinv
    x0 = w * b
    x1, rc = x0 + w * (b - A @ x0), P2.T @ b   # launch 1: both parts read b (and x0) only
    x2, c = x1 + w * (b - A @ x1), T @ rc      # launch 2
    out = x2 + w * (b - A @ x2) + P2 @ c       # launch 3
    terms = np.abs(x2) + w * (np.abs(b) + abs(A) @ np.abs(x2)) + abs(P2) @ np.abs(c)
    return out, rc, terms


def test_three_launches_equal_the_six_on_a_symmetric_level():
    rng = np.random.default_rng(23)
    lv, A = grid_level(31, rng)  # (31 is no multiple of the aggregates' side: ragged aggregates at two edges)
    assert abs(A - A.T).max() == 0.0
    P, G, W, P2, T = operators(lv, A)
    assert np.diff(P.indptr).max() <= ref.PW and np.diff(P2.indptr).max() <= 64  # (the device's caps)
    worst = 0.0
    for trial in range(3):
        b = rng.uniform(-1.0, 1.0, lv["n"])  # both signs
        out6, rc6 = six_launches(A, lv["dinv"], P, W, T, b)
        out3, rc3, terms = three_launches(A, lv["dinv"], P2, T, b)
        assert np.abs(rc3 - rc6).max() <= 1e-12 * (abs(P2).T @ np.abs(b)).max()
        d = np.abs(out3 - out6) / terms
        worst = max(worst, float(d.max()))
        assert (d <= 1e-12).all(), float(d.max())
    print("largest |out3 - out6| over the row's sum of absolute terms", worst)


def test_a_non_symmetric_matrix_breaks_the_restriction_identity():
    """rc = P2^T b uses (I - A w D^-1)^T-free algebra only for A = A^T: with off-diagonals skewed by up to 20 % the two
    restricted residuals differ in the first digits -- the reason the general route keeps its six launches.  The second
    identity, out = sweep(sweep(x1)) + P2 c for one and the same c, holds without symmetry."""
    rng = np.random.default_rng(29)
    lv, A = grid_level(31, rng, skew=0.2)
    assert abs(A - A.T).max() > 0.01
    P, G, W, P2, T = operators(lv, A)
    b = rng.uniform(-1.0, 1.0, lv["n"])
    out6, rc6 = six_launches(A, lv["dinv"], P, W, T, b)
    out3, rc3, terms = three_launches(A, lv["dinv"], P2, T, b)
    rel = np.abs(rc3 - rc6).max() / np.abs(rc6).max()
    print("restricted residuals differ by", rel, "of the largest entry")
    assert rel > 1e-3
    assert (np.abs(out3 - out6) / terms).max() > 1e-6
    # the same coarse correction in both forms: the tail of the visit alone
    w = OMEGA * lv["dinv"]
    x0 = w * b
    x1 = x0 + w * (b - A @ x0)
    c = T @ rc6
    xp = x1 + w * (b - A @ x1) + W @ c
    x2 = x1 + w * (b - A @ x1)
    six = xp + w * (b - A @ xp)
    three = x2 + w * (b - A @ x2) + P2 @ c
    den = np.abs(x2) + w * (np.abs(b) + abs(A) @ np.abs(x2)) + abs(P2) @ np.abs(c)
    assert (np.abs(three - six) / den).max() <= 1e-12
