"""The identity behind k_residual_restrict (csrc/sagg_cycle.h), in fp64 on the CPU: on a level with one pre-smoothing
sweep from a zero guess, x0 = w D^-1 b, and with G = I - w D^-1 A, W = G P,

    rc = P^T (b - A x0) = P^T (I - w A D^-1) b = (G P)^T b = W^T b        when A = A^T (and R = P^T),

so the restricted residual needs the right-hand side only.  The two guards of the setup (decide_folds, csrc/sagg.hip)
are shown to matter: on a non-symmetric A the two forms differ at the size of rc itself, and with a second sweep
(x1 = x0 + w D^-1 (b - A x0)) they do as well."""
import numpy as np
import scipy.sparse as sp

OMEGA = 0.85
N, NC = 300, 40


def laplacian(rng, n=N, extra=3):
    """A random connected graph Laplacian (a path plus `extra` random links per node, conductances in (0.5, 2)) with
    ground links on a tenth of the nodes: symmetric positive definite."""
    a = np.concatenate([np.arange(n - 1), rng.integers(0, n, size=extra * n)])
    b = np.concatenate([np.arange(1, n), rng.integers(0, n, size=extra * n)])
    keep = a != b
    a, b = a[keep], b[keep]
    g = rng.uniform(0.5, 2.0, size=len(a))
    A = sp.coo_matrix((np.concatenate([-g, -g]), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n)).tocsr()
    ground = np.where(rng.random(n) < 0.1, rng.uniform(0.5, 2.0, size=n), 0.0)
    ground[0] = 1.0
    return (A + sp.diags(-np.asarray(A.sum(axis=1)).ravel() + ground)).tocsr()


def prolongator(rng, n=N, nc=NC, per_row=4):
    """Aggregation-shaped: every fine row has its own aggregate and up to three others, weights summing to one."""
    own = np.arange(n) * nc // n
    rows, cols, vals = [], [], []
    for i in range(n):
        c = np.unique(np.concatenate([[own[i]], rng.integers(0, nc, size=per_row - 1)]))
        w = rng.uniform(0.1, 1.0, size=len(c))
        rows += [i] * len(c)
        cols += list(c)
        vals += list(w / w.sum())
    return sp.csr_matrix((vals, (rows, cols)), shape=(n, nc))


def both_forms(A, P, b, sweeps=1):
    dinv = 1.0 / A.diagonal()
    x = OMEGA * dinv * b
    for _ in range(sweeps - 1):
        x = x + OMEGA * dinv * (b - A @ x)
    W = P - sp.diags(OMEGA * dinv) @ (A @ P)
    return P.T @ (b - A @ x), W.T @ b, abs(P).T @ (np.abs(b) + abs(A) @ np.abs(x)) + abs(W).T @ np.abs(b)


def test_restricted_residual_from_b_on_the_symmetric_route():
    rng = np.random.default_rng(7)
    A, P = laplacian(rng), prolongator(rng)
    assert abs(A - A.T).max() == 0.0 and np.linalg.eigvalsh(A.toarray()).min() > 0.0
    worst = 0.0
    for _ in range(5):
        b = rng.uniform(-1.0, 1.0, size=N)
        two, one, den = both_forms(A, P, b)
        worst = max(worst, float((np.abs(two - one) / den).max()))
    # (each form is a sum of fewer than 40 x 12 fp64 products per coarse row: well below 1e3 roundings of 2^-53)
    print("W^T b against P^T (b - A w D^-1 b): largest difference over the sum of absolute terms", worst)
    assert worst <= 1e3 * 2.0 ** -53


def test_a_non_symmetric_matrix_breaks_it():
    """Transconductance stamps make A != A^T (the general route): P^T (I - w A D^-1) b is then ((I - w D^-1 A^T) P)^T b,
    not W^T b.  Measured here: the two differ by 0.39 of the largest entry of rc with a tenth of the off-diagonal
    entries scaled on one side only."""
    rng = np.random.default_rng(8)
    A, P = laplacian(rng).tolil(), prolongator(rng)
    rows, cols = A.nonzero()
    for i, j in zip(rows, cols):
        if i < j and rng.random() < 0.1:
            A[i, j] *= 3.0
    A = A.tocsr()
    b = rng.uniform(-1.0, 1.0, size=N)
    two, one, _ = both_forms(A, P, b)
    factor = float(np.abs(two - one).max() / np.abs(two).max())
    print("non-symmetric A: difference over the largest entry of rc", factor)
    assert factor > 1e-2


def test_a_second_sweep_breaks_it():
    """With two pre-smoothing sweeps the residual is r = (I - w A D^-1)^2 b and rc = (G^2 P)^T b (the three-launch
    visit's P2), not W^T b.  Measured here: the forms differ by 1.3 times the largest entry of rc."""
    rng = np.random.default_rng(9)
    A, P = laplacian(rng), prolongator(rng)
    b = rng.uniform(-1.0, 1.0, size=N)
    two, one, _ = both_forms(A, P, b, sweeps=2)
    factor = float(np.abs(two - one).max() / np.abs(two).max())
    print("two sweeps: difference over the largest entry of rc", factor)
    assert factor > 1e-2
