"""Inputs and host references for the dense path's pieces (tests/test_dense_reference.py pins them down on the CPU,
tests/test_gpu_dense_blocks.py and tests/dense_variant_child.py hold the kernels to them).

THE EXACT FAMILIES.  L is unit lower triangular with integer entries: the first sub-diagonal holds random values in
{-1, 0, 1} and every column c = 0 (mod s) is dense with +-1 below the diagonal; U is built the same way (another seed),
transposed.  A = L U is the non-symmetric family, A = L L^T the symmetric one (SPD, and symmetric bit for bit: integer
sums).  Every leading principal minor of A is 1, so every pivot, every 2 x 2 pivot determinant and every 4 x 4 pivot block
that an elimination WITHOUT pivoting divides by is exactly 1, every intermediate quantity -- Gauss-Jordan steps, the
Schur formula's T1, T2 and S, W = Q A12, the Schur complements -- is a small integer in any summation order, and all of it
is exact in fp64.  The inverse is an integer matrix, and with B = A X for an integer X the solution is X bit for bit.
With s below the narrowest block width every block's update L21 U12 is non-zero in every 128-tile: a tile skipped or
applied twice changes an integer.  The condition numbers reach 1e10: nothing of one ulp stays hidden.

THE FLOAT FAMILIES.  spd_dominant: symmetric, Gaussian off the diagonal (no band), the diagonal twice the row's absolute
off-diagonal sum -- the class the block elimination is meant for.  gaussian: general matrices, which need pivoting.
complex_embedding: [[G, -B], [B, G]] of G + jB, what the AC analyses hand to the pivoted LU.

THE MEASURES, evaluated in numpy.longdouble: e(Q) = max(|Q A - I|, |A Q - I|) for an inverse and the normwise backward
error eta(x) = |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf) for a solution.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
LD = np.longdouble


# ---- the exact families ----

def exact_lower(n, s, seed):
    rng = np.random.default_rng(seed)
    L = np.eye(n)
    if n > 1:
        L[np.arange(1, n), np.arange(n - 1)] = rng.integers(-1, 2, n - 1)
    for c in range(0, n, s):
        L[c + 1:, c] = rng.choice([-1.0, 1.0], n - c - 1)
    return L


def exact_matrix(n, s, symmetric, seed=0):
    """A = L L^T (symmetric) or L U; integer-valued float64."""
    L = exact_lower(n, s, 2 * seed + 11)
    U = L.T if symmetric else exact_lower(n, s, 2 * seed + 12).T
    return L @ U


def inverse_spacing(w):
    """Spacing of the dense columns for a w x w block: several dense columns at every size."""
    return 100 if w > 200 else max(3, w // 5)


SOLVE_SPACING = 90  # below the narrowest block width (128)


def integer_rhs(n, nrhs, seed):
    return np.random.default_rng(seed).integers(-3, 4, (n, nrhs)).astype(np.float64)


# ---- the float families ----

def spd_dominant(n, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    M = np.triu(M, 1)
    M = M + M.T
    M[np.arange(n), np.arange(n)] = 2.0 * np.abs(M).sum(axis=1) + (1.0 if n == 1 else 0.0)
    return M


def gaussian(n, seed):
    return np.random.default_rng(seed).standard_normal((n, n))


def complex_embedding(n, seed):
    """[[G, -B], [B, G]] of order n (even): G a conductance-like matrix (symmetric, weakly dominant), B symmetric."""
    assert n % 2 == 0
    m = n // 2
    rng = np.random.default_rng(seed)
    G = -np.abs(np.triu(rng.standard_normal((m, m)), 1))
    G = G + G.T
    G[np.arange(m), np.arange(m)] = -G.sum(axis=1) + rng.uniform(0.0, 0.1, m)
    Bm = np.triu(rng.standard_normal((m, m)))
    Bm = (Bm + Bm.T) * (m ** 0.5)
    return np.block([[G, -Bm], [Bm, G]])


def conductance_pair_block(w, p):
    """Identity, except one isolated pair [[1, -1], [-1, 1]] at rows p, p + 1: a scalar elimination without pivoting
    meets an exact zero in column p + 1."""
    A = np.eye(w)
    A[p, p + 1] = A[p + 1, p] = -1.0
    return A


# ---- host emulations (fp64, the kernels' order of operations where it matters: nowhere, on the exact families) ----

def gauss_jordan_nopivot(A):
    """In-place Gauss-Jordan inverse without pivoting, one scalar pivot per step.  Returns (Q, stop, biggest): stop = 0
    or the 1-based column whose pivot is zero or NaN (Q is None then); biggest = the largest |entry| seen on the way."""
    a = np.array(A, dtype=np.float64)
    n = a.shape[0]
    big = float(np.abs(a).max())
    for k in range(n):
        p = a[k, k]
        if not (p != 0.0 and p == p):
            return None, k + 1, big
        ip = 1.0 / p
        row = a[k, :] * ip
        row[k] = ip
        col = a[:, k].copy()
        col[k] = 0.0
        a[:, k] = 0.0
        a -= np.outer(col, row)
        a[k, :] = row
        big = max(big, float(np.abs(a).max()))
    return a, 0, big


def schur_inverse(A):
    """The inverse the way invert_diag (csrc/block_elim.hip) forms it: Gauss-Jordan up to 128, above the 2 x 2 Schur
    formula with the leading m1 = 128 (w <= 256) or 256 columns.  Returns (Q, stop, biggest)."""
    w = A.shape[0]
    if w <= 128:
        return gauss_jordan_nopivot(A)
    m1 = 128 if w <= 256 else 256
    A11, B, C, D = A[:m1, :m1], A[:m1, m1:], A[m1:, :m1], A[m1:, m1:]
    Q11, stop, big = schur_inverse(A11)
    if stop:
        return None, stop, big
    T1, T2 = Q11 @ B, C @ Q11
    S = D - C @ T1
    Q22, stop, big2 = schur_inverse(S)
    big = max(big, big2, *(float(np.abs(x).max()) for x in (T1, T2, S)))
    if stop:
        return None, m1 + stop, big
    Q12, Q21 = -(T1 @ Q22), -(Q22 @ T2)
    Q11 = Q11 - Q12 @ T2
    Q = np.block([[Q11, Q12], [Q21, Q22]])
    return Q, 0, max(big, float(np.abs(Q).max()))


def block_boundaries(n, width=None, switch=4608, switch2=0):
    """The block boundaries of dense_block_elimination: NODAL_BI_WIDTH forces one width, otherwise 512 while more than
    NODAL_BI_SWITCH + 512 rows are left, 128 once at most NODAL_BI_SWITCH2 are left, 256 in between."""
    bnd, j = [0], 0
    while j < n:
        left = n - j
        wb = width if width else (512 if left > switch + 512 else (128 if left <= switch2 else 256))
        j = min(j + wb, n)
        bnd.append(j)
    return bnd


def block_eliminate(A, B, bnd):
    """Block elimination with explicitly inverted diagonal blocks on [A | B], as factor_blockinv does it (the full form;
    the symmetric one computes the same numbers from the transposed panel).  Returns (X, biggest, empty_tiles): the
    number of 128 x 128 tiles (aligned with the trailing matrix) of any block update A21 W that are entirely zero."""
    n = A.shape[0]
    M = np.hstack([A, B]).astype(np.float64)
    big, empty = float(np.abs(M).max()), 0
    for k in range(len(bnd) - 1):
        J0, J1 = bnd[k], bnd[k + 1]
        Q, stop, b = schur_inverse(M[J0:J1, J0:J1])
        assert stop == 0, (k, stop)
        W = Q @ M[J0:J1, J1:]
        M[J0:J1, J1:] = W
        big = max(big, b, float(np.abs(W).max()) if W.size else 0.0)
        if J1 < n:
            upd = M[J1:, J0:J1] @ W
            for r in range(0, n - J1, 128):
                for c in range(0, n - J1, 128):
                    empty += not upd[r:r + 128, c:c + 128].any()
            M[J1:, J1:] -= upd
            big = max(big, float(np.abs(upd).max()), float(np.abs(M[J1:, J1:]).max()))
    X = M[:, n:].copy()
    for k in range(len(bnd) - 2, -1, -1):
        J0, J1 = bnd[k], bnd[k + 1]
        X[J0:J1] -= M[J0:J1, J1:n] @ X[J1:]
        big = max(big, float(np.abs(X).max()))
    return X, big, empty


# ---- error measures, in longdouble ----

def _slices(M, axis, bits, count):
    """M = slices[0] + ... + slices[count - 1] + a rest below 2^-(bits * count) of the largest |entry| along `axis`;
    slice i of a row (column) is an integer of at most bits + 1 bits times one power of two (exact fp64 splitting)."""
    _, ex = np.frexp(np.abs(M).max(axis=axis, keepdims=True))  # max < 2^ex
    rest, out = M.astype(np.float64), []
    for i in range(count):
        sigma = np.ldexp(1.5, ex - bits * (i + 1) + 52)
        s = (rest + sigma) - sigma
        out.append(s)
        rest = rest - s
    return out


def matmul_ld(A, B):
    """A @ B in numpy.longdouble for fp64 operands, without numpy's (slow, BLAS-less) longdouble product: both operands
    are cut into four slices of so few bits that every slice product is EXACT in fp64 (K (2^bits + 1)^2 < 2^53), and
    the slice products are summed in longdouble, smallest first.  Dropped: terms below 2^-(4 bits) ~ 1e-24 of
    |row max| |column max|.  tests/test_dense_reference.py holds it to the plain longdouble product."""
    K = A.shape[1]
    bits = int((51 - int(np.ceil(np.log2(max(K, 2))))) // 2)
    As, Bs = _slices(A, 1, bits, 4), _slices(B, 0, bits, 4)
    out = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for total in range(3, -1, -1):
        for i in range(total + 1):
            out += (As[i] @ Bs[total - i]).astype(LD)
    return out


def inverse_error(A, Q):
    """e(Q) = max(|Q A - I|, |A Q - I|) over all entries."""
    I = np.eye(A.shape[0], dtype=LD)
    return float(max(np.abs(matmul_ld(Q, A) - I).max(), np.abs(matmul_ld(A, Q) - I).max()))


def backward_error(A, X, B):
    """eta per column of X: |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf)."""
    X, B = X.reshape(A.shape[0], -1), B.reshape(A.shape[0], -1)
    Al = A.astype(LD)
    R = np.abs(matmul_ld(A, X) - B.astype(LD)).max(axis=0)
    norm_a = np.abs(Al).sum(axis=1).max()
    den = norm_a * np.abs(X).max(axis=0).astype(LD) + np.abs(B).max(axis=0).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):  # (x = b = 0 solves exactly: eta 0; NaN in x stays NaN)
        return np.where((den == 0) & (R == 0), LD(0), R / den).astype(np.float64)


def lapack_pivots(A):
    """(rows, runner_up): the row order dgetrf applies (rows[i] = original row at position i) and, per column, the
    largest |candidate| / |pivot| among the rows NOT chosen (= max |L[i, k]| below the diagonal)."""
    import scipy.linalg
    lu, piv = scipy.linalg.lu_factor(A, check_finite=False)
    rows = np.arange(A.shape[0])
    for c, p in enumerate(piv):
        if p != c:
            rows[c], rows[p] = rows[p], rows[c]
    runner = np.abs(np.tril(lu, -1)).max(axis=0) if A.shape[0] > 1 else np.zeros(1)
    return rows, runner


# ---- the cases both test modules walk ----

INVERSE_SIZES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 200, 255, 256, 257, 300, 384, 511, 512)
ELIM_SIZES = (257, 300, 384, 385, 512, 513, 700, 1100, 1400)
ELIM_NRHS = (1, 2, 7, 17)
# name -> (NODAL_BI_WIDTH, NODAL_BI_SWITCH, NODAL_BI_SWITCH2) as the environment holds them (None: unset)
WIDTH_PATTERNS = {"default": (None, None, None), "w128": ("128", None, None), "w512": ("512", None, None),
                  "mixed": (None, "600", "300")}
GEPP_SIZES = (1, 2, 31, 32, 33, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1280)
TOURNAMENT_SIZES = (1281, 1536)
PIVOT_NRHS = (1, 17, 512)


def pattern_boundaries(n, pattern):
    width, sw, sw2 = WIDTH_PATTERNS[pattern]
    return block_boundaries(n, int(width) if width else None, int(sw) if sw else 4608, int(sw2) if sw2 else 0)


def pivot_rhs(A, nrhs):
    """Right-hand sides for the pivoted LU: Gaussian (at orders 1 and 2 rounded to sixteenths, see pivot_inputs)."""
    n = A.shape[0]
    B = np.random.default_rng(3000 + 7 * n + nrhs).standard_normal((n, nrhs))
    return np.round(B * 16.0) / 16.0 if n <= 2 else B


def pivot_inputs(n):
    """name -> matrix for the pivoted LU at order n: a Gaussian matrix, and (an embedding has even order) the real
    embedding of a complex system.  At orders 1 and 2 one rounding is already more than the n eps / 16 LAPACK has to
    stay below: the inputs there are dyadic matrices (order 2: with an interchange) that any elimination solves
    exactly, and there is no embedding (its second pivot (g^2 + b^2) / b is a power of two only on a tie)."""
    if n == 1:
        return {"dyadic": np.array([[-2.0]])}
    if n == 2:
        return {"dyadic": np.array([[1.0, 1.0], [2.0, 4.0]])}
    out = {"gaussian": gaussian(n, 1000 + n)}
    if n % 2 == 0:
        out["embedding"] = complex_embedding(n, 2000 + n)
    return out
