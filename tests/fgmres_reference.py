"""The general route's flexible GMRES and block preconditioner (nodal_amd/csrc/sparse_general.hip) stated on the host:
node-block extraction, the Schur diagonal, branch_solve, ONE Arnoldi step from given inputs, the back-substitution and
the combination x = Z y.  Values are computed in numpy longdouble (64-bit mantissa on x86: eleven more bits than the
device has) unless a float type is asked for.

Every function returns its value together with a running FIRST-ORDER forward-error bound, per entry, of the fp64
operations the device performs between the same inputs and that value (u = 2^-53):

  a sum or dot product of k terms, in any order, fused or not     (k + 2) u sum|a_i||b_i|
  (the pattern tests/test_gpu_cycle.py uses for the dots of the cycle; an fma chain w - sum h_i v_i of k terms is a sum
  of k + 1)
  one multiplication, division, square root                       u |result|;  hypot 2 u |result|
  an input that itself carries an error d                         |coefficient| d, added

and nothing else: no constant is fitted to what a device returned.  A quotient by a small number appears as what it is
(d_w / hnext for v_{j+1} = w / hnext).  The tests allow 2 x the bound for the second-order terms.

The inputs of a step are taken as exact (the tests pass the DEVICE's own z_j, basis, rotations and g), so nothing
accumulates from one column to the next.

The matrix is a scipy CSR matrix in float64 with sorted column indices (the arrays the device holds)."""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53
RESTART = 40
MAXV = RESTART + 1


def edge_rows(N=24):
    """A grid(N) plus every edge of the preconditioner setup (tests/test_gpu_fgmres.py group A).  Nodes are numbered in
    order of first appearance, so the place of a row decides whether an inserted diagonal lands before, between or
    after the row's other entries:

      mlo, mhi   touched only by two voltage sources in series: the node block's row is EMPTY, the unit diagonal goes at
                 the row's end; mlo has a lower index than both neighbours, mhi a higher one
      clo, cmid, chi   touched only by a voltage source and the output of a CCCS, early, in the middle and late in the
                 numbering: empty rows as well (every dependent source stamps its node rows through a branch column)
      zc         resistors of +1 and -1 ohm: the diagonal cancels to exactly zero.  The device's symbolic assembly
                 stores the zero (replaced by 1); a host assembly that drops it leaves a row of two off-diagonals below the
                 row's index and no diagonal: the unit diagonal is inserted at the END of a row that is not empty
      nd         a negative diagonal (a negative resistor; replaced by 1)
      hv / f1    a CCVS and a CCCS at ordinary nodes
      va, vb     a VCVS va - vb sensing va - g with gain 2, each node on one 1-ohm resistor: S~ = 0, stored as 1."""
    from nodal_amd import generators as gen
    grid = list(gen.grid_rows(N))
    source = grid.pop()
    lab = lambda r, c: gen._label(r * N + c, N * N - 1)  # noqa: E731
    head = [["elo1", "E", "1", "mlo", lab(0, 0)], ["elo2", "E", "2", "mlo", "qlo"], ["rqlo", "R", "1", "qlo", lab(0, 1)],
            ["eclo", "E", "1.5", "clo", "g"]]
    mid_at = (N // 2) * (2 * N - 1)  # (after half of the grid's rows: the nodes of its lower half have no index yet)
    mid = [["ecmid", "E", "-1", "cmid", "g"]]
    tail = [["rqhi", "R", "2", "qhi", lab(3, 3)], ["ehi1", "E", "1", "mhi", lab(2, 5)], ["ehi2", "E", "0.5", "mhi", "qhi"],
            ["echi", "E", "2.5", "chi", "g"],
            ["fclo", "CCCS", "0.3", "clo", "g", lab(4, 4), lab(4, 5), "rh4_4"],
            ["rx", "R", "1", lab(1, 1), lab(N - 2, 2)], ["fcmid", "CCCS", "0.2", "cmid", "g", lab(1, 1), lab(N - 2, 2), "rx"],
            ["fchi", "CCCS", "0.4", "chi", "g", lab(5, 5), lab(5, 6), "rh5_5"],
            ["rz1", "R", "1", "zc", lab(6, 2)], ["rz2", "R", "-1", "zc", lab(7, 3)],
            ["rn1", "R", "-2", "nd", lab(8, 8)], ["rn2", "R", "4", "nd", lab(9, 9)],
            ["hh", "CCVS", "0.3", "hv", "g", lab(10, 2), lab(10, 3), "rh10_2"], ["rhv", "R", "1", "hv", lab(11, 4)],
            ["f1", "CCCS", "0.2", lab(12, 12), "g", lab(3, 7), lab(3, 8), "rh3_7"],
            ["rva", "R", "1", "va", lab(14, 3)], ["rvb", "R", "1", "vb", lab(15, 9)],
            ["dv", "VCVS", "2", "va", "vb", "va", "g"]]
    return head + grid[:mid_at] + mid + grid[mid_at:] + tail + [source]


# The device sums a dot product as strided per-thread partials, a wavefront fold by halves and the workgroups' partials in
# fixed order; numpy sums pairwise.  Both are within the same worst-case bound; this is what the tests allow between what
# the two leave on a vector whose projection cancels every digit (measured on MI355X: the device at 0.19 - 0.73 of the
# float64 reference step or of u, whichever is larger; tests/test_gpu_fgmres.py C4).
SUMMATION_FACTOR = 4.0


# ---- node block, Schur diagonal, branch_solve ---------------------------------------------------------------------

def node_block(indptr, indices, data, K):
    """gn_count / gn_fill: the leading K x K block of the CSR matrix, row by row, with a unit diagonal INSERTED in its
    sorted place where a row has none (at the row's end when every kept column is smaller, or the row is empty) and a
    stored diagonal that is not > 0 (zero, negative, NaN) REPLACED by 1.  Returns a dict of gn_indptr, gn_indices,
    gn_rowidx, gn_data, gn_diag (position of each row's diagonal).  Copies and constants: exact."""
    o_indptr = np.zeros(K + 1, dtype=np.int32)
    cols, rows, vals, diag = [], [], [], np.zeros(K, dtype=np.int32)
    for i in range(K):
        placed = False
        for e in range(indptr[i], indptr[i + 1]):
            j = int(indices[e])
            if j >= K:
                break
            if not placed and j > i:
                diag[i] = len(cols)
                cols.append(i); rows.append(i); vals.append(1.0)
                placed = True
            v = float(data[e])
            if j == i:
                placed = True
                diag[i] = len(cols)
                if not v > 0.0:
                    v = 1.0
            cols.append(j); rows.append(i); vals.append(v)
        if not placed:
            diag[i] = len(cols)
            cols.append(i); rows.append(i); vals.append(1.0)
        o_indptr[i + 1] = len(cols)
    return {"gn_indptr": o_indptr, "gn_indices": np.asarray(cols, dtype=np.int32),
            "gn_rowidx": np.asarray(rows, dtype=np.int32), "gn_data": np.asarray(vals, dtype=np.float64), "gn_diag": diag}


def schur_inverse(A, K, gn):
    """schur_diag: S~_m = D_mm - sum_j Cr_mj Bc_jm / Gn_jj over the stored entries j < K of branch row m, Bc_jm the entry
    (j, m) of A (0 when not stored), Gn_jj the node block's diagonal AS THE PRECONDITIONER HOLDS IT; stored as 1 / S~_m,
    and as 1 where S~_m is exactly zero.  Returns (1 / S~ [n - K], bound [n - K], degenerate [n - K] bool)."""
    n = A.shape[0]
    gdiag = gn["gn_data"][gn["gn_diag"]].astype(LD)
    sinv, bound, degenerate = np.ones(n - K, dtype=LD), np.zeros(n - K, dtype=LD), np.zeros(n - K, dtype=bool)
    Acsc = A.tocsc()
    for m in range(K, n):
        s, mag, local, terms = LD(0), LD(0), LD(0), 0
        for e in range(A.indptr[m], A.indptr[m + 1]):
            j = int(A.indices[e])
            if j == m:
                t = LD(A.data[e])
            elif j >= K:
                continue
            else:
                t = -LD(A.data[e]) * LD(Acsc[j, m]) / gdiag[j]
                local += 2 * U * abs(t)  # (the product and the quotient, each rounded once)
            s += t
            mag += abs(t)
            terms += 1
        ds = (terms + 2) * U * mag + local
        if s == 0:
            degenerate[m - K] = True
            sinv[m - K], bound[m - K] = LD(1), LD(0)
        else:
            sinv[m - K] = 1 / s
            bound[m - K] = ds / (s * s) + U * abs(1 / s)
    return sinv, bound, degenerate


def branch_solve(A, K, sinv, v, z_e):
    """z_i = S~^-1 (v_i - Cr z_e): per branch row m an fma chain over its stored entries j < K, then one product.
    sinv, v (n), z_e (K) are the inputs.  Returns (z_i [n - K], bound)."""
    n = A.shape[0]
    Cr = A[K:, :K]
    acc = np.asarray(v[K:], dtype=LD) - _matvec(Cr, z_e)
    mag = np.abs(np.asarray(v[K:], dtype=LD)) + _matvec(abs(Cr), np.abs(np.asarray(z_e, dtype=LD)))
    terms = np.diff(Cr.indptr)
    z = acc * np.asarray(sinv, dtype=LD)
    bound = np.abs(np.asarray(sinv, dtype=LD)) * (terms + 2) * U * mag + U * np.abs(z)
    assert z.shape == (n - K,)
    return z, bound


def _matvec(A, x):
    """A x in longdouble for a float64 CSR matrix (scipy has no longdouble kernels: by entries)."""
    A = sp.csr_matrix(A)
    x = np.asarray(x, dtype=LD)
    prod = np.append(A.data.astype(LD) * x[A.indices], LD(0))  # (the spare zero: a start index for trailing empty rows)
    out = np.add.reduceat(prod, A.indptr[:-1].astype(np.int64))
    out[np.diff(A.indptr) == 0] = 0  # (reduceat gives an empty segment the entry at its start)
    return out


def spmv(A, z):
    """w = A z with the bound (k_i + 2) u sum_j |a_ij||z_j| of row i's k_i entries (CSR or ELL, any lane order)."""
    w = _matvec(A, z)
    bound = (np.diff(A.indptr) + 2) * U * _matvec(abs(A), np.abs(np.asarray(z, dtype=LD)))
    return w, bound


# ---- one Arnoldi step ------------------------------------------------------------------------------------------------

def arnoldi_step(A, z, V, s0, cs, sn, gj, passes=2, dtype=LD):
    """Column j = len(cs) of the cycle from its inputs: z = z_j (n), V = the basis v_0 .. v_j ([j + 1, n]; only rows s0 ..
    j are read), cs / sn the j earlier rotations, gj = g[j].

      w = A z;  h1 = V_w^T w;  w -= V_w h1;  (passes == 2:)  h2 = V_w^T w;  w -= V_w h2;  h = h1 + h2
      hnext = |w|;  v_next = w (1 / hnext)
      col = (0 .. 0, h_s0 .. h_j, hnext) through the earlier rotations, then the new one:
      d = hypot(col_j, col_j+1), c = col_j / d, s = col_j+1 / d;  g_j+1 = -s g_j, g_j = c g_j, est = |s g_j|

    dtype float64 runs the same statements in plain numpy float64 (values only meaningful; the bounds still describe the
    fp64 device).  Returns a dict: w0 (A z), h (raw column, length j + 1, zeros below s0), hnext, inv_h, v_next, col (the
    rotated column, length j + 2: rows < j rotated, row j = d, row j + 1 = 0), c, s, g_j, g_next, est, and for each the
    bound under the same name with `_b` appended."""
    j = len(cs)
    n = A.shape[0]
    assert V.shape == (j + 1, n) and len(sn) == j and 0 <= s0 <= j
    nv = j + 1 - s0
    if dtype is LD:
        Vw = np.asarray(V[s0:], dtype=LD)
        w, w_b = spmv(A, z)
    else:
        Vw = np.asarray(V[s0:], dtype=dtype)
        w = (A @ np.asarray(z, dtype=dtype)).astype(dtype)
        w_b = (np.diff(A.indptr) + 2) * U * (abs(A) @ np.abs(np.asarray(z, dtype=np.float64)))
    aV = np.abs(Vw)
    out = {"w0": w.copy(), "w0_b": np.asarray(w_b, dtype=LD).copy()}
    w_b = np.asarray(w_b, dtype=LD)
    h = np.zeros(nv, dtype=dtype)
    h_b = np.zeros(nv, dtype=LD)
    for _ in range(passes):
        hp = Vw @ w
        hp_b = (n + 2) * U * (aV @ np.abs(w)) + aV @ w_b
        # w -= sum_i hp_i v_i: an fma chain of nv terms on top of w
        mag = np.abs(w) + np.abs(hp) @ aV
        w_b = w_b + hp_b @ aV + (nv + 2) * U * mag
        w = w - hp @ Vw
        h = h + hp
        h_b = h_b + hp_b
    if passes == 2:
        h_b = h_b + U * np.abs(h)
    ss = w @ w
    ss_b = (n + 2) * U * ss + 2 * (np.abs(w) @ w_b)
    hnext = np.sqrt(ss)
    hnext_b = ss_b / (2 * hnext) + U * hnext
    inv_h = 1 / hnext
    inv_h_b = hnext_b / (hnext * hnext) + U * inv_h
    v_next = w * inv_h
    v_next_b = w_b * inv_h + np.abs(w) * inv_h_b + U * np.abs(v_next)
    raw = np.zeros(j + 1, dtype=dtype)
    raw[s0:] = h
    raw_b = np.zeros(j + 1, dtype=LD)
    raw_b[s0:] = h_b
    out.update(h=raw, h_b=raw_b, hnext=hnext, hnext_b=hnext_b, inv_h=inv_h, inv_h_b=inv_h_b, v_next=v_next,
               v_next_b=v_next_b, w=w, w_b=w_b)
    out.update(rotate_column(raw, raw_b, hnext, hnext_b, cs, sn, gj, dtype))
    return out


def rotate_column(raw, raw_b, hnext, hnext_b, cs, sn, gj, dtype=LD):
    """gs_finish's thread 0 after the sums: the j earlier rotations (cs, sn: inputs) on (raw, hnext), the new rotation,
    g and the estimate."""
    j = len(cs)
    col = np.concatenate([np.asarray(raw, dtype=dtype), [hnext]]).astype(dtype)
    col_b = np.concatenate([np.asarray(raw_b, dtype=LD), [hnext_b]]).astype(LD)
    for i in range(j):
        c, s = dtype(cs[i]), dtype(sn[i])
        a, b = col[i], col[i + 1]
        da, db = col_b[i], col_b[i + 1]
        col[i] = c * a + s * b
        col[i + 1] = -s * a + c * b
        mag = abs(c * a) + abs(s * b)
        mag2 = abs(s * a) + abs(c * b)
        col_b[i] = abs(c) * da + abs(s) * db + 3 * U * mag
        col_b[i + 1] = abs(s) * da + abs(c) * db + 3 * U * mag2
    a, b = col[j], col[j + 1]
    da, db = col_b[j], col_b[j + 1]
    d = np.hypot(a, b)
    d_b = (abs(a) * da + abs(b) * db) / d + 2 * U * d
    c, s = a / d, b / d
    c_b = da / d + abs(a) * d_b / (d * d) + U * abs(c)
    s_b = db / d + abs(b) * d_b / (d * d) + U * abs(s)
    gj = dtype(gj)
    g_next, g_j = -s * gj, c * gj
    col[j], col[j + 1] = d, 0
    col_b[j], col_b[j + 1] = d_b, 0
    return {"col": col, "col_b": col_b, "c": c, "c_b": c_b, "s": s, "s_b": s_b,
            "g_j": g_j, "g_j_b": abs(gj) * c_b + U * abs(g_j), "g_next": g_next, "g_next_b": abs(gj) * s_b + U * abs(g_next),
            "est": abs(g_next), "est_b": abs(gj) * s_b + U * abs(g_next)}


# ---- the end of a cycle --------------------------------------------------------------------------------------------

def back_substitute(R, g, count):
    """gst_solve: y = R^-1 g over `count` columns, from the last row up, each row a chain s = g_i - sum_k R_ik y_k and
    one division; zero beyond.  R (the device's H block, [41, 40]) and g are the inputs.  Returns (y [41], bound [41])."""
    y, y_b = np.zeros(MAXV, dtype=LD), np.zeros(MAXV, dtype=LD)
    R = np.asarray(R, dtype=LD)
    g = np.asarray(g, dtype=LD)
    for i in range(count - 1, -1, -1):
        row = R[i, i + 1:count]
        s = g[i] - row @ y[i + 1:count]
        mag = abs(g[i]) + np.abs(row) @ np.abs(y[i + 1:count])
        s_b = np.abs(row) @ y_b[i + 1:count] + (count - i + 2) * U * mag
        y[i] = s / R[i, i]
        y_b[i] = s_b / abs(R[i, i]) + U * abs(y[i])
    return y, y_b


def combine(Z, y, count):
    """add_combination from x = 0: x = sum_i y_i z_i, an fma chain of `count` terms per row.  Returns (x, bound)."""
    Zc = np.asarray(Z[:count], dtype=LD)
    yc = np.asarray(y[:count], dtype=LD)
    x = yc @ Zc
    return x, (count + 2) * U * (np.abs(yc) @ np.abs(Zc))


def hessenberg_from_rotations(R, cs, sn, count):
    """H-bar [count + 1, count] rebuilt from the rotated columns the device stores (R = the H block) and its rotations:
    column j is (R_0j .. R_jj, 0) through the transposed rotations j, j - 1, .., 0."""
    Hb = np.zeros((count + 1, count), dtype=LD)
    for j in range(count):
        col = np.zeros(j + 2, dtype=LD)
        col[:j + 1] = np.asarray(R[:j + 1, j], dtype=LD)
        for i in range(j, -1, -1):
            c, s = LD(cs[i]), LD(sn[i])
            a, b = col[i], col[i + 1]
            col[i], col[i + 1] = c * a - s * b, s * a + c * b
        Hb[:j + 2, j] = col
    return Hb


def relation_residual(A, Z, V, Hb, window):
    """A z_j - sum_i Hbar_ij v_i per column j with the bound of what the device did between them: the SpMV, two fma chains
    of nv terms, the norm (a dot of n), the scaling by 1 / hnext, and the rotations there and back on the column
    (4 (j + 2) u |column|_1 per coefficient).  Hbar's rows outside the window must be EXACT zeros for the relation to
    hold with the device's basis: they are left in the sum.  Returns (residual [count, n], bound [count, n])."""
    count = Z.shape[0]
    n = A.shape[0]
    Vl = np.asarray(V, dtype=LD)
    res, bnd = np.zeros((count, n), dtype=LD), np.zeros((count, n), dtype=LD)
    for j in range(count):
        w, w_b = spmv(A, Z[j])
        s0 = max(0, j + 1 - window)
        nv = j + 1 - s0
        coef = Hb[:j + 2, j]
        res[j] = w - coef @ Vl[:j + 2]
        mag = np.abs(w) + 2 * (np.abs(coef[:j + 1]) @ np.abs(Vl[:j + 1]))
        hn = abs(coef[j + 1])
        bnd[j] = (w_b + 2 * (nv + 2) * U * mag + np.abs(Vl[j + 1]) * hn * ((n + 2) * U / 2 + 4 * U)
                  + 4 * (j + 2) * U * np.abs(coef).sum() * np.abs(Vl[:j + 2]).sum(axis=0))
    return res, bnd


# ---- the reference chained into a solver ---------------------------------------------------------------------------

def cycle(A, apply_m, b, x, window=MAXV, max_cols=RESTART, rel_tol=0.0, passes=2, dtype=LD):
    """One restart cycle built from the statements above: returns a dict with x (updated), V, Z, R (41 x 40), cs, sn, g,
    y, count, est.  apply_m(v) -> z is the preconditioner."""
    n = A.shape[0]
    r = np.asarray(b, dtype=LD) - _matvec(A, x)
    rnorm = np.sqrt(r @ r)
    V = np.zeros((max_cols + 1, n), dtype=dtype)
    Z = np.zeros((max_cols, n), dtype=dtype)
    R = np.zeros((MAXV, RESTART), dtype=dtype)
    cs, sn, g = np.zeros(RESTART, dtype=dtype), np.zeros(RESTART, dtype=dtype), np.zeros(MAXV, dtype=dtype)
    V[0] = (r / rnorm).astype(dtype)
    g[0] = rnorm
    count, est = 0, rnorm
    for j in range(max_cols):
        Z[j] = apply_m(V[j])
        s0 = max(0, j + 1 - window)
        st = arnoldi_step(A, Z[j], V[:j + 1], s0, cs[:j], sn[:j], g[j], passes, dtype)
        V[j + 1] = st["v_next"]
        R[:j + 2, j] = st["col"]
        cs[j], sn[j], g[j], g[j + 1], est = st["c"], st["s"], st["g_j"], st["g_next"], st["est"]
        count = j + 1
        if est <= rel_tol * rnorm:
            break
    y, _ = back_substitute(R, g, count)
    dx, _ = combine(Z, y, count)
    return {"x": np.asarray(x, dtype=LD) + dx, "V": V[:count + 1], "Z": Z[:count], "R": R, "cs": cs, "sn": sn, "g": g, "y": y,
            "count": count, "est": est}


def orthogonality(V):
    """(max |v_i . v_k|, i != k;  max | |v_k|^2 - 1 |) in longdouble."""
    Vl = np.asarray(V, dtype=LD)
    G = Vl @ Vl.T
    d = np.abs(np.diag(G) - 1).max()
    off = np.abs(G - np.diag(np.diag(G))).max() if len(Vl) > 1 else LD(0)
    return float(off), float(d)
