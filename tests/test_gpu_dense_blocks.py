"""The dense path's GEMMs, block inverses, eliminations and pivoted LU in isolation, on the MI355X.

Through three testing hooks (nodal_debug_gemm_ex, nodal_debug_block_inverse, nodal_debug_dense_solve: host arrays into
scratch, the production function, the results back) and against tests/dense_reference.py, which
tests/test_dense_reference.py pins down on the CPU.  Most checks compare BITS: integer operands for the GEMMs, and for
the inverses and eliminations the exact families (A = L U and L L^T with integer unit triangular factors: every pivot is
1, every intermediate a small integer, the inverse an integer matrix) on which a skipped or doubly applied tile, a term
of the wrong sign or a stale panel changes an integer.  Float inputs follow, held by error measures in longdouble.

The bars.  eta (normwise backward error): n eps, "backward stable"; LAPACK on the same inputs stays below n eps / 16
(CPU test).  e(Q) = max(|QA - I|, |AQ - I|) of a block inverse on the float SPD family, against e of numpy.linalg.inv on
the same matrix: the bar is 4 x the worst device / numpy ratio measured over all w in one run (the factor 4 absorbs
another summation order at another w; e(numpy) is taken as at least 2^-53, it is exactly 0 at w = 1).  Measured on an
MI355X over the 24 sizes of dense_reference.INVERSE_SIZES:

    variant            worst e(device) / e(numpy)    at w
    rank16_dpp         2.732                         257
    rank16_bpermute    2.732 (the same bits)         257
    rank4              2.524                         257
    scalar             2.551                         255

so the bar is 4 x 2.732 = 10.93 for every variant.
"""
import numpy as np
import pytest

from nodal_amd import _ffi
from tests import dense_reference as dr

pytestmark = pytest.mark.gpu

PAD = 24
MODES = _ffi.Handle.GEMM_MODES
VARIANTS = _ffi.Handle.INVERSE_VARIANTS
SENTINEL = -123456.78125

# worst e(device) / e(numpy.linalg.inv) over INVERSE_SIZES on the float SPD family, per variant, as measured; the bar of
# test_block_inverse_float_error is four times the worst of them
E_RATIO_MEASURED = {"rank16_dpp": 2.732, "rank16_bpermute": 2.732, "rank4": 2.524, "scalar": 2.551}
E_RATIO_BAR = 4.0 * max(E_RATIO_MEASURED.values())


@pytest.fixture(scope="module")
def handle():
    h = _ffi.Handle(0)
    yield h
    h.close()


def _padded(M, pad, fill):
    """M in a Fortran array with `pad` more rows holding `fill`."""
    out = np.full((M.shape[0] + pad, M.shape[1]), fill, order="F")
    out[:M.shape[0]] = M
    return out


def _operands(rng, M, N, K, integer, transposed=False):
    draw = (lambda *s: rng.integers(-8, 9, s).astype(float)) if integer else (lambda *s: rng.standard_normal(s))
    return (draw(K, M) if transposed else draw(M, K)), draw(K, N), draw(M, N)


def _expected(mode, A, B, C):
    return {"sub": C - A @ B, "set": A @ B, "setneg": -(A @ B)}[mode]


def _check_product(out, ref, M, K, integer, pad):
    if integer:
        assert np.array_equal(out[:M], ref)
    else:
        assert np.abs(out[:M] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()) * K
    if pad:
        assert np.array_equal(out[M:], np.full((pad, ref.shape[1]), SENTINEL))  # bit for bit


SMALL_SHAPES = [(1, 1, 1), (3, 5, 7), (32, 32, 4), (33, 31, 2), (40, 40, 129), (256, 2100, 256)]
BIG_SHAPES = [(300, 1800, 1), (300, 1800, 15), (300, 1800, 17), (130, 4100, 257), (1000, 600, 16)]


def test_gemm_router_sends_the_shapes_where_the_tables_say():
    small = lambda M, N, K: M * N <= 524288 or (M <= 256 and K <= 256)  # noqa: E731  (gemm_f64 of csrc/gemm_f64.hip)
    assert all(small(*s) for s in SMALL_SHAPES) and not any(small(*s) for s in BIG_SHAPES)


@pytest.mark.parametrize("pad", [0, PAD])
@pytest.mark.parametrize("M,N,K", SMALL_SHAPES + BIG_SHAPES)
def test_gemm_every_mode_and_leading_dimension(handle, M, N, K, pad):
    """gemm_f64 in its three modes, both kernels, exact or padded leading dimensions: NaN in the padding rows of A and B
    must reach nothing, C's padding rows come back bit for bit, and the overwrite modes never read C (NaN there)."""
    rng = np.random.default_rng(M * 7 + N * 3 + K + pad)
    for integer in (True, False):
        A, B, C = _operands(rng, M, N, K, integer)
        for mode in MODES:
            Cin = C if mode == "sub" else np.full_like(C, np.nan)
            out = handle.debug_gemm_ex("plain", mode, (M, N, K), _padded(A, pad, np.nan), _padded(B, pad, np.nan),
                                       _padded(Cin, pad, SENTINEL))
            _check_product(out, _expected(mode, A, B, C), M, K, integer, pad)


@pytest.mark.parametrize("pad", [0, PAD])
@pytest.mark.parametrize("m1,m2", [(128, 1), (128, 72), (128, 128), (256, 1), (256, 200), (256, 256)])
def test_gemm_pair_in_the_shapes_of_the_inverse_chain(handle, m1, m2, pad):
    """gemm_pair_f64: T1 (m1 x m2, K = m1) and T2 (m2 x m1, K = m1) as invert_diag launches them, in every mode."""
    rng = np.random.default_rng(m1 * 5 + m2 + pad)
    for integer in (True, False):
        p = [_operands(rng, m1, m2, m1, integer), _operands(rng, m2, m1, m1, integer)]
        sizes = [(m1, m2, m1), (m2, m1, m1)]
        for mode in MODES:
            args = []
            for (A, B, C), s in zip(p, sizes):
                Cin = C if mode == "sub" else np.full_like(C, np.nan)
                args.append((s, _padded(A, pad, np.nan), _padded(B, pad, np.nan), _padded(Cin, pad, SENTINEL)))
            outs = handle.debug_gemm_ex("pair", mode, *args[0], second=args[1])
            for out, (A, B, C), s in zip(outs, p, sizes):
                _check_product(out, _expected(mode, A, B, C), s[0], s[2], integer, pad)


@pytest.mark.parametrize("pad", [0, PAD])
@pytest.mark.parametrize("M,N,K,band", [(128, 128, 16, 128), (300, 301, 256, 128), (700, 707, 256, 256),
                                        (700, 700, 512, 512), (1100, 1117, 128, 256)])
def test_gemm_transposed_upper(handle, M, N, K, band, pad):
    """gemm_sub_tn_upper_f64, the bulk update of the symmetric elimination: C -= At^T B.  The upper block triangle --
    everything at or right of the `band`-wide diagonal block of its row -- must be exact; below it a tile may be
    skipped or updated, so every entry is bit-equal to the old or to the fully updated value."""
    rng = np.random.default_rng(M + N + K + band + pad)
    rows = np.arange(M)[:, None]
    wanted = np.arange(N)[None, :] >= (rows // band) * band
    for integer in (True, False):
        At, B, C = _operands(rng, M, N, K, integer, transposed=True)
        out = handle.debug_gemm_ex("tn_upper", "sub", (M, N, K), _padded(At, pad, np.nan), _padded(B, pad, np.nan),
                                   _padded(C, pad, SENTINEL), band=band)
        ref = C - At.T @ B
        if pad:
            assert np.array_equal(out[M:], np.full((pad, N), SENTINEL))
        got = out[:M]
        if integer:
            assert np.array_equal(got[wanted], ref[wanted])
            assert ((got == ref) | (got == C))[~wanted].all()
        else:
            bar = 1e-12 * max(1.0, np.abs(ref).max()) * K
            assert np.abs(got - ref)[wanted].max() <= bar
            assert ((np.abs(got - ref) <= bar) | (got == C))[~wanted].all()


# ---- block inverse ----

def _inverse_all_variants(handle, A, w, lda_pad, base=0):
    Ain = _padded(A, lda_pad, np.nan)
    out = {}
    for v in VARIANTS:
        Q, dinfo = handle.debug_block_inverse(Ain, w, v, base=base, Q=np.full((w + lda_pad, w), SENTINEL, order="F"))
        if lda_pad:
            assert np.array_equal(Q[w:], np.full((lda_pad, w), SENTINEL)), v
        out[v] = (Q[:w], dinfo)
    return out


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("w", dr.INVERSE_SIZES)
def test_block_inverse_is_exact_on_the_exact_families(handle, w, symmetric):
    """invert_diag in its four variants on L L^T and L U: Q must be the integer inverse bit for bit, with lda = w and
    lda = w + 24 (NaN in the padding rows)."""
    A = dr.exact_matrix(w, dr.inverse_spacing(w), symmetric, seed=w)
    want, stop, _ = dr.schur_inverse(A)
    assert stop == 0
    for pad in (0, PAD):
        for v, (Q, dinfo) in _inverse_all_variants(handle, A, w, pad).items():
            assert dinfo == 0, (v, pad, dinfo)
            assert np.array_equal(Q, want), (v, pad, np.argwhere(Q != want)[:4])


def _float_inverse_ratios(handle, w):
    A = dr.spd_dominant(w, 5000 + w)
    res = _inverse_all_variants(handle, A, w, PAD)
    assert all(d == 0 for _, d in res.values())
    assert np.array_equal(res["rank16_dpp"][0], res["rank16_bpermute"][0])  # csrc/gj16_wave.h: the same arithmetic
    e_ref = max(dr.inverse_error(A, np.linalg.inv(A)), 2.0 ** -53)
    return {v: dr.inverse_error(A, res[v][0]) / e_ref for v in ("rank16_dpp", "rank4", "scalar")}


@pytest.mark.parametrize("w", dr.INVERSE_SIZES)
def test_block_inverse_float_error(handle, w):
    """The float SPD family: the two lane-exchange forms of the rank-16 kernel give the same bits, and e(Q) of every
    variant stays within E_RATIO_BAR of e(numpy.linalg.inv) on the same matrix."""
    ratios = _float_inverse_ratios(handle, w)
    print("e(Q) ratios w=%d: %s" % (w, {k: round(v, 3) for k, v in ratios.items()}))
    assert max(ratios.values()) <= E_RATIO_BAR, ratios


def _zero_pivot_cases():
    cases = []
    for w in (2, 17, 18, 130, 131, 300):  # inside one 16-block, across 16, across the 128 quadrants, in the Schur half
        for p in (0, 1, 14, 15, 16, 127, 128, w - 2):
            if 0 <= p <= w - 2 and (w, p) not in cases:
                cases.append((w, p))
    return cases


@pytest.mark.parametrize("base", [0, 640])
@pytest.mark.parametrize("w,p", _zero_pivot_cases())
def test_block_inverse_reports_the_exact_zero_pivot(handle, w, p, base):
    """Identity except one isolated pair [[1, -1], [-1, 1]] at rows p, p + 1: dinfo = base + the 1-based column at which
    a scalar elimination stops, in all four variants (the 2 x 2-pivot rule of csrc/gj16_wave.h included)."""
    A = dr.conductance_pair_block(w, p)
    _, stop, _ = dr.gauss_jordan_nopivot(A)
    assert stop == p + 2
    for v, (_, dinfo) in _inverse_all_variants(handle, A, w, 0, base=base).items():
        assert dinfo == base + stop, (v, dinfo)


# ---- elimination through nodal_debug_dense_solve ----

def _set_pattern(monkeypatch, pattern):
    for name, value in zip(("NODAL_BI_WIDTH", "NODAL_BI_SWITCH", "NODAL_BI_SWITCH2"), dr.WIDTH_PATTERNS[pattern]):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def _exact_solves(h, n, symmetric):
    A = dr.exact_matrix(n, dr.SOLVE_SPACING, symmetric, seed=n)
    X0 = dr.integer_rhs(n, max(dr.ELIM_NRHS), n)
    for nrhs in dr.ELIM_NRHS:
        X, info, rows = h.debug_dense_solve(A, A @ X0[:, :nrhs], passive=symmetric, optimistic=not symmetric)
        assert info == 0 and np.array_equal(rows, np.arange(n))
        assert np.array_equal(X, X0[:, :nrhs]), (n, nrhs, symmetric, np.argwhere(X != X0[:, :nrhs])[:4])


@pytest.mark.parametrize("pattern", sorted(dr.WIDTH_PATTERNS))
@pytest.mark.parametrize("n", dr.ELIM_SIZES)
def test_block_elimination_is_exact_on_the_exact_families(handle, n, pattern, monkeypatch):
    """Both forms of the block elimination -- symmetric (L L^T, flagged passive) and full (L U, flagged optimistic) --
    with 1, 2, 7 and 17 right-hand sides B = A X_int: X must be X_int bit for bit, under every block-width pattern."""
    _set_pattern(monkeypatch, pattern)
    for symmetric in (True, False):
        _exact_solves(handle, n, symmetric)


@pytest.mark.parametrize("scalar", ["1", "2"])
def test_block_elimination_is_exact_with_the_other_inverse_kernels(scalar, monkeypatch):
    """One size per width pattern on handles created under NODAL_GJ_SCALAR=1 (scalar steps) and =2 (rank-4 steps)."""
    monkeypatch.setenv("NODAL_GJ_SCALAR", scalar)
    h = _ffi.Handle(0)
    try:
        for pattern, n in (("default", 700), ("w128", 513), ("w512", 1100), ("mixed", 1400)):
            _set_pattern(monkeypatch, pattern)
            for symmetric in (True, False):
                _exact_solves(h, n, symmetric)
    finally:
        h.close()


def test_nopivot_lu_is_exact_on_the_exact_family(monkeypatch):
    """NODAL_DENSE_BLOCKINV=0: the no-pivot LU of dense_lu.hip, n = 1400 > GEPP_MAX."""
    monkeypatch.setenv("NODAL_DENSE_BLOCKINV", "0")
    h = _ffi.Handle(0)
    try:
        _exact_solves(h, 1400, True)
    finally:
        h.close()


@pytest.mark.parametrize("pattern", sorted(dr.WIDTH_PATTERNS))
@pytest.mark.parametrize("n", dr.ELIM_SIZES)
def test_block_elimination_is_backward_stable_on_spd_inputs(handle, n, pattern, monkeypatch):
    """The float family (SPD, diagonally dominant by a factor 2, no band), both forms: eta <= n eps."""
    _set_pattern(monkeypatch, pattern)
    A = dr.spd_dominant(n, n)
    B = np.random.default_rng(n).standard_normal((n, max(dr.ELIM_NRHS)))
    for symmetric in (True, False):
        X, info, _ = handle.debug_dense_solve(A, B, passive=symmetric, optimistic=not symmetric)
        eta = dr.backward_error(A, X, B).max()
        print("eta / (n eps) n=%d %s sym=%d: %.4f" % (n, pattern, symmetric, eta / (n * dr.EPS)))
        assert info == 0 and eta <= n * dr.EPS, (symmetric, eta / (n * dr.EPS))


# ---- pivoted LU ----

def _pivoted_case(h, n, nrhs, panels, compare_rows):
    for name, A in dr.pivot_inputs(n).items():
        B = dr.pivot_rhs(A, nrhs)
        outs = []
        try:
            for panel in panels:
                h.set_option(_ffi.OPT_GEPP_PANEL, panel)
                outs.append(h.debug_dense_solve(A, B))
        finally:
            h.set_option(_ffi.OPT_GEPP_PANEL, 1)
        X, info, rows = outs[0]
        assert info == 0
        for Xo, infoo, rowso in outs[1:]:  # the panel kernel and the per-column kernels: the same bits
            assert infoo == 0 and np.array_equal(rowso, rows) and np.array_equal(Xo, X), name
        if compare_rows:
            want, _ = dr.lapack_pivots(A)
            assert np.array_equal(rows, want), (name, np.flatnonzero(rows != want)[:4])
        Xl = np.linalg.solve(A, B)
        eta, eta_l = dr.backward_error(A, X, B), dr.backward_error(A, Xl, B)
        print("eta / (n eps) n=%d nrhs=%d %s: device %.4f lapack %.4f" % (n, nrhs, name, eta.max() / (n * dr.EPS),
                                                                           eta_l.max() / (n * dr.EPS)))
        assert eta.max() <= n * dr.EPS, (name, eta.max() / (n * dr.EPS))
        kappa = np.linalg.cond(A, np.inf)
        bound = 4.0 * kappa * (eta + eta_l) * np.abs(X).max(axis=0)
        assert (np.abs(X - Xl).max(axis=0) <= bound).all(), name


@pytest.mark.parametrize("nrhs", dr.PIVOT_NRHS)
@pytest.mark.parametrize("n", dr.GEPP_SIZES)
def test_partial_pivoting_matches_lapack_rows_and_is_backward_stable(handle, n, nrhs):
    """Partial pivoting (n <= 1280) on Gaussian matrices and on the real embedding of a complex system, with up to 512
    right-hand sides: the panel kernel and the per-column kernels give the same bits, the row order applied is
    dgetrf's (scipy.linalg.lu_factor; its choices on these inputs are clear by 1e-6, CPU test), eta <= n eps, and
    |x - x_lapack| <= 4 kappa_inf (eta_device + eta_lapack) |x|, the first-order perturbation bound with a factor 4."""
    _pivoted_case(handle, n, nrhs, (1, 0), True)


@pytest.mark.parametrize("nrhs", [1, 17])
@pytest.mark.parametrize("n", dr.TOURNAMENT_SIZES)
def test_tournament_pivoting_is_backward_stable(handle, n, nrhs):
    """Tournament pivoting (n > 1280) on the same families: eta and the perturbation bound (its pivots are not
    LAPACK's)."""
    _pivoted_case(handle, n, nrhs, (1,), False)


# ---- the switches that are read once per process ----

def test_elimination_switches_give_identical_bits():
    """tests/dense_variant_child.py, one process at a time: the bulk update on all CUs (NODAL_BI_MASKED=0), the two side
    streams swapping roles at 500 rows left (NODAL_BI_UNMASK_ROWS), the next panel's first columns copied on the chain
    (NODAL_BI_EARLY_COPY=0) and the bpermute lane exchanges (NODAL_GJ_DPP=0) change streams or exchanges only
    (csrc/block_elim.hip, csrc/gj16_wave.h): the digests over the float solutions must be EQUAL.  The full form for
    passive systems (NODAL_BI_SYM=0) and one block of first columns (NODAL_BI_FIRST_BLOCKS=1) change the arithmetic or
    the split of columns over GEMM kernels: for them the child's own assertions (exact families bit for bit, eta <= n
    eps) are the check."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    digests = {}
    for name, extra, same_bits in (("default", {}, True), ("unmasked", {"NODAL_BI_MASKED": "0"}, True),
                                   ("adaptive mask", {"NODAL_BI_UNMASK_ROWS": "500"}, True),
                                   ("late copy", {"NODAL_BI_EARLY_COPY": "0"}, True),
                                   ("bpermute", {"NODAL_GJ_DPP": "0"}, True),
                                   ("full form", {"NODAL_BI_SYM": "0"}, False),
                                   ("one first block", {"NODAL_BI_FIRST_BLOCKS": "1"}, False)):
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "dense_variant_child.py")],
                           env=dict(os.environ, **extra), cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "dense variant digest" in r.stdout, (name, r.stdout[-2000:], r.stderr[-2000:])
        if same_bits:
            digests[name] = r.stdout.split("dense variant digest")[1].split()[0]
    assert len(set(digests.values())) == 1, digests
