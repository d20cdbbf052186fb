"""What tests/test_gpu_dense_blocks.py relies on, pinned down on the CPU (tests/dense_reference.py): the exact families
ARE inverted and solved exactly by an elimination without pivoting at every size and width pattern the GPU tests use,
every 128-tile of every block update is non-zero, the intermediates stay far below 2^53, LAPACK's own backward error on
the float inputs leaves the device a factor 16, and no pivot choice of LAPACK on the pivot-comparison inputs is close."""
import numpy as np
import pytest

from tests import dense_reference as dr

INTERMEDIATE_LIMIT = 2.0 ** 40  # a wide margin below 2^53


def test_sliced_longdouble_product_matches_the_plain_one():
    rng = np.random.default_rng(3)
    A = rng.standard_normal((150, 170)) * 10.0 ** rng.uniform(-8, 8, (150, 170))
    B = rng.standard_normal((170, 90)) * 10.0 ** rng.uniform(-8, 8, (170, 90))
    plain = A.astype(dr.LD) @ B.astype(dr.LD)
    bound = np.abs(A).astype(dr.LD) @ np.abs(B).astype(dr.LD)
    eps_ld = np.finfo(dr.LD).eps
    assert (np.abs(dr.matmul_ld(A, B) - plain) <= 170 * eps_ld * bound).all()
    # ... and is exact where the plain one is: small integers
    Ai, Bi = rng.integers(-8, 9, (40, 2000)).astype(float), rng.integers(-8, 9, (2000, 30)).astype(float)
    assert np.array_equal(dr.matmul_ld(Ai, Bi), (Ai @ Bi).astype(dr.LD))


@pytest.mark.parametrize("symmetric", [True, False])
def test_exact_families_are_inverted_exactly(symmetric):
    for w in dr.INVERSE_SIZES:
        A = dr.exact_matrix(w, dr.inverse_spacing(w), symmetric, seed=w)
        assert np.array_equal(A, np.round(A)) and np.abs(A).max() <= 64
        if symmetric:
            assert np.array_equal(A, A.T)
            if w > 1:
                assert np.linalg.eigvalsh(A).min() > 0
        Q, stop, big = dr.schur_inverse(A)
        assert stop == 0 and big < INTERMEDIATE_LIMIT, (w, stop, big)
        assert np.array_equal(Q, np.round(Q)), w
        I = np.eye(w)
        assert np.array_equal(Q @ A, I) and np.array_equal(A @ Q, I), w  # (integers below 2^53: exact products)
        Qs, stop, big = dr.gauss_jordan_nopivot(A)  # scalar steps all the way: the same integers
        assert stop == 0 and big < INTERMEDIATE_LIMIT and np.array_equal(Qs, Q), w


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("pattern", sorted(dr.WIDTH_PATTERNS))
def test_exact_families_are_eliminated_exactly_with_every_tile_updated(pattern, symmetric):
    for n in dr.ELIM_SIZES:
        A = dr.exact_matrix(n, dr.SOLVE_SPACING, symmetric, seed=n)
        X0 = dr.integer_rhs(n, max(dr.ELIM_NRHS), n)
        bnd = dr.pattern_boundaries(n, pattern)
        X, big, empty = dr.block_eliminate(A, A @ X0, bnd)
        assert np.array_equal(X, X0), (n, bnd)
        assert empty == 0 and big < INTERMEDIATE_LIMIT, (n, bnd, empty, big)
        assert np.array_equal(np.linalg.solve(A, A @ X0[:, :1]), X0[:, :1]) or np.linalg.cond(A) > 1e9, n


def test_width_patterns_reach_every_width():
    assert dr.pattern_boundaries(1400, "mixed") == [0, 512, 768, 1024, 1280, 1400]  # 512 -> 256 -> 128 (-> 120)
    assert dr.pattern_boundaries(1400, "default") == [0, 256, 512, 768, 1024, 1280, 1400]
    assert dr.pattern_boundaries(513, "w128") == [0, 128, 256, 384, 512, 513]
    assert dr.pattern_boundaries(1100, "w512") == [0, 512, 1024, 1100]


def test_zero_pivot_blocks_stop_where_the_pair_ends():
    for w, p in ((2, 0), (17, 15), (130, 127), (300, 128), (300, 298)):
        Q, stop, _ = dr.gauss_jordan_nopivot(dr.conductance_pair_block(w, p))
        assert Q is None and stop == p + 2
        assert dr.schur_inverse(dr.conductance_pair_block(w, p))[1] == p + 2


def _lapack_eta(A, nrhs, seed):
    B = np.random.default_rng(seed).standard_normal((A.shape[0], nrhs))
    return dr.backward_error(A, np.linalg.solve(A, B), B).max()


def test_lapack_leaves_the_device_a_factor_sixteen_on_every_float_input():
    for n in dr.ELIM_SIZES:
        assert _lapack_eta(dr.spd_dominant(n, n), max(dr.ELIM_NRHS), n) <= n * dr.EPS / 16, n
    for n in dr.GEPP_SIZES + dr.TOURNAMENT_SIZES:
        for name, A in dr.pivot_inputs(n).items():
            for nrhs in dr.PIVOT_NRHS:
                B = dr.pivot_rhs(A, nrhs)
                eta = dr.backward_error(A, np.linalg.solve(A, B), B).max()
                assert eta <= n * dr.EPS / 16, (n, name, nrhs, eta / (n * dr.EPS))
    for w in dr.INVERSE_SIZES:  # (the inverse test's float family: symmetric positive definite, well conditioned)
        A = dr.spd_dominant(w, 5000 + w)
        assert np.linalg.cond(A) <= 64, w


def test_lapack_pivot_choices_are_clear_on_every_comparison_input():
    for n in dr.GEPP_SIZES:
        for name, A in dr.pivot_inputs(n).items():
            rows, runner = dr.lapack_pivots(A)
            assert sorted(rows) == list(range(n))
            assert runner.max() <= 1.0 - 1e-6, (n, name, runner.max())
