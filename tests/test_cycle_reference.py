"""tests/cycle_reference.py is itself shown to bite (no GPU).

The hierarchy is the host-built one of tests/test_hierarchy_reference.py (900 -> 100 -> 50 rows, raw layouts), run
with two parameter sets so that every branch of the reference runs:

  K   K-cycle from level 0 to 1, tail from level 2 (level 1 hands over to the dense bottom), sweeps 3 / 1, level 0
      and level 1 fold their first post-smoothing sweep (W)
  T   tail from level 1 (level 0 directly above a two-level tail with two sweeps per side), no K-cycle, no fold

Three sweeps at level 0, not the solver's two: the reference's third-sweep branch (NODAL_SA_NU=3xx on the device) runs
in no other way, the second sweep runs on the way to it, and the block mode cuts the count to two, so both counts are
covered.  It also decides whether the 2-norm of the residual shrinks on the smooth vector: this hierarchy coarsens by
nine with a prolongator cut to four entries per row, so the error a coarse correction leaves of a smooth right-hand side
is rough, and |A e|_2 stands at 5.4 |r|_2 behind the correction; every post-smoothing sweep takes it down by about
0.45 -- 1.115 after two, 0.64 after three (a textbook two-grid cycle with an EXACT coarse solve on the same A, P, R, six
lines of numpy, gives the same 1.115 after two).  The energy norm of the error, which is what a cycle contracts, falls
to 0.32 / 0.31 of the solution's with two / three sweeps.

First it is shown to be a multigrid cycle at all (the residual shrinks in the 2-norm, the error in energy -- with two
sweeps as well --, a frozen cycle is linear, zero gives zero),
then one planted defect at a time must move the `stored` result by at least 10 E on at least one test vector, E being
what f32 storage alone does to that vector's answer (max|z_stored - z_exact| / max|z_exact|).  Every defect and the
set it is planted in are listed in DEFECT_CASES; the test prints the ratios it found.  Ratios of this hierarchy
(shift / E, best vector), all above the bar of 10, one of them closely:

  skip_second_presweep 1.6e+05   post_omega_p 1.8e+05   r_last_block 8.1e+04   drop_s2c2 7.6e+04
  swap_gamma_beta 7.5e+04   rho2_guard 7.5e+04   t_from_frozen0 7.8e+05   w_value 1.4e+04   tail_sweep 3.2e+04
  coarse_inv 12.2 (the largest entry of the 50 x 50 inverse off by 1e-3: E is 1.9e-7)   block_column 2.9e+05

No defect of the list is undetectable."""
import numpy as np
import pytest

from tests.cycle_reference import DEFECTS, CycleReference, a_of, host_fcg, reference_pair
from tests.test_hierarchy_reference import built  # noqa: F401  (the module-scoped fixture)

PARAMS_K = {"nu0": 3, "nu1": 1, "nu2": 2, "tail_nu": 2, "kcycle": 1, "klevels": 1, "tail": 2, "tail_dense": 0, "nlev": 3,
            "fold_mask": 3, "restrict_mask": 0, "visit_mask": 0}
PARAMS_T = dict(PARAMS_K, tail=1, fold_mask=0)
FROZEN = np.array([1.1, 0.6, 0.9])

# defect -> (parameter set, reference mode, frozen)
DEFECT_CASES = {
    "skip_second_presweep": ("K", 0, False), "post_omega_p": ("T", 0, False), "r_last_block": ("K", 0, False),
    "drop_s2c2": ("K", 0, False), "swap_gamma_beta": ("K", 0, False), "rho2_guard": ("K", 0, False),
    "t_from_frozen0": ("K", 0, True), "w_value": ("K", 0, False), "tail_sweep": ("T", 0, False),
    "coarse_inv": ("K", 0, False), "block_column": ("K", 2, True),
}


def vectors(n, side):
    """[n, 4]: random, smooth (the product of two half sine waves over the grid), a unit vector, zero."""
    rng = np.random.default_rng(11)
    s = np.sin(np.pi * (np.arange(side) + 0.5) / side)
    unit = np.zeros(n)
    unit[n // 2 + side // 3] = 1.0
    return np.stack([rng.standard_normal(n), np.outer(s, s).ravel(), unit, np.zeros(n)], axis=1)


def block_vectors(n, side):
    """[n, 16]: sixteen different columns, the zero and the unit vector among them."""
    rng = np.random.default_rng(12)
    v4 = vectors(n, side)
    cols = [v4[:, 0], v4[:, 1], v4[:, 2], v4[:, 3]]
    for k in range(12):
        cols.append(rng.standard_normal(n) * (1.0 + k) + (k % 3) * v4[:, 1])
    return np.stack(cols, axis=1)


@pytest.fixture(scope="module")
def levels(built):  # noqa: F811
    return built[0]


def params_of(name):
    return PARAMS_K if name == "K" else PARAMS_T


VECTOR_NAMES = ("random", "smooth", "unit")


@pytest.mark.parametrize("which", range(3), ids=VECTOR_NAMES)
@pytest.mark.parametrize("name", ["K", "T"])
def test_the_residual_shrinks(levels, name, which):
    """|r - A z|_2 < |r|_2 in `exact` mode, on every test vector: 0.077 / 0.64 / 0.081 (K), 0.077 / 0.64 / 0.082 (T).
    (Why the smooth vector stands where it does, and where it stands with two sweeps: the module's docstring.)"""
    A = a_of(levels[0], "aval")
    r = vectors(900, 30)[:, which:which + 1]
    z = CycleReference(levels, params_of(name), 0, False).apply(r)
    ratio = float(np.linalg.norm(r - A @ z) / np.linalg.norm(r))
    print(name, VECTOR_NAMES[which], "residual |r - A z| / |r|", ratio)
    assert ratio < 1.0, ratio


@pytest.mark.parametrize("nu0", [2, 3])
@pytest.mark.parametrize("name", ["K", "T"])
def test_the_energy_error_shrinks(levels, name, nu0):
    """|x - z|_A < 0.5 |x|_A with x = A^-1 r: the contraction a multigrid cycle has, on every test vector, with the
    solver's two sweeps at level 0 as with three."""
    A = a_of(levels[0], "aval")
    r = vectors(900, 30)[:, :3]
    x = np.linalg.solve(A.toarray(), r)
    e = x - CycleReference(levels, dict(params_of(name), nu0=nu0), 0, False).apply(r)
    ratio = np.sqrt(np.einsum("ij,ij->j", e, A @ e) / np.einsum("ij,ij->j", x, A @ x))
    print(name, nu0, "energy error ratio per vector", ratio)
    assert (ratio < 0.5).all(), ratio


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("stored", [False, True])
def test_zero_gives_exactly_zero(levels, mode, stored):
    for name in ("K", "T"):
        ref = CycleReference(levels, params_of(name), mode, stored)
        z = ref.apply(np.zeros((900, 2)))
        assert not np.isnan(z).any() and (z == 0.0).all()
        z = ref.apply(vectors(900, 30))  # (a zero column beside others stays zero: columns do not mix)
        assert not np.isnan(z).any() and (z[:, 3] == 0.0).all()


def test_a_frozen_cycle_is_linear(levels):
    ref = CycleReference(levels, PARAMS_K, 0, False)
    v = vectors(900, 30)
    f = np.tile(FROZEN, (1, 1))
    a, b = v[:, :1], v[:, 1:2]
    za, zb, zab = ref.apply(a, f), ref.apply(b, f), ref.apply(2.0 * a - 3.0 * b, f)
    err = np.abs(zab - (2.0 * za - 3.0 * zb)).max() / np.abs(zab).max()
    assert err <= 1e-13, err
    # ... and an adaptive one is not (the coefficients depend on r): the frozen path is a different statement
    ya, yb, yab = ref.apply(a), ref.apply(b), ref.apply(2.0 * a - 3.0 * b)
    assert np.abs(yab - (2.0 * ya - 3.0 * yb)).max() / np.abs(yab).max() > 1e-8


def test_the_block_is_the_single_cycle_per_column(levels):
    """mode 2 with <= 2 sweeps and no fold is mode 1 without folds, column by column."""
    v = block_vectors(900, 30)
    two = dict(PARAMS_K, nu0=2)
    zb = CycleReference(levels, two, 2, True).apply(v)
    for y in (0, 2, 7, 15):
        z1 = CycleReference(levels, dict(two, fold_mask=0), 1, True).apply(v[:, y:y + 1])
        assert np.array_equal(z1[:, 0], zb[:, y]), y
    assert PARAMS_K["nu0"] == 3
    assert np.array_equal(CycleReference(levels, PARAMS_K, 2, True).apply(v), zb)  # (the block has no third sweep)


def test_the_folded_forms_are_the_same_algebra(levels):
    """`stored` with W differs from `stored` without it by roundings only (of the order of E)."""
    v = vectors(900, 30)[:, :3]
    ze, zs, E = reference_pair(levels, PARAMS_K, 0, v)
    zu = CycleReference(levels, dict(PARAMS_K, fold_mask=0), 0, True).apply(v)
    d = np.abs(zu - zs).max(axis=0) / np.abs(ze).max(axis=0)
    print("fold vs no fold / E", d / E)
    assert (d <= 4.0 * E).all(), d / E


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_planted_defect_shows(levels, defect):
    name, mode, frozen = DEFECT_CASES[defect]
    params = params_of(name)
    v = block_vectors(900, 30) if mode == 2 else vectors(900, 30)
    k = v.shape[1]
    f = None
    if frozen:
        f = np.tile(FROZEN, (k, 1)) * (1.0 + 0.05 * np.arange(k))[:, None]  # (a column's own coefficients)
    ze, zs, E = reference_pair(levels, params, mode, v, f)
    zd = CycleReference(levels, params, mode, True, defect=defect).apply(v, f)
    scale = np.abs(ze).max(axis=0)
    live = scale > 0.0
    shift = np.abs(zd - zs).max(axis=0)[live] / scale[live]
    ratio = shift / E[live]
    print(f"{defect}: E {E[live].max():.2e}, shift / E per vector {np.array2string(ratio, precision=3)}")
    assert (E[live] > 0.0).all() and (E[live] < 1e-5).all(), E  # (f32 storage: a few 2^-24)
    assert ratio.max() >= 10.0, (defect, ratio)
    assert not np.isnan(zd).any()
    assert (zd[:, ~live] == 0.0).all()  # (zero stays zero under every defect)


def test_the_host_iteration_converges_and_sees_a_worse_cycle(levels):
    """host_fcg (what tests/test_gpu_cycle.py counts the device's iterations against) solves to the solver's 1e-13,
    and a cycle made worse costs it iterations: the count is a statement about the cycle."""
    A = a_of(levels[0], "aval")
    b = vectors(900, 30)[:, 0]
    k, x = host_fcg(levels, PARAMS_K, b)
    assert 0 < k < 40 and np.linalg.norm(b - A @ x) <= 1e-12 * np.linalg.norm(b)
    k1, _ = host_fcg(levels, dict(PARAMS_K, nu0=1, fold_mask=0), b)
    print("host iterations", k, "with one sweep at level 0", k1)
    assert k1 > k
