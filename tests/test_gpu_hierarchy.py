"""The multigrid setup's operators, level by level, against an fp64 host reference (tests/hierarchy_reference.py).

Every other test of csrc/sagg.hip looks at the solution and the residual, which a flexible Krylov iteration with an fp64
residual repairs whatever the preconditioner holds: a product dropped from a Galerkin row, a stale value after the
values-only refresh, an R entry paired with the wrong slot of P, a non-zero in a padding slot, an f32 copy that lags
its f64 value or a W row that misses a column would cost iterations and nothing else.  Here the hierarchy is exported
raw (nodal_debug_hierarchy_info / nodal_debug_hierarchy_array: stream waits and copies, no kernel) and held to the
setup's own algebra, P = (I - w D^-1 A) P_tent cut to four entries, R = P^T, A_{l+1} = R A_l P, dinv = 1 / diag, f32
copies = casts, W = P - w D^-1 (A P), a dense inverse at the bottom, with the bounds of hierarchy_reference's docstring.

Shapes (random resistances, uniform in [1, 3] ohm, fixed seeds: a uniform grid would make transpositions and slot mix-ups
invisible): the 100 x 100 grid (level-0 rows of at most five), a 16 x 16 x 16 seven-point grid (level-0 rows of seven:
the 64-slot A P kernel and a width class of 8 already at level 0), and config 5 on a 66 x 66 grid (the general path:
the presolve leaves a non-symmetric node system, whose hierarchy the same handle exports; the check uses no symmetry).
The passive shapes are solved with SPARSE_PCG (small networks take the direct route by default); config 5 with
SPARSE_LU, the general route -- its branch equations keep the full system out of the multigrid under SPARSE_PCG, and
below 4097 reduced unknowns (N <= 64) the reduced system is solved densely without any hierarchy.

Measured on MI355X -- level sizes as rows/longest row/aggregates per level, and the largest error / bound per quantity:
  grid100    9999/5/1458  1458/15/89  89/17/4  4/4/0     P 0  Galerkin 0.335  W 0.499  coarse_inv 0.0013
  grid3d_16  4095/7/432   432/41/11   11/11/0            P 0  Galerkin 0.373  W 0.495  coarse_inv 0.0006
  cfg5_66    4355/5/627   627/15/39   39/17/0            P 0  Galerkin 0.305  W 0.496  coarse_inv 0.0016
  grid100 after a values-only refresh                    P 0  Galerkin 0.350  W 0.497  coarse_inv 0.0015
  grid100 with NODAL_SA_GCAP=64 NODAL_SA_GG=8            P 0  Galerkin 0.335  W 0.499  coarse_inv 0.0008
(P 0: pval has the bits of the numpy reference; W's half is the f32 rounding against a bound of one ulp.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from nodal_amd import _ffi
from tests import hierarchy_child as shapes
from tests import hierarchy_reference as ref
from tests.hierarchy_reference import check_hierarchy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"grid100": (shapes.grid100, _ffi.SPARSE_PCG), "grid3d_16": (shapes.grid3d, _ffi.SPARSE_PCG),
          "cfg5_66": (shapes.cfg5, _ffi.SPARSE_LU)}
PATTERNS = ("acol", "alen", "agg", "pcol", "rcol", "rlen", "wcol", "wlen")


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def exported():
    """Every shape set up once: {shape: (levels, csr or None)}; nothing changes the exports afterwards."""
    out = {}
    for name, (table, method) in SHAPES.items():
        h, (levels,) = shapes.solve_and_export(table(), method)
        csr = h.export_csr() if method == _ffi.SPARSE_PCG else None
        h.close()
        out[name] = (levels, csr)
    return out


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fresh_setup_matches_the_reference(exported, shape):
    levels, csr = exported[shape]
    stats = check_hierarchy(levels)
    print(shape, "levels", ref.coverage(levels)[1], "error / bound", {k: f"{v:.3g}" for k, v in stats.items()})
    assert levels[0]["refreshed"] == 0
    if csr is not None:  # the hierarchy's level 0 is the assembled matrix itself
        indptr, indices, data, _ = csr
        A0 = ref.csr_of_level(levels[0])
        assert A0.shape[0] == len(indptr) - 1
        assert np.array_equal(A0.indptr, indptr) and np.array_equal(A0.indices, indices)
        assert same_bytes(np.ascontiguousarray(A0.data), np.ascontiguousarray(data))


def test_the_shapes_reach_every_path_of_the_setup_kernels(exported):
    """Conditions on the exported data, over the shapes together, so that no path goes untested silently: 16- and
    64-slot A P rows (ap_rows / ap_rows_lds), a folded level >= 1 above 1024 rows, a coarse row whose R entries need a
    second Galerkin group (more than 40 at a 16-slot level, 16 at a 64-slot one), coarse rows of <= 16, 17-32 and > 32
    columns (the four-, two- and one-segment accumulation), R rows of <= 32 and > 32 entries (r_sort_short /
    r_sort_medium), a fine row that lumps (more than four aggregates among its columns).

    Seen on MI355X (level sizes in the module's docstring): grid100 reaches everything but a coarse row of more than 32
    columns (its level 1, 1458 rows, is the folded level above 1024 rows), which grid3d_16's level 1 has (rows of up to
    41); cfg5_66 adds nothing of its own but goes through both A P kernels, both sorts and a second group on the general
    path's matrix."""
    seen = set()
    for name, (levels, _) in exported.items():
        here, sizes = ref.coverage(levels)
        print(name, sizes, sorted(here))
        seen |= here
    assert seen == ref.COVERAGE, sorted(ref.COVERAGE - seen)


def refresh_members():
    table = shapes.grid100()
    v0 = table.value.copy()
    v1 = v0.copy()
    v1[:-1] *= np.random.default_rng(101).uniform(0.5, 2.0, size=len(v0) - 1)
    return table, np.stack([v0, v1, v0])


def test_values_only_refresh():
    """Three members on one handle, the third the first again: the second and third setups are values-only refreshes
    (refreshed = 1) that leave every pattern as it was; the second passes the reference for the second member's values
    (no stale value anywhere), and the third agrees with the FRESH setup of the same values, the first export --
    patterns, pval and rval bit for bit (same kernels, same inputs; r_refresh against r_to_ell), and the coarse
    matrices with their dinv bit for bit as well: galerkin_rows<true, .> sums a row's products in the list order of
    galerkin_rows<false, .>, and on MI355X the two gave the same bits on every level, which is therefore what is asserted
    (the Galerkin bound against the reference holds for both through check_hierarchy).

    The refresh is not compared level by level with a fresh handle set up on the second member's values alone: the
    aggregation joins a node at distance two to its STRONGEST assigned neighbour (assign_far), so other values give
    other aggregates (measured: they differ on this grid), and the refresh keeps the first member's by design.  What
    does not depend on the aggregates -- level 0's matrix, its f32 copy and dinv -- is compared with such a handle
    bit for bit."""
    table, members = refresh_members()
    h, (first, second, third) = shapes.solve_and_export(table, members=members)
    h.close()
    assert first[0]["refreshed"] == 0 and second[0]["refreshed"] == 1 and third[0]["refreshed"] == 1
    assert len(first) == len(second) == len(third)
    for a, b, c in zip(first, second, third):
        for name in PATTERNS:
            assert same_bytes(a[name], b[name]) and same_bytes(a[name], c[name]), name
    assert not same_bytes(first[1]["aval"], second[1]["aval"])  # (the values did move)
    print("refreshed: error / bound", check_hierarchy(second))
    print("refreshed back: error / bound", check_hierarchy(third))
    for l, (a, c) in enumerate(zip(first, third)):
        for name in ("pval", "pvalf", "rval", "rvalf", "wval", "dinv"):
            assert same_bytes(a[name], c[name]), (l, name)
        assert same_bytes(ref.csr_of_level(a).data.copy(), ref.csr_of_level(c).data.copy()), (l, "aval")
    print("coarse_inv of the refresh bit-equal to the fresh setup's:", same_bytes(first[-1]["coarse_inv"], third[-1]["coarse_inv"]))
    h, (fresh,) = shapes.solve_and_export(shapes.gen.grid_table(100, members[1][:-1]))
    h.close()
    for name in ("acol", "alen", "aval", "avalf", "adcol", "dinv"):
        assert same_bytes(second[0][name], fresh[0][name]), name
    print("aggregates of a fresh setup on the second member's values equal to the kept ones:",
          same_bytes(second[0]["agg"], fresh[0]["agg"]))


def test_second_stream_builds_the_same_hierarchy(exported):
    """OPT_EXTRA_STREAMS: R is built on the hierarchy's second stream beside A P -- "same kernels, same results": every
    exported array of every level has the bits of the default handle's."""
    h, (levels,) = shapes.solve_and_export(shapes.grid100(), extra_streams=True)
    h.close()
    base = exported["grid100"][0]
    assert len(levels) == len(base)
    for l, (a, b) in enumerate(zip(levels, base)):
        assert set(a) == set(b)
        for name in a:
            if isinstance(a[name], np.ndarray):
                assert same_bytes(a[name], b[name]), (l, name)
            else:
                assert a[name] == b[name], (l, name)


def test_the_export_hook_reads_and_nothing_else():
    """nodal_debug_hierarchy_*: NODAL_E_INVALID on a handle without a ready hierarchy (a network the dense route took),
    the size alone for dst == NULL, NODAL_E_INVALID for a destination that is too small, a level or an array that does
    not exist; two exports in a row have the same bits and leave solution and residual where they were."""
    import ctypes as C
    h = _ffi.Handle(0)
    h.upload(shapes.gen.grid_table(20))
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    assert h.solve_sparse()[1] == 0
    with pytest.raises(_ffi.NodalHipError) as exc:
        h.debug_hierarchy()
    assert exc.value.status == _ffi.E_INVALID
    h.close()
    h, (levels,) = shapes.solve_and_export(shapes.grid3d())
    x, resid = h.download_x().copy(), h.residual()
    again = h.debug_hierarchy()
    for a, b in zip(levels, again):
        assert all(same_bytes(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)
    assert same_bytes(h.download_x(), x) and h.residual() == resid
    size = C.c_int64(-1)
    call = h.lib.nodal_debug_hierarchy_array
    assert call(h._h, 0, 1, None, 0, C.byref(size)) == _ffi.OK
    assert size.value == levels[0]["width"] * levels[0]["ld"] * 8 == levels[0]["aval"].nbytes
    small = np.empty(8)
    assert call(h._h, 0, 1, C.c_void_p(small.ctypes.data), small.nbytes, C.byref(size)) == _ffi.E_INVALID
    assert call(h._h, len(levels), 1, None, 0, C.byref(size)) == _ffi.E_INVALID
    assert call(h._h, 0, len(_ffi.HIERARCHY_ARRAYS), None, 0, C.byref(size)) == _ffi.E_INVALID
    last = len(levels) - 1
    for which, (name, _) in enumerate(_ffi.HIERARCHY_ARRAYS):  # (a last level has its matrix and nothing else)
        assert call(h._h, last, which, None, 0, C.byref(size)) == _ffi.OK
        assert (size.value > 0) == (name in ("acol", "aval", "avalf", "alen", "dinv")), name
    h.close()


def test_row_loop_and_small_groups():
    """NODAL_SA_GCAP=64 NODAL_SA_GG=8 (latched per process: tests/hierarchy_child.py): 64 Galerkin workgroups walk all
    coarse rows -- the loop the 1e6-node grid takes -- and level-0 rows of R need several groups of eight entries."""
    env = dict(os.environ, NODAL_SA_GCAP="64", NODAL_SA_GG="8")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "hierarchy_child.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-500:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert any(line.startswith("hierarchy child ok ") for line in r.stdout.splitlines()), r.stdout[-2000:]
