"""The Galerkin sums A_c = R (A P) with four small coarse rows per wavefront (NODAL_SA_GROWS) and with groups cut by the
products that fit the list (NODAL_SA_GDYN), looked at in the exported operators: tests/hierarchy_reference.py checks
every level in fp64 with its own bounds; this module adds the shapes that send rows down every path of the new kernel,
asserts on the exported arrays that they do, and holds the knob settings against each other in child processes (the
knobs are latched per process: tests/galerkin_rows_child.py).

A coarse row takes the shared path when it fits the capacities of nodal_amd/csrc/galerkin_groups.h (mirrored in
nodal_amd/_ffi.py): R entries, products, columns.  All three are functions of the exported level: the row's length in
R, the lengths of the rows of A P it names, the row's length in A_c."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from nodal_amd import _ffi
from tests import galerkin_rows_child as shapes
from tests import hierarchy_reference as ref
from tests.hierarchy_child import solve_and_export
from tests.hierarchy_reference import check_hierarchy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "galerkin_rows_child.py")
KNOBS = ("NODAL_SA_GROWS", "NODAL_SA_GDYN", "NODAL_SA_GCAP", "NODAL_SA_GG", "NODAL_SA_GLIST")
CHILD_SHAPES = ("chord10", "grid100")
SETTINGS = {"grows0": {"NODAL_SA_GROWS": "0"}, "gdyn0": {"NODAL_SA_GDYN": "0"},
            "both0": {"NODAL_SA_GROWS": "0", "NODAL_SA_GDYN": "0"}, "gcap64": {"NODAL_SA_GCAP": "64"},
            "gg8": {"NODAL_SA_GG": "8"}}


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def clean_env(extra=()):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def exported():
    """Every shape set up twice in this process, under the default knobs: {shape: (levels, levels of the second setup)}."""
    assert not any(k in os.environ for k in KNOBS), "these tests compare against the default knobs"
    out = {}
    for name, table in shapes.SHAPES.items():
        both = []
        for _ in range(2):
            h, (levels,) = solve_and_export(table())
            h.close()
            both.append(levels)
        out[name] = tuple(both)
    return out


def row_figures(levels, l):
    """Per coarse row of level l + 1: R entries, products (the lengths of the A P rows its R entries name), columns."""
    lv = levels[l]
    nc = lv["nc"]
    R, A, P = ref.check_R(l, lv), ref.csr_of_level(lv), ref.p_csr(lv)
    ap_len = np.diff((ref._ones(A) @ ref._ones(P)).indptr)
    entries = lv["rlen"][:nc].astype(np.int64)
    products = np.asarray(ref._ones(R) @ ap_len, dtype=np.int64)
    columns = levels[l + 1]["alen"][:nc].astype(np.int64)
    return entries, products, columns


def fits_shared(entries, products, columns):
    return ((entries <= _ffi.GALERKIN_SUB_ENTRIES) & (products <= _ffi.GALERKIN_SUB_PRODUCTS) &
            (columns <= _ffi.GALERKIN_SUB_COLUMNS))


@pytest.mark.parametrize("shape", list(shapes.SHAPES))
def test_every_level_matches_the_reference(exported, shape):
    stats = check_hierarchy(exported[shape][0])
    print(shape, ref.coverage(exported[shape][0])[1], {k: f"{v:.3g}" for k, v in stats.items()})


@pytest.mark.parametrize("shape", list(shapes.SHAPES))
def test_two_setups_give_the_same_bytes(exported, shape):
    first, second = exported[shape]
    assert len(first) == len(second)
    for l, (a, b) in enumerate(zip(first, second)):
        for name in shapes.MATRIX:
            assert same_bytes(a[name], b[name]), (l, name)


def test_the_chord_shapes_reach_every_path_of_the_shared_kernel(exported):
    """Level 0 of both chord shapes is a 16-slot level.  With 10 % chords: fours of consecutive coarse rows in which every
    row fits the sub-groups, in which some do, and in which none does; a last, partial four.  With 20 % chords most rows
    do not fit (30 % is declined on the device: galerkin_rows_child.chord20).  Over both: a row above each of the three
    capacities.  Seen on MI355X: chord10 525 coarse rows, R rows up to 33, up to 193 products and 44 columns, 57 % of
    the rows fit, fours 12 / 117 / 2; chord20 497 rows, up to 33 / 215 / 55, 16 % fit, fours 1 / 61 / 62."""
    over = np.zeros(3, dtype=bool)
    for name in ("chord10", "chord20"):
        levels = exported[name][0]
        assert levels[0]["maxlen"] <= 6, levels[0]["maxlen"]
        entries, products, columns = row_figures(levels, 0)
        fits = fits_shared(entries, products, columns)
        nc = len(fits)
        full = fits[:nc // 4 * 4].reshape(-1, 4).sum(axis=1)
        print(name, "coarse rows", nc, "R entries <=", entries.max(), "products <=", products.max(), "columns <=",
              columns.max(), "rows that fit", int(fits.sum()), "fours all / mixed / none",
              int((full == 4).sum()), int(((full > 0) & (full < 4)).sum()), int((full == 0).sum()))
        over |= np.array([(entries > _ffi.GALERKIN_SUB_ENTRIES).any(), (products > _ffi.GALERKIN_SUB_PRODUCTS).any(),
                          (columns > _ffi.GALERKIN_SUB_COLUMNS).any()])
        assert columns.max() <= 64  # (under the row cap: the hierarchy is not declined)
        if name == "chord10":
            assert nc % 4 != 0, nc
            assert (full == 4).any() and ((full > 0) & (full < 4)).any() and (full == 0).any(), np.bincount(full)
        else:
            assert fits.mean() < 0.5, fits.mean()
    assert over.all(), over


def test_the_grids_reach_the_run_time_groups(exported):
    """grid100: every level-0 row fits the shared path, and 64-slot levels below have rows of R of more than 16 entries
    whose products fit the list: one group where groups of 16 entries took several.  grid3d: level 0 is a 64-slot level
    (rows of seven), so the shared path stays out and the run-time groups are in."""
    levels = exported["grid100"][0]
    assert levels[0]["maxlen"] <= 6 and fits_shared(*row_figures(levels, 0)).all()
    assert exported["grid3d"][0][0]["maxlen"] > 6
    for name, first in (("grid100", 1), ("grid3d", 0)):
        levels = exported[name][0]
        one_group = 0
        for l in range(first, len(levels) - 1):
            assert levels[l]["maxlen"] > 6, (name, l)
            entries, products, _ = row_figures(levels, l)
            one_group += int(((entries > 16) & (entries <= 64) & (products <= _ffi.GALERKIN_DYN_PRODUCTS)).sum())
            print(name, "level", l, "R entries <=", entries.max(), "products <=", products.max())
        assert one_group > 0, name


def run_child(args, env):
    r = subprocess.run([sys.executable, CHILD, *args], env=clean_env(env), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_knob_settings_in_child_processes(exported, setting, tmp_path):
    """Every setting passes the reference (the child runs check_hierarchy itself).  NODAL_SA_GCAP=64: another grid, every
    byte the same.  Both knobs at 0: one coarse row per wavefront, fixed groups -- the same patterns, and values within
    twice the reference's Galerkin bound of the default's (each is within the bound of the exact product)."""
    out = str(tmp_path / "export.npz")
    report = run_child([out, *CHILD_SHAPES], SETTINGS[setting])
    print(setting, {s: (r["sizes"], {k: f"{v:.3g}" for k, v in r["stats"].items()}) for s, r in report.items()})
    got = np.load(out)
    for shape in CHILD_SHAPES:
        levels = exported[shape][0]
        if setting == "gcap64":
            for key, array in shapes.matrices(levels).items():
                assert same_bytes(got[f"{shape}/{key}"], array), (shape, key)
        if setting == "both0":
            for l, lv in enumerate(levels):
                for name in ("acol", "alen"):
                    assert same_bytes(got[f"{shape}/{l}/{name}"], lv[name]), (shape, l, name)
            # (a 16-slot level: the shared path sums in the order of the kernel of before, the same bytes come out)
            assert levels[0]["maxlen"] <= 6
            for name in shapes.MATRIX:
                assert same_bytes(got[f"{shape}/1/{name}"], levels[1][name]), (shape, name)
            for l in range(len(levels) - 1):
                lv, nxt = levels[l], levels[l + 1]
                R, A, P = ref.check_R(l, lv), ref.csr_of_level(lv), ref.p_csr(lv)
                cnt = ref._sorted(ref._ones(R) @ ref._ones(A) @ ref._ones(P))
                bound = (cnt.data + 3) * ref.U * ref._on_pattern(abs(R) @ abs(A) @ abs(P), cnt)
                other = dict(nxt, aval=got[f"{shape}/{l + 1}/aval"])
                diff = np.abs(ref.csr_of_level(nxt).data - ref.csr_of_level(other).data)
                print(shape, "level", l + 1, "largest difference / bound", float((diff / bound).max()))
                assert (diff <= 2.0 * bound).all(), (shape, l + 1)


def test_a_declined_hierarchy_is_declined_as_before():
    """grid(40) with a chord at every node, and grid(60) with chords over 30 % of the nodes: coarse rows above the row
    cap of 64 columns, no smoothed-aggregation hierarchy to export.  The same outcome, the same iterations and levels,
    and a residual of at most 1e-12, under the defaults and with both knobs at 0."""
    off = run_child(["declined"], SETTINGS["both0"])
    for name in shapes.DECLINED:
        here = list(shapes.solve_declined(name))
        print(name, "default", here, "both knobs 0", off[name])
        assert here[:3] == off[name][:3]
        assert here[3] <= 1e-12 and off[name][3] <= 1e-12
        assert here[0] == 0 and not here[4] and not off[name][4]


def test_values_only_refresh_on_the_chord_shape():
    """Three members on one handle, the third the first again (tests/test_gpu_hierarchy.py's refresh, on the shape with
    rows on both paths): every member passes the reference, and the third, a values-only refresh, has the bytes of the
    first, a fresh setup -- galerkin_rows<true> sends every row down the path galerkin_rows<false> sent it."""
    table = shapes.chord10()
    v0 = table.value.copy()
    v1 = v0.copy()
    v1[:-1] *= np.random.default_rng(611).uniform(0.5, 2.0, size=len(v0) - 1)
    h, (first, second, third) = solve_and_export(table, members=np.stack([v0, v1, v0]))
    h.close()
    assert first[0]["refreshed"] == 0 and second[0]["refreshed"] == 1 and third[0]["refreshed"] == 1
    for levels in (first, second, third):
        check_hierarchy(levels)
    assert not same_bytes(first[1]["aval"], second[1]["aval"])
    for l, (a, c) in enumerate(zip(first, third)):
        for name in shapes.MATRIX:
            assert same_bytes(a[name], c[name]), (l, name)
