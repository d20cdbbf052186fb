"""The level directly above the dense tail visited in three launches (csrc/sagg_cycle.h: k_visit_first / _second /
_last; csrc/sagg.hip: p2_rows_wave, d2_scatter, build_visit) against the six launches it replaces
(NODAL_SA_FOLD_VISIT=0).  The switches are read once per process: a child per setting (tests/fold_visit_child.py)
solves every shape; the identities themselves in fp64: tests/test_fold_visit_identity.py.

Shapes.  The production sweep counts give level 1 one sweep per side, so the path needs a fourth level above 1024 rows:
the random-valued grid(400) (160 k -> 23 k -> 1.4 k -> tail) is the smallest such shape; the random-valued 100 x 100
grid under NODAL_SA_NU=222 reaches it at its 1458-row level 1.  Disqualified: config 5 on a 100 x 100 grid under the
same sweep counts (the general route: A != A^T) and the 100 x 100 grid with the byte cap of the dense P2^T forced below
its 524 KB (NODAL_SA_VISIT_CAP=1000); both against the oracle.

Measured on MI355X (the level, its rows / n_t / longest P2 row, the self-check's d and d over its bound 2^-23,
iterations with the three launches / with the six, difference of the solutions over the largest entry):
  grid100_222   level 1  1458 / 89 / 12   d 1.4e-10 (0.0012)   19 / 19
  grid400       level 2  1429 / 67 / 13   d 1.8e-10 (0.0015)   21 / 21
(d is small against 2^-24 because its denominator carries the coarse chain's absolute terms through |T|.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from tests import hierarchy_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLDING = ["grid100_222", "grid400"]
RUNS = {  # setting: (environment, shapes)
    "fold": ({}, FOLDING + ["refresh100_222", "cfg5_100_222"]),
    "off": ({"NODAL_SA_FOLD_VISIT": "0"}, FOLDING),
    "cap": ({"NODAL_SA_VISIT_CAP": "1000"}, ["grid100_222"]),
    "poison": ({"NODAL_POISON": "2"}, FOLDING + ["refresh100_222"]),
}
VISIT = re.compile(r"\[sagg\] level (\d+) \((\d+) rows\): visit in three launches")
CHECK = re.compile(r"\[sagg\] visit check: level (\d+), rows (\d+), n_t (\d+), longest P2 row (\d+), three launches against "
                   r"the six d = (\S+) \(against the bound 2\^-23: (\S+)\)")
P2CAP = 64
U = 2.0 ** -52


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: {shape: (info, iterations per solve, solution, trace lines, [exported arrays per solve])}}"""
    out = {}
    for name, (extra, shapes) in RUNS.items():
        d = str(tmp_path_factory.mktemp(name))
        env = dict(os.environ, NODAL_TRACE="1", NODAL_SA_VISIT_CHECK="1", **extra)
        for k in ("NODAL_SA_FOLD_VISIT", "NODAL_SA_VISIT_CAP", "NODAL_POISON", "NODAL_SA_NU", "NODAL_SA_FOLD_POST"):
            if k not in extra:
                env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fold_visit_child.py"), d] + shapes, env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "fold visit child ok" in r.stdout, (name, r.stdout[-2000:], r.stderr[-2000:])
        out[name] = collect(d, r.stdout, r.stderr)
        assert set(out[name]) == set(shapes), (name, r.stdout[-2000:])
    return out


def collect(d, stdout, stderr):
    trace, cur = {}, None
    for line in stderr.splitlines():
        if line.startswith("SHAPE "):
            cur = line.split()[1]
        elif cur is not None:
            trace.setdefault(cur, []).append(line)
    res = {}
    for line in stdout.splitlines():
        if line.startswith("RESULT "):
            _, shape, info, its = line.split()
            its = [int(i) for i in its.split(",")]
            exports = [dict(np.load(os.path.join(d, f"{shape}.{k}.npz"))) for k in range(len(its))]
            res[shape] = (int(info), its, np.load(os.path.join(d, shape + ".npy")), trace.get(shape, []), exports)
    return res


# ---- the exported operators ---------------------------------------------------------------------------------------------
def ell_csr(col, val, length, ld, slots, n, nc):
    """A column-major ELL operator's first `length[i]` slots per row as CSR (f64), entries in slot order."""
    c, v = ref.ell(col, ld, slots, n), ref.ell(val, ld, slots, n)
    vt = (np.arange(slots)[:, None] < length[None, :]).T
    rows = np.broadcast_to(np.arange(n), (slots, n)).T[vt]
    return sp.csr_matrix((v.T[vt].astype(np.float64), (rows, c.T[vt].astype(np.int64))), shape=(n, nc))


def check_p2(lv):
    """P2 against W - w D^-1 (A W) in fp64 from the exported A, dinv and W: the row's column set is the pattern of
    (I + 1_A) 1_W, every value within one f32 ulp of the reference plus (N + 3) u (|W| + w dinv |A||W|), N the entry's
    number of products (the bound of W itself, tests/hierarchy_reference.py).  Returns the largest error / bound."""
    n, ld, nc, wslots = (int(lv[k]) for k in ("n", "ld", "nc", "wslots"))
    lv = dict(lv, n=n, ld=ld, maxlen=int(lv["maxlen"]))
    A = ref.csr_of_level(lv)
    wlen, p2len = lv["wlen"][:n], lv["p2len"][:n]
    assert ((p2len >= 0) & (p2len <= P2CAP)).all()
    W = ell_csr(lv["wcol"], lv["wval"], wlen, ld, wslots, n, nc)
    P2 = ell_csr(lv["p2col"], lv["p2val"], p2len, ld, P2CAP, n, nc)
    assert P2.indices.min() >= 0 and P2.indices.max() < nc
    assert (np.diff(ref._sorted(P2).indptr) == p2len).all()  # (no column twice in a row: the sum keeps every entry)
    ones = ref._sorted(ref._ones(A) @ ref._ones(W) + ref._ones(W))
    assert np.array_equal(np.diff(ones.indptr), p2len), "row lengths are not those of (I + 1_A) 1_W"
    dev = ref._sorted(P2)
    assert np.array_equal(dev.indices, ones.indices), "columns are not those of (I + 1_A) 1_W"
    wd = sp.diags(float(lv["omega"]) * lv["dinv"][:n])
    want = ref._on_pattern(W - wd @ (A @ W), ones)
    absb = ref._on_pattern(abs(W) + wd @ (abs(A) @ abs(W)), ones)
    bound = 2.0 ** -23 * np.abs(want) + (ones.data + 3) * U * absb
    err = np.abs(dev.data - want)
    ratio = err / np.maximum(bound, 1e-300)
    assert (err <= bound).all(), float(ratio.max())
    return float(ratio.max())


def check_d2(lv):
    """d2 is the scatter of P2, bit for bit, zeros everywhere else (the columns n .. ld included)."""
    n, ld, nc = (int(lv[k]) for k in ("n", "ld", "nc"))
    col, val = ref.ell(lv["p2col"], ld, P2CAP, n), ref.ell(lv["p2val"], ld, P2CAP, n)
    valid = np.arange(P2CAP)[:, None] < lv["p2len"][:n][None, :]
    want = np.zeros((nc, ld), dtype=np.float32)
    rows = np.broadcast_to(np.arange(n), (P2CAP, n))
    want[col[valid], rows[valid]] = val[valid]
    assert lv["d2"].dtype == np.float32 and lv["d2"].size == nc * ld
    assert same_bytes(lv["d2"].reshape(nc, ld), want)


def visit_export(run, solve=0):
    lv = run[4][solve]
    assert int(lv["level"]) >= 1, ("no level exports P2", lv["sizes"])
    return lv


@pytest.mark.parametrize("shape", FOLDING)
def test_the_level_above_the_tail_folds(runs, shape):
    """From the trace: the fold is reported for exactly one level >= 1 of more than 1024 rows, its self-check line is
    there, and neither line appears with NODAL_SA_FOLD_VISIT=0 (which exports no P2 either)."""
    fold, off = runs["fold"][shape], runs["off"][shape]
    said = [m for m in map(VISIT.search, fold[3]) if m]
    assert len(said) == 1 and int(said[0].group(1)) >= 1 and int(said[0].group(2)) > 1024, (shape, fold[3][-6:])
    lv = visit_export(fold)
    assert int(lv["level"]) == int(said[0].group(1)) and int(lv["n"]) == int(said[0].group(2)) and int(lv["fold"]) == 1
    assert not any(VISIT.search(line) or CHECK.search(line) for line in off[3])
    assert int(off[4][0]["level"]) == -1


@pytest.mark.parametrize("shape", FOLDING)
def test_exported_p2_and_its_dense_transpose(runs, shape):
    lv = visit_export(runs["fold"][shape])
    worst = check_p2(lv)
    check_d2(lv)
    print(shape, "level", int(lv["level"]), "rows", int(lv["n"]), "n_t", int(lv["nc"]), "longest P2 row", int(lv["p2len"].max()),
          "P2 error / bound", worst)


@pytest.mark.parametrize("shape", FOLDING)
def test_self_check_is_under_its_bound(runs, shape):
    """NODAL_TRACE with NODAL_SA_VISIT_CHECK=1: d = max_i |out_3 - out_6|_i over the row's sum of the absolute terms
    that carry one f32 rounding each; the derivation next to visit_check_level (csrc/sagg_checks.h) gives d <= 2^-24 to first
    order and 2^-23 as the bound, whatever the slot counts (every sum is fp64)."""
    checks = [m for m in map(CHECK.search, runs["fold"][shape][3]) if m]
    assert checks, runs["fold"][shape][3][-6:]
    for m in checks:
        d, q = float(m.group(5)), float(m.group(6))
        print(shape, m.groups())
        assert int(m.group(4)) <= P2CAP
        assert d <= 2.0 ** -23 and q <= 1.0, (shape, m.groups())  # (a NaN fails both)


@pytest.mark.parametrize("shape", FOLDING)
def test_three_launches_against_six(runs, shape):
    """The same iteration count, the same info, and x within 1e-10 of its largest entry (the --dump-outputs bar)."""
    fold, off = runs["fold"][shape], runs["off"][shape]
    assert fold[0] == 0 and off[0] == 0
    assert fold[1] == off[1], (shape, fold[1], off[1])
    scale = np.abs(off[2]).max()
    err = np.abs(fold[2] - off[2]).max()
    print(shape, "iterations", fold[1], off[1], "difference", err / scale)
    assert err <= 1e-10 * scale, (shape, err, scale)


def test_values_only_refresh(runs):
    """Three members on one handle, the third the first again: the refreshes rebuild P2 and d2 on the kept pattern; the
    export after the third has the bits of the first, the second has the pattern with other values and passes the
    reference for ITS matrix."""
    first, second, third = (visit_export(runs["fold"]["refresh100_222"], k) for k in range(3))
    assert int(first["refreshed"]) == 0 and int(second["refreshed"]) == 1 and int(third["refreshed"]) == 1
    n, ld = int(first["n"]), int(first["ld"])
    valid = np.arange(P2CAP)[:, None] < first["p2len"][:n][None, :]
    for name in ("p2len", "d2"):
        assert same_bytes(first[name], third[name]), name
    assert same_bytes(first["p2len"], second["p2len"])
    for name in ("p2col", "p2val"):
        a, b, c = (ref.ell(x[name], ld, P2CAP, n)[valid] for x in (first, second, third))
        assert same_bytes(a, c), name
        assert same_bytes(a, b) == (name == "p2col"), name  # (the pattern stays, the values did move)
    assert not same_bytes(first["d2"], second["d2"])
    print("refreshed: P2 error / bound", check_p2(second))
    check_d2(second)
    check_d2(third)


def oracle_error(table, x):
    from oracle import nodal_oracle as oracle
    Go, Ao = oracle.assemble_fast(table)
    xo, _ = oracle.solve(Go.tocsr(), Ao, True)
    return np.abs(x - xo).max() / np.abs(xo).max()


@pytest.mark.parametrize("setting,shape", [("fold", "cfg5_100_222"), ("cap", "grid100_222")])
def test_disqualified_levels_keep_their_six_launches(runs, setting, shape):
    """Config 5 (the general route: rc = P2^T b needs A = A^T) and a dense P2^T over the byte cap: the level does not
    fold, nothing is built or exported, and the solve agrees with the oracle (1e-9 of the largest entry, the bar of
    smoke())."""
    from tests import fold_visit_child as child
    run = runs[setting][shape]
    assert run[0] == 0
    assert not any(VISIT.search(line) or CHECK.search(line) for line in run[3]), run[3][-6:]
    assert int(run[4][0]["level"]) == -1
    sizes = run[4][0]["sizes"]
    assert len(sizes) >= 3 and sizes[1] > 1024 and sizes[2] <= 1024, sizes  # (level 1 IS directly above the tail)
    err = oracle_error(child.SHAPES[shape]()[0], run[2])
    print(setting, shape, "levels", list(sizes), "against the oracle", err)
    assert err <= 1e-9, err


@pytest.mark.parametrize("shape", FOLDING + ["refresh100_222"])
def test_poisoned_buffers_change_nothing(runs, shape):
    """The child once more under NODAL_POISON=2 (growing buffers start as 0xFF bytes, the scratch buffers are poisoned
    again at every solve entry): nothing the new kernels read may be a slot nobody wrote -- the same folds, iteration
    counts and bound, P2's valid slots and all of d2 bit for bit, the solutions within 1e-10."""
    clean, dirty = runs["fold"][shape], runs["poison"][shape]
    assert dirty[0] == 0 and dirty[1] == clean[1], (dirty[:2], clean[:2])
    scale = np.abs(clean[2]).max()
    assert np.abs(dirty[2] - clean[2]).max() <= 1e-10 * scale
    for m in (m for m in map(CHECK.search, dirty[3]) if m):
        assert float(m.group(6)) <= 1.0, m.groups()
    for a, b in zip(clean[4], dirty[4]):
        n, ld = int(a["n"]), int(a["ld"])
        assert int(a["level"]) == int(b["level"]) >= 1
        valid = np.arange(P2CAP)[:, None] < a["p2len"][:n][None, :]
        assert same_bytes(a["p2len"][:n], b["p2len"][:n]) and same_bytes(a["d2"], b["d2"])
        for name in ("p2col", "p2val"):
            assert same_bytes(ref.ell(a[name], ld, P2CAP, n)[valid], ref.ell(b[name], ld, P2CAP, n)[valid]), name
