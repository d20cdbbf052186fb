"""A level with one sweep per side forms its residual and its restricted residual rc = W^T b in one launch
(csrc/sagg_cycle.h: k_residual_restrict; csrc/sagg.hip: build_wt, wt_pack, wt_refresh, decide_folds) instead of
k_smooth_residual + k_restrict (NODAL_SA_RESTRICT_B=0).  The switches are read once per process: a child per setting
(tests/restrict_from_b_child.py) solves every shape; the identity itself in fp64: tests/test_restrict_from_b_identity.py.

Shapes, the smallest that reach each form:
  grid100       random-valued 100 x 100 grid, default sweeps: level 1 (1458 rows) is chosen, its coarse level is the tail:
                rc in f64, no x0c
  grid400       random-valued 400 x 400 grid (160 k -> 23 k -> 1.4 k -> tail): level 1 (23 k rows) is chosen: rc in f32
                with x0c, feeding the three-launch visit of level 2
  cfg5_100      config 5 on a 100 x 100 grid: the general route (A != A^T): no level may be chosen
  grid100_222   NODAL_SA_NU=222: no level has one sweep: no level may be chosen
  refresh100    three members on one handle through the values-only refresh, the third the first again

Measured on MI355X (the chosen level's rows / coarse rows / entries of W^T / longest coarse row; the self-check's d and
d over its bound 2^-23; iterations from b / with the two launches; largest error against the oracle):
  grid100      1458 /   89 /   6 948 / 115   d 6.1e-9 (0.051)   19 / 19   6.6e-14
  grid400    22 746 / 1429 / 120 196 / 130   d 1.9e-8 (0.163)   21 / 21   2.8e-13
  refresh100 members 19 / 20 / 19 iterations, d 6.1e-9 / 6.9e-9 / 6.1e-9; the same figures under NODAL_POISON=2."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHOSEN_SHAPES = ["grid100", "grid400"]
RUNS = {  # setting: (environment, shapes)
    "on": ({}, CHOSEN_SHAPES + ["cfg5_100", "grid100_222", "refresh100"]),
    "off": ({"NODAL_SA_RESTRICT_B": "0"}, CHOSEN_SHAPES),
    "poison": ({"NODAL_POISON": "2"}, CHOSEN_SHAPES + ["refresh100"]),
}
CHOSEN = re.compile(r"\[sagg\] level (\d+) \((\d+) rows\): restriction from b beside the residual launch")
ANY = re.compile(r"\[sagg\] level \d+ \(\d+ rows\): restriction ")
CHECK = re.compile(r"\[sagg\] restrict check: level (\d+), rows (\d+), coarse rows (\d+), rc from b against the two launches "
                   r"d = (\S+) \(against the bound 2\^-23: (\S+)\)")


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{setting: {shape: dict(info, its, xs, again, trace, exports)}}"""
    out = {}
    for name, (extra, shapes) in RUNS.items():
        d = str(tmp_path_factory.mktemp(name))
        env = dict(os.environ, NODAL_TRACE="1", NODAL_SA_RESTRICT_CHECK="1", **extra)
        for k in ("NODAL_SA_RESTRICT_B", "NODAL_POISON", "NODAL_SA_NU", "NODAL_SA_FOLD_POST", "NODAL_SA_FOLD_VISIT",
                  "NODAL_SA_FORK"):
            if k not in extra:
                env.pop(k, None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "restrict_from_b_child.py"), d] + shapes, env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "restrict from b child ok" in r.stdout, (name, r.stdout[-2000:], r.stderr[-2000:])
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
            again = os.path.join(d, f"{shape}.again.npy")
            res[shape] = dict(info=int(info), its=its, trace=trace.get(shape, []),
                              xs=[np.load(os.path.join(d, f"{shape}.{k}.npy")) for k in range(len(its))],
                              again=np.load(again) if os.path.exists(again) else None,
                              exports=[dict(np.load(os.path.join(d, f"{shape}.{k}.npz"))) for k in range(len(its))])
    return res


@pytest.fixture(scope="module")
def oracle_solutions():
    """The oracle's solution per network, computed once: {shape: [x per member]}."""
    from oracle import nodal_oracle as oracle
    from tests import restrict_from_b_child as child

    def solve(table):
        Go, Ao = oracle.assemble_fast(table)
        return oracle.solve(Go.tocsr(), Ao, True)[0]

    out = {}
    for shape in ("grid100", "grid400", "cfg5_100"):
        out[shape] = [solve(child.SHAPES[shape]()[0])]
    out["grid100_222"] = out["grid100"]
    table, members = child.fv.refresh_members()  # (member 0 is the table's own values, member 2 the same again)
    table.value[:] = members[1]
    out["refresh100"] = [out["grid100"][0], solve(table), out["grid100"][0]]
    return out


def level_arrays(export, l):
    names = ("wcol", "wval", "wlen", "wtstart", "wtcol", "wtval", "wtsrc", "n", "ld", "nc", "wslots", "fold", "refreshed")
    return {k: export[f"{k}{l}"] for k in names}


def check_transpose(lv):
    """W^T as exported is the transpose of W as exported, bit for bit: consistent row starts, every entry names a slot of
    W below its row's length whose column is the entry's coarse row and whose value has the entry's bits, no slot twice,
    as many entries as W has, fine rows ascending within a coarse row."""
    n, ld, nc, wslots = (int(lv[k]) for k in ("n", "ld", "nc", "wslots"))
    start = lv["wtstart"].astype(np.int64)
    assert start.shape == (nc + 1,) and start[0] == 0 and (np.diff(start) >= 0).all()
    total = int(start[nc])
    wlen = lv["wlen"][:n].astype(np.int64)
    assert total == int(wlen.sum()) and total <= len(lv["wtcol"])
    col, val, src = lv["wtcol"][:total].astype(np.int64), lv["wtval"][:total], lv["wtsrc"][:total].astype(np.int64)
    coarse = np.repeat(np.arange(nc), np.diff(start))
    slot, fine = src // ld, src % ld
    assert (fine == col).all() and (col >= 0).all() and (col < n).all()
    assert (slot >= 0).all() and (slot < wlen[col]).all() and slot.max() < wslots
    assert len(np.unique(src)) == total  # (with the count above: every entry of W exactly once)
    assert np.array_equal(lv["wcol"][src].astype(np.int64), coarse)
    assert same_bytes(lv["wval"][src], val)
    inner = np.ones(total, dtype=bool)
    inner[start[:-1][np.diff(start) > 0]] = False  # (the first entry of every row has no predecessor)
    assert (np.diff(col)[inner[1:]] > 0).all(), "fine rows do not ascend within a coarse row"
    return total, int(np.diff(start).max())


@pytest.mark.parametrize("shape", CHOSEN_SHAPES)
def test_exactly_level_one_is_chosen(runs, shape):
    on, off = runs["on"][shape], runs["off"][shape]
    said = [m for m in map(CHOSEN.search, on["trace"]) if m]
    sizes = on["exports"][0]["sizes"]
    assert len(said) == 1 and int(said[0].group(1)) == 1 and int(said[0].group(2)) == sizes[1], (shape, on["trace"][-8:])
    assert len([line for line in on["trace"] if ANY.search(line)]) == 1
    assert list(on["exports"][0]["levels"]) == [1]
    assert not any(ANY.search(line) or CHECK.search(line) for line in off["trace"])
    assert len(off["exports"][0]["levels"]) == 0
    if shape == "grid100":
        assert len(sizes) >= 3 and sizes[1] > 1024 and sizes[2] <= 1024, sizes  # (rc goes to the tail: the f64 form)
    else:
        assert len(sizes) >= 4 and sizes[2] > 1024, sizes  # (rc and x0c go to a level of the cycle: the f32 form)


@pytest.mark.parametrize("shape", ["cfg5_100", "grid100_222"])
def test_disqualified_shapes_keep_their_two_launches(runs, oracle_solutions, shape):
    """The general route (rc = W^T b needs A = A^T) and a hierarchy without a one-sweep level: nothing is chosen, built
    or exported, and the solution agrees with the oracle."""
    run = runs["on"][shape]
    assert run["info"] == 0
    assert not any(ANY.search(line) or CHECK.search(line) for line in run["trace"]), run["trace"][-8:]
    assert len(run["exports"][0]["levels"]) == 0 and len(run["exports"][0]["sizes"]) >= 2
    xo = oracle_solutions[shape][0]
    err = np.abs(run["xs"][0] - xo).max() / np.abs(xo).max()
    print(shape, "levels", list(run["exports"][0]["sizes"]), "against the oracle", err)
    assert err <= 1e-9, err


@pytest.mark.parametrize("shape", CHOSEN_SHAPES)
def test_exported_transpose_of_w(runs, shape):
    lv = level_arrays(runs["on"][shape]["exports"][0], 1)
    assert int(lv["fold"]) == 1
    total, longest = check_transpose(lv)
    print(shape, "rows", int(lv["n"]), "coarse rows", int(lv["nc"]), "entries", total, "longest coarse row", longest)
    assert longest <= 512  # (the per-row sort's cap)


def test_values_only_refresh(runs):
    """Three members on one handle, the third the first again: after every refresh W^T is the transpose of the refreshed
    W; the pattern stays, the values move and come back."""
    first, second, third = (level_arrays(runs["on"]["refresh100"]["exports"][k], 1) for k in range(3))
    assert [int(x["refreshed"]) for x in (first, second, third)] == [0, 1, 1]
    for lv in (first, second, third):
        total, _ = check_transpose(lv)
    for name in ("wtstart", "wtcol", "wtsrc"):
        assert same_bytes(first[name][:total], second[name][:total]) and same_bytes(first[name][:total], third[name][:total]), name
    assert same_bytes(first["wtval"][:total], third["wtval"][:total])
    assert not same_bytes(first["wtval"][:total], second["wtval"][:total])


@pytest.mark.parametrize("setting", ["on", "poison"])
@pytest.mark.parametrize("shape", CHOSEN_SHAPES + ["refresh100"])
def test_self_check_is_under_its_bound(runs, setting, shape):
    """NODAL_TRACE with NODAL_SA_RESTRICT_CHECK=1: d = max_I |rc_new - rc_old|_I over the coarse row's sum of absolute
    terms (derivation beside restrict_check_level, csrc/sagg_checks.h); one line per setup or refresh."""
    run = runs[setting][shape]
    checks = [m for m in map(CHECK.search, run["trace"]) if m]
    assert len(checks) == len(run["its"]), run["trace"][-8:]
    for m in checks:
        print(setting, shape, m.groups())
        assert int(m.group(1)) == 1
        assert float(m.group(4)) <= 2.0 ** -23 and float(m.group(5)) <= 1.0, m.groups()  # (a NaN fails both)


@pytest.mark.parametrize("setting,shape", [(setting, shape) for setting, (_, shapes) in RUNS.items() for shape in shapes
                                           if shape in CHOSEN_SHAPES + ["refresh100"]])
def test_solutions_against_the_oracle(runs, oracle_solutions, setting, shape):
    run = runs[setting][shape]
    assert run["info"] == 0
    for x, xo in zip(run["xs"], oracle_solutions[shape]):
        err = np.abs(x - xo).max() / np.abs(xo).max()
        print(setting, shape, "iterations", run["its"], "against the oracle", err)
        assert err <= 1e-9, err


@pytest.mark.parametrize("shape", CHOSEN_SHAPES)
def test_iteration_counts_with_and_without(runs, shape):
    on, off = runs["on"][shape], runs["off"][shape]
    print(shape, "iterations from b", on["its"], "two launches", off["its"])
    assert len(on["its"]) == len(off["its"])
    assert all(abs(a - b) <= 1 for a, b in zip(on["its"], off["its"])), (on["its"], off["its"])


@pytest.mark.parametrize("setting", ["on", "poison"])
@pytest.mark.parametrize("shape", CHOSEN_SHAPES)
def test_two_solves_give_the_same_bytes(runs, setting, shape):
    run = runs[setting][shape]
    assert run["again"] is not None and same_bytes(run["xs"][0], run["again"])


@pytest.mark.parametrize("shape", CHOSEN_SHAPES + ["refresh100"])
def test_poisoned_buffers_change_nothing(runs, shape):
    """The child once more under NODAL_POISON=2 (growing buffers start as 0xFF bytes, scratch is poisoned again at every
    solve entry): the same level chosen, the same iteration counts, the same W^T bit for bit on the entries it has."""
    clean, dirty = runs["on"][shape], runs["poison"][shape]
    assert dirty["info"] == 0 and dirty["its"] == clean["its"], (dirty["its"], clean["its"])
    assert [bool(CHOSEN.search(line)) for line in dirty["trace"] if ANY.search(line)] == \
           [bool(CHOSEN.search(line)) for line in clean["trace"] if ANY.search(line)]
    for a, b in zip(clean["exports"], dirty["exports"]):
        assert list(a["levels"]) == list(b["levels"]) == [1]
        la, lb = level_arrays(a, 1), level_arrays(b, 1)
        total, _ = check_transpose(lb)
        for name in ("wtcol", "wtval", "wtsrc"):
            assert same_bytes(la[name][:total], lb[name][:total]), name
        assert same_bytes(la["wtstart"], lb["wtstart"])
