"""The first post-smoothing sweep folded into the prolongation (csrc/sagg_cycle.h: k_prolong_post applies
W = P - w D^-1 (A P), which the setup writes beside A P) against the two launches it replaces (k_prolong + k_post,
NODAL_SA_FOLD_POST=0).  The switch is read once per process: a child per setting (tests/fold_post_child.py) solves
every shape; reference call replaced: nodal/nodal.py:325, whose answer does not depend on how a preconditioner is
applied."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["grid400", "grid300", "cfg5_300", "batch16x60", "batch100x24", "pairs32_grid300", "grid1000"]
FOLDED = re.compile(r"\[sagg\] level (\d+) \((\d+) rows\): first post-smoothing sweep folded into the prolongation")
CHECK = re.compile(r"\[sagg\] fold check: level (\d+), rows (\d+), slots (\d+), width (\d+), fused launch against the two "
                   r"d = (\S+) \(worst row against its own bound: (\S+)\)")
BLOCK = re.compile(r"\[sagg\] block of \d+ \w+: (\d+) iterations")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Both settings, every shape: {setting: {shape: (info, iterations, solution, trace lines)}}"""
    out = {}
    for name, extra in (("fold", {}), ("two", {"NODAL_SA_FOLD_POST": "0"})):
        d = str(tmp_path_factory.mktemp(name))
        env = dict(os.environ, NODAL_TRACE="1", NODAL_SA_FOLD_CHECK="1", **extra)
        if not extra:
            env.pop("NODAL_SA_FOLD_POST", None)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fold_post_child.py"), d] + SHAPES, env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "fold post child ok" in r.stdout, (name, r.stdout[-2000:], r.stderr[-2000:])
        trace = {}
        cur = None
        for line in r.stderr.splitlines():
            if line.startswith("SHAPE "):
                cur = line.split()[1]
            elif cur is not None:
                trace.setdefault(cur, []).append(line)
        res = {}
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                _, shape, info, its = line.split()
                lines = trace.get(shape, [])
                its = [int(m.group(1)) for m in map(BLOCK.search, lines) if m] if its == "-" else [int(i) for i in its.split(",")]
                res[shape] = (int(info), its, np.load(os.path.join(d, shape + ".npy")), lines)
        assert set(res) == set(SHAPES), (name, r.stdout[-2000:])
        out[name] = res
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_folded_post_sweep_matches_the_two_launches(runs, shape):
    """Per shape, the fold on (default) against NODAL_SA_FOLD_POST=0: info 0 both ways, outer iteration counts within
    one, solutions within 1e-10 x the largest entry -- the bars of
    test_frozen_kcycle_coefficients_keep_the_iteration_count for a schedule change that is not bit-exact.  Every level
    the setup reports as folded has its self-check line (NODAL_TRACE with NODAL_SA_FOLD_CHECK=1), no such line with the
    fold off, and the line's figures meet the bound: both forms take operands stored in f32 (matrix, W, P, the
    vectors) and sum in f64, so per row
        d_i = |m_fused - m_two|_i / (|x_i| + w dinv_i (|b_i| + sum_j |a_ij| |xp_j|) + sum_s |w_is| |e|)
            <= (slots_i + width_i + 8) 2^-23
    with the row's own slot count of W and length of A; the line carries max_i d_i and the largest d_i over its own
    bound, which must not exceed 1.

    Measured on MI355X (per folded level: rows, slots allocated / longest row of A, d, worst row against its own bound):
      grid400          0: 159999 16/5  8.6e-08 0.042    1: 22746 64/17 6.9e-08 0.026    2: 1457 64/26 6.3e-08 0.026
      grid300          0:  89999 16/5  7.4e-08 0.039    1: 12829 64/21 6.5e-08 0.024
      cfg5_300         0:  89999 16/5  7.4e-08 0.039    1: 12829 64/21 6.9e-08 0.023
      batch16x60       0:  57584 16/5  7.4e-08 0.037    1:  8416 64/19 6.5e-08 0.028
      batch100x24      0:  57500 16/5  7.8e-08 0.046    1:  8662 64/16 6.7e-08 0.030
      pairs32_grid300  0:  89999 16/5  7.4e-08 0.039    1: 12829 64/21 6.5e-08 0.024
      grid1000         1: 142283 64/18 9.0e-08 0.034    2:  8882 64/25 7.1e-08 0.022   (level 0: 999999 rows, not folded
                       by default; with NODAL_SA_FOLD_POST=1: 1.1e-07, 0.050)
    Iteration counts were equal in every shape (20 / 18 / 17 / 20 / 20 / 8 + 8 / 21); the solutions differed by 1.5e-14 /
    1.8e-15 / 5.8e-16 / 4.3e-14 / 1.3e-14 / 0 / 6.3e-15 of their largest entry (the pair sweep's blocks go through the
    block iteration, which does not fold)."""
    fold, two = runs["fold"][shape], runs["two"][shape]
    folded = [m for m in map(FOLDED.search, fold[3]) if m]
    checks = [m for m in map(CHECK.search, fold[3]) if m]
    print(shape, "fold", fold[:2], "two", two[:2], "folded", [m.groups() for m in folded], "checks", [m.groups() for m in checks])
    assert folded, (shape, "no level folds on this shape", fold[3][-5:])
    # (a values-only refresh repeats the check of the same levels: every folded level at least once, nothing else)
    assert {m.group(1) for m in checks} == {m.group(1) for m in folded}, (shape, fold[3][-8:])
    assert not any(CHECK.search(line) or FOLDED.search(line) for line in two[3])  # (the other setting really is the other path)
    for m in checks:
        rows, slots, width, d, q = int(m.group(2)), int(m.group(3)), int(m.group(4)), float(m.group(5)), float(m.group(6))
        assert rows > 0 and q <= 1.0, (shape, m.groups())
        assert d <= (slots + width + 8) * 2.0 ** -23, (shape, m.groups())
    assert fold[0] == 0 and two[0] == 0
    assert fold[1] and len(fold[1]) == len(two[1]), (fold[1], two[1])
    for a, b in zip(fold[1], two[1]):
        assert abs(a - b) <= 1, (shape, fold[1], two[1])
    scale = np.abs(two[2]).max()
    err = np.abs(fold[2] - two[2]).max()
    print(shape, "difference", err / scale)
    assert err <= 1e-10 * scale, (shape, err, scale)
