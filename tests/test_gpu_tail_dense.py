"""The multigrid tail as one precomputed dense operator (csrc/sagg_cycle.h: k_tail_pack_op forms T = the tail cycle
applied to the unit vectors once per setup, k_tail_apply computes T rc per visit) against the kernel that walks the
cycle on every visit (k_tail, NODAL_SA_TAIL_DENSE=0).  The switch is read once per process: a child per setting
(tests/tail_dense_child.py) solves every shape; reference call replaced: nodal/nodal.py:325, whose answer does not
depend on how a preconditioner is applied."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# shape -> the tail it is here for (level sizes of the CPU prototype, tools/sa_proto.py; the device's differ in detail)
SHAPES = {
    "grid400": "a small tail (n_t ~ 69) under flexible CG",
    "grid300": "a large tail (n_t ~ 816: four rounds of the forming launch) under flexible CG",
    "cfg5_300": "the presolved FGMRES",
    "batch16x60": "sixteen members as one block-diagonal system (on the device its last level has 45 rows: dense inverse)",
    "batch100x24": "a hundred members: more than 64 rows at one node per member, the last level is their diagonal",
    "pairs32_grid300": "the block iteration: sixteen interleaved right-hand sides per application",
}
CHECK = re.compile(r"\[sagg\] tail check: n_t (\d+), dense operator against the cycle d = (\S+) \(product alone (\S+)\)")
BLOCK = re.compile(r"\[sagg\] block of \d+ \w+: (\d+) iterations")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Both settings, every shape: {setting: {shape: (info, iterations, solution, trace lines)}}"""
    out = {}
    for name, extra in (("dense", {"NODAL_SA_TAIL_DENSE": "1"}), ("cycle", {"NODAL_SA_TAIL_DENSE": "0"})):
        d = str(tmp_path_factory.mktemp(name))
        env = dict(os.environ, NODAL_TRACE="1", NODAL_SA_TAIL_CHECK="1", **extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tail_dense_child.py"), d] + list(SHAPES), env=env,
                           cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "tail dense child ok" in r.stdout, (name, r.stdout[-2000:], r.stderr[-2000:])
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


@pytest.mark.parametrize("shape", list(SHAPES))
def test_dense_tail_operator_matches_the_cycle(runs, shape):
    """Per shape, T applied (default) against the cycle walked (NODAL_SA_TAIL_DENSE=0): info 0 both ways, outer
    iteration counts within one, solutions within 1e-10 x the largest entry -- the bar of
    test_frozen_kcycle_coefficients_keep_the_iteration_count for a schedule change that is not bit-exact.  The shape
    must HAVE a tail: the setup's self-check line (NODAL_TRACE with NODAL_SA_TAIL_CHECK=1; no tail, no line) is there, and
    its figure d = max_i |y_dense - y_cycle|_i / sum_j |T_ij| |b_j| for a fixed vector b of both signs satisfies
    d <= 64 n_t 2^-53: the bound gamma_n ~ n u of an n-term fp64 dot product against sum |T_ij| |b_j|, times 64 as an
    allowance for the rounding that the cycle and the columns of T carry.  The dense product alone, against the same
    product in long double on the host, must meet 2 n_t 2^-53 (gamma_n with room for the reference's own rounding).

    Measured on MI355X (n_t on the device, d, product alone; bound on d at that n_t):
      grid400          75   6.1e-17   3.3e-17   (5.3e-13)
      grid300         796   3.5e-17   2.7e-17   (5.7e-12)
      cfg5_300        796   3.0e-16   1.7e-16   (5.7e-12)
      batch16x60      558   1.7e-16   1.2e-16   (4.0e-12; its last level has 45 coupled rows: dense inverse)
      batch100x24     714   4.2e-16   1.7e-16   (5.1e-12; last level: the isolated nodes' diagonal)
      pairs32_grid300 796   3.5e-17   2.7e-17   (5.7e-12)
    Iteration counts were equal in every shape (20 / 18 / 17 / 20 / 20 / 8 + 8) and every solution but the pair sweep's
    bit-identical (the cycle's vectors above the tail are f32); the pair sweep's differed by 1.1e-16 of its largest."""
    dense, cycle = runs["dense"][shape], runs["cycle"][shape]
    checks = [m for m in map(CHECK.search, dense[3]) if m]
    print(shape, "dense", dense[:2], "cycle", cycle[:2], "checks", [m.groups() for m in checks])
    assert checks, (shape, "no tail on this shape", dense[3][-5:])
    if shape == "batch100x24":  # (the shape that is here for the tail's `d.inv == nullptr` branch)
        assert any("coarsest diagonal" in line for line in dense[3]), dense[3][-5:]
    assert not any(CHECK.search(line) for line in cycle[3])  # (the other setting really is the other path)
    for m in checks:
        n_t, d, dp = int(m.group(1)), float(m.group(2)), float(m.group(3))
        assert d <= 64 * n_t * 2.0 ** -53, (shape, n_t, d)
        assert dp <= 2 * n_t * 2.0 ** -53, (shape, n_t, dp)
    assert dense[0] == 0 and cycle[0] == 0
    assert dense[1] and len(dense[1]) == len(cycle[1]), (dense[1], cycle[1])
    for a, b in zip(dense[1], cycle[1]):
        assert abs(a - b) <= 1, (shape, dense[1], cycle[1])
    scale = np.abs(cycle[2]).max()
    err = np.abs(dense[2] - cycle[2]).max()
    print(shape, "difference", err / scale)
    assert err <= 1e-10 * scale, (shape, err, scale)
