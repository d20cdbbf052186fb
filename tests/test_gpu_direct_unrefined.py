"""What the sparse direct route's kernels compute, before anything repairs it (through nodal_debug_direct_apply).

Every public entry point hands back the factors' answer AFTER a refinement (FGMRES to 1e-13 in sparse_direct_solve, one
step plus a redo-alone fallback in the sweeps), so factors or substitutions that are wrong at the 1e-6 level only cost
iterations.  The hook factors and applies once: z = U^-1 L^-1 r, nothing else.  Each column is judged on its own
against SciPy's SuperLU (splu, which does not refine either) of the oracle's matrix:

    scaled(z)  <=  16 * max(scaled(x_SuperLU), 2^-53),      scaled(x) = |Mx - b|_inf / (|M|_inf |x|_inf + |b|_inf)

with both residuals formed in np.longdouble (an fp64 `G @ x` rounds by as much as the quantity measured).  2^-53: no
solver is owed less than one unit roundoff.  16: the host emulation of the same algorithm (tools/slu_host_check.cpp)
stays within 2.5 of SuperLU on these tables; the device sums fronts and tiles in another order and multiplies by the
inverted lower triangles of its 32 x 32 diagonal blocks instead of substituting through them, a small constant factor,
where a defective kernel -- or one replaced pivot, about 1e-8 -- moves the figure by orders of magnitude.  Also: no
replaced pivots, info 0, and |z - x_SuperLU|_inf <= 1e-9 |x_SuperLU|_inf.

What it found when it was written: the backward sweep multiplied by inverted UPPER triangles too, and on the grids
over six decades that put the device at 10.3 (grid45_6dec) and 77.7 (grid140_6dec) times SuperLU's residual, every
other table below 1.7.  The sweep substitutes through U_bb since (csrc/sparse_direct.hip upper_block_solve); the worst
ratio of all cases is 2.19 now (profiles/direct_unrefined.json).

The tables (tests/direct_cases.py) put their widest front into every kernel regime of slu_factor / slu_apply_nr; the
variants switch each selectable form of those kernels on the smallest table that reaches it.  Knobs read once per
process go through tests/direct_unrefined_child.py, one child per setting, one at a time.

Every figure is printed before it is judged (`RATIO ...` lines: tools/direct_unrefined_record.py turns the output of
`pytest -s` into profiles/direct_unrefined.json)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from nodal_amd import _ffi
from oracle import nodal_oracle as oracle
from tests.direct_cases import (CASES, COLS, SINGLE, ZERO_COLUMN, apply_all, block_rhs, single_rhs, width_class)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FACTOR = 16.0
TOL = 1e-9  # north_star: 1e-9 rel-tol fp64, norm-wise
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "direct_unrefined_child.py")
L = np.longdouble


class Reference:
    """One table: the oracle's matrix, SuperLU of it (and of its transpose, on demand), and per right-hand side the
    unrefined SuperLU solution with its scaled residual -- each computed once."""

    def __init__(self, name):
        self.name = name
        self.table = CASES[name][0]()
        G, A = oracle.assemble_fast(self.table)
        self.A = np.asarray(A, dtype=np.float64).ravel()
        self.G = G.tocsr()
        self.n = self.G.shape[0]
        self.single, self.block = single_rhs(self.A), block_rhs(self.A)
        self._lu, self._csr, self._columns = {}, {}, {}

    def _matrix(self, transposed):
        if transposed not in self._csr:
            M = (self.G.T if transposed else self.G).tocsr()
            M.sort_indices()
            assert np.diff(M.indptr).min() >= 1  # (reduceat needs every row to hold an entry)
            data = M.data.astype(L)
            self._csr[transposed] = (M.indptr.astype(np.int64), M.indices.astype(np.int64), data,
                                     np.add.reduceat(np.abs(data), M.indptr[:-1].astype(np.int64)).max())
        return self._csr[transposed]

    def scaled(self, transposed, x, b):
        """|Mx - b|_inf / (|M|_inf |x|_inf + |b|_inf) in np.longdouble"""
        indptr, indices, data, an = self._matrix(transposed)
        xx, bb = np.asarray(x).astype(L), np.asarray(b).astype(L)
        r = np.add.reduceat(data * xx[indices], indptr[:-1]) - bb
        den = an * np.abs(xx).max() + np.abs(bb).max()
        return float(np.abs(r).max() / den) if den > 0 else 0.0

    def column(self, transposed, key, b):
        """(x_SuperLU, its scaled residual) for the right-hand side `key`"""
        if (transposed, key) not in self._columns:
            if transposed not in self._lu:
                self._lu[transposed] = spla.splu((self.G.T if transposed else self.G).tocsc())
            x = self._lu[transposed].solve(b)
            self._columns[(transposed, key)] = (x, self.scaled(transposed, x, b))
        return self._columns[(transposed, key)]


@pytest.fixture(scope="module")
def refs():
    kept = {}

    def get(name):
        if name not in kept:
            kept[name] = Reference(name)
        return kept[name]
    return get


def open_handle(table):
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    return h


def judge(ref, setting, z1, z16, verdicts, transposed=False):
    """Every column of a case against SuperLU's, each on its own; all figures are printed, then the failures raised."""
    label = f"{setting} | {ref.name} | {'G^T' if transposed else 'G'}"
    assert z1.shape == (len(SINGLE), ref.n) and z16.shape == (COLS, ref.n) and verdicts.shape == (len(SINGLE) + 1, 2)
    failures = []
    if verdicts.any():
        failures.append(f"(replaced pivots, info) of the four calls: {verdicts.tolist()}")
    columns = [(f"1:{SINGLE[k]}", ref.single[k], z1[k]) for k in range(len(SINGLE))]
    columns += [(f"16:{y}", ref.block[y], z16[y]) for y in range(COLS)]
    for key, b, z in columns:
        if not b.any():  # the all-zero column: exactly zero, not merely small
            assert key == f"16:{ZERO_COLUMN}"
            print(f"RATIO | {label} | {key} | zero column, max|z| = {np.abs(z).max():.3e}")
            if not (z == 0.0).all():
                failures.append(f"{key}: the all-zero column came back with max|z| = {np.abs(z).max():.3e}")
            continue
        if not np.isfinite(z).all():
            print(f"RATIO | {label} | {key} | not finite")
            failures.append(f"{key}: z is not finite")
            continue
        xo, so = ref.column(transposed, key, b)
        sd = ref.scaled(transposed, z, b)
        ratio = sd / max(so, U)
        err = np.abs(z - xo).max() / np.abs(xo).max()
        print(f"RATIO | {label} | {key} | device {sd:.3e} | SuperLU {so:.3e} | ratio {ratio:.3f} | normwise {err:.3e}")
        if not sd <= FACTOR * max(so, U):
            failures.append(f"{key}: scaled residual {sd:.3e} > 16 * max({so:.3e}, 2^-53) (ratio {ratio:.3g})")
        if not err <= TOL:
            failures.append(f"{key}: |z - x_SuperLU| / |x_SuperLU| = {err:.3e} > 1e-9")
    assert not failures, label + "\n  " + "\n  ".join(failures)


def largest_front(trace):
    m = re.search(r"largest front (\d+)", trace)
    assert m, trace[-600:]
    return int(m.group(1))


# ---- the default forms: every table, and the regime it was chosen for ----

@pytest.mark.parametrize("name", list(CASES))
def test_unrefined_factors_and_substitutions_match_superlu(name, refs, monkeypatch, capfd):
    ref = refs(name)
    monkeypatch.setenv("NODAL_TRACE", "1")
    h = open_handle(ref.table)
    capfd.readouterr()
    z1, z16, verdicts = apply_all(h, ref.A)
    trace = capfd.readouterr().err
    h.close()
    assert width_class(largest_front(trace)) == CASES[name][1], (name, largest_front(trace))
    judge(ref, "default", z1, z16, verdicts)


# ---- G^T through the adjoint's own child context: the same kernels on a structurally different matrix ----

@pytest.mark.parametrize("name", ["cfg5_48", "cfg5_90"])
def test_unrefined_transposed_factors_match_superlu_of_the_transpose(name, refs):
    ref = refs(name)
    h = open_handle(ref.table)
    _x, info, _it, _rr = h.solve_sparse()
    assert info == 0
    zero, minus = np.zeros(1, dtype=np.int32), np.full(1, -1, dtype=np.int32)
    _s, _y, _lam, _resid, sinfo = h.sensitivities(zero, zero, minus, dense=False)  # (one output: e(node 0))
    assert sinfo[0] == 0
    z1, z16, verdicts = apply_all(h, ref.A, transposed=True)
    h.close()
    judge(ref, "default", z1, z16, verdicts, transposed=True)


# ---- knobs read per call ----

SMALL_FRONTS = ["grid45_6dec", "cfg5_48", "tree3000", "ladder4000"]  # (grid45_6dec: interchanges inside small fronts)
CHAINS = ["grid60", "cfg5_90", "grid140_6dec"]  # per-front chains: panel_factor_regs, apply_swaps, trsm_u12, thin MFMA GEMM
CALL_SCOPE = [({"NODAL_DIRECT_WAVE": "0"}, SMALL_FRONTS),
              ({"NODAL_DIRECT_FRONT_LDS": "0"}, SMALL_FRONTS),
              ({"NODAL_DIRECT_PANEL_REGS": "0"}, ["grid60", "grid140_6dec"])]
CALL_SCOPE += [({"NODAL_DIRECT_BATCHED": "0", "NODAL_DIRECT_NB": str(nb)}, CHAINS) for nb in (16, 32, 48, 64)]
CALL_SCOPE += [({"NODAL_DIRECT_BATCHED": "0", "NODAL_DIRECT_PANEL_REGS": "0"}, CHAINS)]


def setting_name(env):
    return " ".join(f"{k}={v}" for k, v in env.items())


@pytest.mark.parametrize("env,name", [pytest.param(env, name, id=f"{setting_name(env)}-{name}")
                                      for env, names in CALL_SCOPE for name in names])
def test_unrefined_call_scope_variants_match_superlu(env, name, refs, monkeypatch):
    ref = refs(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h = open_handle(ref.table)
    z1, z16, verdicts = apply_all(h, ref.A)
    h.close()
    judge(ref, setting_name(env), z1, z16, verdicts)


# ---- knobs read once per process: a fresh child per setting, one at a time ----

PROCESS_SCOPE = [({"NODAL_DIRECT_SUPER": "0"}, ["grid200", "cfg5_420"]),
                 ({"NODAL_DIRECT_APPLY_STEPPED": "0"}, ["grid200", "cfg5_420"]),
                 ({"NODAL_DIRECT_LDS_BS": "128"}, ["grid45_6dec", "cfg5_48"]),
                 ({"NODAL_DIRECT_LDS_BS": "256"}, ["grid45_6dec", "cfg5_48"]),
                 # factor_fronts<1024>, extend_add<1024>, forward_level<1024, ...> / backward_level<1024, ...>
                 ({"NODAL_DIRECT_BIG_DIM": "512"}, ["grid140_6dec", "grid200"])]
child_failures = []  # a child that failed or was killed: no further child is started


@pytest.mark.parametrize("env,names", [pytest.param(env, names, id=setting_name(env)) for env, names in PROCESS_SCOPE])
def test_unrefined_process_scope_variants_match_superlu(env, names, refs, tmp_path):
    if child_failures:
        pytest.fail(f"no further child is started: the child for {child_failures[0]} failed")
    setting = setting_name(env)
    try:
        r = subprocess.run([sys.executable, CHILD, str(tmp_path)] + names, capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, NODAL_TRACE="1", **env))
    except subprocess.TimeoutExpired as e:
        child_failures.append(setting)
        pytest.fail(f"{setting}: the child was killed at its time limit\n{(e.stderr or b'')[-3000:]}")
    if r.returncode != 0:
        child_failures.append(setting)
        pytest.fail(f"{setting}: the child ended with status {r.returncode}\n{r.stderr[-3000:]}")
    assert "direct unrefined child ok" in r.stdout
    traces = dict(zip(names, re.split(r"^CASE \w+$", r.stderr, flags=re.M)[1:]))
    for name in names:
        # (the knob moves kernels, not the ordering: the table still sits in its class)
        assert width_class(largest_front(traces[name])) == CASES[name][1], (setting, name)
        if "NODAL_DIRECT_BIG_DIM" in env:  # (the one process knob whose effect the trace shows: no front takes the panel steps)
            assert "(0 fronts wider than" in traces[name], traces[name][-600:]
        with np.load(os.path.join(str(tmp_path), name + ".npz")) as got:
            judge(refs(name), setting, got["z1"], got["z16"], got["verdicts"])
