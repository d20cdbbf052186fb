"""The general route's restarted flexible GMRES and its block preconditioner (nodal_amd/csrc/sparse_general.hip), kernel
by kernel, against the host statement of the same algebra in longdouble, tests/fgmres_reference.py.  A whole solve,
judged by a true residual, repairs a lost orthogonalisation pass, a padded lane counted with a non-zero coefficient, a
wrong block in gs_reduce, a rotation applied to the wrong pair, a Schur entry from the wrong row or a window that is off
by one at the price of iterations -- or hands the system to a pivoting solver without a word.  Here nothing is behind a
restart cycle: nodal_debug_fgmres_cycle runs the production setup and exactly ONE production cycle with the window, the
column cap and the tolerance as arguments, and returns the basis, the preconditioned vectors and the small
least-squares problem as the device holds them; nodal_debug_general_array returns what the setup left.

Bars.  Every comparison is exact or bounded by the reference's own a-priori, per-entry, first-order bound of the fp64
operations between the same inputs and that value (fgmres_reference's docstring), times 2 for the second-order terms.
Each step is checked from the DEVICE's own inputs (its z_j, its basis, its rotations, its g), so nothing accumulates.
The bounds are worst-case: loose by up to sqrt(n).  The errors this is for are orders above them; the one that hides
inside -- a missing second Gram-Schmidt pass -- is C4's.

Exact where stated: G_COUNT; the zero the new rotation leaves under the diagonal (H[j + 1, j]; rows below that are never
written and hold what the buffer held); rows < s0 - 1 of a windowed column (zero before the rotations, and a rotation of
two zeros is zero); y beyond `count`; the copies of the node block.

Shapes: cfg5_table(12) n = 156 (one partial workgroup), cfg5_table(31) n = 992 (three workgroups and 224 rows),
cfg5_table(512) n = 271185 (9041 rows in the second grid-stride trip, gd = 1024, 12 columns), cfg5_table(66) after a
default solve (system 1: the presolved system, n = 4355), and fgmres_reference.edge_rows() (n = 600: the setup's edges).
With window 41 and 40 columns, column j runs the Gram-Schmidt kernels with nv = j + 1: every instantiation NV = 4 .. 40
(NV = 44 is unreachable: nv <= 40 because j < 40).  Breakdown paths (d == 0, hnext == 0) are not provoked.

MEASURED on MI355X (worst device error / bound per case, as each test prints it; the bar is 2):

  case                          v_next   H column  cs / sn / g[j]  est, inv_h  A Z = V Hbar   y      x      |b - A x|
  cfg5_12  window 41            0.13     0.010     <= 0.0038       4e-06       0.13           0.32   0.033  0.0037
  cfg5_12  window 2             0.13     0.010     <= 0.0038       5e-04       0.13           0.062  0.029  0.0026
  cfg5_31  window 41            0.12     0.00024   <= 0.0006       1e-06       0.12           0.23   0.096  0.00077
  cfg5_31  window 2             0.12     0.00040   <= 0.0006       4e-05       0.13           0.16   0.031  0.00052
  cfg5_512 12 columns           0.16     2e-06     <= 2e-06        2e-08       0.19           0.050  0.12   2e-06
  cfg5_66  presolved, window 8  0.047    6e-05     <= 3e-05        2e-06       0.064          0.14   0.21   0.0016
  cfg5_66  presolved, window 41 0.047    6e-05     <= 3e-05        7e-08       0.064          0.22   0.20   0.0023
  cfg5_31  behind the LU, 3     0.087    0.00016   <= 0.0046       3e-04       0.13
  cfg5_31  stopped at 3 (C2)                                                                  0.0061 0.16   0.00063
  A2  1 / S~                    edges 0.072 (13 branch rows, the degenerate one exactly 1), cfg5_31 0.12 (18)
  A3  branch part of z_j        edges 0.29, cfg5_31 0.25 (40 columns each)
  the presolved cfg5_66 met use_sa = 1 and ell_spmv = 1 (three levels); the full systems plain aggregation and the CSR SpMV

  C4, max |v_i . v_k| in longdouble: behind the LU the device 2.9e-17 (| |v|^2 - 1 | 2.0e-16), the reference's two-pass
  float64 step from the same inputs 4.3e-17, its ONE-pass step 0.30.  Under the block preconditioner, inside the
  window: cfg5_12 8.2e-17 (reference 9.0e-17), cfg5_31 9.1e-17 (1.5e-16), cfg5_31 window 2 4.9e-17 (2.6e-16).  The device
  over max(reference, u) is 0.26 / 0.73 / 0.59 / 0.19: the order of the sums costs less than a factor of 1, and
  fgmres_reference.SUMMATION_FACTOR = 4 is what the tests allow -- 4.4e-16 behind the LU, nine orders below one pass.
  C5: one column, |r| / |b| 1.8e-15, scaled residual 5.3e-17.
  The hooks found no defect in the kernels.  The largest case takes 2.9 s, every other one under 0.5 s.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd import generators as gen
from nodal_amd.lowering import lower
from tests import fgmres_reference as ref

pytestmark = pytest.mark.gpu

LD = ref.LD
U = ref.U
BAR = 2.0  # over the first-order bound, for the second-order terms
_runs = {}


def table_of(shape):
    if shape == "edges":
        return lower(n.Netlist.from_rows(ref.edge_rows()))
    return gen.cfg5_table(int(shape.split("_")[1]))


def open_handle(shape):
    h = _ffi.Handle(0)
    h.upload(table_of(shape))
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    return h


def csr(arr):
    nn = len(arr["indptr"]) - 1
    A = sp.csr_matrix((arr["data"], arr["indices"], arr["indptr"]), shape=(nn, nn))
    assert A.has_sorted_indices or not A.sort_indices()
    return A


def run(shape, system=0, precond=0, window=41, max_cols=40, rel_tol=0.0, scale=None):
    """One hook call on a fresh handle (cached): (out, arrays, A).  system 1: after a default solve.  precond 1: after a
    one-column precond-0 call, whose export gives the matrix.  scale: b = scale x the system's own right-hand side."""
    key = (shape, system, precond, window, max_cols, rel_tol, scale)
    if key not in _runs:
        h = open_handle(shape)
        nn = None
        if system == 1:
            assert h.solve_sparse()[1] == 0
            nn = h.debug_hierarchy()[0]["n"]
        if precond == 1 or scale is not None:
            h.debug_fgmres_cycle(system, 0, 41, 1, 0.0, n=nn)
        b = None if scale is None else scale * h.debug_general_arrays()["rhs"]
        out = h.debug_fgmres_cycle(system, precond, window, max_cols, rel_tol, b=b, n=nn)
        arr = h.debug_general_arrays()
        out["b"] = arr["rhs"] if b is None else b
        h.close()
        _runs[key] = (out, arr, csr(arr))
    return _runs[key]


def written(H, m):
    """The entries m columns of a cycle write: column j down to row j + 1 (what lies below is never touched)."""
    return np.ascontiguousarray(np.triu(H[:m + 1, :m], -1))


def ratio(err, bound, what):
    """max err / bound; where the bound is exactly zero the error must be."""
    err, bound = np.atleast_1d(np.asarray(err, dtype=LD)), np.atleast_1d(np.asarray(bound, dtype=LD))
    assert np.isfinite(err).all(), what
    dead = bound == 0
    assert (err[dead] == 0).all(), (what, "an entry with a zero bound is not exact")
    return float((err[~dead] / bound[~dead]).max()) if (~dead).any() else 0.0


def hold_steps(o, A, window, label):
    """Group B: every column of the cycle from the device's own inputs.  Returns the worst ratio per quantity."""
    count, V, Z, H, cs, sn = o["count"], o["V"], o["Z"], o["H"], o["cs"], o["sn"]
    assert o["gcount"] == count and V.shape[0] == count + 1 and Z.shape[0] == count
    assert not np.isnan(V).any() and not np.isnan(Z).any()
    worst = {}

    def note(name, r):
        worst[name] = max(worst.get(name, 0.0), r)

    gj = np.float64(o["bnorm"])  # g[0] = |r_0| = |b| as the device summed it (x = 0)
    for j in range(count):
        s0 = max(0, j + 1 - window)
        st = ref.arnoldi_step(A, Z[j], V[:j + 1], s0, cs[:j], sn[:j], gj)
        note("v_next", ratio(np.abs(V[j + 1] - st["v_next"]), st["v_next_b"], (label, j, "v_next")))
        note("H column", ratio(np.abs(H[:j + 1, j] - st["col"][:j + 1]), st["col_b"][:j + 1], (label, j, "H")))
        assert H[j + 1, j] == 0.0, (label, j, "below the diagonal")
        assert (H[:max(s0 - 1, 0), j] == 0.0).all(), (label, j, "rows above the window")
        note("cs", ratio(abs(cs[j] - st["c"]), st["c_b"], (label, j, "cs")))
        note("sn", ratio(abs(sn[j] - st["s"]), st["s_b"], (label, j, "sn")))
        note("g[j]", ratio(abs(o["g"][j] - st["g_j"]), st["g_j_b"], (label, j, "g")))
        gj = np.float64(-sn[j] * gj)  # one fp64 product: the device's own g[j + 1], to the bit
        if j == count - 1:
            assert o["g"][count] == gj, (label, "g[count]")
            note("g[j+1]", ratio(abs(o["g"][count] - st["g_next"]), st["g_next_b"], (label, j, "g next")))
            note("est", ratio(abs(o["est"] - st["est"]), st["est_b"], (label, j, "est")))
            note("inv_h", ratio(abs(o["inv_h"] - st["inv_h"]), st["inv_h_b"], (label, j, "inv_h")))
    assert (o["g"][count + 1:] == 0.0).all()
    # once per case, from the exported state alone: A Z = V H-bar
    Hb = ref.hessenberg_from_rotations(H, cs, sn, count)
    res, bnd = ref.relation_residual(A, Z, V, Hb, window)
    note("A Z = V Hbar", ratio(np.abs(res), bnd, (label, "relation")))
    print(f"{label} window {window} count {count}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= BAR, (label, k, v)
    return worst


def hold_end(o, A, label):
    """C1: y, x and the true residual norm."""
    count = o["count"]
    y, y_b = ref.back_substitute(o["H"], o["g"], count)
    r_y = ratio(np.abs(o["y"] - y), y_b, (label, "y"))
    assert (o["y"][count:] == 0.0).all()
    x, x_b = ref.combine(o["Z"], o["y"], count)
    r_x = ratio(np.abs(o["x"] - x), x_b, (label, "x"))
    Ax, Ax_b = ref.spmv(A, o["x"])
    r = np.asarray(o["b"], dtype=LD) - Ax
    r_b = Ax_b + U * np.abs(r)
    nrm = np.sqrt(r @ r)
    nn = A.shape[0]
    nrm_b = np.sqrt(r_b @ r_b) + ((nn + 2) / 2 + 2) * U * nrm
    r_n = ratio(abs(o["rnorm"] - nrm), nrm_b, (label, "rnorm"))
    print(f"{label} end of cycle: y {r_y:.3g}, x {r_x:.3g}, |b - A x| {r_n:.3g} (device {o['rnorm']:.3e})")
    assert max(r_y, r_x, r_n) <= BAR, (label, r_y, r_x, r_n)


def window_orthogonality(o, window):
    """max |v_i . v_k| over pairs inside one window, and max | |v_k|^2 - 1 |, in longdouble."""
    Vl = np.asarray(o["V"], dtype=LD)
    G = Vl @ Vl.T
    k = np.arange(len(Vl))
    inside = (np.abs(k[:, None] - k[None, :]) < window) & (k[:, None] != k[None, :])
    return float(np.abs(G[inside]).max()), float(np.abs(np.diag(G) - 1).max())


def step_orthogonality(o, A, j, passes):
    """What the reference's plain-float64 step leaves from the device's own inputs of column j: max |V^T v_next|."""
    st = ref.arnoldi_step(A, o["Z"][j], o["V"][:j + 1], 0, o["cs"][:j], o["sn"][:j], 1.0, passes, np.float64)
    return float(np.abs(np.asarray(o["V"][:j + 1], dtype=LD) @ np.asarray(st["v_next"], dtype=LD)).max())


# ---- A. preconditioner setup ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["edges", "cfg5_31"])
def test_a1_node_block_is_copied_exactly(shape):
    o, arr, A = run(shape)
    K = o["K"]
    want = ref.node_block(arr["indptr"], arr["indices"], arr["data"], K)
    for name in ("gn_indptr", "gn_indices", "gn_rowidx", "gn_diag"):
        assert np.array_equal(arr[name], want[name]), name
    assert np.array_equal(arr["gn_data"].view(np.uint64), want["gn_data"].view(np.uint64))
    if shape == "edges":  # the edges are there, on the device's own pattern
        assert o["n"] == 600 and o["n"] - K == 13
        Gn = A[:K, :K].tocsr()
        empty = np.flatnonzero(np.diff(Gn.indptr) == 0)
        assert len(empty) == 5 and empty[0] == 0 and empty[-1] > K - 10
        for i in empty:  # the unit diagonal is the row
            p = arr["gn_indptr"][i]
            assert arr["gn_indptr"][i + 1] == p + 1 and arr["gn_indices"][p] == i and arr["gn_data"][p] == 1.0
        stored = np.array([A[i, i] if i in A.indices[A.indptr[i]:A.indptr[i + 1]] else np.nan for i in range(K)])
        assert (stored == 0.0).sum() == 1 and (stored < 0.0).sum() == 1  # a cancelled and a negative diagonal, both stored
        assert (arr["gn_data"][arr["gn_diag"]] > 0.0).all()


@pytest.mark.parametrize("shape", ["edges", "cfg5_31"])
def test_a2_schur_diagonal(shape):
    o, arr, A = run(shape)
    K = o["K"]
    gn = {k: arr[k] for k in ("gn_indptr", "gn_indices", "gn_rowidx", "gn_data", "gn_diag")}
    sinv, bound, degenerate = ref.schur_inverse(A, K, gn)
    assert len(arr["schur"]) == o["n"] - K > 0
    assert (arr["schur"][degenerate] == 1.0).all() and degenerate.sum() == (1 if shape == "edges" else 0)
    r = ratio(np.abs(arr["schur"] - sinv)[~degenerate], bound[~degenerate], (shape, "schur"))
    print(f"{shape}: 1 / S~ over {len(sinv)} branch rows, worst error / bound {r:.3g}")
    assert r <= BAR


@pytest.mark.parametrize("shape", ["edges", "cfg5_31"])
def test_a3_branch_solve(shape):
    o, arr, A = run(shape)
    K = o["K"]
    worst = 0.0
    for j in range(o["count"]):
        z, v = o["Z"][j], o["V"][j]
        want, bound = ref.branch_solve(A, K, arr["schur"], v, z[:K])
        worst = max(worst, ratio(np.abs(z[K:] - want), bound, (shape, j, "branch_solve")))
    print(f"{shape}: branch part of z_j over {o['count']} columns, worst error / bound {worst:.3g}")
    assert worst <= BAR


# ---- B. Arnoldi steps ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["cfg5_12", "cfg5_31"])
@pytest.mark.parametrize("window", [41, 2])
def test_b_steps_on_the_full_system(shape, window):
    o, arr, A = run(shape, window=window)
    assert o["n"] == {"cfg5_12": 156, "cfg5_31": 992}[shape] and o["count"] == 40 and o["window"] == window
    assert o["K"] < o["n"] and o["ell_spmv"] == 0 and o["gd"] == -(-o["n"] // 256)
    hold_steps(o, A, window, shape)
    hold_end(o, A, f"{shape} window {window}")
    off, unit = window_orthogonality(o, window)
    print(f"{shape} window {window}: max |v_i.v_k| inside the window {off:.3g}, max ||v|^2 - 1| {unit:.3g}")


def test_b_steps_in_the_second_grid_stride_trip():
    o, arr, A = run("cfg5_512", max_cols=12)
    assert o["n"] == 271185 and o["gd"] == 1024 and o["n"] - 1024 * 256 == 9041 and o["count"] == 12
    hold_steps(o, A, 41, "cfg5_512")
    hold_end(o, A, "cfg5_512")


@pytest.mark.parametrize("window", [8, 41])
def test_b_steps_on_the_presolved_system(window):
    o, arr, A = run("cfg5_66", system=1, window=window)
    print(f"cfg5_66 system 1: n {o['n']} use_sa {o['use_sa']} ell_spmv {o['ell_spmv']} levels {o['levels']}")
    assert o["K"] == o["n"] == 4355 and len(arr["schur"]) == 0 and o["count"] == 40
    assert o["use_sa"] == 1 and o["ell_spmv"] == 1  # the smoothed hierarchy took it; the SpMV ran on its ELL copy
    hold_steps(o, A, window, "cfg5_66 presolved")
    hold_end(o, A, f"cfg5_66 presolved window {window}")


# ---- C. end of cycle and control flow ------------------------------------------------------------------------------

def test_c2_early_stop_inside_a_batch():
    """The first batch is six columns whatever the tolerance; the estimate |g[m]| after column m - 1 is taken from a
    rel_tol 0 run, and a tolerance between it and the one before stops the second run at m = 3 columns, inside that
    batch: columns 3 .. 5 are enqueued and must leave everything alone."""
    full, _, A = run("cfg5_31")
    m = 3
    chain = full["bnorm"] * np.cumprod(np.abs(full["sn"][:m]))  # the estimate |g[k + 1]| after column k, k < m
    est_before, est_m = chain[m - 2], chain[m - 1]
    assert est_m < 0.5 * est_before
    rel_tol = float(np.sqrt(est_m * est_before) / full["bnorm"])
    o, _, _ = run("cfg5_31", rel_tol=rel_tol)
    assert o["count"] == m and o["gcount"] == m and o["done"] == 1.0 and o["tolb"] == rel_tol * o["bnorm"]
    assert o["est"] <= o["tolb"] < est_before
    for name in ("V", "Z"):  # (row m of V is not written: the kernel that scales v_m returns once the flag is up)
        assert np.array_equal(o[name][:m].view(np.uint64), full[name][:m].view(np.uint64)), name
    assert np.array_equal(written(o["H"], m).view(np.uint64), written(full["H"], m).view(np.uint64))
    assert np.array_equal(o["cs"][:m].view(np.uint64), full["cs"][:m].view(np.uint64))
    assert np.array_equal(o["sn"][:m].view(np.uint64), full["sn"][:m].view(np.uint64))
    assert np.array_equal(o["g"][:m].view(np.uint64), full["g"][:m].view(np.uint64)) and (o["g"][m + 1:] == 0).all()
    assert not np.array_equal(o["x"], full["x"])
    hold_end(o, A, "cfg5_31 stopped at 3")  # x is built from three columns only


def test_c3_zero_and_scaled_right_hand_side():
    base, arr, A = run("cfg5_31", max_cols=10)
    h = open_handle("cfg5_31")
    z = h.debug_fgmres_cycle(0, 0, 41, 10, 0.0, b=np.zeros(h.n))
    h.close()
    assert z["count"] == 0 and (z["x"] == 0.0).all() and z["bnorm"] == 0.0 and z["rnorm"] == 0.0
    assert len(z["V"]) == 0 and len(z["Z"]) == 0 and (z["gst"] == 0.0).all() and (z["y"] == 0.0).all()
    k = 2.0 ** 20
    o, _, _ = run("cfg5_31", max_cols=10, scale=k)
    assert o["count"] == base["count"] == 10
    for name in ("V", "Z"):
        assert np.array_equal(o[name].view(np.uint64), base[name].view(np.uint64)), name
    assert np.array_equal(written(o["H"], 10).view(np.uint64), written(base["H"], 10).view(np.uint64))
    for name in ("cs", "sn"):
        assert np.array_equal(o[name][:10].view(np.uint64), base[name][:10].view(np.uint64)), name
    for name in ("x", "g", "y"):
        assert np.array_equal(o[name], k * base[name]), name
    assert o["bnorm"] == k * base["bnorm"] and o["rnorm"] == k * base["rnorm"] and o["est"] == k * base["est"]


def test_c4_orthogonality_behind_the_direct_factors():
    """Behind the sparse LU A M^-1 = I + O(1e-10) or better: column 1 onwards, the first projection cancels every digit
    it has.  The device's basis, measured in longdouble, against what the reference's own two-pass step in plain float64
    leaves from the same inputs, with SUMMATION_FACTOR for the order of the sums (the device: strided partials in fixed
    order; numpy: pairwise) and a floor of u for the rounding of v_next's own entries (u |v_i||v_k| summed is <= u).
    The allowance stays 100 x below what ONE pass leaves from the same inputs, so a lost second pass cannot pass.

    MEASURED on MI355X: see the module docstring."""
    o, arr, A = run("cfg5_31", precond=1, max_cols=3)
    assert o["count"] == 3 and o["K"] == o["n"]
    off, unit = window_orthogonality(o, 41)
    two = max(step_orthogonality(o, A, j, 2) for j in range(3))
    one = max(step_orthogonality(o, A, j, 1) for j in range(1, 3))
    allowed = ref.SUMMATION_FACTOR * max(two, U)
    print(f"cfg5_31 behind the LU: device max |v_i.v_k| {off:.3g}, ||v|^2 - 1| {unit:.3g}; reference two passes {two:.3g}, "
          f"one pass {one:.3g}; allowed {allowed:.3g}; device / max(two, u) {off / max(two, U):.3g}")
    assert 100.0 * allowed <= one
    # (| |v|^2 - 1 |: twice the relative error of v = w (1 / hnext) -- the product, the reciprocal, the square root and
    # what a sum of n squares of one sign leaves when it is not summed in sequence, about u each: 4 u, times the factor)
    assert off <= allowed and unit <= ref.SUMMATION_FACTOR * 4 * U
    hold_steps(o, A, 41, "cfg5_31 behind the LU")


@pytest.mark.parametrize("shape,window", [("cfg5_12", 41), ("cfg5_31", 41), ("cfg5_31", 2)])
def test_c4_orthogonality_with_the_block_preconditioner(shape, window):
    """The same measure inside the window under the block preconditioner, held to the margin over the fp64 reference
    step alone."""
    o, arr, A = run(shape, window=window)
    off, _ = window_orthogonality(o, window)
    two = 0.0
    for j in range(o["count"]):
        s0 = max(0, j + 1 - window)
        st = ref.arnoldi_step(A, o["Z"][j], o["V"][:j + 1], s0, o["cs"][:j], o["sn"][:j], 1.0, 2, np.float64)
        two = max(two, float(np.abs(np.asarray(o["V"][s0:j + 1], dtype=LD) @ np.asarray(st["v_next"], dtype=LD)).max()))
    print(f"{shape} window {window}: device max |v_i.v_k| inside the window {off:.3g}, reference two passes {two:.3g}")
    assert off <= ref.SUMMATION_FACTOR * max(two, U)


def test_c5_direct_preconditioner_converges_within_three_columns():
    h = open_handle("cfg5_31")
    o = h.debug_fgmres_cycle(0, 1, 41, 3, 1e-13)
    scaled = h.debug_residual(o["x"])[0]
    h.close()
    print(f"cfg5_31 behind the LU, rel_tol 1e-13: count {o['count']}, |r| / |b| {o['rnorm'] / o['bnorm']:.3g}, scaled {scaled:.3g}")
    assert 1 <= o["count"] <= 3 and o["done"] == 1.0 and o["est"] <= 1e-13 * o["bnorm"]
    assert scaled <= 1e-14


# ---- the hooks themselves ------------------------------------------------------------------------------------------

def test_the_hooks_leave_a_solve_alone():
    """solve, solve on one handle; solve, every kind of hook call, solve on another: the second solves agree to the bit,
    in iterations and in residual.  NODAL_E_INVALID for what the hooks decline."""
    def two_solves(hook):
        h = open_handle("cfg5_66")
        first = h.solve_sparse()
        assert first[1] == 0 and first[2] > 0
        if hook:
            nn = h.debug_hierarchy()[0]["n"]
            h.debug_fgmres_cycle(1, 0, 8, 40, 0.0, n=nn)
            assert len(h.debug_general_arrays()["rhs"]) == nn
            h.debug_fgmres_cycle(1, 0, 41, 5, 1e-3, b=np.ones(nn), n=nn)
            h.debug_fgmres_cycle(0, 0, 41, 7, 0.0)
            assert len(h.debug_general_arrays()["rhs"]) == h.n
            h.debug_fgmres_cycle(0, 1, 41, 2, 0.0)
            assert np.array_equal(h.download_x(), first[0])
            for bad in (dict(system=2), dict(precond=2), dict(system=1, precond=1, n=nn), dict(window=1), dict(window=42),
                        dict(max_cols=0), dict(max_cols=41), dict(rel_tol=-1.0), dict(system=1, n=nn + 1)):
                with pytest.raises(_ffi.NodalHipError) as exc:
                    h.debug_fgmres_cycle(**bad)
                assert exc.value.status == _ffi.E_INVALID, bad
        second = h.solve_sparse()
        h.close()
        return first, second
    plain, hooked = two_solves(False), two_solves(True)
    for a, b in zip(plain, hooked):
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and a[1:] == b[1:], (a[1:], b[1:])
    h = open_handle("cfg5_12")  # nothing solved, nothing set up: no presolved system, no export
    with pytest.raises(_ffi.NodalHipError) as exc:
        h.debug_fgmres_cycle(1, 0, 41, 40, 0.0, n=h.n)
    assert exc.value.status == _ffi.E_INVALID
    with pytest.raises(_ffi.NodalHipError) as exc:
        h.debug_general_arrays()
    assert exc.value.status == _ffi.E_INVALID
    h.close()
