"""tests/fgmres_reference.py on its own, without a GPU: the host statement of the general route's flexible GMRES is a
solver, its bounds hold for plain float64 numpy from the same inputs, and the inputs the GPU tests rely on (C4: a
projection that cancels; A3: branch rows that couple to the node part; group A: the hand-written netlist's edges) are
what those tests take them to be."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import nodal_amd as n
from nodal_amd import generators as gen
from nodal_amd.lowering import lower
from oracle import nodal_oracle as oracle
from tests import fgmres_reference as ref

LD = ref.LD


def system(N):
    table = gen.cfg5_table(N)
    G, b = oracle.assemble_fast(table)
    G = sp.csr_matrix(G)
    G.sort_indices()
    return G, np.asarray(b, dtype=np.float64), table.K


def block_preconditioner(A, K, dtype=LD):
    """The device's block preconditioner with an EXACT solve of the node block in the multigrid cycle's place."""
    gn = ref.node_block(A.indptr, A.indices, A.data, K)
    Gn = sp.csr_matrix((gn["gn_data"], gn["gn_indices"], gn["gn_indptr"]), shape=(K, K))
    lu = spla.splu(Gn.tocsc())
    sinv, _, _ = ref.schur_inverse(A, K, gn)

    def apply(v):
        z_e = lu.solve(np.asarray(v[:K], dtype=np.float64))
        z_i, _ = ref.branch_solve(A, K, sinv, v, z_e)
        return np.concatenate([z_e, np.asarray(z_i, dtype=np.float64)]).astype(dtype)
    return apply, gn, sinv


def test_node_block_rules():
    """Unit diagonal inserted in front of, between and behind a row's entries and in an empty row; a zero, a negative
    and a NaN diagonal replaced; columns >= K cut off."""
    K = 6
    dense = np.zeros((8, 8))
    dense[0, 1], dense[0, 2] = -1, -2               # no diagonal, columns above: in front
    dense[1, 0], dense[1, 3], dense[1, 7] = -1, -3, 5  # between; the branch column goes
    dense[2, 0], dense[2, 1] = -4, -5               # behind
    dense[3, 6] = 1                                 # empty within the block
    dense[4, 4], dense[4, 0] = -2, 7                # negative
    dense[5, 5], dense[5, 2] = 3, -1                # kept
    A = sp.csr_matrix(dense)
    A.sort_indices()
    gn = ref.node_block(A.indptr, A.indices, A.data, K)
    Gn = sp.csr_matrix((gn["gn_data"], gn["gn_indices"], gn["gn_indptr"]), shape=(K, K)).toarray()
    want = dense[:K, :K].copy()
    want[[0, 1, 2, 3, 4], [0, 1, 2, 3, 4]] = 1.0
    assert np.array_equal(Gn, want)
    assert gn["gn_indices"].tolist() == [0, 1, 2, 0, 1, 3, 0, 1, 2, 3, 0, 4, 2, 5]
    assert gn["gn_diag"].tolist() == [0, 4, 8, 9, 11, 13]
    assert np.array_equal(gn["gn_rowidx"], np.repeat(np.arange(K), np.diff(gn["gn_indptr"])))
    for bad in (0.0, np.nan):  # (a stored zero, as the device's symbolic pattern keeps it)
        data = A.data.copy()
        data[A.indptr[5] + 1] = bad
        assert ref.node_block(A.indptr, A.indices, data, K)["gn_data"][13] == 1.0


def test_edge_netlist_holds_its_edges():
    nl = n.Netlist.from_rows(ref.edge_rows())
    table = lower(nl)
    G, b, _ = oracle.build_model(nl, True)
    G = sp.csr_matrix(G)
    G.sort_indices()
    K, nn = table.K, table.n
    assert nn == 600 and G.shape == (nn, nn)
    x, warned = oracle.solve(G, b, True)
    assert not warned and np.isfinite(x).all()
    gn = ref.node_block(G.indptr, G.indices, G.data, K)
    Gn = G[:K, :K].tocsr()
    empty = [i for i in range(K) if Gn.indptr[i] == Gn.indptr[i + 1]]
    assert len(empty) == 5 and empty[0] == 0 and empty[-1] > K - 10 and 100 < empty[2] < K - 100
    for i in empty:
        assert gn["gn_indptr"][i + 1] - gn["gn_indptr"][i] == 1 and gn["gn_data"][gn["gn_diag"][i]] == 1.0
    stored = Gn.diagonal()
    assert (stored < 0).sum() == 1 and (gn["gn_data"][gn["gn_diag"]] > 0).all()
    sinv, bound, degenerate = ref.schur_inverse(G, K, gn)
    assert degenerate.sum() == 1 and degenerate[-1] and sinv[-1] == 1.0  # the VCVS whose Schur term cancels
    assert (np.abs(sinv[~degenerate]) <= 1.0).all() and (bound < 1e-14).all()
    from nodal_amd import constants as c
    assert {c.T_E, c.T_VCVS, c.T_CCVS, c.T_CCCS} <= set(table.type.tolist())


def run_solver(A, b, apply_m, window, dtype=LD, max_cycles=6):
    x = np.zeros(A.shape[0], dtype=LD)
    bn = np.linalg.norm(b)
    cycles = []
    for _ in range(max_cycles):
        c = ref.cycle(A, apply_m, b, x, window=window, rel_tol=1e-14, dtype=dtype)
        cycles.append(c)
        x = c["x"]
        if np.linalg.norm(np.asarray(b - ref._matvec(A, x), dtype=np.float64)) <= 1e-13 * bn:
            break
    return np.asarray(x, dtype=np.float64), cycles


def test_the_reference_is_a_solver():
    """cfg5_table(12), n = 156: the chained reference with its own exact node-block solve and the Schur diagonal as
    preconditioner reaches spsolve's answer."""
    A, b, K = system(12)
    assert A.shape[0] == 156
    apply_m, _, _ = block_preconditioner(A, K)
    x, cycles = run_solver(A, b, apply_m, ref.MAXV)
    xo = spla.spsolve(A.tocsc(), b)
    assert np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max(), (np.abs(x - xo).max(), [c["count"] for c in cycles])
    assert 2 <= cycles[0]["count"] <= 40


@pytest.mark.parametrize("window", [41, 8, 2])
def test_relation_holds_for_float64_within_the_bound(window):
    """A Z = V H-bar, H-bar rebuilt from the rotated columns and the rotations, for one cycle run in plain float64 numpy
    (pairwise sums: inside the any-order bound) and in longdouble (far inside).  With a window, H-bar's rows above the
    window are exact zeros."""
    A, b, K = system(12)
    for dtype in (np.float64, LD):
        apply_m, _, _ = block_preconditioner(A, K, dtype)
        c = ref.cycle(A, apply_m, b, np.zeros(A.shape[0]), window=window, max_cols=20, dtype=dtype)
        count = c["count"]
        assert count == 20
        Hb = ref.hessenberg_from_rotations(c["R"], c["cs"], c["sn"], count)
        res, bnd = ref.relation_residual(A, c["Z"], c["V"], Hb, window)
        ratio = float((np.abs(res) / bnd).max())
        print(f"window {window} {np.dtype(dtype).name}: worst |A z - V Hbar| / bound {ratio:.3g}")
        assert ratio <= 2.0
        if dtype is LD:
            assert ratio <= 2.0 ** -8
        for j in range(count):
            s0 = max(0, j + 1 - window)
            assert (np.abs(Hb[:s0, j]) <= 4 * (j + 2) * ref.U * np.abs(Hb[:, j]).sum()).all()
            assert (c["R"][j + 2:, j] == 0).all()


def test_each_step_of_a_float64_cycle_is_within_the_bounds():
    """The per-column comparison the GPU test makes, made here on a float64 numpy cycle: every quantity of a step,
    recomputed in longdouble from that cycle's own inputs, is within 2 x its bound."""
    A, b, K = system(12)
    apply_m, _, _ = block_preconditioner(A, K, np.float64)
    for window in (41, 2):
        c = ref.cycle(A, apply_m, b, np.zeros(A.shape[0]), window=window, max_cols=12, dtype=np.float64)
        worst = 0.0
        for j in range(c["count"]):
            s0 = max(0, j + 1 - window)
            gj = gnext if j else np.float64(np.sqrt(np.asarray(b, dtype=LD) @ np.asarray(b, dtype=LD)))  # g[j] as the step found it
            gnext = -c["sn"][j] * gj
            st = ref.arnoldi_step(A, c["Z"][j], c["V"][:j + 1], s0, c["cs"][:j], c["sn"][:j], gj)
            for name, got in (("v_next", c["V"][j + 1]), ("col", c["R"][:j + 2, j]), ("c", c["cs"][j]), ("s", c["sn"][j]),
                              ("g_j", c["g"][j])):
                err = np.abs(np.asarray(got, dtype=LD) - st[name])
                bound = st[name + "_b"]
                live = bound > 0
                assert (err[~live] == 0).all() if np.ndim(err) else True
                worst = max(worst, float(np.max(err[live] / bound[live])) if np.ndim(err) else float(err / bound))
        print(f"window {window}: worst error / bound {worst:.3g}")
        assert worst <= 2.0


def direct_inputs(N):
    """What C4 runs on: the system preconditioned by its own float64 LU, three columns."""
    A, b, K = system(N)
    lu = spla.splu(A.tocsc())
    return A, b, (lambda v: lu.solve(np.asarray(v, dtype=np.float64)))


def test_c4_inputs_separate_one_pass_from_two():
    """C4's condition on cfg5_table(31): behind an LU, A M^-1 = I + O(eps), the first projection cancels every digit it
    has, and ONE Gram-Schmidt pass leaves a v_{j+1} at least 100 x SUMMATION_FACTOR less orthogonal than two passes
    do -- from the same inputs, in plain float64."""
    A, b, apply_m = direct_inputs(31)
    c = ref.cycle(A, apply_m, b, np.zeros(A.shape[0]), max_cols=3, dtype=np.float64)
    assert c["count"] == 3
    two, one = 0.0, 0.0
    for j in range(1, 3):
        gj = c["g"][j]  # (any value: the orthogonality of v_next does not depend on it)
        s2 = ref.arnoldi_step(A, c["Z"][j], c["V"][:j + 1], 0, c["cs"][:j], c["sn"][:j], gj, 2, np.float64)
        s1 = ref.arnoldi_step(A, c["Z"][j], c["V"][:j + 1], 0, c["cs"][:j], c["sn"][:j], gj, 1, np.float64)
        Vl = np.asarray(c["V"][:j + 1], dtype=LD)
        two = max(two, float(np.abs(Vl @ np.asarray(s2["v_next"], dtype=LD)).max()))
        one = max(one, float(np.abs(Vl @ np.asarray(s1["v_next"], dtype=LD)).max()))
    print(f"orthogonality of v_next against the basis: two passes {two:.3g}, one pass {one:.3g}")
    assert two <= 1e-14
    assert 100.0 * ref.SUMMATION_FACTOR * two <= one


def test_a3_branch_rows_couple_to_the_node_part():
    """A3's identity for the reference alone on cfg5_table(31): a float64 evaluation of S~^-1 (v - Cr z_e) is within
    2 x the bound of the longdouble one, and the term Cr z_e matters (dropping it breaks the identity by far more)."""
    A, b, K = system(31)
    assert A.shape[0] == 992
    apply_m, gn, sinv = block_preconditioner(A, K, np.float64)
    c = ref.cycle(A, apply_m, b, np.zeros(A.shape[0]), max_cols=6, dtype=np.float64)
    s64 = np.asarray(sinv, dtype=np.float64)
    Cr = A[K:, :K]
    for j in range(c["count"]):
        v, z = c["V"][j], c["Z"][j]
        want, bound = ref.branch_solve(A, K, s64, v, z[:K])
        got = s64 * (v[K:] - Cr @ z[:K])
        assert (np.abs(got - want) <= 2 * bound).all()
        without = s64 * v[K:]
        assert np.abs(without - want).max() > 1e6 * bound.max()
