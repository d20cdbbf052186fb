"""The device's residual judges against exact host references (through nodal_debug_residual).

Two pieces of device code decide every verdict of the library: residual_kernel<LPR> + csr_scaled_residual (the
single-vector judge: nodal_residual, the acceptance test of the general routes) and resid_norms_multi +
scaled_from_norms (the block judge: resid_out / info_out of the source sweeps and the adjoint solves).  The hook runs
exactly that code on vectors chosen here, which are NOT solutions, so the residual is O(1) and a comparison is sharp.

  A, B  integer-valued matrices and vectors: every product and sum is exact in any order, so the device's four maxima
        must EQUAL numpy's and the quotient is numpy's to one ulp;
  C     real data against np.longdouble, within the standard dot-product rounding bound (nothing measured);
  D     what the public entry points report == what the hook computes for the vectors they returned, bit for bit.

The host reference is `host_norms` below: |Gx-b|_inf, |G|_inf, |x|_inf, |b|_inf from export_csr(), restated in numpy.
"""
import copy

import numpy as np
import pytest
import scipy.sparse as spsp

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd import generators as gen
from tests import sensitivity_reference as ref

pytestmark = pytest.mark.gpu

TB = 256                # threads of a workgroup (csrc/sparse.hip)
MAX_BLOCKS = 1024       # cap of both judges' grids
COLS = 16               # columns of a block (SLU_MULTI)
RES = np.array([1.0, 0.5, 0.25, 0.125])  # conductances 1, 2, 4, 8: every stamp and every diagonal sum is an integer
U = 2.0 ** -53


def lanes_per_row(nn, nnz):
    """the rule of csrc/sparse.hip, restated: the smallest power of two >= the average row length, 2 .. 64"""
    avg = nnz / nn if nn > 0 else 1.0
    lpr = 2
    while lpr < 64 and lpr < avg:
        lpr *= 2
    return lpr


# ---- the host reference ----------------------------------------------------------------------------------------------
def host_norms(G, x, b, dtype=np.float64):
    """(max|Gx-b|, max row sum |G|, max|x|, max|b|) in `dtype`"""
    indptr, indices, data = G
    assert np.diff(indptr).min() >= 1  # (reduceat needs every row to hold an entry; every row has its diagonal)
    d, xx = data.astype(dtype), np.asarray(x).astype(dtype)
    gx = np.add.reduceat(d * xx[indices], indptr[:-1])
    an = np.add.reduceat(np.abs(d), indptr[:-1]).max()
    return np.abs(gx - np.asarray(b).astype(dtype)).max(), an, np.abs(xx).max(), np.abs(np.asarray(b).astype(dtype)).max()


def host_gx(G, x):
    indptr, indices, data = G
    return np.add.reduceat(data * np.asarray(x, dtype=np.float64)[indices], indptr[:-1])


def host_scaled(r, an, xn, bn):
    den = an * xn + bn
    return r / den if den > 0 else 0.0


def one_ulp(got, want):
    return abs(got - want) <= np.spacing(abs(want))


def rounding_bounds(G, x, b):
    """The standard bound of a k-term dot product plus the subtraction of b, for the longest row: (k_max + 2) u times
    max_i (|G||x| + |b|)_i for the numerator and max_i (|G| 1)_i for the row sums (np.longdouble)."""
    indptr, indices, data = G
    L = np.longdouble
    kmax = int(np.diff(indptr).max())
    scale = np.add.reduceat(np.abs(data).astype(L) * np.abs(x).astype(L)[indices], indptr[:-1]) + np.abs(b).astype(L)
    rows = np.add.reduceat(np.abs(data).astype(L), indptr[:-1])
    return (kmax + 2) * L(U) * scale.max(), (kmax + 2) * L(U) * rows.max(), kmax


# ---- the networks ----------------------------------------------------------------------------------------------------
def network(nn, ea, eb, rng, hub=0, values=None):
    """Nodes 0 .. nn-1, every one tied to ground, joined by the edges (ea, eb); hub > 0 adds a node tied to ground and
    to the nodes 0 .. hub-1.  Resistances from RES, or log-uniform over two decades (values == "real")."""
    ground = nn + (1 if hub else 0)
    a = [np.arange(nn, dtype=np.int64), np.asarray(ea, dtype=np.int64)]
    b = [np.full(nn, ground, dtype=np.int64), np.asarray(eb, dtype=np.int64)]
    if hub:
        a += [np.full(hub, nn, dtype=np.int64), np.array([nn], dtype=np.int64)]
        b += [np.arange(hub, dtype=np.int64), np.array([ground], dtype=np.int64)]
    a, b = np.concatenate(a), np.concatenate(b)
    vals = 10.0 ** rng.uniform(-1.0, 1.0, len(a)) if values == "real" else rng.choice(RES, len(a))
    return gen.passive_table(a, b, vals, 0, ground)


def ground_only(nn, rng, **kw):
    return network(nn, [], [], rng, **kw)


def chain(nn, rng, **kw):
    k = np.arange(nn - 1, dtype=np.int64)
    return network(nn, k, k + 1, rng, **kw)


def circulant(nn, offsets, rng, **kw):
    """node i joined to i + s (mod nn) for every offset s < nn / 2: rows of 2 len(offsets) + 1 entries"""
    assert all(0 < s < nn / 2 for s in offsets) and len(set(offsets)) == len(offsets)
    i = np.arange(nn, dtype=np.int64)
    return network(nn, np.tile(i, len(offsets)), np.concatenate([(i + s) % nn for s in offsets]), rng, **kw)


def random_offsets(nn, count, seed):
    return sorted(int(s) for s in np.random.default_rng(seed).choice(np.arange(1, nn // 2), count, replace=False))


def grid200(rng, values=None):
    count = gen.grid_resistor_count(200)
    return gen.grid_table(200, 10.0 ** rng.uniform(-1.0, 1.0, count) if values == "real" else rng.choice(RES, count))


# name -> (builder(rng, values=...), the instantiation of DISPATCH_LPR it is meant to hit)
# n = TB / LPR +- 1 puts dead rows next to live ones inside a wave; a row cannot hold more entries than the matrix has
# columns, so LPR 32 (n = 7, 9) and LPR 64 (n = 3, 5) cannot be reached at those sizes.
NETWORKS = {
    "one node": (lambda rng, **kw: ground_only(1, rng, **kw), 2),
    "two nodes": (lambda rng, **kw: chain(2, rng, **kw), 2),
    "ground only 127": (lambda rng, **kw: ground_only(127, rng, **kw), 2),
    "ground only 129": (lambda rng, **kw: ground_only(129, rng, **kw), 2),
    "chain 17": (lambda rng, **kw: chain(17, rng, **kw), 4),
    "chain 63": (lambda rng, **kw: chain(63, rng, **kw), 4),
    "chain 65": (lambda rng, **kw: chain(65, rng, **kw), 4),
    "ring2 31": (lambda rng, **kw: circulant(31, [1, 2], rng, **kw), 8),
    "ring2 33": (lambda rng, **kw: circulant(33, [1, 2], rng, **kw), 8),
    "complete 15": (lambda rng, **kw: circulant(15, range(1, 8), rng, **kw), 16),
    "degree12 17": (lambda rng, **kw: circulant(17, range(1, 7), rng, **kw), 16),
    "degree10 300": (lambda rng, **kw: circulant(300, random_offsets(300, 5, 1), rng, **kw), 16),
    "degree20 300": (lambda rng, **kw: circulant(300, random_offsets(300, 10, 2), rng, **kw), 32),
    "complete 49": (lambda rng, **kw: circulant(49, range(1, 25), rng, **kw), 64),
    "hub 3000 on chain 6000": (lambda rng, **kw: chain(6000, rng, hub=3000, **kw), 4),
    "grid 200": (lambda rng, **kw: grid200(rng, **kw), 8),
}


def open_handle(table):
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    return h


def csr_of(h):
    indptr, indices, data, rhs = h.export_csr()
    return (indptr.astype(np.int64), indices.astype(np.int64), data), rhs


class Net:
    def __init__(self, name, values=None):
        build, self.lpr = NETWORKS[name]
        self.name = name
        self.table = build(np.random.default_rng(sum(map(ord, name))), values=values)
        self.h = open_handle(self.table)
        self.G, self.rhs = csr_of(self.h)
        self.n = self.h.n
        assert lanes_per_row(self.h.n, self.h.nnz) == self.lpr, (name, self.h.n, self.h.nnz)
        if values is None:
            assert np.array_equal(self.G[2], np.round(self.G[2]))  # integers throughout

    def rows_of_interest(self):
        """row 0, row n-1, the longest row and one of its neighbours, the last row of the single judge's first
        grid-stride pass and the first of its second, a row that only the last, partial workgroup serves"""
        nn, per_block = self.n, TB // self.lpr
        indptr, indices, _ = self.G
        hubrow = int(np.argmax(np.diff(indptr)))
        rows = {0, nn - 1, hubrow, int(indices[indptr[hubrow]]), int(indices[indptr[hubrow + 1] - 1])}
        per_pass = MAX_BLOCKS * per_block
        if nn > per_pass:
            rows |= {per_pass - 1, per_pass}
        if nn % per_block:
            rows.add(nn - (nn % per_block))  # first row of the partial workgroup
        return sorted(rows)

    def block_rows(self):
        """row 0, n-1, the middle, the longest row, the last row of the block judge's first grid-stride pass and the
        first of its second"""
        nn = self.n
        rows = {0, nn - 1, nn // 2, int(np.argmax(np.diff(self.G[0])))}
        per_pass = MAX_BLOCKS * TB // COLS
        if nn > per_pass:
            rows |= {per_pass - 1, per_pass}
        return sorted(rows)


KEPT = ("grid 200", "hub 3000 on chain 6000")  # built once for the module; the small ones per test


@pytest.fixture(scope="module")
def kept_nets():
    kept = {}
    yield kept
    for net in kept.values():
        net.h.close()


@pytest.fixture
def nets(kept_nets):
    made = []

    def get(name, values=None):
        if name in KEPT:
            if (name, values) not in kept_nets:
                kept_nets[(name, values)] = Net(name, values)
            return kept_nets[(name, values)]
        made.append(Net(name, values))
        return made[-1]
    yield get
    for net in made:
        net.h.close()


def check_single(net_or_h, G, x, b, tag):
    h = getattr(net_or_h, "h", net_or_h)
    scaled, norms = h.debug_residual(x, b)
    want = host_norms(G, x, b)
    assert np.array_equal(norms[:4], np.array(want)), (tag, norms, want)
    assert norms[4] == 0.0, tag
    assert one_ulp(scaled, host_scaled(*want)), (tag, scaled, host_scaled(*want))
    return scaled, norms


def integer_vectors(rng, nn):
    return rng.integers(-8, 9, nn).astype(np.float64), rng.integers(-8, 9, nn).astype(np.float64)


# ---- A: exact data, the single-vector judge ---------------------------------------------------------------------------
def test_every_lanes_per_row_instantiation_is_covered():
    assert {lpr for _, lpr in NETWORKS.values()} == {2, 4, 8, 16, 32, 64}


@pytest.mark.parametrize("name", list(NETWORKS))
def test_single_judge_exact(nets, name):
    """Random integer vectors, then the largest defect, |x_i| and |b_i| alone at each row of interest."""
    net = nets(name)
    rng = np.random.default_rng(7)
    if net.n > TB // net.lpr * MAX_BLOCKS:
        assert name == "grid 200"  # the one case whose grid-stride loop makes a second pass
    for draw in range(2):
        x, b = integer_vectors(rng, net.n)
        check_single(net, net.G, x, b, (name, draw))
    x, b0 = integer_vectors(rng, net.n)
    for row in net.rows_of_interest():
        # the defect: b = G x exactly, except at `row`
        b = host_gx(net.G, x)
        b[row] += 2.0 ** 20
        _, norms = check_single(net, net.G, x, b, (name, "defect", row))
        assert norms[0] == 2.0 ** 20
        # |x|: one entry far above the others (and its column far above every other product)
        xx = x.copy()
        xx[row] = -(2.0 ** 20)
        _, norms = check_single(net, net.G, xx, b0, (name, "x", row))
        assert norms[2] == 2.0 ** 20
        # |b|
        bb = b0.copy()
        bb[row] = -(2.0 ** 25)
        _, norms = check_single(net, net.G, x, bb, (name, "b", row))
        assert norms[3] == 2.0 ** 25


@pytest.mark.parametrize("name", ["ground only 129", "chain 65", "degree20 300", "hub 3000 on chain 6000", "grid 200"])
def test_single_judge_heaviest_row(nets, name):
    """|G|_inf sits at each row of interest in turn: a resistance of 2^-20 at that node (to ground where the node has
    such a resistor, else two of them to two neighbours) makes its row sum the largest, with no tie."""
    net = nets(name)
    t = net.table
    ty, a, b = np.asarray(t.type), np.asarray(t.a), np.asarray(t.b)
    rng = np.random.default_rng(11)
    x, bvec = integer_vectors(rng, net.n)
    for row in net.rows_of_interest():
        at = np.flatnonzero((ty == 0) & ((a == row) | (b == row)))
        tie = [i for i in at if min(a[i], b[i]) < 0]
        heavy = copy.copy(t)
        heavy.value = np.array(t.value, dtype=np.float64)
        heavy.value[tie[:1] or list(at[:2])] = 2.0 ** -20
        h = open_handle(heavy)
        G, _ = csr_of(h)
        sums = np.add.reduceat(np.abs(G[2]), G[0][:-1])
        assert int(np.argmax(sums)) == row and (sums == sums.max()).sum() == 1, (name, row)
        _, norms = check_single(h, G, x, bvec, (name, "heavy", row))
        assert norms[1] == sums[row]
        h.close()


@pytest.mark.parametrize("name", ["one node", "two nodes", "chain 65", "hub 3000 on chain 6000", "grid 200"])
def test_single_judge_degenerate_values(nets, name):
    net = nets(name)
    rng = np.random.default_rng(13)
    nn = net.n
    x, b = integer_vectors(rng, nn)
    x[0] = 3.0  # (not all zero, whatever the draw)
    b[nn - 1] = -5.0
    zero = np.zeros(nn)
    scaled, norms = net.h.debug_residual(zero, zero)
    assert scaled == 0.0 and np.array_equal(norms, [0.0, host_norms(net.G, zero, zero)[1], 0.0, 0.0, 0.0])
    scaled, _ = check_single(net, net.G, zero, b, (name, "x = 0"))
    assert scaled == 1.0
    check_single(net, net.G, x, zero, (name, "b = 0"))
    # -0.0 entries count as zeros
    scaled, norms = net.h.debug_residual(-zero, -zero)
    assert scaled == 0.0 and not norms[[0, 2, 3, 4]].any()
    xm, bm = np.where(x == 0.0, -0.0, x), np.where(b == 0.0, -0.0, b)
    xm[nn - 1] = bm[0] = -0.0
    xp, bp = xm + 0.0, bm + 0.0  # (the same vectors with +0.0)
    got, want = net.h.debug_residual(xm, bm), check_single(net, net.G, xp, bp, (name, "+0.0"))
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    # a NaN anywhere in x: NaN, and the poison flag
    indptr, indices, _ = net.G
    hubrow = int(np.argmax(np.diff(indptr)))
    for at in sorted({0, nn - 1, int(indices[indptr[hubrow + 1] - 1])}):
        xn = x.copy()
        xn[at] = np.nan
        scaled, norms = net.h.debug_residual(xn, b)
        assert np.isnan(scaled) and norms[4] == 1.0, (name, at)


def test_single_judge_null_b_is_the_assembled_rhs(nets):
    net = nets("grid 200")
    x, _ = integer_vectors(np.random.default_rng(17), net.n)
    assert net.rhs.any()
    got, want = net.h.debug_residual(x), net.h.debug_residual(x, net.rhs)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    check_single(net, net.G, x, net.rhs, "assembled rhs")


# ---- B: exact data, the block judge -------------------------------------------------------------------------------------
def interleaved(V, nn):
    """[cols][n] rows as the [n][16] block; the columns past `cols` hold NaN: the judge must not look at them"""
    out = np.full((nn, COLS), np.nan)
    out[:, :V.shape[0]] = V.T
    return out


def block_vectors(net, cols, rng):
    """cols different integer vectors: column y has its own scale, its own largest |x| and its own defect row"""
    nn = net.n
    X = rng.integers(-8, 9, (cols, nn)).astype(np.float64) * (np.arange(cols)[:, None] + 1)
    B = np.empty_like(X)
    rows = net.block_rows()
    for y in range(cols):
        X[y, rows[(y + 3) % len(rows)]] = 2.0 ** (8 + y)
        B[y] = host_gx(net.G, X[y])
        B[y, rows[y % len(rows)]] -= 2.0 ** (26 + y)
    if cols >= 15:
        X[7] = B[7] = 0.0  # an all-zero column
    return X, B


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("cols", [1, 2, 15, 16])
@pytest.mark.parametrize("name", ["one node", "two nodes", "chain 17", "hub 3000 on chain 6000", "grid 200"])
def test_block_judge_exact(nets, name, cols):
    net = nets(name)
    nn, h = net.n, net.h
    if name == "grid 200":
        assert nn * COLS > MAX_BLOCKS * TB  # the capped grid strides
    X, B = block_vectors(net, cols, np.random.default_rng(100 + cols))
    s0, n0 = h.debug_residual(X, B, cols=cols, layout=0)
    s1, n1 = h.debug_residual(interleaved(X, nn), interleaved(B, nn), cols=cols, layout=1)
    assert same_bits(s0, s1) and same_bits(n0, n1)
    assert not n0[cols:].any() and not n0[1:cols, 3].any()  # (the slots nobody owns stay zero)
    an = host_norms(net.G, X[0], B[0])[1]
    assert n0[0, 3] == an
    for y in range(cols):
        r, _, xn, bn = host_norms(net.G, X[y], B[y])
        assert np.array_equal(n0[y, :3], [r, xn, bn]), (name, cols, y, n0[y], (r, xn, bn))
        assert one_ulp(s0[y], host_scaled(r, an, xn, bn)), (name, cols, y)
        if cols >= 15 and y == 7:
            assert s0[y] == 0.0 and not n0[y, :3].any()
        elif nn > 1:
            assert r >= 2.0 ** 25 and s0[y] > 0.0
        # the same vector judged alone: the same bits, in every layout
        alone = [h.debug_residual(X[y], B[y], cols=1, layout=2), h.debug_residual(X[y:y + 1], B[y:y + 1], cols=1, layout=0)]
        if y in (0, cols - 1):
            alone.append(h.debug_residual(interleaved(X[y:y + 1], nn), interleaved(B[y:y + 1], nn), cols=1, layout=1))
        for sa, na in alone:
            assert same_bits(sa[0], s0[y]) and same_bits(na[0, :3], n0[y, :3]) and na[0, 3] == an, (name, cols, y)
    # and the single-vector judge agrees on the four maxima of a column
    _, single = h.debug_residual(X[cols - 1], B[cols - 1])
    assert np.array_equal(single[:4], [n0[cols - 1, 0], an, n0[cols - 1, 1], n0[cols - 1, 2]])
    # a NaN in column y (0 owns the slot of |G|_inf) poisons that column alone
    for y in sorted({0, cols - 1}):
        Xn = X.copy()
        Xn[y, nn // 2] = np.nan
        for layout, (xs, bs) in enumerate([(Xn, B), (interleaved(Xn, nn), interleaved(B, nn))]):
            sn, nb = h.debug_residual(xs, bs, cols=cols, layout=layout)
            assert np.isnan(sn[y]), (name, cols, y, layout)
            others = np.arange(cols) != y
            assert same_bits(sn[others], s0[others]) and same_bits(nb[:cols][others, :3], n0[:cols][others, :3])
            assert nb[0, 3] == an
    sn, _ = h.debug_residual(np.where(np.arange(nn) == nn - 1, np.nan, X[0]), B[0], cols=1, layout=2)
    assert np.isnan(sn[0])


# ---- C: real data, the rounding bound ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NETWORKS))
def test_real_data_within_the_dot_product_bound(nets, name):
    """Resistances over two decades, Gaussian x and b that solve nothing (the scaled residual is O(1)).  Against
    np.longdouble: |device - host| <= (k_max + 2) 2^-53 max_i (|G||x| + |b|)_i for the numerator and the same with
    |x| = 1 for |G|_inf (k_max the longest row); |x|_inf and |b|_inf are equal.  Every network of parts A and B, sixteen
    columns each, every column through the block judge in both layouts, the single-vector judge and alone."""
    net = nets(name, "real")
    nn, h, L = net.n, net.h, np.longdouble
    rng = np.random.default_rng(23)
    X, B = rng.standard_normal((COLS, nn)), rng.standard_normal((COLS, nn))
    blocks = [h.debug_residual(X, B, cols=COLS, layout=0),
              h.debug_residual(interleaved(X, nn), interleaved(B, nn), cols=COLS, layout=1)]
    assert same_bits(blocks[0][0], blocks[1][0]) and same_bits(blocks[0][1], blocks[1][1])
    for y in range(COLS):
        r, an, xn, bn = host_norms(net.G, X[y], B[y], L)
        bound_r, bound_an, kmax = rounding_bounds(net.G, X[y], B[y])
        got = [blocks[0][1][y, 0], blocks[0][1][0, 3], blocks[0][1][y, 1], blocks[0][1][y, 2], blocks[0][0][y]]
        views = [("block", got)]
        scaled, norms = h.debug_residual(X[y], B[y])
        assert norms[4] == 0.0
        views.append(("single", list(norms[:4]) + [scaled]))
        sa, na = h.debug_residual(X[y], B[y], cols=1, layout=2)
        views.append(("alone", [na[0, 0], na[0, 3], na[0, 1], na[0, 2], sa[0]]))
        for which, (dr, dan, dxn, dbn, ds) in views:
            assert abs(L(dr) - r) <= bound_r, (name, which, y, kmax, float(abs(L(dr) - r)), float(bound_r))
            assert abs(L(dan) - an) <= bound_an, (name, which, y, kmax, float(abs(L(dan) - an)), float(bound_an))
            assert dxn == float(xn) and dbn == float(bn), (name, which, y)
            assert 0.0 < ds <= 1.0, (name, which, y, ds)  # (O(1); never above 1, by the triangle inequality)


# ---- the hook itself -----------------------------------------------------------------------------------------------------
def test_hook_arguments_and_that_it_leaves_the_handle_alone():
    table = gen.grid_table(20)
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    x = np.ones(h.n)
    with pytest.raises(_ffi.NodalHipError) as exc:  # no numeric assembly yet
        h.debug_residual(x)
    assert exc.value.status == _ffi.E_INVALID
    assert h.assemble_numeric()[0] == _ffi.OK
    for cols, layout in [(0, 1), (0, 2), (1, 3), (2, 2), (17, 0), (-1, 0)]:
        with pytest.raises(_ffi.NodalHipError) as exc:  # (past the wrapper's own shape checks)
            scaled, norms = np.zeros(16), np.zeros(64)
            big = np.zeros(17 * h.n)
            h._check(h.lib.nodal_debug_residual(h._h, 0, cols, layout, _ffi._ptr(big, _ffi.C.c_double),
                                                _ffi._ptr(big, _ffi.C.c_double), _ffi._ptr(scaled, _ffi.C.c_double),
                                                _ffi._ptr(norms, _ffi.C.c_double)))
        assert exc.value.status == _ffi.E_INVALID, (cols, layout)
    with pytest.raises(_ffi.NodalHipError) as exc:  # a passive network keeps no G^T
        h.debug_residual(x, x, transposed=True)
    assert exc.value.status == _ffi.E_INVALID
    with pytest.raises(_ffi.NodalHipError) as exc:  # the block judge has no default right-hand side
        h.debug_residual(x, None, cols=1, layout=2)
    assert exc.value.status == _ffi.E_INVALID
    xs, info = h.solve_dense()
    assert info == 0
    before = h.residual()
    G, rhs = csr_of(h)
    rng = np.random.default_rng(3)
    h.debug_residual(rng.standard_normal(h.n), rng.standard_normal(h.n))
    h.debug_residual(rng.standard_normal((3, h.n)), rng.standard_normal((3, h.n)), cols=3, layout=0)
    assert same_bits(h.download_x(), xs) and h.residual() == before  # (x, its flag and the rhs are where they were)
    G2, rhs2 = csr_of(h)
    assert np.array_equal(G2[2], G[2]) and np.array_equal(rhs2, rhs)
    h.close()


# ---- D: the public numbers are the judge's numbers -----------------------------------------------------------------------
# what NODAL_TRACE=1 must (and must not) say on stderr when the solve takes the route a case is named after; the
# multigrid's trace is read once per process, so that route is recognised by its level and iteration counts instead
ROUTE_TRACE = {"multigrid": ([], ["[lowdeg]", "[presolve]", "[direct]"]),
               "low-degree elimination": (["[lowdeg]"], ["[presolve]", "[direct]"]),
               "general with presolve": (["[presolve] accepted"], ["[lowdeg]"]),
               "sparse direct": (["[direct] analysis"], ["[lowdeg]", "[presolve]"]),
               "dense passive": ([], ["[lowdeg]", "[presolve]", "[direct]"]),
               "dense pivoted": ([], ["[lowdeg]", "[presolve]", "[direct]"])}


def _solve(route):
    h = _ffi.Handle(0)
    if route == "dense pivoted":
        h.set_option(_ffi.OPT_FORCE_PIVOTING, 1)
    table = {"multigrid": lambda: gen.grid_table(64), "low-degree elimination": lambda: gen.ladder_table(2000),
             "general with presolve": lambda: gen.cfg5_table(30), "sparse direct": lambda: gen.cfg5_table(30),
             "dense passive": lambda: gen.grid_table(20), "dense pivoted": lambda: gen.cfg5_table(12)}[route]()
    h.upload(table)
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    if route.startswith("dense"):
        _, info = h.solve_dense()
    else:
        method = {"multigrid": _ffi.SPARSE_PCG, "low-degree elimination": _ffi.SPARSE_AUTO,
                  "general with presolve": _ffi.SPARSE_LU, "sparse direct": _ffi.SPARSE_DIRECT}[route]
        _, info, _, _ = h.solve_sparse(method=method)
    assert info == 0
    return h


@pytest.mark.parametrize("route", ["multigrid", "low-degree elimination", "general with presolve", "sparse direct",
                                   "dense passive", "dense pivoted"])
def test_nodal_residual_is_the_hook_on_the_solution(route, monkeypatch, capfd):
    """After a solve on each route nodal_residual() has the bits the hook gives for download_x() and the assembled
    right-hand side -- and that number is within the rounding bound of part C of the host's.  That the solve took the
    route the case is named after is read from the library's trace and from nodal_last_solve_info."""
    monkeypatch.setenv("NODAL_TRACE", "1")
    capfd.readouterr()
    h = _solve(route)
    err = capfd.readouterr().err
    monkeypatch.delenv("NODAL_TRACE")
    said, unsaid = ROUTE_TRACE[route]
    assert all(tag in err for tag in said) and not any(tag in err for tag in unsaid), (route, err)
    iterations, levels, _ = h.solve_info()
    if route == "multigrid":
        assert levels > 0 and iterations > 0, (route, iterations, levels)
    elif route.startswith("dense"):
        assert levels == 0 and iterations == 0, (route, iterations, levels)
    x = h.download_x()
    reported = h.residual()
    scaled, norms = h.debug_residual(x)
    assert reported == scaled and norms[4] == 0.0, (route, reported, scaled)
    G, rhs = csr_of(h)
    L = np.longdouble
    r, an, xn, bn = host_norms(G, x, rhs, L)
    bound_r, bound_an, _ = rounding_bounds(G, x, rhs)
    assert abs(L(norms[0]) - r) <= bound_r, (route, reported, norms[0], float(r), float(bound_r))
    assert abs(L(norms[1]) - an) <= bound_an, (route, norms[1], float(an), float(bound_an))
    assert norms[2] == float(xn) and norms[3] == float(bn)
    assert reported <= 1e-12
    h.close()


def _check_sweep_members(h, rows, values, x, info, resid, tag):
    rhs = h.debug_sources_rhs(rows, values)
    for m in range(values.shape[0]):
        if info[m] > 0:
            assert np.isnan(resid[m]) and np.isnan(x[m]).all(), (tag, m)
            continue
        scaled, _ = h.debug_residual(x[m], rhs[m], cols=1, layout=2)
        assert resid[m] == scaled[0], (tag, m, resid[m], scaled[0])


@pytest.fixture(scope="module")
def sweep_handles():
    made = {}

    def get(which):
        if which not in made:
            table = {"grid(300): multigrid, blocks": lambda: gen.grid_table(300),
                     "cfg5(100): sparse LU": lambda: gen.cfg5_table(100),
                     "cfg5(20): dense": lambda: gen.cfg5_table(20)}[which]()
            made[which] = (open_handle(table), table)
        return made[which]
    yield get
    for h, _ in made.values():
        h.close()


@pytest.mark.parametrize("M", [1, 16, 17])
@pytest.mark.parametrize("which", ["grid(300): multigrid, blocks", "cfg5(100): sparse LU", "cfg5(20): dense"])
def test_sweep_residuals_are_the_hook_on_the_members(sweep_handles, which, M):
    """resid_out[m] of a source sweep == the block judge on (x_out[m], the member's right-hand side), bit for bit: a full
    block, a tail block and a lone member on each route (member 0 of the multigrid route is always solved alone)."""
    h, table = sweep_handles(which)
    rows = np.flatnonzero(np.isin(np.asarray(table.type), (1, 2)))  # every independent source, A and E
    rng = np.random.default_rng(M)
    values = rng.uniform(-5.0, 5.0, (M, len(rows)))
    if M > 2:
        values[M // 2] = 0.0  # an all-zero member
    if which.startswith("grid(300)"):
        assert h.n > 4096 and len(rows) == 1
    elif which.startswith("cfg5(100)"):
        assert h.n > 8192
    x, info, resid = h.solve_sources(rows, values, dense=which.endswith("dense"))
    assert (info == 0).all() and (resid <= 1e-12).all()
    _check_sweep_members(h, rows, values, x, info, resid, which)
    if M > 2:
        assert resid[M // 2] == 0.0


def test_sweep_members_of_a_singular_network_have_nan_residuals():
    from nodal_amd.lowering import lower
    rows = list(gen.grid_rows(70))
    rows += [[f"f{i}", "R", "1", f"x{i}", f"x{i + 1}"] for i in range(40)] + [["fa", "A", "1", "x3", "x17"]]
    table = lower(n.Netlist.from_rows(rows))
    h = open_handle(table)
    src = np.flatnonzero(np.asarray(table.type) == 1)
    values = np.random.default_rng(5).uniform(-1.0, 1.0, (3, len(src)))
    x, info, resid = h.solve_sources(src, values, dense=False)
    assert (info > 0).all()
    _check_sweep_members(h, src, values, x, info, resid, "floating island")
    scaled, _ = h.debug_residual(x[0], h.debug_sources_rhs(src, values)[0], cols=1, layout=2)
    assert np.isnan(scaled[0])  # (the judge itself answers NaN for such a row)
    h.close()


@pytest.mark.parametrize("which", ["grid(80): passive", "cfg5(95): transposed child"])
def test_adjoint_residuals_are_the_hook_on_the_adjoints(which):
    """resid_out[q] of nodal_sensitivities == the block judge on (adjoint_out[q], c_q) -- against G itself on a passive
    network (symmetric bit for bit), against the child's G^T otherwise.  c_q is sensitivity_reference.output_vector's:
    e_p - e_q for the potentials and voltages, (e_a - e_b) / v or the unit vector of a branch unknown for the currents."""
    passive = which.startswith("grid")
    nl = n.Netlist.from_rows(list(gen.grid_rows(80)) if passive else gen.cfg5_rows(95))
    c = n.Circuit(nl, sparse=True)
    h = c._handle
    assert h.n > (4096 if passive else 8192)
    c.solve()
    specs = ref.sample_outputs(nl, c.table, 18, 18)
    specs[9] = ("e", nl.ground)  # an all-zero column
    sens = c.sensitivities(specs, adjoints=True)
    assert (sens.info == 0).all() and (sens.scaled_residual <= 1e-12).all()
    assert {s[0] for s in specs} == {"e", "v", "i"}
    other = 0
    for q, spec in enumerate(specs):
        cq, _ = ref.output_vector(nl, c.table, spec)
        lam = np.asarray(sens.adjoints[q])
        scaled, _ = h.debug_residual(lam, cq, cols=1, layout=2, transposed=not passive)
        assert sens.scaled_residual[q] == scaled[0], (which, q, spec, sens.scaled_residual[q], scaled[0])
        if not passive:  # (judged against G instead, the number is another one: the transpose matters)
            other += h.debug_residual(lam, cq, cols=1, layout=2)[0][0] != scaled[0]
    assert sens.scaled_residual[9] == 0.0
    assert passive or other > 0


def test_the_adjoint_judge_scales_by_the_one_norm_of_G():
    """cfg5 with every resistance and gain a power of two (through a value table): G is exact, and on integer vectors
    the hook with transposed=True must give the maxima of G^T taken from export_csr() -- |G^T|_inf = |G|_1 among them --
    where the untransposed judge gives those of G."""
    table = gen.cfg5_table(12)
    ty = np.asarray(table.type)
    rng = np.random.default_rng(29)
    vals = np.array(table.value, dtype=np.float64)[None, :].copy()
    vals[0, ty == 0] = rng.choice(RES, int((ty == 0).sum()))
    gains = (ty == 3) | (ty == 4) | (ty == 5)
    assert gains.any() and (ty == 2).any()
    # (gains far above the conductances: the row sums of G and of G^T then differ, 1025 against 524)
    vals[0, gains] = rng.choice([32.0, 64.0, 128.0], int(gains.sum()))
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    h.upload_values(vals)
    assert h.assemble_numeric(0)[0] == _ffi.OK
    _, info, _, _ = h.solve_sparse()
    assert info == 0
    h.sensitivities([0], [0], [-1], dense=False)  # (leaves the child with G^T on the handle)
    G, _ = csr_of(h)
    assert np.array_equal(G[2] * 8, np.round(G[2] * 8))  # exact: multiples of 1/8
    nn = h.n
    Gt = spsp.csr_matrix((G[2], G[1], G[0]), shape=(nn, nn)).T.tocsr()
    Gt.sort_indices()
    Gt = (Gt.indptr.astype(np.int64), Gt.indices.astype(np.int64), Gt.data)
    x, b = integer_vectors(rng, nn)
    want_t, want = host_norms(Gt, x, b), host_norms(G, x, b)
    assert want_t[0] != want[0] and want_t[1] != want[1]  # (the two matrices tell themselves apart on this data)
    for cols, layout in ((0, 0), (1, 2), (1, 0)):
        for transposed, w in ((True, want_t), (False, want)):
            if cols == 0:
                scaled, norms = h.debug_residual(x, b, transposed=transposed)
                got = list(norms[:4])
            else:
                xs, bs = (x, b) if layout == 2 else (x[None, :], b[None, :])
                s, nr = h.debug_residual(xs, bs, cols=1, layout=layout, transposed=transposed)
                scaled, got = s[0], [nr[0, 0], nr[0, 3], nr[0, 1], nr[0, 2]]
            assert np.array_equal(got, w), (cols, layout, transposed, got, w)
            assert one_ulp(scaled, host_scaled(*w))
    h.close()


def test_batch_residual_against_the_members_exports():
    """nodal_residual() after nodal_run_batch is the single-vector judge (parts A and D pin it) on the block-diagonal
    system of the members.  At a converged solution the numerator is rounding noise, so against the host this is mostly
    an upper-side check: |device - host| within the bound of part C carried through the quotient,
        (bound_r + r (k_max + 6) u) / den,
    the second term for the roundings of |G|_inf, the product, the sum and the division.  (grid(24) with a 1 A source:
    every member's right-hand side already lies in [1, 2), so the batch's per-member scales are all 1.)"""
    table = gen.grid_table(24)
    members = 3
    rng = np.random.default_rng(31)
    vals = np.tile(np.asarray(table.value, dtype=np.float64), (members, 1))
    vals[:, :-1] = 10.0 ** rng.uniform(-1.0, 1.0, (members, table.ncomp - 1))
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    h.upload_values(vals)
    exports = []
    for m in range(members):
        assert h.assemble_numeric(m)[0] == _ffi.OK
        exports.append(csr_of(h))
    assert all(1.0 <= np.abs(rhs).max() < 2.0 for _, rhs in exports)  # the premise: every member's scale is 1
    x, info = h.run_batch(0, members)
    assert not info.any()
    reported = h.residual()
    L = np.longdouble
    parts = [host_norms(G, x[m], rhs, L) for m, (G, rhs) in enumerate(exports)]
    bounds = [rounding_bounds(G, x[m], rhs) for m, (G, rhs) in enumerate(exports)]
    r, an, xn, bn = (max(p[k] for p in parts) for k in range(4))
    den = an * xn + bn
    bound_r, kmax = max(bd[0] for bd in bounds), max(bd[2] for bd in bounds)
    allow = (bound_r + r * (kmax + 6) * L(U)) / den
    assert abs(L(reported) - r / den) <= allow, (reported, float(r / den), float(allow))
    assert 0.0 <= reported <= 1e-12
    h.close()
