"""Branch currents, power and sweep envelopes on the GPU (Circuit.branches / nodal_branches,
Circuit.solve_sources(branches=True) / nodal_solve_sources_branches).  Every expected value is computed here with
numpy from the solution vector and the columns of the lowered table, never by product code."""
import math
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd import generators as gen
from nodal_amd.circuit import MatrixRankWarning
from nodal_amd.lowering import lower
from nodal_amd.sweep import resolve_sources
from oracle import nodal_oracle as oracle
from tests.conftest import load_golden
from tests.test_gpu_sweep import _grid_with_loads, _random_rows, rebuilt, sweep_of

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


# ---- the definitions, in numpy ------------------------------------------------------------------------------------
def expected(table, x, value=None):
    """voltage, current, power per table row from x (value: the value column in force)"""
    value = np.asarray(table.value if value is None else value, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    a, b, k, t = (np.asarray(col) for col in (table.a, table.b, table.k, table.type))
    xe = np.append(x, 0.0)  # (index -1, the ground lead, reads the appended +0.0)
    v = xe[a] - xe[b]
    with np.errstate(all="ignore"):
        res = v / value
    branch = xe[np.where(k >= 0, table.K + k, -1)]
    cur = np.where(t == 0, res, np.where(t == 1, value, branch))
    with np.errstate(all="ignore"):
        vc = v * cur
    return v, cur, np.where(t == 0, vc, -vc)


def net_currents(table, cur):
    a, b, t = np.asarray(table.a), np.asarray(table.b), np.asarray(table.type)
    K = table.K
    signed = np.where(t == 0, 1.0, -1.0) * cur
    into = np.bincount(np.where(a < 0, K, a), weights=signed, minlength=K + 1)
    out = np.bincount(np.where(b < 0, K, b), weights=signed, minlength=K + 1)
    return (into - out)[:K]


def check_rows(table, x, v, cur, p, dissipated, absorbed, value=None, tag=None):
    """the bars of test 1 on every row"""
    wv, wc, _ = expected(table, x, value)
    t = np.asarray(table.type)
    assert np.array_equal(v, wv, equal_nan=True), tag
    other = t != 0
    assert np.array_equal(cur[other], wc[other], equal_nan=True), tag
    with np.errstate(all="ignore"):
        off = np.abs(cur[~other] - wc[~other])
        print(tag, "R rows:", int((~other).sum()), "max |current - numpy| / spacing:",
              float(np.nanmax(off / np.spacing(np.abs(wc[~other])), initial=0.0)))
        assert (off <= np.spacing(np.abs(wc[~other]))).all(), tag
        vc = v * cur
    assert np.array_equal(p, np.where(other, -vc, vc), equal_nan=True), tag
    tol = 1e-12 * math.fsum(np.abs(p))
    print(tag, "totals off by", abs(dissipated - math.fsum(p[~other])), abs(absorbed - math.fsum(p[other])), "bar", tol)
    assert abs(dissipated - math.fsum(p[~other])) <= tol, tag
    assert abs(absorbed - math.fsum(p[other])) <= tol, tag


def kcl_bar(G, A, x, r):
    G = G.tocsr()
    maxdeg = int(np.diff(G.indptr).max())
    gnorm = float(abs(G).sum(axis=1).max())
    return (r + 2 * (maxdeg + 2) * EPS) * (gnorm * np.abs(x).max() + np.abs(A).max())


def scaled_residual(G, A, x):
    G = G.tocsr()
    den = float(abs(G).sum(axis=1).max()) * np.abs(x).max() + np.abs(A).max()
    return np.abs(G @ x - A).max() / den


def check_kirchhoff(table, G, A, x, r, cur, p, dissipated, absorbed, tag=None):
    bar = kcl_bar(G, np.asarray(A, dtype=np.float64).ravel(), x, r)
    net = np.abs(net_currents(table, cur)).max(initial=0.0)
    tel = abs(dissipated + absorbed)
    tel_bar = np.abs(x[:table.K]).sum() * bar + 1e-12 * math.fsum(np.abs(p))
    print(tag, "max|net|", net, "bar", bar, "Tellegen", tel, "bar", tel_bar)
    assert net <= bar, tag
    assert tel <= tel_bar, tag


# ---- inputs -------------------------------------------------------------------------------------------------------
def _golden():
    out = []
    for case in load_golden("cases.json"):
        if not case.get("rows") or "x" not in case.get("dense", {}) or "x" not in case.get("sparse", {}):
            continue
        if not (np.isfinite(np.asarray(case["dense"]["x"], dtype=float)).all()
                and np.isfinite(np.asarray(case["sparse"]["x"], dtype=float)).all()):
            continue
        out.append((case["name"], case["rows"]))
    return out


GOLDEN = _golden()
RANDOM = [(f"random{s}", _random_rows(s)) for s in range(4)]
INPUTS = GOLDEN + RANDOM + [("grid(60)", list(gen.grid_rows(60))), ("cfg5(24)", gen.cfg5_rows(24))]
# Kirchhoff / Tellegen: the inputs whose right-hand side is all zero (the bar is 0 / 0) and the 1e-17 ohm self-loop
# whose stamps destroy the low bits of G (G no longer describes the network) are left out, these four and no others
NO_KCL = ("doc/resistive_1", "doc/resistive_2", "doc/resistive_3", "edge/self_loop_r_bits")


def test_the_inputs_are_the_ones_the_checks_were_sized_for():
    assert len(GOLDEN) == 23 and len(INPUTS) == 29
    assert all(name in [g[0] for g in GOLDEN] for name in NO_KCL)


# ---- 1, 2: element parity, Kirchhoff and Tellegen after solve() ----------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("k", range(len(INPUTS)), ids=[i[0] for i in INPUTS])
def test_branches_after_solve(k, sparse):
    name, rows = INPUTS[k]
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    x = np.array(c.solve().result)
    br = c.branches()
    table = lower(nl)
    assert br.names == nl.component_keys and len(br) == table.ncomp
    v, cur, p = (np.asarray(q) for q in (br.voltage, br.current, br.power))
    check_rows(table, x, v, cur, p, br.dissipated, br.absorbed_by_sources, tag=(name, sparse))
    if name in NO_KCL:
        return
    G, A, _ = oracle.build_model(nl, True)
    A = np.asarray(A, dtype=np.float64).ravel()
    check_kirchhoff(table, G, A, x, scaled_residual(G, A, x), cur, p, br.dissipated, br.absorbed_by_sources,
                    tag=(name, sparse))
    # the container's own host-side check agrees with the test's
    assert np.abs(br.kcl_residual()).max(initial=0.0) <= kcl_bar(G, A, x, scaled_residual(G, A, x))


# ---- 3: full size through the handle ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["grid1000", "cfg5_1000", "ladder100000", "grid60_dense"])
def test_full_size_through_the_handle(which):
    import scipy.sparse as spsp
    table, dense = {"grid1000": (lambda: gen.grid_table(1000), False), "cfg5_1000": (lambda: gen.cfg5_table(1000), False),
                    "ladder100000": (lambda: gen.ladder_table(100000), False),
                    "grid60_dense": (lambda: gen.grid_table(60), True)}[which]
    table = table()
    h = _ffi.Handle(0)
    try:
        h.upload(table)
        assert h.run(dense) == 0
        v, cur, p, dissipated, absorbed = h.branches()
        x = np.array(h.download_x())
        r = h.residual()
        indptr, indices, data, rhs = h.export_csr()
    finally:
        h.close()
    v, cur, p = np.array(v), np.array(cur), np.array(p)
    check_rows(table, x, v, cur, p, dissipated, absorbed, tag=which)
    G = spsp.csr_matrix((data, indices, indptr), shape=(len(x), len(x)))
    check_kirchhoff(table, G, np.array(rhs), x, r, cur, p, dissipated, absorbed, tag=which)


# ---- 4: the value column in force is the member's ------------------------------------------------------------------
def test_value_table_member():
    table = gen.grid_table(60)
    vals = np.ones((3, table.ncomp))
    for b in range(3):
        vals[b, :-1] = gen.cfg4_values(b, 60)
    h = _ffi.Handle(0)
    try:
        h.upload(table)
        h.upload_values(vals)
        assert h.run(False, member=2) == 0
        v, cur, p, dissipated, absorbed = h.branches()
        x = np.array(h.download_x())
    finally:
        h.close()
    v, cur, p = np.array(v), np.array(cur), np.array(p)
    check_rows(table, x, v, cur, p, dissipated, absorbed, value=vals[2], tag="member 2")
    res = np.asarray(table.type) == 0
    other = expected(table, x, vals[0])[1]
    assert (np.abs(cur[res] - other[res]) > np.spacing(np.abs(other[res]))).any()


# ---- 5: sweep envelopes against the sweep's own result -------------------------------------------------------------
def check_envelope(nl, sources, sw, tag=None):
    table = lower(nl)
    tab_rows, values = resolve_sources(nl, sources)
    M, K = values.shape[0], table.K
    env = sw.envelope
    assert (sw.info == 0).all(), tag
    res = sw.result
    assert np.array_equal(env.potential_min, res[:, :K].min(0)), tag
    assert np.array_equal(env.potential_max, res[:, :K].max(0)), tag
    assert np.array_equal(env.potential_min_member, np.argmin(res[:, :K], axis=0)), tag
    assert np.array_equal(env.potential_max_member, np.argmax(res[:, :K], axis=0)), tag
    curs = np.empty((M, table.ncomp))
    t = np.asarray(table.type)
    other = t != 0
    for m in range(M):
        value = np.array(table.value, dtype=np.float64)
        value[tab_rows] = values[m]
        _, curs[m], p = expected(table, res[m], value)
        tol = 1e-12 * math.fsum(np.abs(p))
        assert abs(env.dissipated[m] - math.fsum(p[~other])) <= tol, (tag, m)
        assert abs(env.absorbed_by_sources[m] - math.fsum(p[other])) <= tol, (tag, m)
    want = np.abs(curs).max(0)
    assert np.array_equal(env.current_absmax[other], want[other]), tag
    assert (np.abs(env.current_absmax[~other] - want[~other]) <= np.spacing(want[~other])).all(), tag
    assert ((env.current_member >= 0) & (env.current_member < M)).all(), tag
    attained = np.abs(curs[env.current_member, np.arange(table.ncomp)])
    assert (np.abs(attained - env.current_absmax) <= np.spacing(env.current_absmax)).all(), tag
    for j, row in enumerate(tab_rows):
        if t[row] == 1:
            assert env.current_absmax[row] == np.abs(values[:, j]).max(), tag


SWEEPABLE = [(name, rows, sorted({r[0] for r in rows if len(r) > 1 and r[1] in ("A", "E")})) for name, rows in GOLDEN]
SWEEPABLE = [s for s in SWEEPABLE if s[2]] + [(name, rows, ["a0", "a1", "e0"]) for name, rows in RANDOM]


@pytest.mark.parametrize("M", [19, 37])
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_envelope_small_networks(sparse, M):
    for k, (name, rows, names) in enumerate(SWEEPABLE):
        sources = sweep_of(rows, names, M, 50 + k)
        nl = n.Netlist.from_rows(rows)
        sw = n.Circuit(nl, sparse=sparse).solve_sources(sources, branches=True)
        assert sw.result.shape[0] == M
        check_envelope(nl, sources, sw, tag=(name, sparse, M))


def test_envelope_dense_chunk_edge():
    """513 members on the dense route: the envelope is fed one full chunk of 512 and a chunk of one"""
    rows, names = _grid_with_loads(6, 3, 6)
    sources = sweep_of(rows, names, 513, 513)
    nl = n.Netlist.from_rows(rows)
    sw = n.Circuit(nl, sparse=False).solve_sources(sources, branches=True)
    assert sw.result.shape[0] == 513
    check_envelope(nl, sources, sw, tag=("grid(6) with loads", 513))


@pytest.fixture(scope="module")
def grid300():
    rows, names = _grid_with_loads(300, 6, 3)
    return rows, names, n.Netlist.from_rows(rows)


@pytest.fixture(scope="module")
def cfg5_100():
    rows = gen.cfg5_rows(100)
    names = sorted(r[0] for r in rows if r[1] == "E")[:3]
    return rows, names, n.Netlist.from_rows(rows)


@pytest.mark.parametrize("M", [19, 37])
def test_envelope_block_multigrid_route(grid300, M):
    rows, names, nl = grid300
    sources = sweep_of(rows, names, M, M)
    sw = n.Circuit(nl, sparse=True).solve_sources(sources, branches=True)
    check_envelope(nl, sources, sw, tag=("grid300", M))


@pytest.mark.parametrize("M", [19, 37])
def test_envelope_sparse_lu_route(cfg5_100, M):
    rows, names, nl = cfg5_100
    sources = sweep_of(rows, names, M, M)
    c = n.Circuit(nl, sparse=True)
    assert c._handle.n > 8192
    sw = c.solve_sources(sources, branches=True)
    check_envelope(nl, sources, sw, tag=("cfg5(100)", M))


def test_defaults_are_todays_sweep(grid300):
    rows, names, nl = grid300
    sources = sweep_of(rows, names, 5, 1)
    c = n.Circuit(nl, sparse=True)
    plain = c.solve_sources(sources)
    assert plain.envelope is None and plain.result.shape == (5, c._handle.n)
    with_env = c.solve_sources(sources, branches=True)
    assert np.array_equal(plain.result, with_env.result) and np.array_equal(plain.info, with_env.info)
    empty = c.solve_sources({names[0]: []}, branches=True)
    assert len(empty) == 0 and empty.result.shape == (0, c._handle.n)
    assert np.isnan(empty.envelope.current_absmax).all() and (empty.envelope.potential_min_member == -1).all()
    assert empty.envelope.current_absmax.shape == (len(nl.component_keys),)


# ---- 6: without the members' solutions, against the CPU reference model --------------------------------------------
# Members: 19 = the first member alone, a full block of sixteen, a partial block.  The reference model is built once per
# member from the rebuilt netlist (its G does not depend on the member, so it is factored once).
def _reference_envelope(rows, sources, nl, M):
    import scipy.sparse.linalg as spla
    table = lower(nl)
    tab_rows, values = resolve_sources(nl, sources)
    G, _, _ = oracle.build_model(nl, True)
    lu = spla.splu(G.tocsc())
    xs, curs = [], []
    for m in range(M):
        _, A, _ = oracle.build_model(n.Netlist.from_rows(rebuilt(rows, sources, m)), True)
        x = lu.solve(np.asarray(A, dtype=np.float64).ravel())
        value = np.array(table.value, dtype=np.float64)
        value[tab_rows] = values[m]
        xs.append(x)
        curs.append(expected(table, x, value)[1])
    return table, np.array(xs), np.array(curs)


def _check_against_reference(rows, names, nl, M, tag):
    sources = sweep_of(rows, names, M, 77)
    c = n.Circuit(nl, sparse=True)
    sw = c.solve_sources(sources, branches=True, keep_solutions=False)
    assert sw.result is None and len(sw) == M and (sw.info == 0).all()
    with pytest.raises(ValueError):
        sw[0]
    table, xs, curs = _reference_envelope(rows, sources, nl, M)
    K, env = table.K, sw.envelope
    scale = np.abs(xs).max()
    pot = max(np.abs(env.potential_min - xs[:, :K].min(0)).max(), np.abs(env.potential_max - xs[:, :K].max(0)).max())
    print(tag, "potentials off by", pot / scale, "of the scale (bar 1e-9)")
    assert pot / scale <= 1e-9
    res = np.asarray(table.type) == 0
    bar = 2e-9 * scale * max(1.0, 1.0 / np.abs(np.asarray(table.value)[res]).min())
    off = np.abs(env.current_absmax - np.abs(curs).max(0)).max()
    print(tag, "currents off by", off, "bar", bar)
    assert off <= bar
    assert ((env.current_member >= 0) & (env.current_member < M)).all()


def test_no_solutions_kept_grid(grid300):
    rows, names, nl = grid300
    _check_against_reference(rows, names, nl, 19, "grid300")


def test_no_solutions_kept_branches(cfg5_100):
    rows, names, nl = cfg5_100
    _check_against_reference(rows, names, nl, 19, "cfg5(100)")


# ---- 7: singular networks -----------------------------------------------------------------------------------------
def _island():
    rows = list(gen.grid_rows(70))
    rows += [[f"f{i}", "R", "1", f"x{i}", f"x{i + 1}"] for i in range(40)]
    rows += [["fa", "A", "1", "x3", "x17"]]
    return rows


def test_floating_island_envelope_is_empty():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        sw = c.solve_sources({"a1": [1.0, 2.0, 3.0], "fa": [0.5, 0.0, 1.0]}, branches=True)
    assert (sw.info > 0).all() and np.isnan(sw.result).all()
    assert sum(issubclass(i.category, MatrixRankWarning) for i in w) == 1
    env = sw.envelope
    for arr in (env.current_absmax, env.potential_min, env.potential_max, env.dissipated, env.absorbed_by_sources):
        assert np.isnan(arr).all()
    for arr in (env.current_member, env.potential_min_member, env.potential_max_member):
        assert (arr == -1).all()
    assert env.dissipated.shape == (3,) and env.current_absmax.shape == (len(nl.component_keys),)


def test_branches_of_a_singular_sparse_solution_are_nan():
    nl = n.Netlist.from_rows(_island())
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x = c.solve().result
    assert np.isnan(x).all()
    br = c.branches()
    table = lower(nl)
    src = np.asarray(table.type) == 1
    assert np.isnan(br.voltage).all() and np.isnan(br.power).all()
    assert np.isnan(np.asarray(br.current)[~src]).all()
    assert np.array_equal(np.asarray(br.current)[src], np.asarray(table.value)[src])
    assert np.isnan(br.dissipated) and np.isnan(br.absorbed_by_sources)


# ---- 8: call order ------------------------------------------------------------------------------------------------
def test_call_order():
    rows = _random_rows(1)
    c = n.Circuit(n.Netlist.from_rows(rows), sparse=True)
    with pytest.raises(ValueError, match="no solution"):
        c.branches()
    c.solve()
    first = c.branches()
    c.solve_sources({"a0": [1.0, 2.0]})
    with pytest.raises(_ffi.NodalHipError) as exc:
        c._handle.branches()
    assert exc.value.status == _ffi.E_INVALID
    with pytest.raises(ValueError, match="no solution"):
        c.branches()
    c.solve()
    again = c.branches()
    assert np.array_equal(first.current, again.current) and first.dissipated == again.dissipated


# ---- 9: the totals repeat bit for bit ------------------------------------------------------------------------------
def test_totals_repeat_bit_for_bit(grid300):
    rows, names, nl = grid300
    sources = sweep_of(rows, names, 20, 9)
    c = n.Circuit(nl, sparse=True)
    one = c.solve_sources(sources, branches=True)
    two = c.solve_sources(sources, branches=True)
    if not np.array_equal(one.result, two.result):
        pytest.skip("the two sweeps' solutions differ in their bits: the solver's business, not the envelope's")
    assert np.array_equal(one.envelope.dissipated, two.envelope.dissipated)
    assert np.array_equal(one.envelope.absorbed_by_sources, two.envelope.absorbed_by_sources)
    assert np.array_equal(one.envelope.current_absmax, two.envelope.current_absmax)
