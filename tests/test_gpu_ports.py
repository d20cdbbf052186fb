"""Multiport Thevenin / Norton equivalents on the GPU (Circuit.thevenin / nodal_port_matrix, equiv.resistance_matrix).
Every expected value comes from the numpy restatement of tests/port_reference.py (the oracle's G, an LU of it, the
definitions of Z and V_oc), never from product code; the bars are stated there."""
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd import generators as gen
from nodal_amd.circuit import MatrixRankWarning
from nodal_amd.equiv import equivalent_resistance_sweep, resistance_matrix
from oracle import nodal_oracle as oracle
from tests import port_reference as ref
from tests.port_reference import TOL
from tests.test_gpu_branches import INPUTS, _island
from tests.test_gpu_sensitivity import _ladder_rows
from tests.test_gpu_sweep import _grid_with_loads, _random_rows

pytestmark = pytest.mark.gpu

SMALL = 60  # unknowns up to which every node is a port


def check_parity(eq, r, tag, resid_bar=1e-12):
    """info, residuals, Z and V_oc within their bars, the entries defined as 0 exactly 0; returns the worst
    |got - want| / bar"""
    count = len(r.ports)
    assert eq.z.shape == (count, count) and eq.info.shape == (count,) and eq.scaled_residual.shape == (count,)
    assert (eq.info == 0).all(), tag
    print(tag, "ports", count, "largest scaled residual:", float(eq.scaled_residual.max(initial=0.0)))
    assert (eq.scaled_residual <= resid_bar).all(), (tag, float(eq.scaled_residual.max()))
    off = np.abs(eq.z - r.z)
    worst = r.worst_miss(eq.z)
    print(tag, "worst |Z - Z_ref| / bar:", worst)
    assert (off <= r.z_bar).all(), (tag, worst)
    for p in np.flatnonzero(r.ia == r.ib):  # (ground, ground) and (node, same node)
        assert not eq.z[p, :].any() and not eq.z[:, p].any(), (tag, int(p))
    if eq.v_oc is not None:
        voff = np.abs(eq.v_oc - r.v_oc)
        with np.errstate(all="ignore"):
            print(tag, "worst |V_oc - V_ref| / bar:", float(np.where(r.v_bar > 0, voff / r.v_bar, 0.0).max(initial=0.0)))
        assert (voff <= r.v_bar).all(), tag
        assert not eq.v_oc[r.ia == r.ib].any(), tag
    return worst


# ---- 1: parity on every small input --------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("k", range(len(INPUTS)), ids=[i[0] for i in INPUTS])
def test_parity_on_every_small_input(k, sparse):
    name, rows = INPUTS[k]
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    c.solve()
    table = ref.table_of(nl)
    small = table.K + table.B <= SMALL
    ports = ref.small_ports(nl) if small else ref.sample_ports(nl, 33, 200 + k)
    if not small:
        ia, ib = ref.port_indices(nl, ports)
        assert len(ports) == 33 and (ia == -1).any() and ((ia == ib) & (ia >= 0)).any()
    eq = c.thevenin(ports)
    r = ref.PortReference(ref.Reference(nl, sparse=not small, transposed=False), ports)
    check_parity(eq, r, (name, sparse))
    assert eq.ports == ports
    if small and table.K > 0:  # the reversed port: its row is the negative, bit for bit
        fwd, rev = table.K + 1, table.K + 2
        assert np.array_equal(eq.z[rev], -eq.z[fwd])


# ---- 2, 3: the multigrid route -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid300():
    rows, _ = _grid_with_loads(300, 6, 3)
    nl = n.Netlist.from_rows(rows)
    return rows, nl, ref.Reference(nl, sparse=True, transposed=False)


@pytest.fixture(scope="module")
def cfg5_95():
    rows = gen.cfg5_rows(95)  # 9025 grid nodes plus branches: above 8192 unknowns, not passive
    nl = n.Netlist.from_rows(rows)
    return rows, nl, ref.Reference(nl, sparse=True, transposed=False)


def _with_ground(nl, count, seed):
    ports = ref.sample_ports(nl, count, seed)
    ports[count // 2] = (nl.ground, nl.ground)  # an all-zero column and row in the middle
    return ports


@pytest.mark.parametrize("P", [1, 2, 16, 17, 33])
def test_block_boundaries_on_the_multigrid_route(grid300, P):
    rows, nl, r0 = grid300
    c = n.Circuit(nl, sparse=True)
    assert c._handle.n == 89999
    c.solve()
    ports = _with_ground(nl, P, P)
    eq = c.thevenin(ports)
    r = ref.PortReference(r0, ports)
    check_parity(eq, r, ("grid300", P))
    print("grid300", P, "reciprocity:", eq.reciprocity())
    assert eq.reciprocity() <= 4 * TOL
    assert not eq.z[P // 2, :].any() and not eq.z[:, P // 2].any()


def test_block_failure_falls_back(grid300, monkeypatch):
    rows, nl, r0 = grid300
    c = n.Circuit(nl, sparse=True)
    c.solve()
    ports = _with_ground(nl, 20, 11)
    monkeypatch.setenv("NODAL_FCG_MAXIT", "3")
    eq = c.thevenin(ports)
    monkeypatch.delenv("NODAL_FCG_MAXIT")
    check_parity(eq, ref.PortReference(r0, ports), ("grid300, block iteration capped", 20))


# ---- 4: the sparse LU route, and G not G^T -------------------------------------------------------------------------
CFG5_SEED = 18  # the port sample for which G^T in place of G misses the bars by a factor above 100 (computed on the CPU
                # from the two references: see test_ports_frontend.py::test_the_transposed_reference_is_far_away)


def test_sparse_lu_route_and_the_matrix_is_not_transposed(cfg5_95):
    rows, nl, r0 = cfg5_95
    c = n.Circuit(nl, sparse=True)
    assert c._handle.n > 8192
    c.solve()
    ports = ref.sample_ports(nl, 18, CFG5_SEED)
    eq = c.thevenin(ports)
    check_parity(eq, ref.PortReference(r0, ports), ("cfg5(95)", 18), resid_bar=1e-14)
    wrong = ref.PortReference(ref.Reference(nl, sparse=True, transposed=True), ports)
    miss = wrong.worst_miss(eq.z)
    print("cfg5(95): with G^T in place of G the bar is missed by a factor", miss)
    assert miss > 100.0


def test_redo_branch_of_the_sparse_lu_route(cfg5_95, monkeypatch):
    """NODAL_MULTI_BAR=-1: every column fails the bar, is redone alone and the factors are made anew; then the same
    call with the switch off, on the same Circuit, meets the refinement's own bar again"""
    rows, nl, r0 = cfg5_95
    c = n.Circuit(nl, sparse=True)
    assert c._handle.n > 8192
    c.solve()
    ports = ref.sample_ports(nl, 18, CFG5_SEED)
    r = ref.PortReference(r0, ports)
    monkeypatch.setenv("NODAL_MULTI_BAR", "-1")
    redone = c.thevenin(ports)
    monkeypatch.delenv("NODAL_MULTI_BAR")
    check_parity(redone, r, ("cfg5(95), every column redone", 18))
    check_parity(c.thevenin(ports), r, ("cfg5(95), after the redo", 18), resid_bar=1e-14)
    wrong = ref.PortReference(ref.Reference(nl, sparse=True, transposed=True), ports)
    assert wrong.worst_miss(redone.z) > 100.0


# ---- 5, 6: the dense switch on a grid, a low-degree network -----------------------------------------------------------
def test_dense_switch_on_a_grid():
    nl = n.Netlist.from_rows(list(gen.grid_rows(40)))
    c = n.Circuit(nl, sparse=False)
    c.solve()
    ports = _with_ground(nl, 19, 40)
    eq = c.thevenin(ports)
    check_parity(eq, ref.PortReference(ref.Reference(nl, sparse=True, transposed=False), ports), ("grid(40) dense", 19))


def test_dense_chunk_edge():
    """513 ports on the dense route: Z is gathered from one full chunk of 512 columns and a chunk of one"""
    rows, _ = _grid_with_loads(6, 3, 6)
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=False)
    c.solve()
    ports = ref.sample_ports(nl, 513, 513)  # (drawn with repetition from 36 nodes and ground)
    ports[512], ports[511] = ports[0], ports[3]  # equal ports on both sides of the chunk edge
    eq = c.thevenin(ports)
    check_parity(eq, ref.PortReference(ref.Reference(nl, sparse=False, transposed=False), ports), ("grid(6) dense", 513))
    first = {}
    repeated = 0
    for q, port in enumerate(ports):
        p = first.setdefault(port, q)
        if p != q:
            repeated += 1
            assert np.array_equal(eq.z[:, q], eq.z[:, p]), (p, q)
    assert repeated > 100 and first[ports[0]] == 0


def test_low_degree_network():
    nl = n.Netlist.from_rows(_ladder_rows(20000))
    c = n.Circuit(nl, sparse=True)
    assert c._handle.n > 4096
    c.solve()
    ports = _with_ground(nl, 18, 7)
    eq = c.thevenin(ports)
    check_parity(eq, ref.PortReference(ref.Reference(nl, sparse=True, transposed=False), ports), ("ladder(20000)", 18))


# ---- 7: Thevenin under load, end to end ------------------------------------------------------------------------------
def _distinct_lead_ports(nl, seed):
    """five ports with ten distinct leads, one of them ground"""
    rng = np.random.default_rng(seed)
    labels = ref.node_labels(nl)
    picks = [labels[int(k)] for k in rng.choice(len(labels), size=9, replace=False)]
    return [(picks[0], picks[1]), (picks[2], picks[3]), (picks[4], nl.ground), (picks[5], picks[6]), (picks[7], picks[8])]


@pytest.mark.parametrize("which", ["grid300", "cfg5(95)"])
def test_thevenin_under_load(grid300, cfg5_95, which):
    rows, nl, r0 = grid300 if which == "grid300" else cfg5_95
    ports = _distinct_lead_ports(nl, 70)
    loads = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    loaded_rows = list(rows) + [[f"zl{p}", "R", repr(float(loads[p])), a, b] for p, (a, b) in enumerate(ports)]
    nl_loaded = n.Netlist.from_rows(loaded_rows)
    r = ref.PortReference(r0, ports)
    want, kappa = r.loaded(loads)
    x_loaded_ref = ref.Reference(nl_loaded, sparse=True, transposed=False).x
    bar = 3 * TOL * kappa * (np.abs(r0.x).max() + np.abs(x_loaded_ref).max())
    # the reference's own prediction meets the bar
    resolved = ref.port_voltages(nl_loaded, x_loaded_ref, ports)
    print(which, "kappa", kappa, "bar", bar, "reference prediction off by", float(np.abs(want - resolved).max()))
    assert np.abs(want - resolved).max() <= bar
    c = n.Circuit(nl, sparse=True)
    c.solve()
    predicted = c.thevenin(ports).loaded(loads)
    x_loaded = np.array(n.Circuit(nl_loaded, sparse=True).solve().result)
    got = ref.port_voltages(nl_loaded, x_loaded, ports)
    print(which, "predicted against re-solved on the device:", float(np.abs(predicted - got).max()))
    assert np.abs(predicted - got).max() <= bar
    assert np.abs(predicted - resolved).max() <= bar


# ---- 8: the reduced netlist ------------------------------------------------------------------------------------------
def test_reduced_netlist(grid300, cfg5_95):
    rows, nl, r0 = grid300
    ports = ref.grounded_ports(nl, 5, 80)
    t = [a for a, _ in ports]
    external = [["xr0", "R", "2", t[0], t[1]], ["xr1", "R", "3", t[1], "xn"], ["xr2", "R", "1.5", "xn", t[2]],
                ["xr3", "R", "4", t[3], t[4]], ["xa", "A", "0.5", "xn", "g"]]
    c = n.Circuit(nl, sparse=True)
    c.solve()
    eq = c.thevenin(ports)
    reduced = eq.rows() + external
    nl_red = n.Netlist.from_rows(reduced)
    x_red = np.array(n.Circuit(nl_red, sparse=True).solve().result)
    nl_full = n.Netlist.from_rows(list(rows) + external)
    x_full = np.array(n.Circuit(nl_full, sparse=True).solve().result)
    # kappa' from the reference: the reduced system is Y_ref on the terminals plus the external circuit's stamps
    r = ref.PortReference(r0, ports)
    G_red = np.zeros((6, 6))
    G_red[:5, :5] = np.linalg.inv(r.z)
    for i, j, ohms in [(0, 1, 2.0), (1, 5, 3.0), (5, 2, 1.5), (3, 4, 4.0)]:
        G_red[i, i] += 1 / ohms
        G_red[j, j] += 1 / ohms
        G_red[i, j] -= 1 / ohms
        G_red[j, i] -= 1 / ohms
    kappa = float(np.linalg.cond(G_red, np.inf))
    x_full_ref = ref.Reference(nl_full, sparse=True, transposed=False).x
    bar = 3 * TOL * kappa * np.abs(x_full_ref).max()
    names = t + ["xn"]
    got = np.array([x_red[nl_red.nodenum[name]] for name in names])
    want = np.array([x_full[nl_full.nodenum[name]] for name in names])
    want_ref = np.array([x_full_ref[nl_full.nodenum[name]] for name in names])
    print("reduced netlist: rows", len(reduced), "kappa'", kappa, "bar", bar, "off by", float(np.abs(got - want).max()),
          "against the reference", float(np.abs(got - want_ref).max()))
    assert np.abs(got - want).max() <= bar
    assert np.abs(got - want_ref).max() <= bar
    # a network with dependent sources is not reciprocal: no such netlist
    rows5, nl5, _ = cfg5_95
    c5 = n.Circuit(nl5, sparse=True)
    c5.solve()
    eq5 = c5.thevenin(ref.grounded_ports(nl5, 5, 81))
    assert eq5.reciprocity() > 1e-9
    with pytest.raises(ValueError, match="reciprocal"):
        eq5.rows()


# ---- 9: the resistance matrix ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_resistance_matrix(sparse):
    rows = [row for row in gen.grid_rows(60) if row[1] == "R"]
    nl = n.Netlist.from_rows(rows)
    terminals = [a for a, _ in ref.grounded_ports(nl, 6, 90)]
    R = resistance_matrix(nl, terminals, sparse=sparse)
    assert R.shape == (6, 6) and np.array_equal(R, R.T) and not np.diag(R).any()
    pairs = [(terminals[i], terminals[j]) for i in range(6) for j in range(i + 1, 6)]
    sweep = equivalent_resistance_sweep(nl, pairs, sparse=sparse)
    r = ref.PortReference(ref.Reference(nl, sparse=True, transposed=False), [(t, terminals[0]) for t in terminals[1:]])
    zp = np.zeros((6, 6))
    zp[1:, 1:] = r.z
    worst = 0.0
    for (i, j), want in zip([(i, j) for i in range(6) for j in range(i + 1, 6)], sweep):
        bar = TOL * (zp[i, i] + zp[j, j] + 2 * abs(zp[i, j])) + TOL * want
        worst = max(worst, abs(R[i, j] - want) / bar)
        assert abs(R[i, j] - want) <= bar, (i, j, R[i, j], want)
        assert abs(R[i, j] - (zp[i, i] + zp[j, j] - zp[i, j] - zp[j, i])) <= bar
    print("resistance matrix", "sparse" if sparse else "dense", "worst |R - sweep| / bar:", worst)


# ---- 10: nothing else moved ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("which", ["random0", "cfg5(24)"])
def test_nothing_else_moved(which, sparse):
    rows = _random_rows(0) if which == "random0" else gen.cfg5_rows(24)
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    x = np.array(c.solve().result)
    from tests import sensitivity_reference as sref
    specs = sref.sample_outputs(nl, sref.table_of(nl), 5, 3)

    def state():
        br = c.branches()
        sens = c.sensitivities(specs)
        c._G = c._A = None  # (exported anew)
        G = c.G
        parts = (G.indptr.copy(), G.indices.copy(), G.data.copy()) if hasattr(G, "indptr") else (np.array(G),)
        return (np.array(br.voltage), np.array(br.current), np.array(br.power), np.array(sens.values),
                np.array(sens.output_values), np.array(c._handle.download_x()), np.array(c.A),
                np.array(c._handle.solve_info())) + parts

    before = state()
    ports = ref.sample_ports(nl, 19, 4)
    one = c.thevenin(ports)
    after = state()
    assert len(before) == len(after)
    for b, a in zip(before, after):
        assert np.array_equal(b, a)
    assert np.array_equal(before[5], x)
    two = c.thevenin(ports)
    for name in ("z", "v_oc", "info", "scaled_residual"):
        assert np.array_equal(getattr(one, name), getattr(two, name)), name


# ---- 11: call order and empties --------------------------------------------------------------------------------------
def test_call_order_and_empties():
    rows = _random_rows(1)
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    with pytest.raises(ValueError, match="no solution"):
        c.thevenin([("1", "g")])
    early = c.thevenin([("1", "g"), "2"], sources=False)
    assert early.v_oc is None and early.z.shape == (2, 2) and early.ports == [("1", "g"), ("2", "g")]
    c.solve()
    first = c.thevenin([("1", "g"), "2"])
    assert np.array_equal(first.z, early.z) and first.v_oc.shape == (2,)
    c.solve_sources({"a0": [1.0, 2.0]})
    with pytest.raises(ValueError, match="no solution"):
        c.thevenin([("1", "g")])
    assert np.array_equal(c.thevenin([("1", "g"), "2"], sources=False).z, early.z)
    c.solve()
    empty = c.thevenin([])
    assert empty.z.shape == (0, 0) and empty.v_oc.shape == (0,) and empty.info.shape == (0,) and len(empty) == 0
    with pytest.raises(KeyError, match="not found in netlist"):
        c.thevenin([("1", "no such node")])
    K = nl.nums["kcl"]
    for ia, ib in [([K], [-1]), ([0], [K]), ([-2], [0]), ([0], [-2])]:
        with pytest.raises(_ffi.NodalHipError) as exc:
            c._handle.port_matrix(ia, ib, dense=False)
        assert exc.value.status == _ffi.E_INVALID
    assert np.array_equal(c.thevenin([("1", "g"), "2"]).z, first.z)


# ---- 12: a floating island -------------------------------------------------------------------------------------------
def test_floating_island():
    rows = _island()
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c.solve()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        eq = c.thevenin([("1", "g"), ("x3", "x17"), ("g", "g"), ("5", "5")])
    assert (eq.info > 0).all() and np.isnan(eq.z).all()
    assert sum(issubclass(i.category, MatrixRankWarning) for i in w) == 1
    cd = n.Circuit(nl, sparse=False)
    with pytest.raises(n.UnconnectedCircuitError):
        cd.thevenin([("1", "g"), ("x3", "x17")], sources=False)


# ---- 13: full size through the handle --------------------------------------------------------------------------------
def test_full_size_through_the_handle():
    table = gen.grid_table(1000)
    rng = np.random.default_rng(13)
    ia = rng.choice(table.K, size=17, replace=False).astype(np.int32)
    ib = np.full(17, -1, dtype=np.int32)
    h = _ffi.Handle(0)
    try:
        h.upload(table)
        h.assemble_symbolic()
        assert h.assemble_numeric(0)[0] == _ffi.OK
        z, v_oc, info, resid = h.port_matrix(ia, ib, dense=False, voc=False)
        pairs, pinfo = h.solve_pairs(ia, ib, dense=False)
    finally:
        h.close()
    assert v_oc is None and (info == 0).all() and pinfo == 0
    print("grid(1000): largest scaled residual", float(resid.max()))
    assert (resid <= 1e-12).all()
    reciprocity = float(np.abs(z - z.T).max() / np.abs(z).max())
    print("grid(1000): reciprocity", reciprocity, "worst |Z_qq - pair| / Z_qq", float((np.abs(np.diag(z) - pairs) / np.diag(z)).max()))
    assert reciprocity <= 4 * TOL
    assert (np.abs(np.diag(z) - pairs) <= 4 * TOL * np.diag(z)).all()
