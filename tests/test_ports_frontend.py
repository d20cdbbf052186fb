"""Multiport equivalents without a device: resolve_ports, the PortEquivalent container built from the arrays of the
numpy restatement (tests/port_reference.py), and the argument checks of equiv.resistance_matrix."""
import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import generators as gen
from nodal_amd.equiv import resistance_matrix
from nodal_amd.ports import PortEquivalent, resolve_ports
from oracle import nodal_oracle as oracle
from tests import port_reference as ref
from tests.test_gpu_sweep import _random_rows

ROWS = [["r1", "R", "2", "1", "2"], ["r2", "R", "3", "2", "g"], ["r3", "R", "4", "1", "g"], ["a1", "A", "1", "1", "g"],
        ["r4", "R", "5", "3", "2"], ["r5", "R", "6", "3", "g"], ["a2", "A", "-0.5", "3", "2"]]


def _equivalent(rows, ports, sources=True):
    nl = n.Netlist.from_rows(rows)
    r = ref.PortReference(ref.Reference(nl, sparse=False, transposed=False), ports)
    count = len(ports)
    return nl, r, PortEquivalent(nl, ports, r.z, r.v_oc if sources else None, np.zeros(count, dtype=np.int32),
                                 np.zeros(count))


# ---- resolve_ports -------------------------------------------------------------------------------------------------
def test_resolve_ports_forms():
    nl = n.Netlist.from_rows(ROWS)
    idx, g = nl.nodenum, nl.ground
    ia, ib = resolve_ports(nl, [("1", "2"), ("2", g), (g, "3"), "3", ["1", "1"], (g, g)])
    assert ia.dtype == ib.dtype == np.int32
    assert ia.tolist() == [idx["1"], idx["2"], -1, idx["3"], idx["1"], -1]
    assert ib.tolist() == [idx["2"], -1, idx["3"], -1, idx["1"], -1]
    empty = resolve_ports(nl, [])
    assert all(len(a) == 0 and a.dtype == np.int32 for a in empty)
    assert n.resolve_ports is resolve_ports and n.PortEquivalent is PortEquivalent


def test_resolve_ports_errors():
    nl = n.Netlist.from_rows(ROWS)
    with pytest.raises(KeyError) as exc:
        resolve_ports(nl, [("1", "no such node")])
    assert exc.value.args[0] == "Node `no such node` not found in netlist"
    with pytest.raises(KeyError):
        resolve_ports(nl, ["nowhere"])
    for bad in [("1",), ("1", "2", "3"), ()]:
        with pytest.raises(ValueError):
            resolve_ports(nl, [bad])


# ---- PortEquivalent ------------------------------------------------------------------------------------------------
def test_norton_and_loaded():
    ports = [("1", "g"), ("3", "2"), ("2", "g")]
    nl, r, eq = _equivalent(ROWS, ports)
    assert len(eq) == 3 and eq.ports == ports
    y, i_sc = eq.norton()
    assert np.array_equal(y, np.linalg.inv(r.z)) and np.array_equal(i_sc, np.linalg.inv(r.z) @ r.v_oc)
    assert np.array_equal(eq.loaded([np.inf] * 3), r.v_oc)
    loads = np.array([1.0, np.inf, 2.5])
    # the loaded network solved anew by the oracle
    rows = ROWS + [["zl0", "R", "1.0", "1", "g"], ["zl2", "R", "2.5", "2", "g"]]
    nl2 = n.Netlist.from_rows(rows)
    G, A, _ = oracle.build_model(nl2, False)
    x2 = np.linalg.solve(np.asarray(G, dtype=np.float64), np.asarray(A, dtype=np.float64).ravel())
    assert np.abs(eq.loaded(loads) - ref.port_voltages(nl2, x2, ports)).max() <= 1e-13
    with pytest.raises(ValueError):
        eq.loaded([1.0, 2.0])
    _, _, passive = _equivalent(ROWS, ports, sources=False)
    assert passive.v_oc is None and passive.norton()[1] is None
    with pytest.raises(ValueError, match="sources=False"):
        passive.loaded([1.0, 1.0, 1.0])
    text = str(eq)
    assert text.splitlines()[0] == "Ports: 3" and "port 1 (3, 2)" in text and "V_oc" in text


def test_reciprocity():
    _, r, eq = _equivalent(ROWS, [("1", "g"), ("3", "2")])
    assert eq.reciprocity() == float(np.abs(r.z - r.z.T).max() / np.abs(r.z).max()) <= 1e-15
    rows = gen.cfg5_rows(12)
    nl = n.Netlist.from_rows(rows)
    _, r5, eq5 = _equivalent(rows, ref.grounded_ports(nl, 5, 1))
    assert eq5.reciprocity() == float(np.abs(r5.z - r5.z.T).max() / np.abs(r5.z).max())
    nl0 = n.Netlist.from_rows(ROWS)
    assert PortEquivalent(nl0, [], np.zeros((0, 0)), np.zeros(0), [], []).reciprocity() == 0.0
    assert PortEquivalent(nl0, [("g", "g")], np.zeros((1, 1)), np.zeros(1), [0], [0.0]).reciprocity() == 0.0


def test_rows_refusals():
    nl, r, eq = _equivalent(ROWS, [("1", "g"), ("3", "2")])
    with pytest.raises(ValueError, match="ground-referenced"):
        eq.rows()
    with pytest.raises(ValueError, match="ground-referenced"):
        _equivalent(ROWS, [("1", "g"), ("g", "2")])[2].rows()
    with pytest.raises(ValueError, match="distinct"):
        _equivalent(ROWS, [("1", "g"), ("1", "g")])[2].rows()
    good = [("1", "g"), ("3", "g")]
    nl, r, eq = _equivalent(ROWS, good)
    singular = PortEquivalent(nl, good, r.z, r.v_oc, [0, 1], [0.0, 0.0])
    with pytest.raises(ValueError, match="singular"):
        singular.rows()
    skew = r.z.copy()
    skew[0, 1] *= 1.0 + 1e-8
    with pytest.raises(ValueError, match="reciprocal"):
        PortEquivalent(nl, good, skew, r.v_oc, [0, 0], [0.0, 0.0]).rows()
    nan = np.full((2, 2), np.nan)
    with pytest.raises(ValueError):
        PortEquivalent(nl, good, nan, r.v_oc, [0, 0], [0.0, 0.0]).rows()
    # a network with dependent sources is refused for what it is
    rows5 = _random_rows(0)
    nl5 = n.Netlist.from_rows(rows5)
    _, _, eq5 = _equivalent(rows5, ref.grounded_ports(nl5, 4, 2))
    assert eq5.reciprocity() > 1e-9
    with pytest.raises(ValueError, match="reciprocal"):
        eq5.rows()


def test_rows_format_and_round_trip():
    ports = [("1", "g"), ("3", "g"), ("2", "g")]
    nl, r, eq = _equivalent(ROWS, ports)
    rows = eq.rows()
    y = np.linalg.inv(r.z)
    i_sc = y @ r.v_oc
    names = [row[0] for row in rows]
    assert len(set(names)) == len(names) and all(name.startswith("eq") for name in names)
    assert all(len(row) == 5 and row[1] in ("R", "A") and isinstance(row[2], str) for row in rows)
    by_name = {row[0]: row for row in rows}
    # nodes 1 and 3 are not adjacent: Y_01 is rounding noise and gets no resistor; 1-2 and 3-2 are
    assert "eqr0_1" not in by_name
    assert by_name["eqr0_2"] == ["eqr0_2", "R", repr(float(-1.0 / y[0, 2])), "1", "2"]
    assert by_name["eqr1_2"][3:] == ["3", "2"]
    for i, node in enumerate(["1", "3", "2"]):
        assert by_name[f"eqr{i}_g"] == [f"eqr{i}_g", "R", repr(float(1.0 / y[i].sum())), node, "g"]
        assert by_name[f"eqa{i}"] == [f"eqa{i}", "A", repr(float(i_sc[i])), node, "g"]
    assert [row[0] for row in eq.rows(prefix="th")][0].startswith("thr")
    # the reduced netlist alone reproduces the terminals' potentials, and with an external circuit attached the
    # full network's
    external = [["xr", "R", "2", "1", "xn"], ["xs", "R", "3", "xn", "3"], ["xa", "A", "0.25", "xn", "g"]]
    for extra in ([], external):
        nl_red = n.Netlist.from_rows(rows + extra)
        nl_full = n.Netlist.from_rows(ROWS + extra)
        xs = []
        for net in (nl_red, nl_full):
            G, A, _ = oracle.build_model(net, False)
            x = np.linalg.solve(np.asarray(G, dtype=np.float64), np.asarray(A, dtype=np.float64).ravel())
            xs.append(np.array([x[net.nodenum[name]] for name in ["1", "3", "2"] + (["xn"] if extra else [])]))
        assert np.abs(xs[0] - xs[1]).max() <= 1e-13
    _, _, passive = _equivalent(ROWS, ports, sources=False)
    assert [row for row in passive.rows() if row[1] == "A"] == []
    assert [row for row in passive.rows()] == [row for row in rows if row[1] == "R"]


# ---- the port sample of the G-not-G^T check --------------------------------------------------------------------------
def test_the_transposed_reference_is_far_away():
    """tests/test_gpu_ports.py test 4 wants Z from G^T to miss the bars by a factor above 100 on its port sample: here
    from the two references alone (the right one standing in for the device's answer)."""
    from tests.test_gpu_ports import CFG5_SEED
    nl = n.Netlist.from_rows(gen.cfg5_rows(95))
    ports = ref.sample_ports(nl, 18, CFG5_SEED)
    right = ref.PortReference(ref.Reference(nl, sparse=True, transposed=False), ports)
    wrong = ref.PortReference(ref.Reference(nl, sparse=True, transposed=True), ports)
    miss = wrong.worst_miss(right.z)
    print("cfg5(95): Z from G^T misses the bars of Z from G by a factor", miss)
    assert miss > 100.0


# ---- resistance_matrix: the checks that need no device ---------------------------------------------------------------
def test_resistance_matrix_argument_checks():
    with pytest.raises(ValueError, match="not resistive"):
        resistance_matrix(n.Netlist.from_rows(ROWS), ["1", "2"])
    resistive = n.Netlist.from_rows([row for row in ROWS if row[1] == "R"])
    with pytest.raises(KeyError) as exc:
        resistance_matrix(resistive, ["1", "nowhere"])
    assert exc.value.args[0] == "Node `nowhere` not found in netlist"
    assert resistance_matrix(resistive, []).shape == (0, 0)
    assert np.array_equal(resistance_matrix(resistive, ["1"]), np.zeros((1, 1)))
