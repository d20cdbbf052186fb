"""Adjoint sensitivities without a device: resolve_outputs, the Sensitivities container, and the numpy restatement
(tests/sensitivity_reference.py) itself against central differences of the oracle's own solves."""
import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import generators as gen
from nodal_amd.sensitivity import Sensitivities, resolve_outputs
from oracle import nodal_oracle as oracle
from tests import sensitivity_reference as ref
from tests.conftest import load_golden
from tests.test_gpu_sweep import _random_rows

ROWS = [["r1", "R", "2", "1", "2"], ["r2", "R", "3", "2", "g"], ["r3", "R", "4", "1", "g"], ["a1", "A", "1", "1", "g"],
        ["e1", "E", "1.5", "3", "g"], ["r4", "R", "5", "3", "2"]]


# ---- 1: resolve_outputs --------------------------------------------------------------------------------------------
def test_resolve_outputs_forms():
    nl = n.Netlist.from_rows(ROWS)
    ground = nl.ground
    nodes = [label for label in nl.nodenum]
    outputs = [("e", nodes[0]), ("e", ground), ("v", nodes[1], nodes[0]), ("v", ground, nodes[1]),
               ("v", nodes[0], ground), ("i", "r4"), ("i", "e1")]
    kind, p, q2 = resolve_outputs(nl, outputs)
    assert kind.dtype == p.dtype == q2.dtype == np.int32
    assert kind.tolist() == [0, 0, 0, 0, 0, 1, 1]
    idx = nl.nodenum
    assert p.tolist() == [idx[nodes[0]], -1, idx[nodes[1]], -1, idx[nodes[0]], 5, 4]
    assert q2.tolist() == [-1, -1, idx[nodes[0]], idx[nodes[1]], -1, -1, -1]
    empty = resolve_outputs(nl, [])
    assert all(len(a) == 0 and a.dtype == np.int32 for a in empty)


def test_resolve_outputs_errors():
    nl = n.Netlist.from_rows(ROWS)
    node = next(iter(nl.nodenum))
    with pytest.raises(KeyError):
        resolve_outputs(nl, [("e", "no such node")])
    with pytest.raises(KeyError):
        resolve_outputs(nl, [("v", node, "no such node")])
    with pytest.raises(KeyError):
        resolve_outputs(nl, [("i", "no such component")])
    for bad in [("e",), ("e", node, node), ("v", node), ("i",), ("x", node), "e", (), 3]:
        with pytest.raises(ValueError):
            resolve_outputs(nl, [bad])
    with pytest.raises(ValueError, match="current source"):
        resolve_outputs(nl, [("i", "a1")])
    twice = n.Netlist.from_rows(ROWS + [["r4", "R", "7", "3", "1"]])
    with pytest.raises(ValueError, match="defined 2 times"):
        resolve_outputs(twice, [("i", "r4")])
    assert resolve_outputs(twice, [("i", "r1")])[1].tolist() == [0]


def test_resolve_outputs_fast_netlist(tmp_path):
    import os
    from nodal_amd import netlist as netlist_mod
    rows = gen.cfg5_rows(12)
    pad = [["# " + "x" * 120]] * (1 + netlist_mod.FAST_PARSE_MIN_BYTES // 120)
    path = tmp_path / "netlist.csv"
    with open(path, "w") as f:
        for r in pad + rows:
            f.write(",".join(r) + "\n")
    assert os.path.getsize(path) >= netlist_mod.FAST_PARSE_MIN_BYTES
    fast = n.Netlist(str(path))
    assert getattr(fast, "_fast", False), "the fast reader declined a regular file"
    slow = n.Netlist.from_rows(rows)
    table = ref.table_of(slow)
    outputs = ref.all_outputs(slow, table)
    assert {o[0] for o in outputs} == {"e", "v", "i"}
    got, want = resolve_outputs(fast, outputs), resolve_outputs(slow, outputs)
    assert getattr(fast, "_fast", False), "resolve_outputs demoted the netlist"
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    source = next(r[0] for r in rows if r[1] == "A")
    with pytest.raises(ValueError, match="current source"):
        resolve_outputs(fast, [("i", source)])
    with pytest.raises(KeyError):
        resolve_outputs(fast, [("i", "no such component")])


# ---- 2: the container ----------------------------------------------------------------------------------------------
def test_container_on_hand_made_arrays():
    rows = ROWS + [["r4", "R", "7", "3", "1"]]  # (r4 twice: every row of the name carries the last value, 7)
    nl = n.Netlist.from_rows(rows)
    table = ref.table_of(nl)
    value = np.asarray(table.value, dtype=np.float64)
    assert value[5] == value[6] == 7.0
    values = np.array([[1.0, -2.0, 0.5, 0.0, 3.0, 0.25, 0.75], [0.0, 0.0, 0.0, 4.0, np.nan, -1.0, 1.0]])
    outputs = [("e", "1"), ("i", "r1")]
    s = Sensitivities(nl, outputs, values, np.array([0.1, 0.2]), np.zeros(2, dtype=np.int32), np.zeros(2), table=table)
    assert len(s) == 2 and s.outputs == outputs and s.adjoints is None
    assert s.names == list(nl.component_keys)
    assert np.array_equal(s.of("r1"), values[:, 0])
    assert np.array_equal(s.of("r4"), values[:, 5] + values[:, 6])
    with pytest.raises(KeyError):
        s.of("nope")
    assert np.array_equal(s.normalized, values * value[None, :], equal_nan=True)
    want = (np.abs(values[0] * value) * 0.01).sum()
    assert s.worst_case(0.01)[0] == pytest.approx(want, rel=1e-15)
    tol = np.linspace(0.01, 0.07, 7)
    assert s.worst_case(tol)[0] == pytest.approx((np.abs(values[0] * value) * tol).sum(), rel=1e-15)
    assert np.isnan(s.worst_case(0.01)[1])
    with pytest.raises(ValueError):
        s.worst_case(np.ones(3))
    norm = values * value[None, :]
    top = s.top(0, 3)
    order = sorted(range(7), key=lambda i: (-abs(norm[0, i]), i))[:3]
    assert top == [(s.names[i], float(norm[0, i])) for i in order]
    top1 = s.top(1, 10)  # (the NaN never, everything else)
    assert len(top1) == 6 and all(name != "e1" for name, _ in top1) and top1[0][0] == "r4"
    # the table is looked up from the netlist when it is not given
    assert np.array_equal(Sensitivities(nl, outputs, values, None, None, None).normalized, s.normalized, equal_nan=True)


# ---- 3: the restatement against central differences of the oracle's solves -----------------------------------------
# Left out by name, these five and no others: a gain of 1e5 (the differences are noise), a 1e-17 ohm self-loop that
# destroys the low bits of G, a name defined twice (every table row carries the last definition's value: perturbing one
# text row is another experiment), the two opmodel cases (text rows are not table rows).
NO_FD = ("doc/buffer", "edge/self_loop_r_bits", "edge/duplicate_r", "doc/opmodel_amplifier", "doc/opmodel_voltage_buffer")


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
FD_INPUTS = ([g for g in GOLDEN if g[0] not in NO_FD] + [(f"random{s}", _random_rows(s)) for s in range(4)]
             + [("cfg5(6)", gen.cfg5_rows(6))])


def test_the_inputs_are_the_ones_the_checks_were_sized_for():
    assert len(GOLDEN) == 23 and len(FD_INPUTS) == 23
    assert all(name in [g[0] for g in GOLDEN] for name in NO_FD)
    assert len([g for g in GOLDEN if g[0] in NO_FD]) == 5


def _outputs_at(rows, specs):
    """y of every specification for the network `rows` describes, by the oracle's own solve"""
    nl = n.Netlist.from_rows(rows)
    table = ref.table_of(nl)
    G, A, _ = oracle.build_model(nl, False)
    x = np.linalg.solve(np.asarray(G, dtype=np.float64), np.asarray(A, dtype=np.float64).ravel())
    return np.array([ref.output_vector(nl, table, spec)[0] @ x for spec in specs])


def _nudged(rows, i, value):
    return [[r[0], r[1], repr(float(value)), *r[3:]] if j == i else r for j, r in enumerate(rows)]


@pytest.mark.parametrize("k", range(len(FD_INPUTS)), ids=[i[0] for i in FD_INPUTS])
def test_restatement_against_central_differences(k):
    """Central differences with the relative steps 1e-4 and 5e-5, combined by Richardson's rule (4 D(h/2) - D(h)) / 3;
    bar per output 1e-7 max_i F_i^abs(lambda, x).  Seen on the CPU: the worst ratio |fd - adjoint| / bar is printed
    per case."""
    name, rows = FD_INPUTS[k]
    rows = [list(r) for r in rows]
    nl = n.Netlist.from_rows(rows)
    r = ref.Reference(nl, sparse=False)
    table = r.table
    assert table.ncomp == len(rows), "text rows are table rows in these inputs"
    specs = ref.all_outputs(nl, table)
    assert {"e", "i"} <= {s[0] for s in specs}
    value = np.asarray(table.value, dtype=np.float64)
    fd = np.empty((len(specs), table.ncomp))
    for i in range(table.ncomp):
        v = value[i]
        assert float(rows[i][2]) == v
        d = []
        for rel in (1e-4, 5e-5):
            h = rel * (abs(v) if v != 0.0 else 1.0)
            d.append((_outputs_at(_nudged(rows, i, v + h), specs) - _outputs_at(_nudged(rows, i, v - h), specs)) / (2 * h))
        fd[:, i] = (4.0 * d[1] - d[0]) / 3.0
    worst = 0.0
    for q, spec in enumerate(specs):
        y, c, row, lam, s = r.output(spec)
        bar = 1e-7 * ref.formulas_abs(table, lam, r.x, explicit_row=row).max()
        off = np.abs(fd[q] - s).max()
        if bar > 0:
            worst = max(worst, off / bar)
        assert off <= bar, (name, spec, off, bar)
    print(name, "outputs", len(specs), "worst |fd - adjoint| / bar:", worst)
