"""The parts of Circuit.operating_point(transistors=...) that need no device: resolve_transistors and its errors, the
companion table with its GM rows, ComponentTable.with_controlled_rows_appended, the hybrid-pi table of
OperatingPoint.linearised_table built from arrays, and gradient()'s refusal.  No GPU."""
import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import constants as c
from nodal_amd.lowering import lower
from nodal_amd.operating_point import (NewtonHistory, OperatingPoint, resolve_diodes, resolve_transistors,
                                       transistor_companion_table)

T_R, T_GM = c.TYPE_CODE["R"], 6  # (NODAL_T_GM of include/nodal_hip.h)


def _netlist():
    return n.Netlist.from_rows([["e1", "E", "10", "1", "g"], ["r1", "R", "47e3", "1", "2"], ["r2", "R", "10e3", "2", "g"],
                                ["rc", "R", "4.7e3", "1", "3"], ["re", "R", "1e3", "4", "g"]])


NPN = ("q1", "npn", 1e-14, 100.0, 2.0, 0.026, "3", "2", "4")
PNP = ("q2", "pnp", 2e-14, 50.0, 4.0, 0.03, "g", "2", "3")


def test_resolve_transistors_expands_both_kinds():
    nl = _netlist()
    node = nl.nodenum
    names, sign, junctions, ta, tb, junction, i_s = resolve_transistors(nl, [NPN, PNP], first=3)
    assert names == ["q1", "q2"] and sign.tolist() == [1.0, -1.0] and i_s.tolist() == [1e-14, 2e-14]
    # an NPN: base -> emitter and base -> collector, the transport from the collector to the emitter
    # a PNP: emitter -> base and collector -> base, the transport from the emitter to the collector
    assert junctions == [("q1.be", 1e-14 / 100.0, 0.026, "2", "4"), ("q1.bc", 1e-14 / 2.0, 0.026, "2", "3"),
                         ("q2.eb", 2e-14 / 50.0, 0.03, "3", "2"), ("q2.cb", 2e-14 / 4.0, 0.03, "g", "2")]
    assert ta.tolist() == [node["3"], node["3"]] and tb.tolist() == [node["4"], -1]
    assert junction.tolist() == [[3, 4], [5, 6]]  # behind the caller's three diodes
    assert ta.dtype == tb.dtype == junction.dtype == np.int32 and i_s.dtype == sign.dtype == np.float64
    # the junctions are diodes like any other
    jnames, i_sat, n_vt, ia, ib = resolve_diodes(nl, junctions)
    assert jnames == ["q1.be", "q1.bc", "q2.eb", "q2.cb"] and ib.tolist() == [node["4"], node["3"], node["2"], node["2"]]
    assert ia.tolist() == [node["2"], node["2"], node["3"], -1]
    empty = resolve_transistors(nl, [])
    assert empty[0] == [] and empty[2] == [] and empty[5].shape == (0, 2) and empty[6].shape == (0,)


def test_resolve_transistors_errors():
    nl = _netlist()
    good = list(NPN)

    def with_(at, value):
        bad = list(good)
        bad[at] = value
        return tuple(bad)

    for bad in ([with_(1, "nmos")], [with_(1, "NPN")], [with_(2, 0.0)], [with_(2, -1e-14)], [with_(2, float("inf"))],
                [with_(3, 0.0)], [with_(3, float("nan"))], [with_(4, -1.0)], [with_(4, float("inf"))], [with_(5, 0.0)],
                [with_(5, float("inf"))], [with_(6, "9")], [with_(7, "nowhere")], [with_(8, "9")], [NPN, NPN],
                [with_(0, "r1")], [NPN[:8]], [NPN + ("extra",)]):
        with pytest.raises(ValueError):
            resolve_transistors(nl, bad)


def _companion(transistors, diodes=()):
    nl = _netlist()
    table = lower(nl)
    diodes = list(diodes)
    _, _, junctions, ta, tb, junction, i_s = resolve_transistors(nl, transistors, first=len(diodes))
    _, i_sat, n_vt, ia, ib = resolve_diodes(nl, diodes + junctions)
    out = transistor_companion_table(table, i_sat, n_vt, ia, ib, ta, tb, junction, i_s, gmin=1e-12)
    return nl, table, (i_sat, n_vt, ia, ib, ta, tb, junction, i_s), out


def test_the_companion_table_has_the_gm_rows_behind_the_diodes():
    same = ("q3", "npn", 1e-14, 100.0, 1.0, 0.026, "2", "2", "2")   # every lead on one node
    tied = ("q4", "npn", 1e-14, 100.0, 1.0, 0.026, "2", "2", "g")   # collector tied to the base
    nl, table, (i_sat, n_vt, ia, ib, ta, tb, junction, i_s), (out, rows, gm_rows) = _companion(
        [NPN, PNP, same, tied], diodes=[("d1", 1e-14, 0.026, "1", "g")])
    node = nl.nodenum
    N = table.ncomp
    assert rows.tolist() == list(range(N, N + 9)) and rows.dtype == np.int64
    assert gm_rows.tolist() == [[N + 9 + 2 * t, N + 10 + 2 * t] for t in range(4)] and gm_rows.dtype == np.int64
    assert out.ncomp == N + 9 + 8 and out.K == table.K and out.B == table.B
    for name in ("type", "value", "a", "b", "c", "d", "drv", "k"):  # the netlist's rows keep their places
        assert np.array_equal(getattr(out, name)[:N], getattr(table, name))
    assert out.type[N:N + 9].tolist() == [T_R] * 9 and out.type[N + 9:].tolist() == [T_GM] * 8
    assert (np.array(out.k[N:]) == -1).all() and (np.array(out.drv[N:]) == -1).all()
    assert (np.array(out.c[N:N + 9]) == -1).all() and (np.array(out.d[N:N + 9]) == -1).all()
    a, b, cc, dd = (np.array(getattr(out, name)[N + 9:]).tolist() for name in ("a", "b", "c", "d"))
    # both rows of a transport carry its leads; one node on both leads: ground and ground
    assert a == [node["3"], node["3"], node["3"], node["3"], -1, -1, node["2"], node["2"]]
    assert b == [node["4"], node["4"], -1, -1, -1, -1, -1, -1]
    # the control leads are the junction rows' leads, forward then reverse
    for t in range(4):
        for q in range(2):
            r = rows[junction[t, q]]
            assert (cc[2 * t + q], dd[2 * t + q]) == (out.a[r], out.b[r])
    assert (cc[0], dd[0], cc[1], dd[1]) == (node["2"], node["4"], node["2"], node["3"])          # NPN: B->E, B->C
    assert (cc[2], dd[2], cc[3], dd[3]) == (node["3"], node["2"], -1, node["2"])                  # PNP: E->B, C->B
    assert (cc[4], dd[4], cc[5], dd[5]) == (-1, -1, -1, -1)                                       # one node
    assert (cc[6], dd[6], cc[7], dd[7]) == (node["2"], -1, -1, -1)                                # C tied to B
    # the linearisation at v = 0
    assert np.array_equal(out.value[N:N + 9], 1.0 / (i_sat / n_vt + 1e-12))
    nf, nr = n_vt[junction[:, 0]], n_vt[junction[:, 1]]
    assert np.array_equal(np.array(out.value[N + 9:]).reshape(4, 2), np.stack([i_s / nf, -i_s / nr], axis=1))
    assert ta.tolist()[2] == tb.tolist()[2] == node["2"]  # (the caller's arrays are not written to)


def test_with_controlled_rows_appended():
    table = lower(_netlist())
    N = table.ncomp
    out = table.with_controlled_rows_appended(np.array([T_GM, T_GM], dtype=np.uint8), [0.5, -0.25], [0, 0], [1, 1], [2, 3],
                                              [-1, 2])
    assert out.ncomp == N + 2 and out.K == table.K and out.B == table.B and table.ncomp == N
    for name in ("type", "value", "a", "b", "c", "d", "drv", "k"):
        assert np.array_equal(getattr(out, name)[:N], getattr(table, name))
    assert out.type[N:].tolist() == [T_GM, T_GM] and out.value[N:].tolist() == [0.5, -0.25]
    assert out.a[N:].tolist() == [0, 0] and out.b[N:].tolist() == [1, 1]
    assert out.c[N:].tolist() == [2, 3] and out.d[N:].tolist() == [-1, 2]
    assert out.k[N:].tolist() == [-1, -1] and out.drv[N:].tolist() == [-1, -1]
    # with_rows_appended stays as it is: no control leads
    plain = table.with_rows_appended(np.array([T_R], dtype=np.uint8), [2.0], [0], [1])
    assert plain.c[N:].tolist() == [-1] and plain.d[N:].tolist() == [-1]


def _operating_point(transistors=True):
    nl, table, (i_sat, n_vt, ia, ib, ta, tb, junction, i_s), _ = _companion([NPN, PNP], diodes=[("d1", 1e-14, 0.026, "1", "g")])
    hist = NewtonHistory([[2, 1, 0.5, 1e-16, 1], [0, 0, 1e-14, 2e-16, 0]], [0, 0], [0, 0], [0, 0])
    g_junctions = np.array([4e-2, 1e-12, 2e-3, 3e-12])
    gm = np.array([[3.9e-2, 1e-13], [1.9e-3, 2e-13]])
    extra = dict(transistors=["q1", "q2"], junction_voltages=np.zeros((2, 2)), collector_currents=np.zeros(2),
                 base_currents=np.zeros(2), emitter_currents=np.zeros(2), transconductances=gm,
                 transport=(ta, tb, junction, g_junctions)) if transistors else {}
    op = OperatingPoint(np.zeros(table.n), ["d1"], np.zeros(1), np.zeros(1), np.array([0.5]), True, 2, hist,
                        leads=(ia, ib) if transistors else (ia[:1], ib[:1]), **extra)
    return nl, table, op, (ia, ib, ta, tb, junction, g_junctions, gm), hist


def test_the_history_reads_the_fifth_word():
    *_, hist = _operating_point()
    assert hist.record.shape == (2, 5) and hist.transistors_not_converged.tolist() == [1, 0]
    assert hist.not_converged.tolist() == [2, 0] and hist.scaled_residual.tolist() == [1e-16, 2e-16]
    four = NewtonHistory([[2, 1, 0.5, 1e-16]], [0], [1], [1])
    assert four.record.shape == (1, 4) and four.transistors_not_converged.tolist() == [0]


def test_the_linearised_table_is_the_hybrid_pi_model():
    nl, table, op, (ia, ib, ta, tb, junction, g_junctions, gm), _ = _operating_point()
    node = nl.nodenum
    N = table.ncomp
    out = op.linearised_table(table)
    assert out.ncomp == N + 5 + 4 and out.K == table.K and out.B == table.B
    for name in ("type", "value", "a", "b", "c", "d"):
        assert np.array_equal(getattr(out, name)[:N], getattr(table, name))
    # every diode and every junction a resistor 1 / g ...
    assert out.type[N:N + 5].tolist() == [T_R] * 5
    assert np.array_equal(out.value[N:N + 5], 1.0 / np.concatenate([[0.5], g_junctions]))
    assert out.a[N:N + 5].tolist() == ia.tolist() and out.b[N:N + 5].tolist() == ib.tolist()
    # ... and every transport its two GM rows gmf, -gmr on the junctions' leads
    assert out.type[N + 5:].tolist() == [T_GM] * 4
    assert out.value[N + 5:].tolist() == [gm[0, 0], -gm[0, 1], gm[1, 0], -gm[1, 1]]
    assert out.a[N + 5:].tolist() == [node["3"]] * 4 and out.b[N + 5:].tolist() == [node["4"], node["4"], -1, -1]
    assert out.c[N + 5:].tolist() == ia[1:].tolist() and out.d[N + 5:].tolist() == ib[1:].tolist()
    # without transistors it is what it was: the diodes alone
    _, _, plain, _, _ = _operating_point(transistors=False)
    out = plain.linearised_table(table)
    assert out.ncomp == N + 1 and out.value[N] == 2.0 and plain.transistors == []
    # a junction that carries nothing at all has no resistor
    op._transport = (ta, tb, junction, np.array([4e-2, 0.0, 2e-3, 3e-12]))
    with pytest.raises(ValueError):
        op.linearised_table(table)


def test_the_gradient_with_transistors_is_refused():
    _, _, op, _, _ = _operating_point()
    with pytest.raises(ValueError, match="the adjoint with transistors is not implemented"):
        op.gradient(np.zeros(len(op.x)))
    with pytest.raises(ValueError, match="not made by Circuit.operating_point"):
        op.linearised()
