"""Transient analysis with inductors, without a device: the argument rules, the inductors' resolution and their loop
check, the table with the companion rows of both kinds, the table of the DC start (branch rows), and the reference's two
formulations against each other and against the closed form (tests/transient_rl_reference.py)."""
import math
import random
import warnings

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd.lowering import lower
from nodal_amd.transient import (METHODS, Transient, check_inductor_arguments, companion_table, dc_table,
                                 resolve_capacitors, resolve_inductors)
from tests import transient_rl_reference as rl

ROWS = [["a1", "A", "2", "1", "g"], ["r1", "R", "3", "1", "2"], ["r2", "R", "5", "2", "g"], ["e1", "E", "1.5", "3", "g"],
        ["r3", "R", "2", "3", "2"], ["r4", "R", "4", "4", "1"]]
COLUMNS = ("type", "value", "a", "b", "c", "d", "drv", "k")


def _nl():
    return n.Netlist.from_rows(ROWS)


# ---- argument errors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("henries", [0.0, -1e-9, math.inf, math.nan])
def test_henries_must_be_positive_and_finite(henries):
    with pytest.raises(ValueError, match="henries"):
        resolve_inductors(_nl(), [("l1", henries, "1", "g")])


def test_an_inductor_needs_two_nodes_of_the_netlist():
    with pytest.raises(ValueError, match="both leads"):
        resolve_inductors(_nl(), [("l1", 1.0, "2", "2")])
    with pytest.raises(ValueError, match="both leads"):
        resolve_inductors(_nl(), [("l1", 1.0, "g", "g")])
    with pytest.raises(KeyError):
        resolve_inductors(_nl(), [("l1", 1.0, "1", "nowhere")])
    with pytest.raises(ValueError, match="node_a, node_b"):
        resolve_inductors(_nl(), [("l1", 1.0, "1")])
    with pytest.raises(ValueError, match="twice"):
        resolve_inductors(_nl(), [("l1", 1.0, "1", "g"), ("l1", 1.0, "2", "3")])


@pytest.mark.parametrize("loop", [
    [("l1", 1.0, "1", "2"), ("l2", 2.0, "1", "2")],                          # two in parallel
    [("l1", 1.0, "1", "2"), ("l2", 2.0, "2", "1")],                          # ... one of them turned round
    [("l1", 1.0, "1", "2"), ("l2", 1.0, "2", "3"), ("l3", 1.0, "3", "1")],   # a triangle
    [("l1", 1.0, "1", "g"), ("l2", 1.0, "g", "2"), ("l3", 1.0, "2", "1")],   # through ground, which is one node
    [("l1", 1.0, "1", "g"), ("l2", 1.0, "1", "g")],                          # in parallel to ground
], ids=["parallel", "antiparallel", "triangle", "through ground", "parallel to ground"])
def test_a_loop_of_inductors_is_refused(loop):
    with pytest.raises(ValueError, match="loop of inductors"):
        resolve_inductors(_nl(), loop)
    resolve_inductors(_nl(), loop[:-1])  # (without the one that closes it: a tree)


def test_a_tree_of_inductors_is_no_loop():
    star = [("l1", 1.0, "1", "g"), ("l2", 1.0, "2", "g"), ("l3", 1.0, "g", "3"), ("l4", 1.0, "4", "3")]
    names, henries, ia, ib = resolve_inductors(_nl(), star)
    num = _nl().nodenum
    assert names == ["l1", "l2", "l3", "l4"] and henries.tolist() == [1.0] * 4
    assert ia.tolist() == [num["1"], num["2"], -1, num["4"]] and ib.tolist() == [-1, -1, num["3"], num["3"]]
    assert ia.dtype == np.int32 and ib.dtype == np.int32 and henries.dtype == np.float64
    empty = resolve_inductors(_nl(), [])
    assert empty[0] == [] and all(len(a) == 0 for a in empty[1:])


def test_initial_currents_and_current_probes():
    names = ["l1", "l2", "l3"]
    with pytest.raises(ValueError, match="initial_currents needs"):
        check_inductor_arguments(names, None, np.zeros(3), ())
    with pytest.raises(ValueError, match="shape"):
        check_inductor_arguments(names, np.zeros(4), np.zeros(2), ())
    with pytest.raises(ValueError, match="shape"):
        check_inductor_arguments(names, np.zeros(4), np.zeros((3, 1)), ())
    with pytest.raises(KeyError):
        check_inductor_arguments(names, None, None, ["l4"])
    with pytest.raises(KeyError):
        check_inductor_arguments([], None, None, ["l1"])
    i0, index = check_inductor_arguments(names, None, None, ["l3", "l1", "l3"])
    assert i0 is None and index.tolist() == [2, 0, 2] and index.dtype == np.int32  # (the DC start supplies i_0)
    i0, index = check_inductor_arguments(names, np.zeros(4), None, ())
    assert i0.tolist() == [0.0, 0.0, 0.0] and index.shape == (0,)  # (`initial` alone: the inductors start at zero)
    i0, _ = check_inductor_arguments(names, np.zeros(4), [1, 2, 3], ())
    assert i0.dtype == np.float64 and i0.tolist() == [1.0, 2.0, 3.0]


# ---- the table with the companion rows ----------------------------------------------------------------------------
CAPS = [("c1", 1e-3, "1", "g"), ("c2", 2e-3, "g", "2"), ("c3", 4e-3, "2", "3")]
INDS = [("l1", 5e-2, "4", "g"), ("l2", 7e-2, "3", "1")]


@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
def test_the_companion_table_capacitors_first_then_inductors(method):
    nl = _nl()
    table = lower(nl)
    _, farads, ia, ib = resolve_capacitors(nl, CAPS)
    _, henries, la, lb = resolve_inductors(nl, INDS)
    dt, first = 0.25, table.ncomp
    aug, cap_rows, ind_rows = companion_table(table, farads, ia, ib, dt, METHODS[method], henries, la, lb)
    assert cap_rows.tolist() == [first, first + 1, first + 2] and ind_rows.tolist() == [first + 3, first + 4]
    assert cap_rows.dtype == np.int64 and ind_rows.dtype == np.int64
    assert (aug.K, aug.B, aug.ncomp) == (table.K, table.B, first + 5)
    for name in COLUMNS:  # the original rows keep their indices
        assert np.array_equal(np.asarray(getattr(aug, name))[:first], np.asarray(getattr(table, name))), name
    scale = 2.0 if method == "trapezoidal" else 1.0
    assert (np.asarray(aug.type)[first:] == 0).all()  # R
    assert np.array_equal(np.asarray(aug.value)[cap_rows], dt / (scale * farads))
    assert np.array_equal(np.asarray(aug.value)[ind_rows], scale * henries / dt)
    assert np.array_equal(np.asarray(aug.a)[first:], np.concatenate([ia, la]))
    assert np.array_equal(np.asarray(aug.b)[first:], np.concatenate([ib, lb]))
    for name in ("c", "d", "drv", "k"):
        assert (np.asarray(getattr(aug, name))[first:] == -1).all(), name
    # the same rows through the parser give the same table but for the rounding of the capacitors' 1 / (C / h)
    r = rl.RLReference(ROWS, CAPS, INDS, dt, method)
    again = lower(n.Netlist.from_rows(r.augmented_rows()))
    for name in COLUMNS:
        if name == "value":
            assert np.array_equal(np.asarray(aug.value)[ind_rows], np.asarray(again.value)[ind_rows])
            assert np.allclose(np.asarray(aug.value), np.asarray(again.value), rtol=4 * 2.0 ** -52, atol=0.0)
        else:
            assert np.array_equal(np.asarray(getattr(aug, name)), np.asarray(getattr(again, name))), name
    # without inductors: the two-element result of before, bit for bit
    only, rows = companion_table(table, farads, ia, ib, dt, METHODS[method])
    assert rows.tolist() == cap_rows.tolist() and only.ncomp == first + 3
    assert np.array_equal(np.asarray(only.value), np.asarray(aug.value)[:first + 3])
    # inductors alone
    ind_only, none, rows = companion_table(table, farads[:0], ia[:0], ib[:0], dt, METHODS[method], henries, la, lb)
    assert len(none) == 0 and rows.tolist() == [first, first + 1]
    assert np.array_equal(np.asarray(ind_only.value)[first:], scale * henries / dt)


# ---- the table of the DC start: one zero-volt E row and one branch unknown per inductor ---------------------------
def test_branch_rows_against_the_lowered_netlist_with_e_rows():
    nl = _nl()
    table = lower(nl)
    inds = INDS + [("l3", 1.0, "g", "2")]
    _, _, la, lb = resolve_inductors(nl, inds)
    dc = dc_table(table, la, lb)
    assert (dc.K, dc.B, dc.ncomp, dc.n) == (table.K, table.B + 3, table.ncomp + 3, table.n + 3) and dc.first_error is None
    explicit = n.Netlist.from_rows(ROWS + [[f"ind__{j}", "E", "0.0", a, b] for j, (_, _, a, b) in enumerate(inds)])
    assert explicit.ground == nl.ground and explicit.nodenum == nl.nodenum  # (the parser agrees here: no overruling)
    want = lower(explicit)
    assert (want.K, want.B, want.ncomp) == (dc.K, dc.B, dc.ncomp)
    for name in COLUMNS:
        assert np.array_equal(np.asarray(getattr(dc, name)), np.asarray(getattr(want, name))), name
    assert np.asarray(dc.k)[table.ncomp:].tolist() == [table.B, table.B + 1, table.B + 2]
    for name in COLUMNS:  # the circuit's own rows keep their indices and their branches
        assert np.array_equal(np.asarray(getattr(dc, name))[:table.ncomp], np.asarray(getattr(table, name))), name
    # the general constructor, with other types and values
    t = table.with_branch_rows_appended(np.array([2, 2], dtype=np.uint8), np.array([1.0, -2.0]), la[:2], lb[:2])
    assert t.B == table.B + 2 and np.asarray(t.value)[-2:].tolist() == [1.0, -2.0] and table.B == lower(nl).B


def test_the_sign_of_the_dc_current_in_the_oracles_matrix():
    """one source of 2 A into node 1, which an inductor shorts to ground: all of it flows from 1 to ground through the
    inductor.  As (1, g) the current is +2, as (g, 1) it is -2; the E row's own unknown is the negative of either."""
    rows = [["a1", "A", "2", "g", "1"], ["r1", "R", "3", "1", "g"]]
    assert rl.RLReference(rows, [], [], 1.0, "euler").cap.A0.tolist() == [-2.0]  # (an A row DRAWS its value from lead a)
    rows = [["a1", "A", "2", "1", "g"], ["r1", "R", "3", "1", "g"]]
    fwd = rl.RLReference(rows, [], [("l1", 1.0, "1", "g")], 1.0, "euler")
    bwd = rl.RLReference(rows, [], [("l1", 1.0, "g", "1")], 1.0, "euler")
    (xf, cf), (xb, cb) = fwd.dc_start(), bwd.dc_start()
    assert xf.tolist() == [0.0] and xb.tolist() == [0.0]
    assert cf.tolist() == [2.0] and cb.tolist() == [-2.0]
    G, A = fwd.dc_system()
    assert np.linalg.solve(G.toarray(), A).tolist() == [0.0, -2.0]  # the oracle's branch unknown: INTO lead a


def test_the_container():
    tr = Transient(np.arange(3.0), np.zeros((3, 1)), [("1", "g")], np.zeros(2, dtype=np.int32), np.zeros(2), np.zeros(2))
    assert tr.currents.shape == (3, 0) and tr.final_currents.shape == (0,) and tr.current_probes == []
    tr = Transient(np.arange(3.0), np.zeros((3, 1)), [("1", "g")], np.zeros(2, dtype=np.int32), np.zeros(2), np.zeros(2),
                   currents=np.ones((3, 2)), current_probes=("l1", "l2"), final_currents=np.ones(4))
    assert tr.currents.shape == (3, 2) and tr.current_probes == ["l1", "l2"] and tr.final_currents.shape == (4,)


# ---- the reference agrees with itself -----------------------------------------------------------------------------
def test_rl_section_euler_closed_form():
    I, R, L, h, steps = 0.7, 3.0, 0.05, 0.011, 60
    r = rl.RLReference(rl.rl_rows(I, R), [], [("l1", L, "1", "g")], h, "euler")
    v, i = rl.rl_euler_closed_form(I, R, L, h, steps)
    assert v[0] == I * R and i[0] == 0.0
    A = [r.cap.A0] * steps
    for X, C in (r.run(np.array([I * R]), np.zeros(1), A), r.run_branch(np.array([I * R]), np.zeros(1), A)):
        off_v, off_i = np.abs(X[:, 0] - v).max() / np.abs(v).max(), np.abs(C[:, 0] - i).max() / np.abs(i).max()
        print("RL Euler against the closed form:", off_v, off_i)
        assert off_v <= 5e-16 and off_i <= 5e-16
    x0, i0 = r.dc_start()  # (and the DC point of the section: the inductor carries everything)
    assert x0.tolist() == [0.0] and i0.tolist() == [I]


@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
def test_the_two_formulations_agree_on_a_grid(method):
    steps = 33
    rows, caps, inds = rl.grid12_mix()
    assert len(caps) == 149 and len(inds) == 9
    r = rl.RLReference(rows, caps, inds, 0.5, method)
    rng = random.Random(1)
    sources = {name: [rng.uniform(-2.0, 2.0) for _ in range(steps)] for name in ("ld0", "ld1", "a1")}
    A = r.rhs_steps(sources, steps)
    x0, i0 = r.dc_start()
    assert np.abs(r.voltages(x0)).max() <= 1e-15 * np.abs(x0).max()  # (a short carries no voltage)
    (Xc, Ic), (Xb, Ib) = r.run(x0, i0, A), r.run_branch(x0, i0, A)
    off_x, off_i = np.abs(Xc - Xb).max() / np.abs(Xb).max(), np.abs(Ic - Ib).max() / np.abs(Ib).max()
    print(method, "companion against branch stepping on grid(12), 33 steps:", off_x, off_i)
    assert off_x <= 1e-15 and off_i <= 1e-15
    assert np.abs(Ib).max() > 0.1 and np.abs(Ib[-1] - Ib[0]).max() > 0.01  # (the currents do move)
    # and the one-step restatement of a run is that run
    Xr, Ir = r.one_step_from(Xc, Ic, A)
    assert np.abs(Xr - Xc[1:]).max() <= 1e-15 * np.abs(Xc).max() and np.abs(Ir - Ic[1:]).max() <= 1e-15 * np.abs(Ic).max()


def test_the_dc_start_of_every_input_of_the_branches_suite_solves():
    """the seeded mix the GPU's one-step parity runs on (tests/test_gpu_transient_inductors.py): on every one of the 29
    inputs the DC system with its zero-volt E rows has full rank and a finite solution, and none has lost its inductors"""
    from tests.test_gpu_branches import INPUTS
    assert len(INPUTS) == 29
    for k, (name, rows) in enumerate(INPUTS):
        caps, inds = rl.seeded_mix(rows, k)
        assert len(caps) == 5 and 1 <= len(inds) <= 4, name
        resolve_inductors(n.Netlist.from_rows([list(r) for r in rows]), inds)  # (no loop among themselves)
        r = rl.RLReference(rows, caps, inds, 0.4, "euler")
        G, A = r.dc_system()
        if G.shape[0] <= 1024:
            assert np.linalg.matrix_rank(G.toarray()) == G.shape[0], name
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            x0, i0 = r.dc_start()
        assert np.isfinite(x0).all() and np.isfinite(i0).all(), name
        e = np.concatenate([x0, -i0])
        resid = np.abs(G @ e - A).max() / (abs(G).sum(axis=1).max() * np.abs(e).max() + np.abs(A).max() + 1e-300)
        assert resid <= 1e-15, (name, resid)
