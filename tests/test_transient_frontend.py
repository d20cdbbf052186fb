"""Transient analysis without a device: the argument rules of Circuit.transient, the capacitors' resolution and the
table with the companion rows, and the reference's two formulations against each other and against the closed form
(tests/transient_reference.py)."""
import math
import random

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import generators as gen
from nodal_amd.lowering import lower
from nodal_amd.transient import METHODS, Transient, check_transient_arguments, companion_table, resolve_capacitors
from tests import transient_reference as ref

ROWS = [["a1", "A", "2", "1", "g"], ["r1", "R", "3", "1", "2"], ["r2", "R", "5", "2", "g"], ["e1", "E", "1.5", "3", "g"],
        ["r3", "R", "2", "3", "2"]]


def _nl():
    return n.Netlist.from_rows(ROWS)


# ---- argument errors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0.0, -1.0, math.inf, math.nan])
def test_dt_must_be_positive(dt):
    with pytest.raises(ValueError, match="dt"):
        check_transient_arguments(dt, 3, "euler", None, 4)


def test_steps_must_not_be_negative():
    with pytest.raises(ValueError, match="steps"):
        check_transient_arguments(1.0, -1, "euler", None, 4)
    assert check_transient_arguments(1.0, 0, "euler", None, 4) == (1.0, 0, 0, None)


def test_method_names():
    assert METHODS == {"euler": 0, "trapezoidal": 1}
    with pytest.raises(ValueError, match="method"):
        check_transient_arguments(1.0, 1, "gear", None, 4)


def test_trapezoidal_needs_the_dc_start():
    with pytest.raises(ValueError, match="euler"):
        check_transient_arguments(1.0, 1, "trapezoidal", np.zeros(4), 4)
    assert check_transient_arguments(1.0, 1, "trapezoidal", None, 4)[2] == 1


def test_initial_shape():
    with pytest.raises(ValueError, match="shape"):
        check_transient_arguments(1.0, 1, "euler", np.zeros(3), 4)
    x0 = check_transient_arguments(0.5, 2, "euler", [1, 2, 3, 4], 4)[3]
    assert x0.dtype == np.float64 and x0.tolist() == [1.0, 2.0, 3.0, 4.0]


@pytest.mark.parametrize("farads", [0.0, -1e-9, math.inf, math.nan])
def test_farads_must_be_positive_and_finite(farads):
    with pytest.raises(ValueError, match="farads"):
        resolve_capacitors(_nl(), [("c1", farads, "1", "g")])


def test_a_capacitor_needs_two_nodes_of_the_netlist():
    with pytest.raises(ValueError, match="both leads"):
        resolve_capacitors(_nl(), [("c1", 1.0, "2", "2")])
    with pytest.raises(ValueError, match="both leads"):
        resolve_capacitors(_nl(), [("c1", 1.0, "g", "g")])
    with pytest.raises(KeyError):
        resolve_capacitors(_nl(), [("c1", 1.0, "1", "nowhere")])
    with pytest.raises(ValueError, match="node_a, node_b"):
        resolve_capacitors(_nl(), [("c1", 1.0, "1")])


# ---- resolution and the augmented table ---------------------------------------------------------------------------
def test_capacitors_resolve_to_node_indices():
    nl = _nl()
    caps = [("c1", 1e-3, "1", "g"), ("c2", 2e-3, "g", "2"), ("c3", 3e-3, "2", "3"), ("c3b", 4e-3, "2", "3"), ("c4", 5e-3, "3", "2")]
    names, farads, ia, ib = resolve_capacitors(nl, caps)
    num = nl.nodenum
    assert names == ["c1", "c2", "c3", "c3b", "c4"]
    assert farads.tolist() == [1e-3, 2e-3, 3e-3, 4e-3, 5e-3]
    assert ia.tolist() == [num["1"], -1, num["2"], num["2"], num["3"]]
    assert ib.tolist() == [-1, num["2"], num["3"], num["3"], num["2"]]
    assert ia.dtype == np.int32 and ib.dtype == np.int32
    empty = resolve_capacitors(nl, [])
    assert empty[0] == [] and all(len(a) == 0 for a in empty[1:])


@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
def test_the_augmented_table(method):
    nl = _nl()
    table = lower(nl)
    caps = [("c1", 1e-3, "1", "g"), ("c2", 2e-3, "g", "2"), ("c3", 4e-3, "2", "3")]
    _, farads, ia, ib = resolve_capacitors(nl, caps)
    dt = 0.25
    aug, rows = companion_table(table, farads, ia, ib, dt, METHODS[method])
    assert rows.tolist() == [table.ncomp, table.ncomp + 1, table.ncomp + 2] and rows.dtype == np.int64
    assert (aug.K, aug.B, aug.ncomp) == (table.K, table.B, table.ncomp + 3)
    for name in ("type", "value", "a", "b", "c", "d", "drv", "k"):  # the original rows keep their indices
        assert np.array_equal(np.asarray(getattr(aug, name))[:table.ncomp], np.asarray(getattr(table, name))), name
    scale = 2.0 if method == "trapezoidal" else 1.0
    assert (np.asarray(aug.type)[table.ncomp:] == 0).all()  # R
    assert np.array_equal(np.asarray(aug.value)[table.ncomp:], dt / (scale * farads))
    assert np.array_equal(np.asarray(aug.a)[table.ncomp:], ia) and np.array_equal(np.asarray(aug.b)[table.ncomp:], ib)
    for name in ("c", "d", "drv", "k"):
        assert (np.asarray(getattr(aug, name))[table.ncomp:] == -1).all(), name
    assert aug.first_error is None and nl.nums["kcl"] == table.K  # the netlist's numbering is untouched
    # the same rows through the parser give the same table: the companion model needs no new stamp
    r = ref.TransientReference(ROWS, caps, dt, method)
    again = lower(n.Netlist.from_rows(r.augmented_rows()))
    for name in ("type", "value", "a", "b", "c", "d", "drv", "k"):
        assert np.array_equal(np.asarray(getattr(aug, name)), np.asarray(getattr(again, name))), name


def test_no_capacitors_leaves_the_table():
    table = lower(_nl())
    aug, rows = companion_table(table, np.zeros(0), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), 1.0, 0)
    assert len(rows) == 0 and aug.ncomp == table.ncomp and np.array_equal(np.asarray(aug.value), np.asarray(table.value))


def test_the_container():
    tr = Transient(np.arange(3.0), np.zeros((3, 1)), [("1", "g")], np.zeros(2, dtype=np.int32), np.zeros(2), np.zeros(2))
    assert len(tr) == 2 and tr.solutions is None and tr.envelope is None and len(tr.solution_steps) == 0


# ---- the reference agrees with itself -----------------------------------------------------------------------------
def test_rc_section_euler_closed_form():
    I, R, C, h, steps = 0.7, 3.0, 0.02, 0.011, 60
    r = ref.TransientReference(ref.rc_rows(I, R), [("c1", C, "1", "g")], h, "euler")
    want = ref.rc_euler_closed_form(I, R, C, h, steps)
    A = [r.A0] * steps
    for X in (r.run(np.zeros(1), A), r.run_state_space(np.zeros(1), A)):
        off = np.abs(X[:, 0] - want).max() / np.abs(want).max()
        print("RC Euler against the closed form:", off)
        assert off <= 9e-16


def test_rc_section_trapezoidal_closed_form():
    I0, I1, R, C, h, steps = 0.7, -0.4, 3.0, 0.02, 0.011, 60
    r = ref.TransientReference(ref.rc_rows(I0, R), [("c1", C, "1", "g")], h, "trapezoidal")
    want = ref.rc_trapezoidal_closed_form(I0, I1, R, C, h, steps)
    A = r.rhs_steps({"a1": [I1] * steps}, steps)
    x0 = r.dc()
    for X in (r.run(x0, A), r.run_state_space(x0, A)):
        off = np.abs(X[:, 0] - want).max() / np.abs(want).max()
        print("RC trapezoidal against the closed form:", off)
        assert off <= steps * 2.0 ** -52  # (rho^(k-1) and each step of the recurrence round once per step: 60 ulps at most)


@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
def test_the_two_formulations_agree_on_a_grid(method):
    N, steps = 100, 33
    rng = random.Random(5)
    rows = list(gen.grid_rows(N))
    picks = rng.sample(range(1, N * N - 1), 4)
    rows += [[f"ld{j}", "A", "1", str(k + 1), "g"] for j, k in enumerate(picks)]
    nl = n.Netlist.from_rows(rows)
    nodes = sorted(nl.nodenum, key=lambda s: nl.nodenum[s])
    caps = [(f"cg{i}", rng.uniform(0.5, 2.0), node, "g") for i, node in enumerate(nodes)]
    caps += [(f"cc{i}", rng.uniform(0.5, 2.0), *rng.sample(nodes, 2)) for i in range(50)]
    assert len(caps) == 10049
    r = ref.TransientReference(rows, caps, 1.0, method)  # (a step of the order of a node's own RC)
    sources = {f"ld{j}": [rng.uniform(-2.0, 2.0) for _ in range(steps)] for j in range(4)}
    A = r.rhs_steps(sources, steps)
    x0 = r.dc()
    Xc, Xs = r.run(x0, A), r.run_state_space(x0, A)
    off = np.abs(Xc - Xs).max() / np.abs(Xs).max()
    print(method, "companion against state space on grid(100), 33 steps:", off)
    assert off <= 3e-15
    # and the one-step restatement of a run is that run
    assert np.abs(r.one_step_from(Xc, A) - Xc[1:]).max() <= 1e-15 * np.abs(Xc).max()


def test_companion_stepping_with_branch_unknowns():
    """a network with E / VCVS rows: the steady state of the companion stepping is the DC solution"""
    rows = gen.cfg5_rows(6)
    caps = ref.seeded_capacitors(rows, 12, seed=3)
    for method in ("euler", "trapezoidal"):
        r = ref.TransientReference(rows, caps, 0.5, method)
        x0 = r.dc()
        X = r.run(x0, [r.A0] * 5)
        assert np.abs(X - x0).max() <= 1e-13 * np.abs(x0).max(), method
