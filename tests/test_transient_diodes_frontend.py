"""Transient analysis with diodes, without a device: the argument rules Circuit.transient applies to its diodes and
tolerances, the child table with the companion rows of all three kinds in their order, the diode probes, and the
Transient container with and without the fields of a run with diodes."""
import math

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import constants as c
from nodal_amd.lowering import lower
from nodal_amd.operating_point import check_operating_point_arguments, resolve_diodes
from nodal_amd.transient import (METHODS, Transient, check_diode_probes, companion_table, diode_companion_table,
                                 resolve_capacitors, resolve_inductors)

ROWS = [["a1", "A", "2", "1", "g"], ["r1", "R", "3", "1", "2"], ["r2", "R", "5", "2", "g"], ["e1", "E", "1.5", "3", "g"],
        ["r3", "R", "2", "3", "2"], ["r4", "R", "4", "4", "1"]]
COLUMNS = ("type", "value", "a", "b", "c", "d", "drv", "k")
CAPS = [("c1", 2.0, "1", "g"), ("c2", 0.5, "2", "3")]
INDS = [("l1", 1.5, "4", "g")]
DIODES = [("d1", 1e-14, 0.02585, "1", "g"), ("d2", 2e-13, 0.03, "g", "2"), ("d3", 1e-12, 0.04, "3", "3"),
          ("d4", 1e-14, 0.05, "2", "4")]


def _nl():
    return n.Netlist.from_rows(ROWS)


# ---- argument errors: the diodes and tolerances are operating_point()'s ---------------------------------------------------
@pytest.mark.parametrize("bad, match", [
    (("d1", 0.0, 0.02585, "1", "g"), "i_sat"), (("d1", 1e-14, math.inf, "1", "g"), "n_vt"),
    (("d1", 1e-14, 0.02585, "1", "nowhere"), "d1"), (("r1", 1e-14, 0.02585, "1", "g"), "name of a component"),
    (("d1", 1e-14, 0.02585, "1"), "anode, cathode")])
def test_a_bad_diode_is_refused(bad, match):
    with pytest.raises(ValueError, match=match):
        resolve_diodes(_nl(), [bad])


def test_a_diode_name_given_twice_is_refused():
    with pytest.raises(ValueError, match="twice"):
        resolve_diodes(_nl(), [DIODES[0], DIODES[0]])


@pytest.mark.parametrize("kw", [dict(max_iter=0), dict(max_iter=2.5), dict(reltol=-1e-3), dict(vntol=math.nan),
                                dict(abstol=math.inf), dict(gmin=-1e-12)])
def test_bad_tolerances_are_refused(kw):
    args = dict(max_iter=50, reltol=1e-3, vntol=1e-6, abstol=1e-12, gmin=1e-12)
    args.update(kw)
    with pytest.raises(ValueError):
        check_operating_point_arguments(args["max_iter"], args["reltol"], args["vntol"], args["abstol"], args["gmin"], None, 6)


def test_the_defaults_of_transient_are_accepted():
    import inspect
    sig = inspect.signature(n.Circuit.transient).parameters
    got = {k: sig[k].default for k in ("diodes", "diode_probes", "max_iter", "reltol", "vntol", "abstol", "gmin")}
    assert got == dict(diodes=(), diode_probes=(), max_iter=50, reltol=1e-3, vntol=1e-6, abstol=1e-12, gmin=1e-12)
    assert check_operating_point_arguments(50, 1e-3, 1e-6, 1e-12, 1e-12, None, 6) == (50, 1e-3, 1e-6, 1e-12, 1e-12, None)


def test_diode_probes_name_diodes():
    names = [d[0] for d in DIODES]
    index = check_diode_probes(names, ["d3", "d1", "d3"])
    assert index.dtype == np.int32 and index.tolist() == [2, 0, 2]
    assert check_diode_probes(names, ()).shape == (0,) and check_diode_probes((), ()).shape == (0,)
    with pytest.raises(KeyError, match="c1"):
        check_diode_probes(names, ["c1"])
    with pytest.raises(KeyError, match="d1"):
        check_diode_probes((), ["d1"])  # (no diodes at all: nothing to probe)


# ---- the child table: capacitors, then inductors, then diodes ---------------------------------------------------------------
@pytest.mark.parametrize("method", ["euler", "trapezoidal"])
@pytest.mark.parametrize("inductors", [INDS, []])
def test_the_child_table_holds_the_companion_rows_in_order(method, inductors):
    nl = _nl()
    table = lower(nl)
    dt, code, gmin = 0.25, METHODS[method], 1e-12
    _, farads, ca, cb = resolve_capacitors(nl, CAPS)
    _, henries, la, lb = resolve_inductors(nl, inductors)
    _, i_sat, n_vt, da, db = resolve_diodes(nl, DIODES)
    out, cap_rows, ind_rows, diode_rows = diode_companion_table(table, farads, ca, cb, dt, code, henries, la, lb, i_sat, n_vt,
                                                                da, db, gmin)
    C, L, D, first = len(CAPS), len(inductors), len(DIODES), table.ncomp
    assert cap_rows.tolist() == list(range(first, first + C))
    assert ind_rows.tolist() == list(range(first + C, first + C + L))
    assert diode_rows.tolist() == list(range(first + C + L, first + C + L + D))
    assert out.ncomp == first + C + L + D and (out.K, out.B) == (table.K, table.B)
    for name in COLUMNS:  # the netlist's own rows keep their place and their content
        assert np.array_equal(np.asarray(getattr(out, name))[:first], np.asarray(getattr(table, name)))
    assert (np.asarray(out.type)[first:] == c.TYPE_CODE["R"]).all()
    # the rows in front of the diodes' are exactly the table of a run without diodes
    linear = companion_table(table, farads, ca, cb, dt, code, henries, la, lb)[0]
    for name in COLUMNS:
        assert np.array_equal(np.asarray(getattr(out, name))[:first + C + L], np.asarray(getattr(linear, name)))
    scale = 2.0 if method == "trapezoidal" else 1.0
    value = np.asarray(out.value)
    assert np.array_equal(value[cap_rows], dt / (scale * farads)) and np.array_equal(value[ind_rows], scale * henries / dt)
    assert np.array_equal(value[diode_rows], 1.0 / (i_sat / n_vt + gmin))  # (placeholders: the linearisation at v = 0)
    a, b = np.asarray(out.a)[diode_rows], np.asarray(out.b)[diode_rows]
    same = da == db
    assert same.tolist() == [False, False, True, False]
    assert np.array_equal(a[~same], da[~same]) and np.array_equal(b[~same], db[~same])
    assert (a[same] == -1).all() and (b[same] == -1).all()  # (both leads on one node: a row that stamps nothing)


# ---- the container ---------------------------------------------------------------------------------------------------------
def test_the_container_without_diodes_has_the_fields_of_a_linear_run():
    steps = 4
    info = np.array([0, 0, 1, 1], dtype=np.int32)
    tr = Transient(0.1 * np.arange(steps + 1), np.zeros((steps + 1, 2)), [("1", "g"), ("2", "g")], info, np.zeros(steps),
                   np.zeros(steps, dtype=np.int32))
    assert len(tr) == steps
    assert tr.newton_iterations.tolist() == [1, 1, 0, 0] and tr.matrix_updates.tolist() == [0, 0, 0, 0]
    assert tr.diode_voltages.shape == (steps + 1, 0) and tr.diode_currents.shape == (steps + 1, 0)
    assert tr.diode_probes == [] and tr.final_junctions.shape == (0,)
    assert tr.currents.shape == (steps + 1, 0) and tr.final_currents.shape == (0,)


def test_the_container_keeps_what_a_run_with_diodes_gives_it():
    steps = 3
    newton, updates = np.array([3, 2, 0], dtype=np.int32), np.array([1, 0, 0], dtype=np.int32)
    v, i, vh = np.ones((steps + 1, 1)), 2 * np.ones((steps + 1, 1)), np.array([0.6, -3.0])
    tr = Transient(0.1 * np.arange(steps + 1), np.zeros((steps + 1, 0)), [], np.array([0, 0, 2], dtype=np.int32),
                   np.zeros(steps), np.zeros(steps, dtype=np.int32), newton_iterations=newton, matrix_updates=updates,
                   diode_voltages=v, diode_currents=i, diode_probes=("d1",), final_junctions=vh)
    assert tr.newton_iterations is newton and tr.matrix_updates is updates and tr.diode_voltages is v
    assert tr.diode_currents is i and tr.diode_probes == ["d1"] and tr.final_junctions is vh
    assert tr.info.tolist() == [0, 0, 2]
    assert "info 2" in Transient.__doc__
