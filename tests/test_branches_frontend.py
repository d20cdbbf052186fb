"""Branches / Envelope containers, the argument rule of solve_sources and the ABI's new names: no device needed."""
import os
import re

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd.branches import Branches, Envelope
from nodal_amd.sweep import SourceSweep, check_sweep_options
from tests.conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the README's circuit (the reference's doc/1.6.1.csv); nodes 1, 4, 2 -> 0, 1, 2; x = e(1) 2, e(4) 8, e(2) -1,
# i(e1) 3, i(d1) -2
README = [["r1", "R", "2", "1", "4"], ["r2", "R", "2", "1", "g"], ["r3", "R", "0.5", "1", "2"],
          ["e1", "E", "8", "4", "g"], ["a1", "A", "4", "1", "2"], ["d1", "CCCS", "2", "2", "g", "1", "g", "r2"]]
# by hand, row by row: voltage = e(a) - e(b); current; absorbed power
README_V = [-6.0, 2.0, 3.0, 8.0, 3.0, -1.0]
README_I = [-3.0, 1.0, 6.0, 3.0, 4.0, -2.0]
README_P = [18.0, 2.0, 18.0, -24.0, -12.0, -2.0]


def readme_branches():
    nl = n.Netlist.from_rows(README)
    return Branches(nl, np.array(README_V), np.array(README_I), np.array(README_P), 38.0, -38.0)


def duplicate_case():
    case = next(c for c in load_golden("cases.json") if c["name"] == "edge/duplicate_r")
    return n.Netlist.from_rows(case["rows"])


def test_lookup_by_name():
    br = readme_branches()
    assert br.names == ["r1", "r2", "r3", "e1", "a1", "d1"]
    assert len(br) == 6
    assert br["r3"] == (3.0, 6.0, 18.0)
    assert br["d1"] == (-1.0, -2.0, -2.0)
    assert br.rows("e1") == [3]
    assert br.dissipated == 38.0 and br.absorbed_by_sources == -38.0
    with pytest.raises(KeyError):
        br["nope"]
    with pytest.raises(KeyError):
        br.rows("nope")


def test_duplicated_names():
    # r1 twice (both rows carry the last definition, 4 ohm between 1 and 2), r2, a1; x = [3, 1]
    nl = duplicate_case()
    assert nl.component_keys == ["r1", "r1", "r2", "a1"]
    br = Branches(nl, np.array([2.0, 2.5, 1.0, 3.0]), np.array([0.5, 0.625, 1.0, 1.0]),
                  np.array([1.0, 1.5625, 1.0, -3.0]), 3.5625, -3.0)
    assert br.rows("r1") == [0, 1]
    assert br["r1"] == (2.5, 0.625, 1.5625)  # the last row that carries the name
    assert br.names == ["r1", "r1", "r2", "a1"]
    text = str(br).splitlines()
    assert text == ["v(a1) \t= 3.0", "i(a1) \t= 1.0", "p(a1) \t= -3.0",
                    "v(r1) \t= 2.5", "i(r1) \t= 0.625", "p(r1) \t= 1.5625",
                    "v(r2) \t= 1.0", "i(r2) \t= 1.0", "p(r2) \t= 1.0"]


def test_str_line_order_and_number_format():
    nl = n.Netlist.from_rows(README)
    third = 1.0 / 3.0
    br = Branches(nl, np.array([third, 1e-20, 3.0, 8.0, 3.0, -1.0]), np.array(README_I), np.array(README_P), 0.0, 0.0)
    lines = str(br).splitlines()
    assert [line.split(" \t= ")[0] for line in lines] == [
        f"{q}({name})" for name in ["a1", "d1", "e1", "r1", "r2", "r3"] for q in "vip"]
    # values as Solution prints them: the shortest repr that round-trips, str(np.float64)
    assert lines[9] == f"v(r1) \t= {str(np.float64(third))}"
    assert lines[12] == "v(r2) \t= 1e-20"
    assert lines[10] == "i(r1) \t= -3.0"
    sol = str(n.Solution(np.array([third, 8.0, -1.0, 3.0, -2.0]), nl, ["e1", "d1"])).splitlines()
    assert sol[1].split(" \t= ")[1] == lines[9].split(" \t= ")[1]


def test_kcl_residual_by_hand():
    br = readme_branches()
    assert np.array_equal(br.kcl_residual(), np.zeros(3))
    # made-up currents 1 .. 6: signed (R +, others -) = 1, 2, 3, -4, -5, -6
    # node 1 (a of r1, r2, r3, a1): 1 + 2 + 3 - 5 = 1; node 4 (b of r1, a of e1): -1 - 4 = -5;
    # node 2 (b of r3, b of a1, a of d1): -3 + 5 - 6 = -4
    odd = Branches(br._netlist, np.zeros(6), np.arange(1.0, 7.0), np.zeros(6), 0.0, 0.0)
    assert np.array_equal(odd.kcl_residual(), np.array([1.0, -5.0, -4.0]))
    # duplicate_r, x = [3, 1]: the true currents balance
    nl = duplicate_case()
    dup = Branches(nl, np.array([2.0, 2.0, 1.0, 3.0]), np.array([0.5, 0.5, 1.0, 1.0]), np.array([1.0, 1.0, 1.0, -3.0]),
                   3.0, -3.0)
    assert np.array_equal(dup.kcl_residual(), np.zeros(2))
    assert dup.dissipated + dup.absorbed_by_sources == 0.0


def test_envelope_worst_lists_with_ties():
    nl = n.Netlist.from_rows(README)
    env = Envelope(nl, np.array([2.0, 7.0, 7.0, 0.5, np.nan, 7.0]), np.array([3, 1, 0, 2, -1, 5], dtype=np.int32),
                   np.array([-4.0, 0.0, -1.0]), np.array([2, 0, 1], dtype=np.int32),
                   np.array([4.0, 9.0, 0.5]), np.array([3, 4, 0], dtype=np.int32),
                   np.array([1.0, 2.0]), np.array([-1.0, -2.0]))
    assert env.worst_current(2) == [("r2", 7.0, 1), ("r3", 7.0, 0)]
    assert env.worst_current(4) == [("r2", 7.0, 1), ("r3", 7.0, 0), ("d1", 7.0, 5), ("r1", 2.0, 3)]
    assert env.worst_current(100) == [("r2", 7.0, 1), ("r3", 7.0, 0), ("d1", 7.0, 5), ("r1", 2.0, 3), ("e1", 0.5, 2)]
    assert env.worst_current(0) == []
    # nodes 1, 4, 2: |.| = 4 (a tie of min and max: the minimum is reported), 9, 1
    assert env.worst_drop(3) == [("4", 9.0, 4), ("1", -4.0, 2), ("2", -1.0, 1)]
    assert env.worst_drop(1) == [("4", 9.0, 4)]
    empty = Envelope.empty(nl, 6, members=3)
    assert np.isnan(empty.current_absmax).all() and (empty.current_member == -1).all()
    assert empty.potential_min.shape == (3,) and (empty.potential_max_member == -1).all()
    assert np.isnan(empty.dissipated).all() and empty.dissipated.shape == (3,)
    assert empty.worst_current(5) == [] and empty.worst_drop(5) == []


class _NoDevice:
    """stands in for a handle: any use is a device call"""

    def __getattr__(self, name):
        raise AssertionError(f"device call: {name}")


def test_argument_rule_is_checked_before_any_device_call():
    with pytest.raises(ValueError, match="branches=True"):
        check_sweep_options(False, False)
    for ok in ((False, True), (True, True), (True, False)):
        check_sweep_options(*ok)
    c = n.Circuit.__new__(n.Circuit)
    c.netlist, c.sparse, c._device, c._handle = n.Netlist.from_rows(README), True, 0, _NoDevice()
    with pytest.raises(ValueError, match="branches=True"):
        c.solve_sources({"a1": [1.0, 2.0]}, keep_solutions=False)
    c._handle = None


def test_sweep_without_solutions_is_a_container():
    nl = n.Netlist.from_rows(README)
    sw = SourceSweep(None, np.zeros(3, dtype=np.int32), np.zeros(3), nl, ["e1", "d1"], envelope=Envelope.empty(nl, 6, 3))
    assert len(sw) == 3 and sw.result is None
    with pytest.raises(ValueError):
        sw[0]
    old = SourceSweep(np.zeros((2, 5)), np.zeros(2, dtype=np.int32), np.zeros(2), nl, ["e1", "d1"])
    assert len(old) == 2 and old.envelope is None and str(old[1]).startswith("Ground node: g")


def test_exports():
    import nodal
    assert nodal.Branches is Branches and n.Envelope is Envelope
    assert callable(n.Circuit.branches)


def test_header_and_binding_name_the_new_entries():
    text = open(os.path.join(ROOT, "include", "nodal_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("nodal_branches", "nodal_solve_sources_branches"):
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in _ffi.SIGNATURES
    # the sweep entry: the nine arguments of nodal_solve_sources, then the seven envelope outputs
    assert _ffi.SIGNATURES["nodal_solve_sources_branches"][1][:9] == _ffi.SIGNATURES["nodal_solve_sources"][1]
    assert len(_ffi.SIGNATURES["nodal_solve_sources_branches"][1]) == 16
