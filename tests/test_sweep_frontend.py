"""Source sweeps, front end (no device): component names to table rows, argument checks
(nodal_amd/sweep.py resolve_sources, what Circuit.solve_sources hands to nodal_solve_sources)."""
import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import constants as c
from nodal_amd import generators as gen
from nodal_amd.lowering import lower
from nodal_amd.sweep import SourceSweep, resolve_sources

ROWS = [["r1", "R", "2", "1", "4"], ["r2", "R", "2", "1", "g"], ["r3", "R", "0.5", "1", "2"],
        ["e1", "E", "8", "4", "g"], ["a1", "A", "4", "1", "2"], ["a2", "A", "1", "2", "g"],
        ["v1", "VCVS", "2", "5", "g", "1", "2"], ["r5", "R", "3", "5", "g"],
        ["d1", "CCCS", "2", "2", "g", "1", "g", "r2"]]


def test_rows_and_values():
    nl = n.Netlist.from_rows(ROWS)
    rows, values = resolve_sources(nl, {"a1": [1.0, 0.5, 2.0], "e1": [5, 5, 4]})
    assert rows.dtype == np.int64 and rows.tolist() == [4, 3]
    assert values.dtype == np.float64 and values.shape == (3, 2)
    assert values.tolist() == [[1.0, 5.0], [0.5, 5.0], [2.0, 4.0]]
    table = lower(nl)
    assert set(table.type[rows].tolist()) == {c.T_A, c.T_E}


def test_unknown_name_raises_key_error():
    nl = n.Netlist.from_rows(ROWS)
    with pytest.raises(KeyError):
        resolve_sources(nl, {"a1": [1.0], "nope": [2.0]})


@pytest.mark.parametrize("name", ["r1", "v1", "d1"])
def test_components_that_enter_g_are_refused(name):
    nl = n.Netlist.from_rows(ROWS)
    with pytest.raises(ValueError, match="nodal_amd.batch"):
        resolve_sources(nl, {name: [1.0, 2.0]})


def test_ragged_lengths():
    nl = n.Netlist.from_rows(ROWS)
    with pytest.raises(ValueError, match="lengths"):
        resolve_sources(nl, {"a1": [1.0, 2.0], "e1": [1.0]})


def test_duplicated_name_sets_every_row_that_carries_it():
    rows = ROWS + [["a1", "A", "7", "2", "g"]]  # a1 twice: the reference resolves both rows to the last definition
    nl = n.Netlist.from_rows(rows)
    got_rows, values = resolve_sources(nl, {"a1": [1.0, 3.0]})
    assert got_rows.tolist() == [4, len(ROWS)]
    assert values.tolist() == [[1.0, 1.0], [3.0, 3.0]]


def test_native_and_dict_netlists_resolve_to_the_same_rows(tmp_path):
    rows = list(gen.grid_rows(200))  # large enough for the vectorised reader
    rows += [[f"ax{k}", "A", "1", str(k + 2), "g"] for k in range(5)] + [["ex", "E", "3", "x", "g"],
                                                                        ["rx", "R", "1", "x", "7"]]
    path = tmp_path / "net.csv"
    gen.write_csv(rows, str(path))
    fast = n.Netlist(str(path))
    assert getattr(fast, "_fast", False)
    slow = n.Netlist.from_rows(rows)
    sweep = {"ax3": [1.0, 2.0], "a1": [0.0, -1.0], "ex": [4.0, 5.0]}
    r_fast, v_fast = resolve_sources(fast, sweep)
    r_slow, v_slow = resolve_sources(slow, sweep)
    assert r_fast.tolist() == r_slow.tolist()
    assert np.array_equal(v_fast, v_slow)
    with pytest.raises(ValueError):
        resolve_sources(fast, {"rx": [1.0]})
    with pytest.raises(KeyError):
        resolve_sources(fast, {"zz": [1.0]})


def test_zero_members():
    nl = n.Netlist.from_rows(ROWS)
    rows, values = resolve_sources(nl, {"a1": [], "e1": []})
    assert rows.tolist() == [4, 3] and values.shape == (0, 2)
    rows, values = resolve_sources(nl, {})
    assert len(rows) == 0 and values.shape == (0, 0)


def test_sweep_result_container():
    nl = n.Netlist.from_rows(ROWS)
    x = np.arange(12.0).reshape(2, 6)
    sw = SourceSweep(x, np.zeros(2, np.int32), np.zeros(2), nl, [])
    assert len(sw) == 2
    assert np.array_equal(sw[1].result, x[1])
    assert [s.result[0] for s in sw] == [0.0, 6.0]
