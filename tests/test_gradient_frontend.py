"""The host side of Circuit.gradient: argument checks, shapes and the Gradient container need no device."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd.gradient import Gradient, check_gradient_arguments
from nodal_amd.lowering import lower

ROWS = [["r1", "R", "2", "1", "g"], ["r2", "R", "3", "1", "2"], ["r2", "R", "5", "2", "g"], ["a1", "A", "1", "1", "g"],
        ["e1", "E", "1.5", "3", "g"], ["r3", "R", "1", "3", "2"], ["e1", "E", "2.5", "4", "g"], ["r4", "R", "1", "4", "2"]]


@pytest.fixture(scope="module")
def nl():
    return n.Netlist.from_rows(ROWS)


def test_single_solve_arguments(nl):
    cot, rows, x, columns = check_gradient_arguments(nl, 6, [1, 2, 3, 4, 5, 6])
    assert cot.shape == (1, 6) and cot.dtype == np.float64 and cot.flags.c_contiguous
    assert rows.shape == (0,) and rows.dtype == np.int64 and x is None and columns == {}
    cot, rows, x, columns = check_gradient_arguments(nl, 6, np.ones(6), solutions=np.arange(6))
    assert x.shape == (1, 6) and x.dtype == np.float64 and rows.shape == (0,)
    for bad in (np.ones(5), np.ones((1, 6)), np.ones((6, 1)), 1.0):
        with pytest.raises(ValueError, match="shape"):
            check_gradient_arguments(nl, 6, bad)
    with pytest.raises(ValueError, match="shape"):
        check_gradient_arguments(nl, 6, np.ones(6), solutions=np.ones((1, 6)))


def test_sweep_arguments(nl):
    sources = {"a1": [1.0, 2.0, 3.0], "e1": [0.5, 0.25, -1.0]}
    cot, rows, x, columns = check_gradient_arguments(nl, 6, np.ones((3, 6)), sources, np.zeros((3, 6)))
    assert cot.shape == (3, 6) and x.shape == (3, 6) and cot.flags.c_contiguous and x.flags.c_contiguous
    # a name the netlist defines twice carries both of its rows
    assert rows.tolist() == [3, 4, 6] and columns == {"a1": [0], "e1": [1, 2]}
    # non-contiguous input is made contiguous, not refused
    wide = np.ones((3, 12))[:, ::2]
    assert check_gradient_arguments(nl, 6, wide, sources, wide)[0].flags.c_contiguous
    for c, s in ((np.ones((2, 6)), np.zeros((3, 6))), (np.ones((3, 6)), np.zeros((2, 6))), (np.ones((3, 5)), np.zeros((3, 5))),
                 (np.ones(6), np.zeros((3, 6))), (np.ones((3, 6)), np.zeros(6))):
        with pytest.raises(ValueError, match="shape"):
            check_gradient_arguments(nl, 6, c, sources, s)
    with pytest.raises(ValueError, match="solutions"):
        check_gradient_arguments(nl, 6, np.ones((3, 6)), sources)
    with pytest.raises(ValueError, match="only independent sources"):
        check_gradient_arguments(nl, 6, np.ones((3, 6)), {"r1": [1.0, 2.0, 3.0]}, np.zeros((3, 6)))
    with pytest.raises(KeyError):
        check_gradient_arguments(nl, 6, np.ones((3, 6)), {"nope": [1.0, 2.0, 3.0]}, np.zeros((3, 6)))
    with pytest.raises(ValueError, match="lengths differ"):
        check_gradient_arguments(nl, 6, np.ones((3, 6)), {"a1": [1.0, 2.0, 3.0], "e1": [1.0]}, np.zeros((3, 6)))
    with pytest.raises(TypeError):
        check_gradient_arguments(nl, 6, np.ones((3, 6)), ["a1"], np.zeros((3, 6)))
    # no members at all
    cot, rows, x, columns = check_gradient_arguments(nl, 6, np.zeros((0, 6)), {"a1": []}, np.zeros((0, 6)))
    assert cot.shape == (0, 6) and rows.tolist() == [3] and columns == {"a1": [0]}


def test_container_from_arrays(nl):
    values = np.arange(8, dtype=np.float64) + 1.0
    g = Gradient(nl, values, {"a1": np.array([1.0, 2.0])}, np.zeros(2, dtype=np.int32), np.zeros(2),
                 adjoints=np.ones((2, 6)))
    assert len(g) == 2 and g.names == [r[0] for r in ROWS] and g.adjoints.shape == (2, 6)
    assert g.of("r1") == 1.0 and g.of("a1") == 4.0
    # a repeated name: the sum over its rows
    assert g.of("r2") == 2.0 + 3.0 and g.of("e1") == 5.0 + 7.0
    with pytest.raises(KeyError):
        g.of("nope")
    assert np.array_equal(g.source_values["a1"], [1.0, 2.0])
    # the value column comes from lowering the netlist when no table is given, else from the table
    assert np.array_equal(g.component_values, np.asarray(lower(nl).value))
    table = lower(nl).with_values(np.full(8, 2.0))
    assert np.array_equal(Gradient(nl, values, {}, [], [], table=table).component_values, np.full(8, 2.0))
    assert np.array_equal(Gradient(nl, values, {}, [], [], table=table).normalized, 2.0 * values)
    assert Gradient(nl, values, {}, [], []).adjoints is None


def test_table_with_values_shares_every_other_column(nl):
    table = lower(nl)
    new = np.asarray(table.value) * 2.0
    other = table.with_values(new)
    assert other.value is new and other.a is table.a and other.type is table.type and other.k is table.k
    assert (other.ncomp, other.K, other.B) == (table.ncomp, table.K, table.B)
    assert np.array_equal(np.asarray(table.value) * 2.0, new)  # (the original column is not written)


def test_binding_declares_the_entry_point():
    res, args = _ffi.SIGNATURES["nodal_gradient"]
    assert len(args) == 12
    assert hasattr(_ffi.Handle, "gradient") and hasattr(n.Circuit, "gradient") and hasattr(n.Circuit, "set_values")
    assert isinstance(n.Circuit.values, property)


def test_import_does_not_import_torch():
    code = "import sys, nodal_amd, nodal_amd.gradient; assert 'torch' not in sys.modules, 'torch was imported'"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)
