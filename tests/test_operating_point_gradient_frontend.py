"""The front end of OperatingPoint.gradient without a device: the argument checks, the OperatingPointGradient container
built from arrays (of, normalized, the cutting of the companion rows) and the ValueErrors."""
import numpy as np
import pytest

import nodal_amd as n
from nodal_amd import _ffi
from nodal_amd.operating_point import NewtonHistory, OperatingPoint, OperatingPointGradient, check_cotangent

ROWS = [["e1", "E", "5", "1", "g"], ["r1", "R", "1000", "1", "2"], ["r2", "R", "50", "2", "g"], ["r2", "R", "75", "2", "g"],
        ["a1", "A", "0.25", "2", "g"]]


def netlist():
    return n.Netlist.from_rows([list(r) for r in ROWS])


def history(count=1):
    return NewtonHistory(np.zeros((count, 4)), np.zeros(count, dtype=np.int32), np.ones(count, dtype=np.int32), [0] * count)


def operating_point(x, circuit=None, **extra):
    return OperatingPoint(np.asarray(x, dtype=np.float64), ["d1"], np.zeros(1), np.zeros(1), np.ones(1), True, 1, history(),
                          circuit=circuit, leads=(np.array([1], dtype=np.int32), np.array([-1], dtype=np.int32)), **extra)


REMEMBERED = dict(i_sat=np.array([1e-14]), n_vt=np.array([0.02585]), gmin=1e-12, source_rows=np.zeros(0, dtype=np.int64),
                  source_values=np.zeros(0), source_columns={})


# ---- the cotangent ------------------------------------------------------------------------------------------------------
def test_check_cotangent():
    cot = check_cotangent([1, 2, 3], 3)
    assert cot.dtype == np.float64 and cot.flags["C_CONTIGUOUS"] and cot.tolist() == [1.0, 2.0, 3.0]
    assert check_cotangent(np.zeros(0), 0).shape == (0,)
    for bad in (np.zeros(2), np.zeros((1, 3)), np.zeros((3, 1)), 1.0):
        with pytest.raises(ValueError, match="shape"):
            check_cotangent(bad, 3)
    for bad in ([0.0, np.nan, 0.0], [np.inf, 0.0, 0.0], [0.0, 0.0, -np.inf]):
        with pytest.raises(ValueError, match="not finite"):
            check_cotangent(bad, 3)


# ---- OperatingPoint remembers what the gradient needs ---------------------------------------------------------------------
def test_results_built_from_arrays_keep_working():
    op = operating_point([1.0, 2.0, 3.0])
    assert op.i_sat is None and op.n_vt is None and op.gmin is None
    assert op.source_rows is None and op.source_values is None and op.source_columns is None
    assert op.converged and op.iterations == 1 and op.scaled_residual == 0.0
    op = operating_point([1.0, 2.0, 3.0], **REMEMBERED)
    assert op.i_sat[0] == 1e-14 and op.n_vt[0] == 0.02585 and op.gmin == 1e-12 and op.source_columns == {}


def test_gradient_needs_the_circuit():
    with pytest.raises(ValueError, match="not made by Circuit.operating_point"):
        operating_point([1.0, 2.0, 3.0]).gradient(np.ones(3))
    with pytest.raises(ValueError, match="not made by Circuit.operating_point"):
        operating_point([1.0, 2.0, 3.0], **REMEMBERED).gradient(np.ones(3))
    with pytest.raises(ValueError, match="not made by Circuit.operating_point"):
        operating_point([1.0, 2.0, 3.0], circuit=object()).gradient(np.ones(3))  # (without the diodes' parameters)


def test_gradient_checks_the_cotangent_and_the_point_before_the_device():
    class NoDevice:
        def _operating_point_gradient(self, *args):
            raise AssertionError("the device is reached only with checked arguments")

    op = operating_point([1.0, 2.0, 3.0], circuit=NoDevice(), **REMEMBERED)
    with pytest.raises(ValueError, match="shape"):
        op.gradient(np.ones(2))
    with pytest.raises(ValueError, match="shape"):
        op.gradient(np.ones((1, 3)))
    with pytest.raises(ValueError, match="not finite"):
        op.gradient([1.0, np.nan, 0.0])
    lost = operating_point([np.nan] * 3, circuit=NoDevice(), **REMEMBERED)
    with pytest.raises(ValueError, match="lost run"):
        lost.gradient(np.ones(3))
    with pytest.raises(AssertionError):
        op.gradient(np.ones(3))


# ---- the container ----------------------------------------------------------------------------------------------------------
def container(**extra):
    nl = netlist()
    handed = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 0.0, 0.0])  # five table rows and two companion rows behind them
    return OperatingPointGradient(nl, handed, ["d1", "d2"], [10.0, 20.0], [-1.0, -2.0], 0.5, {"e1": 7.0}, 0, 1e-17, 2e-16,
                                  **extra)


def test_the_container_cuts_the_companion_rows():
    grad = container()
    assert grad.values.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0] and grad.names == ["e1", "r1", "r2", "r2", "a1"]
    assert grad.gmin == 0.5 and isinstance(grad.gmin, float) and grad.source_values == {"e1": 7.0}
    assert grad.info == 0 and grad.scaled_residual == 1e-17 and grad.operating_point_residual == 2e-16
    assert grad.adjoint is None and grad.timings is None


def test_of_names_components_and_diodes():
    grad = container()
    assert grad.of("r1") == 2.0 and grad.of("a1") == 5.0
    assert grad.of("r2") == 7.0  # (a name the netlist defines twice: the sum over its rows, as Gradient.of)
    assert grad.of("d1") == (10.0, -1.0) and grad.of("d2") == (20.0, -2.0)
    with pytest.raises(KeyError):
        grad.of("nothing")


def test_normalized():
    with pytest.raises(ValueError, match="without the diodes"):
        container().normalized
    grad = container(diode_i_sat=[1e-14, 2e-14], diode_n_vt=[0.025, 0.05])
    values, i_sat, n_vt = grad.normalized
    # (the table lowered from the netlist; a name defined twice carries its last value on every row, as lowering.py)
    assert values.tolist() == [5.0, 2000.0, 225.0, 300.0, 1.25]
    assert i_sat.tolist() == [10.0 * 1e-14, 20.0 * 2e-14] and n_vt.tolist() == [-0.025, -0.1]


def test_the_binding_declares_the_call():
    assert "nodal_newton_gradient" in _ffi.SIGNATURES and len(_ffi.SIGNATURES["nodal_newton_gradient"][1]) == 21
