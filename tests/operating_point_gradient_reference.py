"""The numpy / scipy restatement every operating-point-gradient test is measured against (never product code).

Built on tests/newton_reference.NewtonReference.  At an operating point

    F(x, p) = G(p) x + S i(S^T x; theta) - A(p) = 0,   i(v) = i_sat (exp(v / n_vt) - 1) + gmin v

so with c = dL/dx:  J^T lambda = c,  J = ref.jacobian(x) = G + S diag(g(v)) S^T at v = S^T x,  dL/dp = -lambda^T dF/dp:

    table row i      s_i(lambda, x) of tests/sensitivity_reference.formulas, evaluated on the table with the diodes appended
                     as resistors 1 / g(v) (the CCVS / CCCS cross terms land on their driving resistor); the appended rows
                     are discarded: their value is the device's own, not a parameter
    diode d          D = lambda(a) - lambda(b):   d/di_sat = -D expm1(v / n_vt),   d/dn_vt = D i_sat exp(v / n_vt) v / n_vt^2
    gmin             the sum over the diodes of -D v
    a named source   the formula of its A / E row (it reads neither x nor the value)

J^T lambda = c is solved by SuperLU with one step of refinement (NewtonReference.solve).

Bars, in the project's way (sensitivity_reference.parity_bars extended to the diode formulas): an error of TOL |lambda|_inf
in every entry of lambda and of TOL |x|_inf in every entry of x, propagated to first order through each formula -- for a
diode dD = 2 TOL |lambda|_inf and dv = 2 TOL |x|_inf through the formula's own d/dD and d/dv -- plus 8 eps of the formula's
scale without cancellation (every difference a sum; expm1 as e + 1).  Nothing else is chosen.

Closed forms for one current source I into one diode, gmin = 0, L = v:  v = n_vt log1p(I / i_sat), so
    dL/dI = n_vt / (I + i_sat),   dL/di_sat = -n_vt I / (i_sat (i_sat + I)),   dL/dn_vt = log1p(I / i_sat).

Planted defects (DEFECTS), each a reference gradient that is wrong in a known way:
    "exp_not_expm1"         d/di_sat with exp in place of expm1
    "nvt_sign"              d/dn_vt with the other sign
    "jacobian_at_last_vh"   J linearised at the run's last limited voltages instead of at x
    "no_transpose"          lambda from J, not J^T
    "diode_rows_kept"       the companion rows keep their R formula where the truth is zero ("companion" in the result)
    "gmin_dropped_from_g"   J with g - gmin
"""
import numpy as np

from nodal_amd import constants as c
from tests import newton_reference as nr
from tests.newton_reference import TIGHT, NewtonReference
from tests.sensitivity_reference import EPS, TOL, formulas, parity_bars, table_of

DEFECTS = ("exp_not_expm1", "nvt_sign", "jacobian_at_last_vh", "no_transpose", "diode_rows_kept", "gmin_dropped_from_g")


def polish(ref, x, steps=3):
    """`steps` further reference Newton steps from x, each linearised at the voltages of its own start (no limiting
    acts this close to the answer)"""
    x = np.asarray(x, dtype=np.float64)
    for _ in range(steps):
        x, _, _ = ref.one_step(x, ref.voltages(x))
    return x


def companion_table(ref, g):
    """(the lowered table of ref's netlist with the diodes appended as resistors 1 / g, ncomp of the netlist alone)"""
    table = table_of(ref.nl)
    ia, ib = ref.ia.astype(np.int32), ref.ib.astype(np.int32)
    same = ia == ib  # (a diode between a node and itself: a row between ground and ground)
    ia[same] = -1
    ib[same] = -1
    with np.errstate(divide="ignore"):
        r = 1.0 / np.asarray(g, dtype=np.float64)
    types = np.full(len(r), c.TYPE_CODE["R"], dtype=np.uint8)
    return table.with_rows_appended(types, r, ia, ib), table.ncomp


def _source_rows(ref):
    ty = np.asarray(table_of(ref.nl).type)
    return {key: i for i, key in enumerate(ref.nl.component_keys) if ty[i] in (c.TYPE_CODE["A"], c.TYPE_CODE["E"])}


def gradient(ref, x, cotangent, defect=None, last_vh=None):
    """The reference gradient at x (taken as it is: polish first where the exact operating point is meant).  Returns a
    dict: values [ncomp], companion [D] (zeros: not parameters), i_sat, n_vt [D], gmin, sources (name -> float, every
    A / E row of the netlist), adjoint [n], and bars: the same keys (but adjoint) with the propagated bars.
    defect: one of DEFECTS; "jacobian_at_last_vh" needs last_vh [D], the voltages the run's last step was linearised at."""
    assert defect is None or defect in DEFECTS
    x, cot = np.asarray(x, dtype=np.float64), np.asarray(cotangent, dtype=np.float64)
    v = ref.voltages(x)
    at = np.asarray(last_vh, dtype=np.float64) if defect == "jacobian_at_last_vh" else v
    with np.errstate(all="ignore"):
        g = ref.conductance(at)
    J = ref.matrix(g - ref.gmin if defect == "gmin_dropped_from_g" else g)
    lam = ref.solve(J if defect == "no_transpose" else J.T.tocsr(), cot)
    table, ncomp = companion_table(ref, g)
    with np.errstate(all="ignore"):
        rows = formulas(table, lam, x)
    companion = rows[ncomp:].copy() if defect == "diode_rows_kept" else np.zeros(len(v))
    D = ref.S.T @ lam
    q = v / ref.n_vt
    e = np.exp(q)
    g_isat = -D * (e if defect == "exp_not_expm1" else np.expm1(q))
    g_nvt = D * ref.i_sat * e * v / ref.n_vt ** 2
    if defect == "nvt_sign":
        g_nvt = -g_nvt
    g_gmin = float(np.sum(-D * v))
    sources = {name: float(rows[i]) for name, i in _source_rows(ref).items()}

    # ---- the bars ----
    lmax, xmax = np.abs(lam).max(initial=0.0), np.abs(x).max(initial=0.0)
    with np.errstate(all="ignore"):
        row_bars = parity_bars(table, lam, x, None)
    dD, dv = 2.0 * TOL * lmax, 2.0 * TOL * xmax
    Dabs, vabs = abs(ref.S).T @ np.abs(lam), abs(ref.S).T @ np.abs(x)  # (without cancellation: every difference a sum)
    b_isat = dD * np.abs(np.expm1(q)) + dv * np.abs(D) * e / ref.n_vt + 8 * EPS * Dabs * (e + 1.0)
    scale_nvt = ref.i_sat * e / ref.n_vt ** 2
    b_nvt = dD * scale_nvt * np.abs(v) + dv * np.abs(D) * scale_nvt * np.abs(1.0 + q) + 8 * EPS * Dabs * scale_nvt * vabs
    b_gmin = float(np.sum(dD * np.abs(v) + dv * np.abs(D)) + 8 * EPS * np.sum(Dabs * vabs))
    bars = {"values": row_bars[:ncomp], "companion": np.zeros(len(v)), "i_sat": b_isat, "n_vt": b_nvt, "gmin": b_gmin,
            "sources": {name: float(row_bars[i]) for name, i in _source_rows(ref).items()}}
    return {"values": rows[:ncomp].copy(), "companion": companion, "i_sat": g_isat, "n_vt": g_nvt, "gmin": g_gmin,
            "sources": sources, "adjoint": lam, "bars": bars}


def worst_ratio(got, want, bars):
    """max |got - want| / bar over the entries (an entry with a zero bar must be met exactly: inf otherwise)"""
    got, want, bars = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (got, want, bars))
    err = np.abs(got - want)
    with np.errstate(all="ignore"):
        ratio = np.where(bars > 0.0, err / np.where(bars > 0.0, bars, 1.0), np.where(err == 0.0, 0.0, np.inf))
    ratio = np.where(np.isnan(err), np.inf, ratio)
    return float(ratio.max(initial=0.0))


# ---- closed forms ---------------------------------------------------------------------------------------------------
def source_diode_closed_forms(I, i_sat, n_vt):
    """one current source I into one diode to ground, gmin = 0, L = v: (dL/dI, dL/di_sat, dL/dn_vt)"""
    return n_vt / (I + i_sat), -n_vt * I / (i_sat * (i_sat + I)), float(np.log1p(I / i_sat))


# ---- central differences of the reference's own Newton run ------------------------------------------------------------
def _with_value(rows, name, factor):
    out = [list(r) for r in rows]
    hits = [r for r in out if r[0] == name]
    assert len(hits) == 1, name
    hits[0][2] = repr(float(hits[0][2]) * factor)
    return out


def perturbed(rows, diodes, gmin, kind, name, factor, sources=None):
    """a tightly converged NewtonReference with parameter (kind, name) multiplied by `factor`.  kind: "value" (a table
    row, sources included), "i_sat", "n_vt" (a diode), "gmin" (name ignored)"""
    rows, diodes = [list(r) for r in rows], [tuple(d) for d in diodes]
    if kind == "value":
        if sources and name in sources:
            sources = {**sources, name: sources[name] * factor}
        else:
            rows = _with_value(rows, name, factor)
    elif kind in ("i_sat", "n_vt"):
        at = 1 if kind == "i_sat" else 2
        assert sum(d[0] == name for d in diodes) == 1, name
        diodes = [tuple(d[:at]) + (d[at] * factor,) + tuple(d[at + 1:]) if d[0] == name else d for d in diodes]
    else:
        assert kind == "gmin"
        gmin = gmin * factor
    return NewtonReference(rows, diodes, gmin=gmin, sources=sources, **TIGHT)


def parameter_value(rows, diodes, gmin, kind, name, sources=None):
    if kind == "value":
        return float(sources[name]) if sources and name in sources else float([r for r in rows if r[0] == name][0][2])
    if kind == "gmin":
        return float(gmin)
    d = [d for d in diodes if d[0] == name][0]
    return float(d[1 if kind == "i_sat" else 2])


def central_difference(rows, diodes, gmin, kind, name, cotangent, x_start, step=1e-6, sources=None):
    """dL/dp of L = cotangent . x by a central difference with the relative step `step` in the parameter: each side is the
    reference's own Newton run with TIGHT tolerances from x_start, then polished"""
    p = parameter_value(rows, diodes, gmin, kind, name, sources)
    side = []
    for factor in (1.0 + step, 1.0 - step):
        ref = perturbed(rows, diodes, gmin, kind, name, factor, sources)
        run = ref.run(x_start)
        assert run["converged"], (kind, name)
        side.append(float(np.asarray(cotangent) @ polish(ref, run["x"])))
    return (side[0] - side[1]) / (2.0 * step * p)


def lookup(grad, kind, name, names, component_keys):
    """the entry of a gradient() result that central_difference(kind, name) approximates"""
    if kind == "gmin":
        return grad["gmin"]
    if kind in ("i_sat", "n_vt"):
        return float(grad[kind][list(names).index(name)])
    rows = [i for i, key in enumerate(component_keys) if key == name]
    return float(grad["values"][rows].sum())


# ---- a case whose Jacobian is not symmetric ---------------------------------------------------------------------------
def nonsymmetric_case():
    """newton_reference.lu_case() with one VCVS row and one CCCS row driven by the grid resistor rh0_4 appended: G is
    not symmetric, and the CCCS row's cross term lands on rh0_4.  Returns (rows, diodes, initial [n])."""
    rows, diodes, _ = nr.lu_case()
    rows = rows + [["v1", "VCVS", "0.3", "100", "g", "20", "21"], ["f1", "CCCS", "0.5", "110", "g", "5", "6", "rh0_4"]]
    import nodal_amd as n
    nl = n.Netlist.from_rows([list(r) for r in rows])
    initial = np.zeros(len(nl.nodenum) + len(nl.anomnum))
    initial[nr._index(nl, "30")] = 1.2
    return rows, diodes, initial
