"""tests/presolve_reference.py pinned down without a GPU: the hand-written plans of its families against the oracle's
G, b.  The identities hold for every plan; the reduced system's solution, recovered, is the full solve (np.linalg.solve
refined in longdouble for the potentials, the leaf-peeling recovery for the branch currents); every row of G x - b at
the recovered values is within its a-priori bound; a planted defect in a plan fails an identity BY NAME; the float64
sparse statement used for the large case agrees with the dense longdouble one.  tests/test_gpu_presolve.py asserts the
same plans of the device and holds its reduced system and recovery to the same reference."""
import numpy as np
import pytest

import nodal_amd as n
from oracle import nodal_oracle as oracle
from tests import presolve_reference as ref

LD = ref.LD
BAR = 2.0
TYPE_NAME = {ref.T_R: "R", ref.T_A: "A", ref.T_E: "E", ref.T_VCVS: "VCVS", ref.T_CCVS: "CCVS", ref.T_CCCS: "CCCS"}
FAMILIES = ref.families()
OK = [name for name, (_, plan) in FAMILIES.items() if plan["ok"]]
_systems = {}


def oracle_system(name):
    """(G, b, K, stamps) of a family: the oracle's model of the same rows as a netlist, brought into the table's
    numbering (the front end numbers nodes by first appearance, Net by grid position)."""
    if name not in _systems:
        net = FAMILIES[name][0]
        lab = lambda k: "g" if k < 0 else f"n{k}"  # noqa: E731
        rows = []
        for i, (ty, v, a, b, c, d, drv, _k) in enumerate(net.rows):
            row = [f"x{i}", TYPE_NAME[ty], repr(v), lab(a), lab(b)]
            if ty in (ref.T_VCVS, ref.T_CCVS, ref.T_CCCS):
                row += [lab(c), lab(d)]
            if ty in (ref.T_CCVS, ref.T_CCCS):
                row.append(f"x{drv}")
            rows.append(row)
        nl = n.Netlist.from_rows(rows)
        G, b, _ = oracle.build_model(nl, False)
        K = nl.nums["kcl"]
        assert K == net.K and nl.nums["be"] == net.B
        perm = np.array([nl.nodenum[f"n{k}"] for k in range(K)] + list(range(K, K + net.B)))
        _systems[name] = (G[np.ix_(perm, perm)], b[perm], K, ref.stamps_per_node(net.table()))
    return _systems[name]


def reduction(name, plan=None):
    G, b, K, stamps = oracle_system(name)
    return ref.Reduction(G, b, K, plan or FAMILIES[name][1], stamps)


def test_the_table_of_a_family_is_the_oracle_model():
    """Net.table() through the oracle's table assembler equals the netlist route above: the numbering is the table's."""
    for name in ("combined", "ccvs", "cccs_output_pivot"):
        G, b, _, _ = oracle_system(name)
        Gt, bt = oracle.assemble_fast(FAMILIES[name][0].table())
        assert np.array_equal(Gt.toarray(), G) and np.array_equal(bt, b), name


@pytest.mark.parametrize("name", OK)
def test_identities_hold_for_the_hand_written_plans(name):
    red = reduction(name)
    assert red.identities(BAR) == []
    net, plan = FAMILIES[name]
    assert red.Kr == net.K - len(plan["exprs"])
    assert len(red.kept) + len(red.cccs) + len(red.elim) == net.B


@pytest.mark.parametrize("name", OK)
def test_reduced_solution_recovered_is_the_full_solve(name):
    G, b, K, _ = oracle_system(name)
    red = reduction(name)
    y = red.solve_reduced()
    x, e = red.recover(y)
    assert not np.isnan(x).any()
    full = ref.full_solve(G, b)
    # both are refined in longdouble: what is left is far below fp64's unit roundoff times the condition number
    scale = np.abs(full).max()
    assert np.abs(x[:K] - full[:K]).max() <= 1e-13 * scale, (name, float(np.abs(x[:K] - full[:K]).max()))
    assert np.abs(x[K:] - full[K:]).max() <= 1e-13 * max(scale, np.abs(full[K:]).max())
    r = np.abs(red.G @ x - red.b)
    assert np.all(r <= BAR * red.residual_bounds(x, e, y, True)), name


@pytest.mark.parametrize("name", OK)
def test_branch_and_pivot_rows_hold_whatever_y_is(name):
    red = reduction(name)
    y = np.random.default_rng(7).standard_normal(red.Kr + len(red.kept))
    x, e = red.recover(y)
    bound = red.residual_bounds(x, e, y, False)
    hold = np.isfinite(bound)
    assert hold.sum() == len(red.pivots) + len(red.elim) + len(red.cccs)
    r = np.abs(red.G @ x - red.b)
    assert np.all(r[hold] <= BAR * bound[hold]), name


def _mutated(name, p, **change):
    plan = FAMILIES[name][1]
    q, cst, c, d, g = plan["exprs"][p]
    e = dict(q=q, cst=cst, c=c, d=d, g=g)
    e.update(change)
    exprs = dict(plan["exprs"])
    exprs[p] = (e["q"], e["cst"], e["c"], e["d"], e["g"])
    return dict(plan, exprs=exprs)


def test_planted_plan_defects_fail_an_identity_by_name():
    g = FAMILIES["ccvs"][1]["exprs"][35][4]
    cases = [("ccvs", _mutated("ccvs", 35, g=-g), "I1"),                      # the CCVS gain without its minus
             ("vcvs_surviving", _mutated("vcvs_surviving", 35, c=16, d=3), "I1"),  # the control term's sign
             ("vcvs_pivot_control", _mutated("vcvs_pivot_control", 35, cst=0.0), "I2"),  # a control's constant dropped
             ("stack3", _mutated("stack3", 36, cst=0.75), "I2"),              # a stacked source that does not add up
             ("e_floating", _mutated("e_floating", 20, cst=1.25), "I2"),      # the orientation of a floating source
             ("shared_base", _mutated("shared_base", 22, q=10), "I1"),        # a pivot hung on another base ...
             ("shared_base", _mutated("shared_base", 22, q=10), "I3")]        # ... whose KCL row is merged elsewhere
    for name, plan, which in cases:
        bad = reduction(name, plan).identities(BAR)
        assert any(b.startswith(which) for b in bad), (name, which, bad)
    with pytest.raises(ref.PlanError):  # a base that is itself a pivot
        reduction("stack3", _mutated("stack3", 37, q=36))


def test_the_sparse_statement_agrees_with_the_dense_one():
    for name in ("combined", "cccs_driver_on_pivot", "ccvs"):
        G, b, K, stamps = oracle_system(name)
        red = reduction(name)
        s = ref.sparse_reduction(G, b, K, FAMILIES[name][1], stamps)
        assert s["bad"] == [] and s["Kr"] == red.Kr
        assert np.all(np.abs(s["Gr"].toarray() - red.Gr) <= BAR * s["gGr"].toarray())
        assert np.all(np.abs(s["br"] - red.br) <= BAR * s["gbr"])
        assert np.all(s["gGr"].toarray() >= 2 * red.gGr.astype(np.float64) * (1 - 1e-12))
        assert np.all((s["gGr"].toarray() == 0) == (red.gGr == 0))


def test_host_compaction_keeps_the_untouched_rows_in_order():
    net, plan = FAMILIES["cccs_driver_on_pivot"]
    table = net.table()
    new, cols = ref.host_compaction(table, plan)
    assert new[7] == -1 and new[6] == 6 and new[8] == 7 and new[34] == 33
    touched = sum(1 for r in net.rows if r[0] == ref.T_R and 7 in (r[2], r[3]))
    assert touched == 4
    assert len(cols["type"]) == table.ncomp - touched - 2  # the E and the CCCS whose driver hangs on the pivot
    assert np.count_nonzero(cols["type"] == ref.T_GM) == 0
    net, plan = FAMILIES["cccs_output_pivot"]
    _, cols = ref.host_compaction(net.table(), plan)
    assert np.count_nonzero(cols["type"] == ref.T_GM) == 0  # (its output lead is the pivot: rewritten, not kept)
