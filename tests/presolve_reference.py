"""The presolve (nodal_amd/csrc/presolve.hip) as linear algebra on the original assembled system, for
tests/test_presolve_reference.py (no GPU) and tests/test_gpu_presolve.py.

THE ALGEBRA.  G x = b is the assembled system: K node rows, then B branch rows.  A plan names pivots P with expressions
e_p = e_q + cst + g (e_c - e_d) on SURVIVING nodes q, c, d (-1: ground), and the branches that stay (kept).  Branch
unknowns fall into three classes: C, the CCCS (a unit diagonal in their own row: i = b_C - G_Cn x_n, substituted
outright), Kp, the kept ones, and El, the eliminated voltage-defined ones.

  substitution   x_n = T y + t0     T (K x K'): unit rows for survivors, unit(q) + g (unit(c) - unit(d)) for a pivot,
                                    t0[p] = cst
  supernode rows L (K' x K)         L[new(j), j] = 1 for a survivor, L[new(q), p] = 1 for a pivot with base q (a
                                    ground base drops the row)
  node block     Gt = G_nn - G_nC G_Cn,  bt = b_n - G_nC b_C
  reduced        [ L Gt T    L G_nKp ] [ y    ]   [ L (bt - Gt t0)   ]
                 [ G_Kpn T   0       ] [ i_Kp ] = [ b_Kp - G_Kpn t0  ]
  identities     I1  G_Eln T = 0        I2  G_Eln t0 = b_El       (every eliminated branch row is annihilated)
                 I3  L G_nEl = 0        (the eliminated currents cancel in the merged rows; entries 0, +-1: exact)
  recovery       x_n = T y + t0;  i_C from its own row;  i_Kp = y[K':];  i_El from the pivots' KCL rows,
                 G_nEl[P, .] i_El = b_P - (the rest of row P) -- entries 0, +-1, triangular up to a permutation: solved
                 by peeling rows with one unknown left, so the device's level_of is no input.

A plan is a dict: ok, exprs {p: (q, cst, c, d, g)}, kept [(kk, type, value, a, b, c, d)], level_of [B].  The identities
make a plan taken from the device trustworthy: a wrong expression fails I1 / I2, a wrong base I3, by name.

BOUNDS.  Everything is computed in longdouble (dense) for the named small cases, and a bound goes with every value: the
unit roundoff U = 2^-53 times the number of fp64 operations between the inputs (the entries of G and b as exported, the
plan's constants and gains) and that value, times the sum of the absolute values of the terms.
  - A reduced entry (i, j): the terms are those of |L| |Gt| |T|, with |Gt| = |G_nn| + |G_nC| |G_Cn|.  The device sums
    rewritten stamps: per term a reciprocal, a product with the gain or the constant difference and the difference
    itself (3), and the sum over the terms; an entry of G is itself a sum of at most `stamps` stamps (the largest
    number of components on one node), which the device adds in another order.  ops = 3 terms + stamps + 4.
    A structural zero has bound 0: the device must hold an exact 0 there or nothing.
  - The right-hand side likewise from |L| (|bt| + |Gt| |t0|).
  - A recovered pivot potential: cst + x_q + g (x_c - x_d), 4 operations on |cst| + |x_q| + |g| (|x_c| + |x_d|).
  - A recovered current: the fused chain over its row, (entries + 2) U (|b_row| + |G_row| |x|), plus |G_row| e for the
    bounds e of the recovered values it reads (pivot potentials, currents of the levels below).
  - A residual row at recovered values: (entries + 2) U (|G| |x| + |b|) + |G| e; a surviving node's row adds the rows
    of the pivots merged into it (its own residual is the merged row's minus theirs) and the merged row's bound at y.
The large case runs the same formulas in float64 scipy sparse; its bounds are widened by that arithmetic's own rounding
(one more U per operation counted: the bound is doubled).  The bar over these first-order bounds is the project's 2.
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53
T_R, T_A, T_E, T_VCVS, T_CCVS, T_CCCS, T_GM = range(7)


class PlanError(AssertionError):
    pass


# ---- small networks with hand-written plans ---------------------------------------------------------------------

class Net:
    """An N x N resistor grid (node k = r N + col, the last one is ground; resistances uniform in [0.5, 2)) with a 1 A
    source into node 0, plus whatever the caller adds.  Node numbers are the table's: -1 is ground, node() makes a new
    one (it must become a lead of something)."""

    def __init__(self, N, seed=1):
        rng = np.random.default_rng(seed)
        self.N, self.K, self.B = N, N * N - 1, 0
        self.rows, self.res = [], {}
        for r in range(N):
            for col in range(N):
                k = r * N + col
                if col + 1 < N:
                    self.R(self.g(k), self.g(k + 1), float(rng.uniform(0.5, 2.0)))
                if r + 1 < N:
                    self.R(self.g(k), self.g(k + N), float(rng.uniform(0.5, 2.0)))
        self.A(0, -1, 1.0)

    def g(self, k):
        return -1 if k == self.N * self.N - 1 else k

    def node(self):
        self.K += 1
        return self.K - 1

    def _row(self, t, v, a, b, c=-1, d=-1, drv=-1, branch=False, k=None):
        if branch and k is None:
            k, self.B = self.B, self.B + 1
        self.rows.append((t, float(v), a, b, c, d, drv, k if branch else -1))
        return len(self.rows) - 1

    def R(self, a, b, v):
        row = self._row(T_R, v, a, b)
        self.res[(a, b)] = row
        return row

    def A(self, a, b, v):
        return self._row(T_A, v, a, b)

    def E(self, a, b, v, k=None):
        return self._row(T_E, v, a, b, branch=True, k=k)

    def VCVS(self, a, b, c, d, v):
        return self._row(T_VCVS, v, a, b, c, d, branch=True)

    def _driven(self, t, a, b, drv, v, flip):
        c, d = self.rows[drv][2], self.rows[drv][3]
        if flip:
            c, d = d, c
        return self._row(t, v, a, b, c, d, drv, branch=True)

    def CCVS(self, a, b, drv, v, flip=False):
        return self._driven(T_CCVS, a, b, drv, v, flip)

    def CCCS(self, a, b, drv, v, flip=False):
        return self._driven(T_CCCS, a, b, drv, v, flip)

    def value(self, row):
        return self.rows[row][1]

    def table(self):
        from nodal_amd.lowering import ComponentTable
        t = ComponentTable(len(self.rows), self.K, self.B)
        for i, (ty, v, a, b, c, d, drv, k) in enumerate(self.rows):
            t.type[i], t.value[i], t.a[i], t.b[i], t.c[i], t.d[i], t.drv[i], t.k[i] = ty, v, a, b, c, d, drv, k
        return t


def _plan(exprs, level_of, kept=()):
    full = {p: tuple(e) + (-1, -1, 0.0)[len(e) - 2:] for p, e in exprs.items()}
    return {"ok": True, "exprs": full, "kept": list(kept), "level_of": list(level_of)}


DECLINED = {"ok": False}


def families():
    """name -> (Net, hand-written plan): the pivot, its expression, what stays.  6 x 6 grids: nodes 0 .. 34, new nodes
    from 35.  The constants are written with the operations the plan makes them with."""
    out = {}

    n = Net(6)  # 1: E to ground, either orientation
    n.E(7, -1, 2.5)
    n.E(-1, 12, 1.5)
    out["e_ground"] = (n, _plan({7: (-1, 2.5), 12: (-1, -1.5)}, [1, 1]))

    n = Net(6)  # 2: E between two grid nodes: the lowest-numbered node of a floating tree is its root and survives
    n.E(8, 20, 1.25)
    n.E(30, 3, 0.5)
    out["e_floating"] = (n, _plan({20: (8, -1.25), 30: (3, 0.5)}, [1, 1]))

    n = Net(6)  # 3: a stack of three E on ground: recovery levels 3, 2, 1 from the bottom
    s1, s2, s3 = n.node(), n.node(), n.node()
    n.E(s1, -1, 1.5)
    n.E(s2, s1, 0.75)
    n.E(s3, s2, -2.0)
    n.R(s3, 10, 1.3)
    n.R(s1, 4, 0.9)
    n.R(s2, 22, 1.7)
    out["stack3"] = (n, _plan({s1: (-1, 1.5), s2: (-1, 1.5 + 0.75), s3: (-1, (1.5 + 0.75) + -2.0)}, [3, 2, 1]))

    n = Net(6)  # 4: two E sharing a floating base
    n.E(15, 9, 0.5)
    n.E(9, 22, 1.75)
    out["shared_base"] = (n, _plan({15: (9, 0.5), 22: (9, -1.75)}, [1, 1]))

    n = Net(6)  # 5: E of value 0: no current-source row is emitted
    n.E(7, -1, 0.0)
    n.E(8, 20, 0.0)
    out["e_zero"] = (n, _plan({7: (-1, 0.0), 20: (8, 0.0)}, [1, 1]))

    n = Net(6)  # 6: a resistor parallel to an E, a resistor from a pivot to its base: both leads on one supernode
    n.E(7, -1, 2.5)
    n.R(7, -1, 3.0)
    n.E(8, 20, 1.25)
    n.R(20, 8, 0.7)
    out["parallel_r"] = (n, _plan({7: (-1, 2.5), 20: (8, -1.25)}, [1, 1]))

    n = Net(6)  # 7: a current source with one lead on a pivot, one with both leads in one supernode
    n.E(7, -1, 2.5)
    n.A(7, 12, 0.8)
    n.E(8, 20, 1.25)
    n.A(20, 8, 0.6)
    out["a_on_pivot"] = (n, _plan({7: (-1, 2.5), 20: (8, -1.25)}, [1, 1]))

    n = Net(6)  # 8: a VCVS controlled by surviving nodes
    v = n.node()
    n.VCVS(v, -1, 3, 16, 0.4)
    n.R(v, 10, 1.1)
    n.R(22, v, 0.9)  # (the pivot as the resistor's second lead: the other sign of the control term)
    out["vcvs_surviving"] = (n, _plan({v: (-1, 0.0, 3, 16, 0.4)}, [1]))

    n = Net(6)  # 9: a VCVS controlled by a pivot: the pivot's constant times the gain, its base as the control
    v = n.node()
    n.E(7, -1, 2.5)
    n.VCVS(v, -1, 7, 16, 0.4)
    n.R(v, 10, 1.1)
    out["vcvs_pivot_control"] = (n, _plan({7: (-1, 2.5), v: (-1, 0.0 + 0.4 * (2.5 - 0.0), -1, 16, 0.4)}, [1, 1]))

    n = Net(6)  # 10: a VCVS whose two controls resolve to one base: only the constant is left
    v = n.node()
    n.E(7, -1, 2.5)
    n.E(12, -1, 1.0)
    n.VCVS(v, -1, 7, 12, 0.4)
    n.R(v, 10, 1.1)
    out["vcvs_one_base"] = (n, _plan({7: (-1, 2.5), 12: (-1, 1.0), v: (-1, 0.0 + 0.4 * (2.5 - 1.0))}, [1, 1, 1]))

    n = Net(6)  # 11: a CCVS: its gain is -value / r_driver
    v = n.node()
    drv = n.res[(20, 21)]
    n.CCVS(v, -1, drv, 0.3)
    n.R(v, 10, 1.1)
    n.R(30, v, 1.4)
    out["ccvs"] = (n, _plan({v: (-1, 0.0, 20, 21, -0.3 / n.value(drv))}, [1]))

    n = Net(6)  # 12: a CCCS whose driver hangs on a pivot
    n.E(7, -1, 2.5)
    n.CCCS(14, -1, n.res[(7, 8)], 0.35)
    out["cccs_driver_on_pivot"] = (n, _plan({7: (-1, 2.5)}, [1, 0]))

    n = Net(6)  # 13: a CCCS whose output lead is a pivot
    n.E(7, -1, 2.5)
    n.CCCS(7, 15, n.res[(20, 21)], 0.35)
    out["cccs_output_pivot"] = (n, _plan({7: (-1, 2.5)}, [1, 0]))

    # 14: the three stubborn kinds (tests/test_gpu_parity.py::_stubborn_sources) next to an E that still goes
    n = Net(6)  # cascade: a stage controlled by the previous stage's output: nested control terms
    y1, y2, y3 = n.node(), n.node(), n.node()
    n.E(7, -1, 2.5)
    n.VCVS(y1, -1, 3, 13, 0.5)
    n.R(y1, 17, 1.0)
    n.VCVS(y2, -1, y1, 20, 0.7)
    n.R(y2, 33, 1.0)
    n.VCVS(y3, -1, y2, y1, -0.4)
    n.R(y3, 31, 2.0)
    out["stubborn_cascade"] = (n, _plan({7: (-1, 2.5)}, [1, -1, -1, -1],
                                        [(1, T_VCVS, 0.5, y1, -1, 3, 13), (2, T_VCVS, 0.7, y2, -1, y1, 20),
                                         (3, T_VCVS, -0.4, y3, -1, y2, y1)]))

    n = Net(6)  # feedback: a source controlled by its own output node
    y1, y2 = n.node(), n.node()
    n.E(7, -1, 2.5)
    n.VCVS(y1, -1, y1, 13, 0.5)
    n.R(y1, 17, 1.0)
    n.VCVS(y2, 9, 11, y2, -2.5)
    n.R(y2, 22, 1.5)
    out["stubborn_feedback"] = (n, _plan({7: (-1, 2.5)}, [1, -1, -1],
                                         [(1, T_VCVS, 0.5, y1, -1, y1, 13), (2, T_VCVS, -2.5, y2, 9, 11, y2)]))

    n = Net(6)  # stacked: two controlled sources in series: the upper node would need two control terms; with its CCVS
    y1, y2, y3 = n.node(), n.node(), n.node()
    drv = n.res[(0, 1)]
    n.E(7, -1, 2.5)
    n.VCVS(y1, -1, 3, 13, 0.5)
    n.VCVS(y2, y1, 5, 12, 0.3)
    n.R(y2, 15, 1.0)
    n.CCVS(y3, y2, drv, 0.4)
    n.R(y3, 28, 1.0)
    out["stubborn_stacked"] = (n, _plan({7: (-1, 2.5)}, [1, -1, -1, -1],
                                        [(1, T_VCVS, 0.5, y1, -1, 3, 13), (2, T_VCVS, 0.3, y2, y1, 5, 12),
                                         (3, T_VCVS, -0.4 / n.value(drv), y3, y2, 0, 1)]))

    n = Net(6)  # 15: a loop of sources
    n.E(7, 8, 1.0)
    n.E(8, 9, 0.5)
    n.E(9, 7, -1.5)
    out["loop"] = (n, DECLINED)

    n = Net(6)  # ... a tree that reaches ground twice
    n.E(7, -1, 1.0)
    n.E(8, 7, 0.5)
    n.E(8, -1, 1.5)
    out["ground_twice"] = (n, DECLINED)

    n = Net(6)  # ... a duplicated branch number
    n.E(7, -1, 2.5)
    n.E(12, -1, 1.0, k=0)
    out["duplicated_branch"] = (n, DECLINED)

    n = Net(6)  # 16: a VCVS with c == d behaves as an E of value 0
    v = n.node()
    n.VCVS(v, -1, 5, 5, 0.4)
    n.R(v, 10, 1.1)
    out["vcvs_c_eq_d"] = (n, _plan({v: (-1, 0.0)}, [1]))

    n = Net(8, seed=3)  # the three together on an 8 x 8 grid, the VCVS controlled by a stacked node
    s1, s2, s3, v = n.node(), n.node(), n.node(), n.node()
    n.E(s1, -1, 1.5)
    n.E(s2, s1, 0.75)
    n.E(s3, s2, -2.0)
    n.R(s3, 10, 1.3)
    n.R(s2, 41, 0.8)
    n.E(15, 9, 0.5)
    n.E(9, 22, 1.75)
    n.VCVS(v, -1, s2, 30, 0.4)
    n.R(v, 50, 1.1)
    n.R(3, v, 0.6)
    out["combined"] = (n, _plan({s1: (-1, 1.5), s2: (-1, 1.5 + 0.75), s3: (-1, (1.5 + 0.75) + -2.0), 15: (9, 0.5),
                                 22: (9, -1.75), v: (-1, 0.0 + 0.4 * ((1.5 + 0.75) - 0.0), -1, 30, 0.4)},
                                [3, 2, 1, 1, 1, 1]))
    return out


def plan_from_export(out):
    """The plan dict of what Handle.debug_presolve_build returned."""
    if not out["ok"]:
        return {"ok": False}
    exprs = {int(p): (int(q), float(cst), int(c), int(d), float(g))
             for p, q, cst, c, d, g in zip(out["expr_p"], out["expr_q"], out["expr_cst"], out["expr_c"], out["expr_d"],
                                           out["expr_g"])}
    kept = [(int(kk), int(t), float(v), int(a), int(b), int(c), int(d))
            for kk, t, v, a, b, c, d in zip(out["kept_kk"], out["kept_type"], out["kept_value"], out["kept_a"],
                                            out["kept_b"], out["kept_c"], out["kept_d"])]
    return {"ok": True, "exprs": exprs, "kept": kept, "level_of": [int(v) for v in out["level_of"]]}


def stamps_per_node(table):
    """The largest number of components on one node: what an entry of G sums at the most."""
    leads = np.concatenate([np.asarray(table.a), np.asarray(table.b)])
    leads = leads[leads >= 0]
    return int(np.bincount(leads).max()) if len(leads) else 1


# ---- the algebra, dense longdouble ------------------------------------------------------------------------------

class Reduction:
    """Everything the docstring names for one (G, b, K, plan): T, t0, L, newidx, the branch classes, the reduced system
    Gr, br with its bounds gGr, gbr (first-order, without the bar), and the identities' residuals with theirs."""

    def __init__(self, G, b, K, plan, stamps=8):
        G = np.asarray(G.toarray() if sp.issparse(G) else G, dtype=LD)
        b = np.asarray(b, dtype=LD)
        n = len(b)
        B = n - K
        self.G, self.b, self.K, self.B, self.n, self.plan = G, b, K, B, n, plan
        exprs = plan["exprs"]
        self.pivots = np.array(sorted(exprs), dtype=np.int64)
        new = np.full(K, -1, dtype=np.int64)
        surv = np.setdiff1d(np.arange(K), self.pivots)
        new[surv] = np.arange(len(surv))
        self.newidx, self.Kr = new, len(surv)
        Kr = self.Kr
        T, t0, L = np.zeros((K, Kr), dtype=LD), np.zeros(K, dtype=LD), np.zeros((Kr, K), dtype=LD)
        T[surv, new[surv]] = 1
        L[new[surv], surv] = 1

        def col(node, what, p):
            if node >= K or new[node] < 0:
                raise PlanError(f"pivot {p}: its {what} {node} is no surviving node")
            return new[node]
        for p, (q, cst, c, d, g) in exprs.items():
            t0[p] = cst
            if q >= 0:
                T[p, col(q, "base", p)] += 1
                L[new[q], p] = 1
            if g != 0.0:
                if c >= 0:
                    T[p, col(c, "control", p)] += LD(g)
                if d >= 0:
                    T[p, col(d, "control", p)] -= LD(g)
        self.T, self.t0, self.L = T, t0, L
        Gnn, Gnb, Gbn, Gbb = G[:K, :K], G[:K, K:], G[K:, :K], G[K:, K:]
        bn, bb = b[:K], b[K:]
        diag = np.diag(Gbb) if B else np.zeros(0)
        assert np.array_equal(Gbb, np.diag(diag)), "the branch block is a diagonal"
        self.kept = np.array([k[0] for k in plan["kept"]], dtype=np.int64)
        self.cccs = np.flatnonzero(diag != 0)
        assert np.all(diag[self.cccs] == 1)
        self.elim = np.setdiff1d(np.arange(B), np.union1d(self.kept, self.cccs))
        if len(self.elim) != len(self.pivots):
            raise PlanError(f"{len(self.pivots)} pivots for {len(self.elim)} eliminated branches")
        C, Kp, El = self.cccs, self.kept, self.elim
        Gt = Gnn - Gnb[:, C] @ Gbn[C, :]
        aGt = np.abs(Gnn) + np.abs(Gnb[:, C]) @ np.abs(Gbn[C, :])
        cGt = (Gnn != 0).astype(LD) + (Gnb[:, C] != 0).astype(LD) @ (Gbn[C, :] != 0).astype(LD)
        bt = bn - Gnb[:, C] @ bb[C]
        abt = np.abs(bn) + np.abs(Gnb[:, C]) @ np.abs(bb[C])
        aL, aT, nzL, nzT = np.abs(L), np.abs(T), (L != 0).astype(LD), (T != 0).astype(LD)
        nr = Kr + len(Kp)
        self.Gr, self.gGr = np.zeros((nr, nr), dtype=LD), np.zeros((nr, nr), dtype=LD)
        self.br, self.gbr = np.zeros(nr, dtype=LD), np.zeros(nr, dtype=LD)
        ops = lambda terms: 3 * terms + stamps + 4  # noqa: E731
        self.Gr[:Kr, :Kr] = L @ Gt @ T
        self.gGr[:Kr, :Kr] = U * ops(nzL @ cGt @ nzT) * (aL @ aGt @ aT)
        self.Gr[:Kr, Kr:] = L @ Gnb[:, Kp]
        self.Gr[Kr:, :Kr] = Gbn[Kp, :] @ T
        self.gGr[Kr:, :Kr] = U * ops((Gbn[Kp, :] != 0).astype(LD) @ nzT) * (np.abs(Gbn[Kp, :]) @ aT)
        # (L G_nKp: +-1 entries, exact; a row that merges both leads of a kept branch cannot occur: they survive)
        self.br[:Kr] = L @ (bt - Gt @ t0)
        self.gbr[:Kr] = U * ops(nzL @ (cGt @ (t0 != 0).astype(LD) + (abt != 0))) * (aL @ (abt + aGt @ np.abs(t0)))
        self.br[Kr:] = bb[Kp] - Gbn[Kp, :] @ t0
        self.gbr[Kr:] = U * ops((Gbn[Kp, :] != 0).astype(LD) @ (t0 != 0).astype(LD) + 1) * \
            (np.abs(bb[Kp]) + np.abs(Gbn[Kp, :]) @ np.abs(t0))
        self.agr_rows = aL @ aGt @ aT  # |L| |Gt| |T|: the merged rows' absolute sums, for residual bounds
        self.abr_rows = aL @ (abt + aGt @ np.abs(t0))
        # identities: the plan's constants and gains come from a few fp64 operations per level of its source trees
        depth = 3 * (max([v for v in plan["level_of"]] + [1])) + 3
        self.I1 = Gbn[El, :] @ T
        self.gI1 = U * depth * (np.abs(Gbn[El, :]) @ aT)
        self.I2 = Gbn[El, :] @ t0 - bb[El]
        self.gI2 = U * depth * (np.abs(Gbn[El, :]) @ np.abs(t0) + np.abs(bb[El]))
        self.I3 = L @ Gnb[:, El]

    def identities(self, bar=2.0):
        """The names of the identities that fail."""
        bad = []
        if np.any(np.abs(self.I1) > bar * self.gI1):
            bad.append("I1: G_bn T = 0")
        if np.any(np.abs(self.I2) > bar * self.gI2):
            bad.append("I2: G_bn t0 = b_b")
        if np.any(self.I3 != 0):
            bad.append("I3: L G_nb = 0")
        return bad

    # ---- recovery ----
    def recover(self, y):
        """(x [n] in longdouble, e [n]: the first-order bound of each recovered value as the device computes it from the
        same y)."""
        G, b, K, Kr = self.G, self.b, self.K, self.Kr
        y = np.asarray(y, dtype=LD)
        x, e = np.full(self.n, np.nan, dtype=LD), np.zeros(self.n, dtype=LD)
        x[:K] = self.T @ y[:Kr] + self.t0
        piv = self.pivots
        e[piv] = U * 4 * (np.abs(self.T[piv]) @ np.abs(y[:Kr]) + np.abs(self.t0[piv]))
        x[K + self.kept] = y[Kr:]
        aG = np.abs(G)

        def solve_row(row, col):
            rest = np.arange(self.n) != col
            assert not np.isnan(x[rest][G[row, rest] != 0]).any()
            known = np.where(G[row] != 0, x, 0)
            s = b[row] - G[row, rest] @ known[rest]
            x[col] = s / G[row, col]
            entries = np.count_nonzero(G[row])
            asum = np.abs(b[row]) + aG[row, rest] @ np.abs(known[rest])
            e[col] = (U * (entries + 2) * asum + aG[row, rest] @ e[rest]) / np.abs(G[row, col])
        for k in self.cccs:
            solve_row(K + k, K + k)
        left = set(int(k) for k in self.elim)
        rows = [int(p) for p in piv]
        while left:  # peel: a pivot's KCL row with exactly one unknown current left
            progress = False
            for p in list(rows):
                unknown = [k for k in left if G[p, K + k] != 0]
                if len(unknown) == 1:
                    solve_row(p, K + unknown[0])
                    left.discard(unknown[0])
                    rows.remove(p)
                    progress = True
            if not progress:
                raise PlanError("the pivots' KCL rows do not determine the eliminated currents")
        return x, e

    def residual_bounds(self, x, e, y, solved):
        """First-order bound of every row of G x - b at the values x recovered from y, with their bounds e.  solved
        (y solves the reduced system): all rows -- a surviving node's row is the merged row's residual minus the rows
        merged into it, so it gets the merged row's bound at y plus theirs.  Otherwise only the rows that hold
        whatever y is -- eliminated branch rows, the pivots' KCL rows, CCCS rows -- and inf elsewhere."""
        G, b, K, Kr = self.G, self.b, self.K, self.Kr
        x = np.asarray(x, dtype=LD)
        ay = np.abs(np.asarray(y, dtype=LD))
        aG = np.abs(G)
        entries = np.count_nonzero(G, axis=1)
        own = U * (entries + 2) * (aG @ np.abs(x) + np.abs(b)) + aG @ e
        # an eliminated branch row through the substitution: a cancellation inside a pivot's potential is covered
        El = self.elim
        through = np.abs(self.T) @ ay[:Kr] + np.abs(self.t0)
        own[K + El] = U * (entries[K + El] + 6) * (aG[K + El, :K] @ through + np.abs(b[K + El])) + aG[K + El, :K] @ e[:K]
        out = own.copy()
        surv = np.flatnonzero(self.newidx >= 0)
        if solved:
            merged = U * (np.count_nonzero(self.Gr[:Kr], axis=1) + 2) * \
                (self.agr_rows @ ay[:Kr] + np.abs(self.Gr[:Kr, Kr:]) @ ay[Kr:] + self.abr_rows)
            out[surv] = (merged + np.abs(self.L) @ own[:K])[self.newidx[surv]]
        else:
            out[surv] = np.inf
            out[K + self.kept] = np.inf
        return out

    def solve_reduced(self):
        """y*: the reduced system solved in float64 and refined in longdouble."""
        A = self.Gr.astype(np.float64)
        y = np.linalg.solve(A, self.br.astype(np.float64)).astype(LD)
        for _ in range(3):
            y = y + np.linalg.solve(A, (self.br - self.Gr @ y).astype(np.float64)).astype(LD)
        return y


def full_solve(G, b):
    """The original system in float64, refined in longdouble."""
    Gd = np.asarray(G.toarray() if sp.issparse(G) else G, dtype=LD)
    bd = np.asarray(b, dtype=LD)
    A = Gd.astype(np.float64)
    x = np.linalg.solve(A, bd.astype(np.float64)).astype(LD)
    for _ in range(3):
        x = x + np.linalg.solve(A, (bd - Gd @ x).astype(np.float64)).astype(LD)
    return x


def host_compaction(table, plan, values=None):
    """newidx and the kept rows of the reduced table as the device must compact them: original order, nodes
    renumbered, a CCCS as a GM of value / r_driver.  Returns (newidx, dict of columns as arrays)."""
    K = table.K
    value = np.asarray(table.value if values is None else values, dtype=np.float64)
    new = np.full(K + 1, -1, dtype=np.int32)  # (the last entry answers for ground: index -1)
    surv = np.setdiff1d(np.arange(K), np.array(sorted(plan["exprs"]), dtype=np.int64))
    new[surv] = np.arange(len(surv), dtype=np.int32)
    ty = np.asarray(table.type).astype(np.int64)
    a, b, c, d, drv = (np.asarray(getattr(table, x)).astype(np.int64) for x in ("a", "b", "c", "d", "drv"))
    gone = lambda node: (node >= 0) & (new[node] < 0)  # noqa: E731
    ctl = (ty == T_CCCS) | (ty == T_GM)
    keep = ((ty == T_R) | (ty == T_A) | ctl) & ~gone(a) & ~gone(b) & ~(ctl & (gone(c) | gone(d)))
    v = np.where(ty == T_CCCS, value / value[np.maximum(drv, 0)], value)
    cols = {"type": np.where(ctl, T_GM, ty)[keep].astype(np.uint8), "value": v[keep],
            "a": new[a[keep]], "b": new[b[keep]], "c": np.where(ctl, new[c], -1)[keep].astype(np.int32),
            "d": np.where(ctl, new[d], -1)[keep].astype(np.int32), "k": np.full(int(keep.sum()), -1, dtype=np.int32)}
    return new[:K], cols


# ---- the same in float64 scipy sparse, for the large case -------------------------------------------------------

def sparse_reduction(G, b, K, plan, stamps=8):
    """For a plan without kept branches: (Gr, gGr, br, gbr, T, t0, identities' names that fail) in float64 CSR; the
    bounds are doubled for this arithmetic's own rounding."""
    G = sp.csr_matrix(G)
    n = G.shape[0]
    assert not plan["kept"]
    piv = np.array(sorted(plan["exprs"]), dtype=np.int64)
    ex = np.array([plan["exprs"][int(p)] for p in piv], dtype=np.float64).reshape(len(piv), 5)
    q, cst, c, d, g = ex[:, 0].astype(np.int64), ex[:, 1], ex[:, 2].astype(np.int64), ex[:, 3].astype(np.int64), ex[:, 4]
    new = np.full(K, -1, dtype=np.int64)
    surv = np.setdiff1d(np.arange(K), piv)
    new[surv] = np.arange(len(surv))
    Kr = len(surv)
    for nodes, what in ((q, "base"), (c[g != 0], "control"), (d[g != 0], "control")):
        nodes = nodes[nodes >= 0]
        if np.any(new[nodes] < 0):
            raise PlanError(f"a {what} is no surviving node")
    rows, cols, vals = [surv], [new[surv]], [np.ones(Kr)]
    for nodes, coef in ((q, np.ones(len(piv))), (c, np.where(g != 0, g, 0.0)), (d, np.where(g != 0, -g, 0.0))):
        m = (nodes >= 0) & (coef != 0)
        rows.append(piv[m]); cols.append(new[nodes[m]]); vals.append(coef[m])
    T = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(K, Kr))
    m = q >= 0
    L = sp.csr_matrix((np.ones(Kr + int(m.sum())), (np.concatenate([new[surv], new[q[m]]]), np.concatenate([surv, piv[m]]))),
                      shape=(Kr, K))
    t0 = np.zeros(K)
    t0[piv] = cst
    Gnn, Gnb, Gbn, Gbb = G[:K, :K], G[:K, K:], G[K:, :K], G[K:, K:]
    diag = Gbb.diagonal()
    assert (Gbb - sp.diags(diag)).count_nonzero() == 0
    C = np.flatnonzero(diag != 0)
    El = np.setdiff1d(np.arange(n - K), C)
    if len(El) != len(piv):
        raise PlanError(f"{len(piv)} pivots for {len(El)} eliminated branches")
    bn, bb = b[:K], b[K:]
    pat = lambda M: (sp.csr_matrix(M) != 0).astype(np.float64)  # noqa: E731
    Gt = (Gnn - Gnb[:, C] @ Gbn[C, :]).tocsr()
    aGt = (abs(Gnn) + abs(Gnb[:, C]) @ abs(Gbn[C, :])).tocsr()
    cGt = (pat(Gnn) + pat(Gnb[:, C]) @ pat(Gbn[C, :])).tocsr()
    bt = bn - Gnb[:, C] @ bb[C]
    abt = np.abs(bn) + abs(Gnb[:, C]) @ np.abs(bb[C])
    Gr = (L @ Gt @ T).tocsr()
    terms = (pat(L) @ cGt @ pat(T)).tocsr()
    asum = (abs(L) @ aGt @ abs(T)).tocsr()
    gGr = asum.copy()
    assert np.array_equal(terms.indptr, asum.indptr) and np.array_equal(terms.indices, asum.indices)
    gGr.data = 2 * U * (3 * terms.data + stamps + 4) * asum.data
    br = L @ (bt - Gt @ t0)
    gbr = 2 * U * (3 * (pat(L) @ (cGt @ (t0 != 0).astype(np.float64) + (abt != 0))) + stamps + 4) * \
        (abs(L) @ (abt + aGt @ np.abs(t0)))
    bad = []
    depth = 2 * (3 * max(plan["level_of"] + [1]) + 3)
    r1 = abs((Gbn[El, :] @ T).tocsr()) - 2 * U * depth * (abs(Gbn[El, :]) @ abs(T)).tocsr()
    if r1.nnz and r1.max() > 0:
        bad.append("I1: G_bn T = 0")
    if np.any(np.abs(Gbn[El, :] @ t0 - bb[El]) > 2 * U * depth * (abs(Gbn[El, :]) @ np.abs(t0) + np.abs(bb[El]))):
        bad.append("I2: G_bn t0 = b_b")
    if np.any((L @ Gnb[:, El]).tocsr().data != 0):
        bad.append("I3: L G_nb = 0")
    return {"Gr": Gr, "gGr": gGr, "br": br, "gbr": gbr, "T": T, "t0": t0, "L": L, "newidx": new, "Kr": Kr, "bad": bad,
            "elim": El, "cccs": C, "pivots": piv}
