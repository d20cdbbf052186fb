"""A numpy / scipy statement of ONE multigrid cycle (csrc/sagg.hip cycle(), csrc/sagg_multi.h m_cycle()).

It works from the exported hierarchy (Handle.debug_hierarchy(): raw buffers, decoded here with the decoders of
tests/hierarchy_reference.py) and from the parameter words nodal_debug_cycle_apply reports (`params`: sweep counts,
tail, K-cycle switches, which levels fold).  No symmetry is used: R is decoded from the export, never taken as P^T.

The algebra of a visit of level l with right-hand side b (w = the smoother's weight, D = diag A):

    x   = w D^-1 b;  nu - 1 more sweeps  x <- x + w D^-1 (b - A x)
    r   = b - A x;   rc = R r;  coarse start  w D_c^-1 rc
    e   = the coarse correction:
            the next level is the tail or the last level:  e = last_level(rc)
            l < klevels with the K-cycle on:  c1 = visit(rc);  v1 = A_c c1;  t = alpha1 / rho1;  r2 = rc - t v1;
                c2 = visit(r2);  (s1, s2) by k_kcoef's formula and guards;  e = s1 c1 + s2 c2
                (frozen: t, s1, s2 given; no dot products)
            otherwise:  e = visit(rc)
    xp  = x + P e;   nu sweeps on xp
    tail (levels tail ..): the same V-cycle in fp64 with tail_nu sweeps per side, coarse_inv (or dinv) at the bottom

Two modes.  `exact`: every operator from its f64 array, every vector in fp64, the plain algebra above.  `stored`:
operators from the f32 copies the device reads (avalf, pvalf, rvalf, wval, p2val / d2, wtval) outside the tail, and a
cast to float32 wherever the device stores a cyc_t: x0, x1, r, rc and c on the non-last levels, v1, r2, xp, the sweeps'
results, z in modes 1 and 2.  `stored` also takes the device's folded forms where `params` says a level runs them --
the same algebra with other roundings: m0 + W e for the prolongation and the first post-smoothing sweep, rc = W^T b
on a one-sweep level, and rc = P2^T b, out = sweep(x2) + P2 c on the level that visits in three launches.  The dot
products are fp64 sums of the stored values.

Vectors are [n, k] throughout (k = 1, or the block's 16 columns: the block cycle is the same per column, with at most
two sweeps per side and no folded form).

`defect=` plants one mistake a rewrite of a cycle kernel could make (tests/test_cycle_reference.py shows that each
moves the result far beyond what f32 storage does)."""
import numpy as np
import scipy.sparse as sp

from tests.hierarchy_reference import PW, ell, r_blocked

P2CAP = 64

DEFECTS = ("skip_second_presweep", "post_omega_p", "r_last_block", "drop_s2c2", "swap_gamma_beta", "rho2_guard",
           "t_from_frozen0", "w_value", "tail_sweep", "coarse_inv", "block_column")


def _ell_csr(col, val, length, ld, slots, n, ncols):
    c, v = ell(col, ld, slots, n), ell(val, ld, slots, n)
    valid = (np.arange(slots)[:, None] < length[None, :]).T
    rows = np.broadcast_to(np.arange(n), (slots, n)).T[valid]
    return sp.csr_matrix((v.T[valid].astype(np.float64), (rows, c.T[valid].astype(np.int64))), shape=(n, ncols))


def a_of(lv, key):
    n = lv["n"]
    return _ell_csr(lv["acol"], lv[key], lv["alen"][:n], lv["ld"], lv["maxlen"], n, n)


def p_of(lv, key):
    n, ld = lv["n"], lv["ld"]
    col, val = ell(lv["pcol"], ld, PW, n), ell(lv[key], ld, PW, n)
    k, i = np.nonzero(col >= 0)
    return sp.csr_matrix((val[k, i].astype(np.float64), (i, col[k, i].astype(np.int64))), shape=(n, lv["nc"]))


def r_of(lv, key, drop_last_block_of=None):
    """R from the export's blocks of eight (entries below the row's length)."""
    n, nc, rld = lv["n"], lv["nc"], lv["rld"]
    rlen = lv["rlen"][:nc].astype(np.int64).copy()
    if drop_last_block_of is not None:
        I = drop_last_block_of
        rlen[I] = ((rlen[I] - 1) // 8) * 8
    T = int((rlen.max() + 7) & ~7)
    col, val = r_blocked(lv["rcol"], rld, T, nc), r_blocked(lv[key], rld, T, nc)
    valid = (np.arange(T)[:, None] < rlen[None, :]).T
    rows = np.broadcast_to(np.arange(nc), (T, nc)).T[valid]
    return sp.csr_matrix((val.T[valid].astype(np.float64), (rows, col.T[valid].astype(np.int64))), shape=(nc, n))


def w_of(lv):
    n = lv["n"]
    return _ell_csr(lv["wcol"], lv["wval"], lv["wlen"][:n], lv["ld"], lv["wslots"], n, lv["nc"])


def p2_of(lv):
    n = lv["n"]
    return _ell_csr(lv["p2col"], lv["p2val"], lv["p2len"][:n], lv["ld"], P2CAP, n, lv["nc"])


def d2_of(lv):
    return sp.csr_matrix(lv["d2"].reshape(lv["nc"], lv["ld"])[:, :lv["n"]].astype(np.float64))


def wt_of(lv):
    nc = lv["nc"]
    start = lv["wtstart"][:nc + 1].astype(np.int64)
    m = int(start[-1])
    return sp.csr_matrix((lv["wtval"][:m].astype(np.float64), lv["wtcol"][:m].astype(np.int64), start), shape=(nc, lv["n"]))


def _f32(v):
    return v.astype(np.float32).astype(np.float64)


def _ident(v):
    return v


def _dots(a, b):
    return np.einsum("ij,ij->j", a, b)


class CycleReference:
    """mode: 0 general route (f64 z), 1 flexible CG (f32 z, no fold of a one-sweep level 0), 2 block (f32 z, no folds,
    at most two sweeps).  stored: see the module's docstring."""

    def __init__(self, levels, params, mode, stored, defect=None):
        assert defect is None or defect in DEFECTS, defect
        self.lv, self.p, self.mode, self.stored, self.defect = levels, params, mode, stored, defect
        self.nlev, self.tail = params["nlev"], params["tail"]
        assert self.nlev == len(levels) and self.nlev >= 2 and self.tail != 0
        self.c = _f32 if stored else _ident
        self.w = levels[0]["omega"]
        outside = self.tail if self.tail > 0 else self.nlev - 1  # levels [0, outside) run the cycle's launches
        self.A, self.P, self.R, self.D = {}, {}, {}, {}
        for l, lv in enumerate(levels):
            f32 = stored and l < outside
            self.D[l] = lv["dinv"][:lv["n"]][:, None]
            # (the K-cycle's products at the first coarse level read its f32 copy even when that level's own visits
            # belong to the tail: no such hierarchy exists -- a K-cycle level is outside the tail)
            self.A[l] = a_of(lv, "avalf" if f32 else "aval")
            if l + 1 < self.nlev:
                self.P[l] = p_of(lv, "pvalf" if f32 else "pval")
                drop = None
                if defect == "r_last_block" and l == 0:
                    drop = int(np.argmax(lv["rlen"][:lv["nc"]]))
                self.R[l] = r_of(lv, "rvalf" if f32 else "rval", drop)
        single = stored and mode != 2
        bit = lambda name, l: bool(params.get(name, 0) >> l & 1)  # noqa: E731
        self.fold = {l: single and bit("fold_mask", l) for l in range(outside)}
        self.from_b = {l: single and bit("restrict_mask", l) for l in range(outside)}
        self.visit3 = {l: single and bit("visit_mask", l) for l in range(outside)}
        self.W = {l: w_of(levels[l]) for l in range(outside) if self.fold[l]}
        if defect == "w_value":
            l = min(self.W)
            k = int(np.argmax(np.abs(self.W[l].data)))
            self.W[l] = self.W[l].copy()
            self.W[l].data[k] *= 1.02
        self.WT = {l: wt_of(levels[l]) for l in range(outside) if self.from_b[l]}
        self.P2 = {l: p2_of(levels[l]) for l in range(outside) if self.visit3[l]}
        self.D2 = {l: d2_of(levels[l]) for l in range(outside) if self.visit3[l]}
        last = levels[-1]
        self.inv = None
        if last["dense_coarsest"]:
            self.inv = last["coarse_inv"].reshape(last["n"], last["n"]).copy()
            if defect == "coarse_inv":
                k = np.unravel_index(int(np.argmax(np.abs(self.inv))), self.inv.shape)
                self.inv[k] *= 1.0 + 1e-3
        self.coef = None  # the K-cycle's (s1, s2, t) of the last application, [k, 3]

    # ---- sweeps --------------------------------------------------------------------------------------------------
    def nu(self, l):
        n = self.p[("nu0", "nu1", "nu2")[min(l, 2)]]
        return min(n, 2) if self.mode == 2 else n

    def sweep(self, l, b, x, w=None):
        return x + (self.w if w is None else w) * self.D[l] * (b - self.A[l] @ x)

    # ---- the tail and the last level, fp64 -----------------------------------------------------------------------
    def bottom(self, b):
        l = self.nlev - 1
        return self.inv @ b if self.inv is not None else self.D[l] * b

    def tail_cycle(self, l, b):
        if l == self.nlev - 1:
            return self.bottom(b)
        tnu = self.p["tail_nu"]
        x = self.w * self.D[l] * b
        for _ in range(1, tnu):
            x = self.sweep(l, b, x)
        e = self.tail_cycle(l + 1, self.R[l] @ (b - self.A[l] @ x))
        y = x + self.P[l] @ e
        for _ in range(tnu - 1 if self.defect == "tail_sweep" else tnu):
            y = self.sweep(l, b, y)
        return y

    def last_level(self, l, b):
        return self.tail_cycle(l, b) if l == self.tail else self.bottom(b)

    # ---- one visit of a level outside the tail ---------------------------------------------------------------------
    def kcoef(self, rho1, alpha1, gamma, beta, alpha2):
        if self.defect == "swap_gamma_beta":
            gamma, beta = beta, gamma
        with np.errstate(divide="ignore", invalid="ignore"):
            ok1 = rho1 > 0.0
            rho2 = beta - gamma * gamma / rho1
            ok2 = ok1 & (rho2 > 0.0)
            if self.defect == "rho2_guard":
                ok2 = ok1 & ~(rho2 > 0.0)
            s1 = np.where(ok2, alpha1 / rho1 - gamma * alpha2 / (rho1 * rho2), np.where(ok1, alpha1 / rho1, 0.0))
            s2 = np.where(ok2, alpha2 / rho2, 0.0)
        return s1, s2

    def visit(self, l, b, x0, top, frozen):
        """b, x0 as the device holds them (b f64 at the top, stored cyc_t below); returns the level's result, stored
        as the device stores it (f64 at the top of mode 0)."""
        c, w, D = self.c, self.w, self.D[l]
        sb = top and self.mode == 1
        nu = self.nu(l)
        out = _ident if top and self.mode == 0 else c
        last = l + 1 == self.tail or l + 1 == self.nlev - 1
        Dc = self.D[l + 1]
        if (not top and self.visit3[l] and nu == 2 and l + 1 == self.tail and self.p["tail_dense"]):
            x1 = c(self.sweep(l, b, x0))
            x2 = c(self.sweep(l, b, x1))
            e = self.last_level(l + 1, self.D2[l] @ b)
            return c(self.sweep(l, b, x2) + self.P2[l] @ e)
        fold = self.fold[l] and not (sb and nu == 1)
        x = x0
        if nu >= 2 and not (self.defect == "skip_second_presweep" and l == 0):
            x = c(self.sweep(l, b, x))
        if nu >= 3:
            x = c(self.sweep(l, b, x))
        from_b = not top and self.from_b[l] and fold and nu == 1
        r = c(b - self.A[l] @ x)
        rcu = self.WT[l] @ b if from_b else self.R[l] @ r
        if last:
            e = self.last_level(l + 1, rcu)
        else:
            rc = c(rcu)
            x0c = c(w * Dc * (rc if from_b else rcu))
            if l < self.p["klevels"] and self.p["kcycle"]:
                Ac = self.A[l + 1]
                c1 = self.visit(l + 1, rc, x0c, False, None)
                v1 = c(Ac @ c1)
                if frozen is not None and l == 0:
                    s1, s2, t = frozen[:, 0], frozen[:, 1], frozen[:, 2]
                    if self.defect == "t_from_frozen0":
                        t = frozen[:, 0]
                    if self.defect == "block_column":
                        s1, s2 = np.roll(s1, -1), np.roll(s2, -1)
                else:
                    rho1, alpha1 = _dots(c1, v1), _dots(c1, rc)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        t = np.where(rho1 > 0.0, alpha1 / rho1, 0.0)
                r2u = rc - t[None, :] * v1
                r2 = c(r2u)
                c2 = self.visit(l + 1, r2, c(w * Dc * r2u), False, None)
                if not (frozen is not None and l == 0):
                    v2 = c(Ac @ c2)
                    s1, s2 = self.kcoef(rho1, alpha1, _dots(c2, v1), _dots(c2, v2), _dots(c2, r2))
                if l == 0:
                    self.coef = np.stack([s1, s2, t], axis=1)
                e = s1[None, :] * c1 if self.defect == "drop_s2c2" else s1[None, :] * c1 + s2[None, :] * c2
            else:
                e = self.visit(l + 1, rc, x0c, False, None)
        wpost = self.lv[l]["omega_p"] if self.defect == "post_omega_p" and l == 0 else None
        if fold:
            cur = (x + w * D * r) + self.W[l] @ e
            left = nu - 1
        else:
            cur = c(x + self.P[l] @ e)
            left = nu
        if left == 0:
            return out(cur)
        cur = c(cur) if fold else cur
        for s in range(left):
            cur = self.sweep(l, b, cur, wpost)
            cur = out(cur) if s == left - 1 else c(cur)
        return cur

    def apply(self, r, frozen=None):
        """z [n, k] for r [n, k]; frozen [k, 3] or None."""
        r = np.asarray(r, dtype=np.float64)
        assert r.ndim == 2 and r.shape[0] == self.lv[0]["n"]
        if frozen is not None:
            frozen = np.asarray(frozen, dtype=np.float64).reshape(r.shape[1], 3)
        x0 = self.c(self.w * self.D[0] * r)
        return self.visit(0, r, x0, True, frozen)


def reference_pair(levels, params, mode, r, frozen=None):
    """(z_exact, z_stored, E per column): E = max|z_stored - z_exact| / max|z_exact| (0 for a zero column) is what f32
    storage alone does to the answer."""
    ze = CycleReference(levels, params, mode, False).apply(r, frozen)
    zs = CycleReference(levels, params, mode, True).apply(r, frozen)
    scale = np.abs(ze).max(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        E = np.where(scale > 0.0, np.abs(zs - ze).max(axis=0) / scale, 0.0)
    return ze, zs, E


def host_fcg(levels, params, b, tol=1e-13, maxit=200):
    """The flexible CG of sagg_fcg_solve on the host with the `stored` reference cycle (mode 1, adaptive in every
    iteration) as preconditioner: Polak-Ribiere beta from z.r and z.(A p) of the cycle's result, the level-0 matrix
    in f64, stop at the first iteration count k with |r_k|^2 <= tol^2 |b|^2.  Returns (k, x)."""
    A = a_of(levels[0], "aval")
    cyc = CycleReference(levels, params, 1, True)
    b = np.asarray(b, dtype=np.float64)
    x, r, p, Ap = np.zeros_like(b), b.copy(), np.zeros_like(b), np.zeros_like(b)
    bb = rr = float(r @ r)
    alpha, rz_old = 0.0, 1.0
    for it in range(maxit):
        if bb == 0.0 or rr <= tol * tol * bb:
            return it, x
        z = cyc.apply(r[:, None])[:, 0]
        rz, zap = float(z @ r), float(z @ Ap)
        assert rz >= 0.0, rz
        beta = -alpha * zap / rz_old if it > 0 and rz_old != 0.0 else 0.0
        p = z + beta * p
        Ap = A @ p
        pap = float(p @ Ap)
        assert pap > 0.0, pap
        alpha = rz / pap
        x = x + alpha * p
        r = r - alpha * Ap
        rr, rz_old = float(r @ r), rz
    return maxit, x
