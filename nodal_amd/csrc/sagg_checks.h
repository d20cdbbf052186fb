// The self-checks of the multigrid setup: a folded or precomputed form of the cycle against the launches it replaces, on
// fixed vectors, one "[sagg] ... check:" line each.  They run under NODAL_TRACE with NODAL_SA_{TAIL,FOLD,VISIT,RESTRICT}_CHECK
// and are what the tests of those forms read.  (Fourth part of sagg.hip; included there behind cycle(), same translation unit.)
#pragma once

namespace {

// uniform in (-1, 1) by splitmix64; every check draws its fixed vectors from a stream of its own
struct CheckRng {
    uint64_t seed;
    double unit() {
        uint64_t z = (seed += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        return (double)(z >> 11) * (1.0 / 4503599627370496.0) - 1.0;
    }
};
// the running maximum m with q: a NaN q stays
inline double nan_max(double q, double m) { return !(q <= m) ? q : m; }
// dst = the dst.size() elements at the device address src, unless e already holds an error
template <typename T>
void fetch(hipError_t &e, std::vector<T> &dst, const void *src) {
    if (e == hipSuccess) e = hipMemcpy(dst.data(), src, dst.size() * sizeof(T), hipMemcpyDeviceToHost);
}

// NODAL_SA_FOLD_CHECK (fold_check_level below): per row the difference of the two forms over the sum of the
// magnitudes that enter either of them, d[i], and the same over the row's own bound (slots + width + 8) 2^-23, q[i]
template <typename TC>
__global__ __launch_bounds__(TB) void k_fold_check(Ell A, const double *__restrict__ dinv, const cyc_t *__restrict__ b,
                                                   const cyc_t *__restrict__ x, const cyc_t *__restrict__ xp,
                                                   const int32_t *__restrict__ wcol, const float *__restrict__ wval,
                                                   const int32_t *__restrict__ wlen, const TC *__restrict__ c1,
                                                   const TC *__restrict__ c2, const double *__restrict__ coef,
                                                   const cyc_t *__restrict__ m_two, const cyc_t *__restrict__ m_fused,
                                                   double *__restrict__ d, double *__restrict__ q) {
    const bool two = coef != nullptr;
    const double s1 = two ? coef[0] : 1.0, s2 = two ? coef[1] : 0.0;
    for (int64_t i = (int64_t)xcd_block() * TB + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * TB) {
        double ax = 0.0, we = 0.0;
        const int32_t la = A.len[i], lw = wlen[i];
        for (int32_t s = 0; s < la; ++s)
            ax += fabs((double)A.valf[(int64_t)s * A.ld + i]) * fabs((double)xp[A.col[(int64_t)s * A.ld + i]]);
        for (int32_t s = 0; s < lw; ++s) {
            const int32_t j = wcol[(int64_t)s * A.ld + i];
            const double e = two ? s1 * (double)c1[j] + s2 * (double)c2[j] : (double)c1[j];
            we += fabs((double)wval[(int64_t)s * A.ld + i]) * fabs(e);
        }
        const double den = fabs((double)x[i]) + OMEGA * dinv[i] * (fabs((double)b[i]) + ax) + we;
        const double diff = fabs((double)m_fused[i] - (double)m_two[i]);
        const double di = diff / den;  // (0 / 0: a NaN, which the host's maximum keeps)
        d[i] = di;
        q[i] = di / ((double)(lw + la + 8) * 0x1p-23);
    }
}

// NODAL_TRACE with NODAL_SA_TAIL_CHECK=1: both forms of the tail applied to one fixed vector of both signs,
// d = max_i |y_dense - y_cycle|_i / sum_j |T_ij| |b_j|; the dense product alone against the same product in long double
int tail_self_check(nodal_ctx *h, SHierarchy *H) {
    const int n = H->td.lv[0].n;
    std::vector<double> b((size_t)n), yc((size_t)n), yd((size_t)n), T((size_t)n * n);
    CheckRng rng{0x9e3779b97f4a7c15ull};
    for (auto &x : b) x = rng.unit();
    DevBuf v;
    hipError_t e = v.reserve((size_t)3 * n * 8);
    double *db = v.as<double>(), *dc = db + n, *dd = dc + n;
    int rc = NODAL_OK;
    if (e == hipSuccess) e = hipMemcpyAsync(db, b.data(), (size_t)n * 8, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) rc = tail_walk(h, H, db, dc, 1);
    if (e == hipSuccess && rc == NODAL_OK) rc = tail_apply<1>(h, H, db, dd);
    if (e == hipSuccess && rc == NODAL_OK) e = hipStreamSynchronize(h->stream);
    fetch(e, yc, dc);
    fetch(e, yd, dd);
    fetch(e, T, H->tail_op.p);
    v.release();
    if (rc != NODAL_OK) return rc;
    NODAL_HIP_TRY(h, e);
    double d = 0.0, dp = 0.0;
    for (int i = 0; i < n; ++i) {
        long double y = 0.0L, a = 0.0L;
        for (int j = 0; j < n; ++j) {
            y += (long double)T[(size_t)i * n + j] * b[j];
            a += fabsl((long double)T[(size_t)i * n + j] * b[j]);
        }
        const double den = (double)a;
        const double q = fabs(yd[i] - yc[i]) / den, qp = (double)(fabsl((long double)yd[i] - y) / a);
        d = nan_max(q, d);
        dp = nan_max(qp, dp);
    }
    fprintf(stderr, "[sagg] tail check: n_t %d, dense operator against the cycle d = %.3e (product alone %.3e)\n", n, d, dp);
    return NODAL_OK;
}

// NODAL_TRACE with NODAL_SA_FOLD_CHECK=1: per folded level both forms of the end of a visit -- k_prolong + k_post
// against k_prolong_post -- on fixed vectors of both signs (x, b and the coarse correction uniform in (-1, 1), the
// residual by k_smooth_residual as in the cycle).  Prints the level, its rows and
//   d = max_i |m_fused - m_two|_i / (|x_i| + w dinv_i (|b_i| + sum_j |a_ij| |xp_j|) + sum_s |w_is| |e|),
// and q = the largest d_i over the row's own bound (slots + width + 8) 2^-23 (operands stored f32, sums in f64).
template <typename TC>
int fold_check_level(nodal_ctx *h, SHierarchy *H, int l, bool two) {
    hipStream_t st = h->stream;
    const SLevel *L = H->pool[l];
    const int64_t n = L->n, nc = H->pool[l + 1]->n;
    const Ell A = L->A();
    CheckRng rng{0x9e3779b97f4a7c15ull + (uint64_t)l};
    std::vector<cyc_t> hx((size_t)n), hb((size_t)n);
    std::vector<TC> he((size_t)2 * nc);
    for (auto &v : hx) v = (cyc_t)rng.unit();
    for (auto &v : hb) v = (cyc_t)rng.unit();
    for (auto &v : he) v = (TC)rng.unit();
    const double hcoef[2] = {0.9, 0.4};
    const size_t vb = align256((size_t)n * sizeof(cyc_t)), eb = align256((size_t)nc * sizeof(TC)), db = align256((size_t)n * 8);
    DevBuf buf;
    hipError_t e = buf.reserve(6 * vb + 2 * eb + 2 * db + 256);
    char *p = buf.as<char>();
    cyc_t *x = reinterpret_cast<cyc_t *>(p), *b = reinterpret_cast<cyc_t *>(p + vb), *r = reinterpret_cast<cyc_t *>(p + 2 * vb),
          *xp = reinterpret_cast<cyc_t *>(p + 3 * vb), *mt = reinterpret_cast<cyc_t *>(p + 4 * vb),
          *mf = reinterpret_cast<cyc_t *>(p + 5 * vb);
    TC *c1 = reinterpret_cast<TC *>(p + 6 * vb), *c2 = reinterpret_cast<TC *>(p + 6 * vb + eb);
    double *d = reinterpret_cast<double *>(p + 6 * vb + 2 * eb), *q = reinterpret_cast<double *>(p + 6 * vb + 2 * eb + db);
    double *coef = reinterpret_cast<double *>(p + 6 * vb + 2 * eb + 2 * db);
    std::vector<double> hd((size_t)n), hq((size_t)n);
    if (e == hipSuccess) e = hipMemcpyAsync(x, hx.data(), (size_t)n * sizeof(cyc_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b, hb.data(), (size_t)n * sizeof(cyc_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(c1, he.data(), (size_t)nc * sizeof(TC), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(c2, he.data() + nc, (size_t)nc * sizeof(TC), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(coef, hcoef, sizeof hcoef, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const unsigned g = grid_for(n), tb = L->wfix ? TB : TB * LPR_RAGGED;
        const double *dinv = L->dinv.as<double>(), *cf = two ? coef : nullptr;
        const int32_t *wcol = L->wcol.as<int32_t>(), *wlen = L->wlen.as<int32_t>();
        const float *wval = L->wval.as<float>();
        SAGG_DISPATCH_W(L->wfix, (k_smooth_residual<W, cyc_t><<<g, tb, 0, st>>>(A, b, x, r)));
        k_prolong<TC><<<g, TB, 0, st>>>(n, L->ld, L->pcol.as<int32_t>(), L->pvalf.as<float>(), x, c1, two ? c2 : nullptr, cf, xp);
        SAGG_DISPATCH_W(L->wfix, (k_post<W, false, cyc_t, cyc_t><<<g, tb, 0, st>>>(A, dinv, b, xp, mt, nullptr, nullptr, nullptr)));
        k_prolong_post<TC, cyc_t><<<g, TB, 0, st>>>(n, L->ld, wcol, wval, wlen, x, r, dinv, c1, two ? c2 : nullptr, cf, mf);
        k_fold_check<TC><<<g, TB, 0, st>>>(A, dinv, b, x, xp, wcol, wval, wlen, c1, two ? c2 : nullptr, cf, mt, mf, d, q);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    fetch(e, hd, d);
    fetch(e, hq, q);
    buf.release();
    NODAL_HIP_TRY(h, e);
    double dm = 0.0, qm = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        dm = nan_max(hd[i], dm);
        qm = nan_max(hq[i], qm);
    }
    fprintf(stderr, "[sagg] fold check: level %d, rows %lld, slots %d, width %d, fused launch against the two d = %.3e "
                    "(worst row against its own bound: %.3e)\n", l, (long long)n, (int)L->wslots, (int)L->maxlen, dm, qm);
    return NODAL_OK;
}
int fold_self_check(nodal_ctx *h, SHierarchy *H) {
    static const bool check = knob::TRACE.now() && knob::SA_FOLD_CHECK.now();
    if (!check) return NODAL_OK;
    for (int l = 0; l + 1 < H->nlev; ++l) {
        if (!H->pool[l]->fold) continue;
        const bool last = l + 1 == H->tail || l + 1 == H->nlev - 1;  // (as cycle() tells the two hand-overs apart)
        if (last) NODAL_TRY(fold_check_level<double>(h, H, l, false));
        else NODAL_TRY(fold_check_level<cyc_t>(h, H, l, true));
    }
    return NODAL_OK;
}

// NODAL_TRACE with NODAL_SA_VISIT_CHECK=1: the level that visits in three launches runs both forms of the visit on one
// fixed right-hand side of both signs (b uniform in (-1, 1), x0 = w D^-1 b as its producer leaves it) and prints
//   d = max_i |out_3 - out_6|_i / den_i,
// den_i = the row-wise sum of the absolute terms that carry one f32 rounding each, formed on the host in fp64 from the
// exported operators.  With e = 2^-24, |.| entrywise, |G| v = v + w D^-1 |A| v, and the exact operators (A, P in f64,
// W = G P, P2 = G W) as the reference, the two forms leave it by (first order)
//   six launches:  e_r = |r| + |A||x1|            (r rounded; the sweep reads the f32 copy of A)
//                  e_c = |T| |P|^T (|r| + e_r)     (R = the f32 copy of P^T; T and its product are fp64)
//                  e_xp = |xp| + w D^-1 e_r + |W||c| + |W| e_c
//                  dev_6 = |out| + |G| e_xp + w D^-1 |A||xp|
//   three:         e_x2 = |x2| + w D^-1 |A||x1|
//                  E v = |P2| v + |G||W| v         (an entry of the stored P2: its own rounding and that of the W under it)
//                  e_c' = |T| E^T |b|              (d2 holds P2's entries)
//                  dev_3 = |out| + |G| e_x2 + w D^-1 |A||x2| + E |c| + |P2| e_c'
// times e each (x1 is the same launch on the same operands in both forms: the same bits), so den = dev_6 + dev_3 and
// d <= 2^-24 up to second-order terms and the fp64 sums (each over fewer than n + n_t terms, 2^-53 apiece: below 2^-36
// of their absolute terms at 1e5 rows).  The per-row bound is therefore 2 x 2^-24 = 2^-23 whatever the slot counts: the
// slots enter through den, every sum is fp64 and no rounding is per slot.  q = the largest d_i over 2^-23.
int visit_check_level(nodal_ctx *h, SHierarchy *H, int l) {
    hipStream_t st = h->stream;
    SLevel *L = H->pool[l], *C = H->pool[l + 1];
    const int64_t n = L->n, ld = L->ld, nt = C->n;
    CheckRng rng{0x9e3779b97f4a7c15ull + 977ull * (uint64_t)l};
    std::vector<double> dinv((size_t)n), T((size_t)nt * nt), c6((size_t)nt), c3((size_t)nt);
    std::vector<cyc_t> hb((size_t)n), hx0((size_t)n), x1((size_t)n), x2((size_t)n), r((size_t)n), xp((size_t)n),
        o6((size_t)n), o3((size_t)n);
    std::vector<int32_t> acol((size_t)L->width * ld), alen((size_t)n), pcol((size_t)PW * ld), wcol((size_t)L->wslots * ld),
        wlen((size_t)n), p2col((size_t)P2CAP * ld), p2len((size_t)n);
    std::vector<float> aval((size_t)L->width * ld), pval((size_t)PW * ld), wval((size_t)L->wslots * ld),
        p2val((size_t)P2CAP * ld);
    hipError_t e = hipStreamSynchronize(st);
    fetch(e, dinv, L->dinv.p);
    for (int64_t i = 0; i < n; ++i) {
        hb[i] = (cyc_t)rng.unit();
        hx0[i] = (cyc_t)(OMEGA * dinv[i] * (double)hb[i]);
    }
    const size_t vb = align256((size_t)n * sizeof(cyc_t));
    DevBuf buf;
    if (e == hipSuccess) e = buf.reserve(4 * vb);
    char *p = buf.as<char>();
    cyc_t *b = reinterpret_cast<cyc_t *>(p), *x0 = reinterpret_cast<cyc_t *>(p + vb), *out6 = reinterpret_cast<cyc_t *>(p + 2 * vb),
          *out3 = reinterpret_cast<cyc_t *>(p + 3 * vb);
    if (e == hipSuccess) e = hipMemcpyAsync(b, hb.data(), (size_t)n * sizeof(cyc_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(x0, hx0.data(), (size_t)n * sizeof(cyc_t), hipMemcpyHostToDevice, st);
    int rc = NODAL_OK;
    if (e == hipSuccess) {
        L->visit = false;
        rc = cycle<cyc_t, cyc_t>(h, H, l, b, x0, out6, nullptr);
        L->visit = true;
    }
    if (e == hipSuccess && rc == NODAL_OK) e = hipStreamSynchronize(st);
    fetch(e, r, L->v<cyc_t>(V_R));
    fetch(e, xp, L->v<cyc_t>(V_XP));
    fetch(e, c6, C->v<double>(V_C1));
    if (e == hipSuccess && rc == NODAL_OK) rc = cycle<cyc_t, cyc_t>(h, H, l, b, x0, out3, nullptr);
    if (e == hipSuccess && rc == NODAL_OK) e = hipStreamSynchronize(st);
    fetch(e, x1, L->v<cyc_t>(V_X1));
    fetch(e, x2, L->v<cyc_t>(V_T));
    fetch(e, c3, C->v<double>(V_C1));
    fetch(e, o6, out6);
    fetch(e, o3, out3);
    fetch(e, acol, L->acol.p);
    fetch(e, aval, L->avalf.p);
    fetch(e, alen, L->alen.p);
    fetch(e, pcol, L->pcol.p);
    fetch(e, pval, L->pvalf.p);
    fetch(e, wcol, L->wcol.p);
    fetch(e, wval, L->wval.p);
    fetch(e, wlen, L->wlen.p);
    fetch(e, p2col, L->p2col.p);
    fetch(e, p2val, L->p2val.p);
    fetch(e, p2len, L->p2len.p);
    fetch(e, T, H->tail_op.p);
    buf.release();
    if (rc != NODAL_OK) return rc;
    NODAL_HIP_TRY(h, e);
    using Vec = std::vector<double>;
    auto absv = [](const auto &v) { Vec y(v.size()); for (size_t i = 0; i < v.size(); ++i) y[i] = fabs((double)v[i]); return y; };
    auto add = [](Vec a, const Vec &b2) { for (size_t i = 0; i < a.size(); ++i) a[i] += b2[i]; return a; };
    auto wd = [&](Vec v) { for (int64_t i = 0; i < n; ++i) v[i] *= OMEGA * dinv[i]; return v; };
    auto absA = [&](const Vec &v) {
        Vec y((size_t)n, 0.0);
        for (int64_t i = 0; i < n; ++i)
            for (int32_t s = 0; s < alen[i]; ++s) y[i] += fabs((double)aval[(size_t)s * ld + i]) * v[acol[(size_t)s * ld + i]];
        return y;
    };
    auto absG = [&](const Vec &v) { return add(v, wd(absA(v))); };
    auto absGT = [&](const Vec &v) { return add(v, absA(wd(v))); };  // (|a_ij| = |a_ji|)
    // a column-major ELL operator n x n_t (slots, cols, vals, per-row length or -1 entries): |M| v and |M|^T v
    auto ell = [&](int slots, const std::vector<int32_t> &col, const std::vector<float> &val, const std::vector<int32_t> *len,
                   const Vec &v, bool transposed) {
        Vec y((size_t)(transposed ? nt : n), 0.0);
        for (int64_t i = 0; i < n; ++i) {
            const int32_t m = len ? (*len)[i] : slots;
            for (int32_t s = 0; s < m; ++s) {
                const int32_t J = col[(size_t)s * ld + i];
                if (J < 0) continue;
                const double a = fabs((double)val[(size_t)s * ld + i]);
                if (transposed) y[J] += a * v[i];
                else y[i] += a * v[J];
            }
        }
        return y;
    };
    auto absT = [&](const Vec &v) {
        Vec y((size_t)nt, 0.0);
        for (int64_t i = 0; i < nt; ++i)
            for (int64_t j = 0; j < nt; ++j) y[i] += fabs(T[(size_t)i * nt + j]) * v[j];
        return y;
    };
    auto Pt = [&](const Vec &v) { return ell(PW, pcol, pval, nullptr, v, true); };
    auto Wm = [&](const Vec &v) { return ell(L->wslots, wcol, wval, &wlen, v, false); };
    auto Wt = [&](const Vec &v) { return ell(L->wslots, wcol, wval, &wlen, v, true); };
    auto P2m = [&](const Vec &v) { return ell(P2CAP, p2col, p2val, &p2len, v, false); };
    auto P2t = [&](const Vec &v) { return ell(P2CAP, p2col, p2val, &p2len, v, true); };
    const Vec ax1 = absA(absv(x1));
    const Vec e_r = add(absv(r), ax1);
    const Vec e_c6 = absT(Pt(add(absv(r), e_r)));
    const Vec e_xp = add(add(absv(xp), wd(e_r)), add(Wm(absv(c6)), Wm(e_c6)));
    const Vec dev6 = add(add(absv(o6), absG(e_xp)), wd(absA(absv(xp))));
    const Vec e_x2 = add(absv(x2), wd(ax1));
    const Vec e_c3 = absT(add(P2t(absv(hb)), Wt(absGT(absv(hb)))));
    const Vec ac3 = absv(c3);
    const Vec dev3 = add(add(add(absv(o3), absG(e_x2)), wd(absA(absv(x2)))), add(add(P2m(ac3), absG(Wm(ac3))), P2m(e_c3)));
    double dm = 0.0;
    int maxp2 = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double di = fabs((double)o3[i] - (double)o6[i]) / (dev6[i] + dev3[i]);  // (0 / 0: a NaN, which the maximum keeps)
        dm = nan_max(di, dm);
        maxp2 = p2len[i] > maxp2 ? p2len[i] : maxp2;
    }
    fprintf(stderr, "[sagg] visit check: level %d, rows %lld, n_t %lld, longest P2 row %d, three launches against the six "
                    "d = %.3e (against the bound 2^-23: %.3e)\n", l, (long long)n, (long long)nt, maxp2, dm, dm / 0x1p-23);
    return NODAL_OK;
}
// NODAL_TRACE with NODAL_SA_RESTRICT_CHECK=1: every level that restricts from b forms rc both ways on one fixed
// right-hand side of both signs (b uniform in (-1, 1), x0 = w D^-1 b as its producer leaves it) and prints
//   d = max_I |rc_new - rc_old|_I / den_I,   den_I = sum_i |R_Ii| (|b_i| + sum_j |a_ij| |x0_j|) + sum_i |W_iI| |b_i|,
// den formed on the host in fp64 from the operators as stored.  Against the exact rc (A, P in f64, W = G P) the two
// launches carry the f32 roundings of x0, of the copies of A and of R and of r as stored -- each at most 2^-24 of a
// term of the first sum --, the one launch that of the stored W, 2^-24 of a term of the second; every sum is fp64.  The
// roundings are of either sign and do not add up in practice: the bar is 2^-23 as for the visit check above (measured:
// tests/test_gpu_restrict_from_b.py).
template <typename TO>
int restrict_check_level(nodal_ctx *h, SHierarchy *H, int l) {
    hipStream_t st = h->stream;
    SLevel *L = H->pool[l], *C = H->pool[l + 1];
    const int64_t n = L->n, ld = L->ld, nc = C->n, rld = L->rld;
    CheckRng rng{0x9e3779b97f4a7c15ull + 1297ull * (uint64_t)l};
    const int64_t rslots = (int64_t)rcap_for(nc) * rld;
    std::vector<double> dinv((size_t)n);
    std::vector<cyc_t> hb((size_t)n), hx0((size_t)n);
    std::vector<TO> rc_old((size_t)nc), rc_new((size_t)nc);
    std::vector<int32_t> acol((size_t)L->width * ld), alen((size_t)n), rcol((size_t)rslots), rlen((size_t)nc),
        wcol((size_t)L->wslots * ld), wlen((size_t)n);
    std::vector<float> aval((size_t)L->width * ld), rval((size_t)rslots), wval((size_t)L->wslots * ld);
    hipError_t e = hipStreamSynchronize(st);
    fetch(e, dinv, L->dinv.p);
    for (int64_t i = 0; i < n; ++i) {
        hb[i] = (cyc_t)rng.unit();
        hx0[i] = (cyc_t)(OMEGA * dinv[i] * (double)hb[i]);
    }
    const size_t vb = align256((size_t)n * sizeof(cyc_t)), cb = align256((size_t)nc * sizeof(TO));
    DevBuf buf;
    if (e == hipSuccess) e = buf.reserve(3 * vb + 2 * cb);
    char *p = buf.as<char>();
    cyc_t *b = reinterpret_cast<cyc_t *>(p), *x0 = reinterpret_cast<cyc_t *>(p + vb), *r = reinterpret_cast<cyc_t *>(p + 2 * vb);
    TO *ro = reinterpret_cast<TO *>(p + 3 * vb), *rn = reinterpret_cast<TO *>(p + 3 * vb + cb);
    if (e == hipSuccess) e = hipMemcpyAsync(b, hb.data(), (size_t)n * sizeof(cyc_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(x0, hx0.data(), (size_t)n * sizeof(cyc_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const Ell A = L->A();
        const unsigned g = grid_for(n);
        const unsigned rblocks = restrict_blocks(nc);
        SAGG_DISPATCH_W(L->wfix, (k_smooth_residual<W, cyc_t><<<g, TB, 0, st>>>(A, b, x0, r)));
        k_restrict<TO><<<grid_for(nc * RL), TB, 0, st>>>(nc, rld, L->rcol.as<int32_t>(), L->rvalf.as<float>(),
                                                        L->rlen.as<int32_t>(), r, ro, C->dinv.as<double>(), nullptr);
        SAGG_DISPATCH_W(L->wfix, (k_residual_restrict<W, TO><<<rblocks + g, TB, 0, st>>>(
                                     A, b, x0, r, rblocks, nc, L->wtstart.as<uint32_t>(), L->wtcol.as<int32_t>(),
                                     L->wtval.as<float>(), rn, C->dinv.as<double>(), nullptr)));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    fetch(e, rc_old, ro);
    fetch(e, rc_new, rn);
    fetch(e, acol, L->acol.p);
    fetch(e, aval, L->avalf.p);
    fetch(e, alen, L->alen.p);
    fetch(e, rcol, L->rcol.p);
    fetch(e, rval, L->rvalf.p);
    fetch(e, rlen, L->rlen.p);
    fetch(e, wcol, L->wcol.p);
    fetch(e, wval, L->wval.p);
    fetch(e, wlen, L->wlen.p);
    buf.release();
    NODAL_HIP_TRY(h, e);
    std::vector<double> t((size_t)n), den((size_t)nc, 0.0);
    for (int64_t i = 0; i < n; ++i) {  // |b_i| + sum_j |a_ij| |x0_j|
        double s = fabs((double)hb[i]);
        for (int32_t q = 0; q < alen[i]; ++q)
            s += fabs((double)aval[(size_t)q * ld + i]) * fabs((double)hx0[acol[(size_t)q * ld + i]]);
        t[i] = s;
    }
    for (int64_t I = 0; I < nc; ++I)
        for (int32_t q = 0; q < rlen[I]; ++q) {
            const size_t at = ((size_t)(q >> 3) * rld + I) * 8 + (q & 7);
            den[I] += fabs((double)rval[at]) * t[rcol[at]];
        }
    for (int64_t i = 0; i < n; ++i)
        for (int32_t q = 0; q < wlen[i]; ++q)
            den[wcol[(size_t)q * ld + i]] += fabs((double)wval[(size_t)q * ld + i]) * fabs((double)hb[i]);
    double dm = 0.0;
    for (int64_t I = 0; I < nc; ++I) {
        const double di = fabs((double)rc_new[I] - (double)rc_old[I]) / den[I];  // (0 / 0: a NaN, which the maximum keeps)
        dm = nan_max(di, dm);
    }
    fprintf(stderr, "[sagg] restrict check: level %d, rows %lld, coarse rows %lld, rc from b against the two launches "
                    "d = %.3e (against the bound 2^-23: %.3e)\n", l, (long long)n, (long long)nc, dm, dm / 0x1p-23);
    return NODAL_OK;
}
int restrict_self_check(nodal_ctx *h, SHierarchy *H) {
    static const bool check = knob::TRACE.now() && knob::SA_RESTRICT_CHECK.now();
    if (!check) return NODAL_OK;
    for (int l = 1; l + 1 < H->nlev; ++l) {
        if (!H->pool[l]->restrict_b) continue;
        const bool last = l + 1 == H->tail || l + 1 == H->nlev - 1;  // (as cycle() tells the two forms apart)
        if (last) NODAL_TRY(restrict_check_level<double>(h, H, l));
        else NODAL_TRY(restrict_check_level<cyc_t>(h, H, l));
    }
    return NODAL_OK;
}

int visit_self_check(nodal_ctx *h, SHierarchy *H) {
    static const bool check = knob::TRACE.now() && knob::SA_VISIT_CHECK.now();
    if (!check) return NODAL_OK;
    for (int l = 1; l + 1 < H->nlev; ++l) {
        const SLevel *L = H->pool[l];
        if (L->visit && l + 1 == H->tail && H->tail_dense && H->nu[l < 2 ? l : 2] == 2) NODAL_TRY(visit_check_level(h, H, l));
    }
    return NODAL_OK;
}

// behind a fresh setup and behind a values-only refresh
int setup_self_checks(nodal_ctx *h, SHierarchy *H) {
    NODAL_TRY(fold_self_check(h, H));
    NODAL_TRY(visit_self_check(h, H));
    return restrict_self_check(h, H);
}

}  // namespace
