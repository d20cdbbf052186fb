// What the analyses that walk the component table share: a lead's value, the value column in force, the launch
// arithmetic -- and the ONE statement in code of the per-row adjoint formulas (row_term, cross_term).
#pragma once

#include "ctx.h"

// workgroups of `threads` lanes that cover `items`
static inline unsigned groups_of(int64_t items, int threads) { return (unsigned)((items + threads - 1) / threads); }

// the value column the last numeric assembly used (stamp_numeric's choice)
static inline const double *assembled_values(nodal_ctx *h) {
    return h->batch > 0 ? h->values_batch.as<double>() + (int64_t)h->member * h->ncomp : h->value.as<double>();
}

// x[node], +0.0 for the ground lead
__device__ __forceinline__ double lead(const double *__restrict__ x, int32_t node) { return node < 0 ? 0.0 : x[node]; }
// element (node, y) of a block, `at` = y * cs, +0.0 for the ground lead
__device__ __forceinline__ double lead(const double *__restrict__ v, int32_t node, int64_t rs, int64_t at) {
    return node < 0 ? 0.0 : v[(int64_t)node * rs + at];
}

// The adjoint term of one table row, as the comment at the head of sensitivity.hip tabulates it (the single written
// statement of the formulas): D * w with D = L(j1) - L(j2) and w = (X(p1) - X(p2)) / den when reads_x, else 1.
// A lead of -1 is ground (or, for j2, absent: the rows that read their branch unknown K + k alone).
struct RowTerm {
    int32_t j1 = -1, j2 = -1;  // the leads of lambda
    int32_t p1 = -1, p2 = -1;  // the leads of x
    double den = 1.0;          // v * v (R), 1 (VCVS), -Rd (CCVS, CCCS)
    bool reads_x = false;
    bool none = false;         // a row without a term
};

// the R case alone: what a companion resistor's history term (transient_gradient.hip) shares with its table term
__device__ __forceinline__ RowTerm resistor_term(int64_t i, const double *__restrict__ value,
                                                 const int32_t *__restrict__ a, const int32_t *__restrict__ b) {
    RowTerm r;
    r.j1 = r.p1 = a[i];
    r.j2 = r.p2 = b[i];
    const double v = value[i];
    r.den = v * v;
    r.reads_x = true;
    return r;
}

__device__ __forceinline__ RowTerm row_term(int64_t i, int32_t K, const uint8_t *__restrict__ type,
                                            const double *__restrict__ value, const int32_t *__restrict__ a,
                                            const int32_t *__restrict__ b, const int32_t *__restrict__ c,
                                            const int32_t *__restrict__ d, const int32_t *__restrict__ drv,
                                            const int32_t *__restrict__ k) {
    const int t = type[i];
    if (t == NODAL_T_R) return resistor_term(i, value, a, b);
    RowTerm r;
    if (t == NODAL_T_A) {
        r.j1 = a[i];
        r.j2 = b[i];
    } else if (t <= NODAL_T_CCCS && k[i] >= 0) {
        r.j1 = K + k[i];
        if (t != NODAL_T_E) {
            r.p1 = c[i];
            r.p2 = d[i];
            r.reads_x = true;
            if (t != NODAL_T_VCVS) {
                const int32_t dr = drv[i];
                r.den = -(dr >= 0 ? value[dr] : 1.0);
            }
        }
    } else {
        r.none = true;
    }
    return r;
}

// What the CCVS / CCCS row j adds to the resistor of value v that drives it: L(m_j) v_j (X(c_j) - X(d_j)) / v^2, from
// column `lat` = y * cs of lam and `xat` = y * xcs of x.  The caller adds the rows of a driver's group in table order,
// each with a statement of its own (the library is built with -ffp-contract=on: a sum inside this expression would fuse).
__device__ __forceinline__ double cross_term(int32_t j, int32_t K, double v, const double *__restrict__ value,
                                             const int32_t *__restrict__ c, const int32_t *__restrict__ d,
                                             const int32_t *__restrict__ k, const double *__restrict__ lam, int64_t rs,
                                             int64_t lat, const double *__restrict__ x, int64_t xrs, int64_t xat) {
    const double u = lead(x, c[j], xrs, xat) - lead(x, d[j], xrs, xat);
    const double lm = lam[((int64_t)K + k[j]) * rs + lat];
    return lm * value[j] * u / (v * v);
}

// ---- the complex evaluation of the same formulas (ac_gradient.hip) ----
// x and lam are phasors interleaved by unknown: the real part of unknown i at [2i], the imaginary part at [2i + 1].
struct Phasor {
    double re, im;
};
// v(j1) - v(j2), +0.0 for a ground (or absent) lead
__device__ __forceinline__ Phasor phasor_diff(const double *__restrict__ v, int32_t j1, int32_t j2) {
    return {lead(v, j1, 2, 0) - lead(v, j2, 2, 0), lead(v, j1, 2, 1) - lead(v, j2, 2, 1)};
}
// Re(d u) and Im(d u): every product and the sum a statement of its own (-ffp-contract=on would fuse one of the products
// into the sum, and the two parts of a term would round differently)
__device__ __forceinline__ double re_product(Phasor d, Phasor u) {
    const double p = d.re * u.re;
    const double q = d.im * u.im;
    return p - q;
}
__device__ __forceinline__ double im_product(Phasor d, Phasor u) {
    const double p = d.re * u.im;
    const double q = d.im * u.re;
    return p + q;
}
// the term of row_term's row at one frequency: Re(D U) / den; exactly +0.0 for an A or E row -- the small-signal
// excitation never reads the table value -- and for a row without a term
__device__ __forceinline__ double row_term_complex(const RowTerm &r, const double *__restrict__ x, const double *__restrict__ lam) {
    if (r.none || !r.reads_x) return 0.0;
    const double re = re_product(phasor_diff(lam, r.j1, r.j2), phasor_diff(x, r.p1, r.p2));
    return re / r.den;
}
// cross_term with complex L(m_j) and X: Re(L(m_j) (X(c_j) - X(d_j))) v_j / v^2
__device__ __forceinline__ double cross_term_complex(int32_t j, int32_t K, double v, const double *__restrict__ value,
                                                     const int32_t *__restrict__ c, const int32_t *__restrict__ d,
                                                     const int32_t *__restrict__ k, const double *__restrict__ lam,
                                                     const double *__restrict__ x) {
    const double re = re_product(phasor_diff(lam, K + k[j], -1), phasor_diff(x, c[j], d[j]));
    return re * value[j] / (v * v);
}
