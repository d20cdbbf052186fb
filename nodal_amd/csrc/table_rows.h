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
