// The per-diode arithmetic that the kernels of newton.hip, transient_nl.hip and newton_gradient.hip share: the
// companion model at a junction voltage, SPICE's junction limiting and the convergence test.  Device code only; every
// product is a statement of its own (the library is built with -ffp-contract=on), so that g, i and J are the roundings
// the formulas of include/nodal_hip.h name, whichever kernel a lane runs in.
#pragma once
#include "table_rows.h"

constexpr int TTB = 256;  // one lane per diode, 256 to a block

// grouping enumerator (group.h): diode i touches its anode (slot 0: +J) and its cathode (slot 1: -J); one column
struct DiodeLeads {
    static constexpr int SLOTS = 2;
    const int32_t *rows, *a, *b;
    int64_t nitems;
    template <class F>
    __device__ void for_each(int64_t i, F f) const {
        const int32_t r = rows[i];
        const int ia = a[r], ib = b[r];
        if (ia >= 0) f(0, ia, 0);
        if (ib >= 0) f(1, ib, 0);
    }
};

// g = i_sat e / n_vt + gmin and i = i_sat (e - 1) + gmin v at v, e = exp(v / n_vt)
__device__ __forceinline__ void diode_model(double v, double is, double nv, double gmin, double *g_out, double *i_out) {
    const double e = exp(v / nv);
    const double ge = is * e;
    const double gl = gmin * v;
    const double g = ge / nv + gmin;
    const double ie = is * (e - 1.0);
    *g_out = g;
    *i_out = ie + gl;
}

// the bits of a non-negative double order as the values do, every NaN above +inf
__device__ __forceinline__ unsigned long long magnitude_bits(double m) {
    return (unsigned long long)__double_as_longlong(fabs(m));
}

// After a solve: from the raw v of the new x and the voltage `old` its linearisation (gk, ik) was taken at, the limited
// voltage of the next linearisation (returned), whether the limiter changed it, whether this diode passes the
// convergence test (false with a NaN anywhere), and dv = v - old.
__device__ __forceinline__ double diode_limit_and_test(double v, double old, double is, double nv, double gmin, double reltol,
                                                       double vntol, double abstol, double gk, double ik, bool *limited_out,
                                                       bool *ok_out, double *dv_out) {
    const double dv = v - old;
    const double vcrit = nv * log(nv / (1.4142135623730951 * is));
    const bool limited = v > vcrit && fabs(dv) > 2.0 * nv;
    double next = v;
    if (limited) {
        if (old > 0.0) {
            const double arg = 1.0 + dv / nv;
            const double step = nv * log(arg);
            next = arg > 0.0 ? old + step : vcrit;
        } else {
            next = nv * log(v / nv);
        }
    }
    // the current the junction carries at v against the current its linearisation predicted there
    const double ee = is * (exp(v / nv) - 1.0);
    const double gl = gmin * v;
    const double iv = ee + gl;
    const double slope = gk * dv;
    const double ihat = ik + slope;
    const double vbar = reltol * fmax(fabs(v), fabs(old)) + vntol;
    const double ibar = reltol * fmax(fabs(iv), fabs(ihat)) + abstol;
    *limited_out = limited;
    *ok_out = fabs(dv) <= vbar && fabs(iv - ihat) <= ibar;
    *dv_out = dv;
    return next;
}
