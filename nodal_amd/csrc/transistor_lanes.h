// The per-transistor arithmetic of newton.hip's transport lanes: the transport current of the Ebers-Moll model in its
// transport form, its linearisation and its convergence test.  A bipolar transistor is two junction diodes -- plain
// members of the call's DiodeSet, whose model, limiting and test are diode_lanes.h's -- plus ONE current source that
// those same two junction voltages control,
//     i_T = i_s (exp(v_f / n_f) - exp(v_r / n_r))        from lead a to lead b through the element,
// v_f, v_r the voltages and n_f, n_r the n_vt of the junctions jf, jr (indices into the call's diodes).  The lanes know
// nothing of NPN or PNP: the kind is the caller's choice of leads.  The transport has no gmin (it stays on the
// junctions), no limiting and no state word of its own: it is linearised at the junctions' limited voltages.  Device
// code only, one lane per transport, TTB to a block; every product is a statement of its own (the library is built with
// -ffp-contract=on), so that gmf, gmr, iT and JT are the roundings the formulas of include/nodal_hip.h name.
#pragma once
#include "diode_lanes.h"

// grouping enumerator (group.h): transport t touches its lead a (slot 0: +JT) and its lead b (slot 1: -JT), the leads
// of its forward GM row gm_rows[2 t]; one column
struct TransportLeads {
    static constexpr int SLOTS = 2;
    const int32_t *gm_rows, *a, *b;
    int64_t nitems;
    template <class F>
    __device__ void for_each(int64_t i, F f) const {
        const int32_t r = gm_rows[2 * i];
        const int ia = a[r], ib = b[r];
        if (ia >= 0) f(0, ia, 0);
        if (ib >= 0) f(1, ib, 0);
    }
};

// gmf = i_s ef / n_f, gmr = i_s er / n_r and iT = i_s ef - i_s er at (vf, vr), ef = exp(vf / n_f), er = exp(vr / n_r)
__device__ __forceinline__ void transport_model(double vf, double vr, double is, double nf, double nr, double *gmf_out,
                                                double *gmr_out, double *it_out) {
    const double ef = exp(vf / nf);
    const double er = exp(vr / nr);
    const double jf = is * ef;
    const double jr = is * er;
    *gmf_out = jf / nf;
    *gmr_out = jr / nr;
    *it_out = jf - jr;
}

// JT = gmf vhf - gmr vhr - iT: injected into lead a, drawn from lead b (the diodes' convention)
__device__ __forceinline__ double transport_history(double vhf, double vhr, double gmf, double gmr, double it) {
    const double pf = gmf * vhf;
    const double pr = gmr * vhr;
    const double both = pf - pr;
    return both - it;
}

// After a solve: the transport current at the raw (vf, vr) of the new x against what the linearisation (gmf, gmr, iT
// at vhf, vhr) predicted there; false with a NaN anywhere
__device__ __forceinline__ bool transport_test(double vf, double vr, double vhf, double vhr, double is, double nf, double nr,
                                               double gmf, double gmr, double it, double reltol, double abstol) {
    const double jf = is * exp(vf / nf);
    const double jr = is * exp(vr / nr);
    const double iv = jf - jr;
    const double sf = gmf * (vf - vhf);
    const double sr = gmr * (vr - vhr);
    const double up = it + sf;
    const double ihat = up - sr;
    const double ibar = reltol * fmax(fabs(iv), fabs(ihat)) + abstol;
    return fabs(iv - ihat) <= ibar;
}
