// Nonlinear DC analysis: networks with diodes, solved by Newton's method with the loop's lane work on the device.
//
// Replaces a host loop of download x, evaluate the junctions in numpy, upload a value column, re-assemble and solve per
// iteration (with the reference: a new netlist, a new `Circuit` and a `.solve()` per iteration, reference
// nodal/nodal.py:306-336, plus a host pass over the diodes).
//
// The handle holds the circuit with one extra R row per diode, as nodal_transient holds one per capacitor.  A diode
// carries i(v) = i_sat (exp(v / n_vt) - 1) + gmin v from its anode (lead a) to its cathode (lead b) at v = x(a) - x(b).
// One state word vh per diode is the limited junction voltage the next linearisation is taken at.  Iteration k is, on
// the handle's stream,
//     k_newton_linearise    one lane per diode: e = exp(vh / n_vt), g = i_sat e / n_vt + gmin, i = i_sat (e - 1) + gmin vh;
//                           1 / g into the diode's row of the value column the assembly reads, J = g vh - i into the
//                           history array (injected into lead a, drawn from lead b: the capacitors' convention)
//     stamp_numeric         G from the value column, the symbolic phase kept
//     stamp_rhs_multi       the sources (one setting) into a zeroed vector
//     k_signed_list_add     one lane per node with diodes: +-J of its diodes in list order, no atomics
//     the solve             transient_solver_begin / transient_solver_step: the dense panel (n <= 64), the sparse LU
//                           factored anew on its kept analysis, or the multigrid iteration on a hierarchy whose values
//                           are refreshed on its kept symbolic setup (a step it gives up on: the sparse direct solve)
//     the judgement         the block judge of multi_rhs_solve on one column
//     k_newton_update       one lane per diode: raw v from the new x, SPICE's junction limiting vh' = pnjlim(v, vh), this
//                           diode's convergence test, and into the iteration's record two integer counts (atomicAdd) and
//                           the largest |v - vh| (atomicMax on the bits of a non-negative double, NaN above everything):
//                           no floating-point sums, a repeated call gives the same bits
// and then ONE read of the record's words, the scaled residual among them.  The loop ends when no diode failed its
// test, on max_iter, on info > 0 or on a record that is not finite; k_newton_outputs then forms v, i(v), g(v) from x.
//
// The iteration is newton_iteration below, and the call's diodes on the device are a DiodeSet (ctx.h): both serve
// nodal_transient_nl (transient_nl.hip), which nests the loop inside every time step, and the DiodeSet serves
// nodal_newton_gradient (newton_gradient.hip) as well.
//
// Bipolar transistors (nodal_newton_dc_bjt).  In the transport form of Ebers-Moll a transistor is two junction diodes,
// plain members of the call's diodes, plus the transport current i_T = i_s (exp(v_f / n_f) - exp(v_r / n_r)) that those
// two junction voltages control (transistor_lanes.h).  The call's transports are a TransportSet (ctx.h); the table holds
// two GM rows per transport behind the diodes' R rows.  With a set, an iteration has three more launches:
//     k_transport_linearise behind k_newton_linearise: one lane per transport at the SAME words vh[jf], vh[jr] the
//                           junctions are linearised at: gmf into the forward GM row, -gmr into the reverse one,
//                           JT = gmf vhf - gmr vhr - iT into the transports' history array
//     k_signed_list_add     a second one behind the diodes': one lane per node with transports, +-JT in list order
//     k_transport_update    behind k_newton_update: the transport's test at the raw vf, vr of the new x, and an integer
//                           atomicAdd into word NEWTON_REC_TRANSPORTS of the record
// and the loop has converged when no diode and no transport failed.  Limiting is the junctions' alone.  A gmf or gmr that
// is not finite is an overflow as the diodes' 1 / g == 0 is.  GM rows make the network non-passive, so a network with
// transports never takes the multigrid route: the dense panel (n <= 64) or the sparse LU.  Without a set
// every launch and every bit is as before.
#include "transistor_lanes.h"
#include "group.h"

#include <cmath>

namespace {

// bad[0] |= 1 for a diode row that is not a resistor, |= 2 for a saturation current or an n_vt that is not > 0 and finite
__global__ __launch_bounds__(TTB) void k_newton_check(int64_t nd, const int32_t *__restrict__ rows,
                                                      const uint8_t *__restrict__ type, const double *__restrict__ isat,
                                                      const double *__restrict__ nvt, int32_t *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (i >= nd) return;
    if (type[rows[i]] != NODAL_T_R) atomicOr(bad, 1);
    if (!(isat[i] > 0.0 && isat[i] < INFINITY && nvt[i] > 0.0 && nvt[i] < INFINITY)) atomicOr(bad, 2);
}

// vh_0 = x0(a) - x0(b)
__global__ __launch_bounds__(TTB) void k_newton_start(int64_t nd, const int32_t *__restrict__ rows,
                                                      const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                      const double *__restrict__ x, double *__restrict__ vh) {
    const int64_t i = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (i >= nd) return;
    const int32_t r = rows[i];
    vh[i] = lead(x, a[r]) - lead(x, b[r]);
}

// One lane per diode: the companion model at vh.  Every product is a statement of its own (the library is built with
// -ffp-contract=on), so that g, i and J are the roundings the formulas name.
__global__ __launch_bounds__(TTB) void k_newton_linearise(int64_t nd, const int32_t *__restrict__ rows,
                                                          const double *__restrict__ isat, const double *__restrict__ nvt,
                                                          double gmin, const double *__restrict__ vh,
                                                          double *__restrict__ value, double *__restrict__ hist,
                                                          double *__restrict__ gk, double *__restrict__ ik) {
    const int64_t d = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (d >= nd) return;
    const double v = vh[d];
    double g, i;
    diode_model(v, isat[d], nvt[d], gmin, &g, &i);
    const double gv = g * v;
    value[rows[d]] = 1.0 / g;
    hist[d] = gv - i;
    gk[d] = g;
    ik[d] = i;
}

// One lane per diode after the solve: the limited voltage of the next linearisation, the convergence test against the
// linearisation (gk, ik at vh) this x was solved with, and the record: rec[0] diodes that failed, rec[1] diodes that
// were limited, rec[2] the bits of max |v - vh|.  COUNT_MOVED (nodal_transient_nl's reuse): 1 / g of the NEXT
// linearisation as well, compared bit for bit with the value column; rec[4] diodes where it differs.
template <bool COUNT_MOVED>
__global__ __launch_bounds__(TTB) void k_newton_update(int64_t nd, const int32_t *__restrict__ rows,
                                                       const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                       const double *__restrict__ isat, const double *__restrict__ nvt,
                                                       double gmin, double reltol, double vntol, double abstol,
                                                       const double *__restrict__ x, const double *__restrict__ vh,
                                                       const double *__restrict__ gk, const double *__restrict__ ik,
                                                       double *__restrict__ vh_next, unsigned long long *__restrict__ rec,
                                                       const double *__restrict__ value) {
    const int64_t d = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (d >= nd) return;
    const int32_t r = rows[d];
    const double v = lead(x, a[r]) - lead(x, b[r]);
    const double old = vh[d], is = isat[d], nv = nvt[d];
    bool limited, ok;
    double dv;
    const double next = diode_limit_and_test(v, old, is, nv, gmin, reltol, vntol, abstol, gk[d], ik[d], &limited, &ok, &dv);
    vh_next[d] = next;
    double inverse = 0.0;
    if constexpr (COUNT_MOVED) {
        double g, i;
        diode_model(next, is, nv, gmin, &g, &i);  // (k_newton_linearise's g at vh': the same statements, the same bits)
        inverse = 1.0 / g;
    }
    if (!ok) atomicAdd(rec, 1ull);
    if (limited) atomicAdd(rec + 1, 1ull);
    atomicMax(rec + 2, magnitude_bits(dv));
    if constexpr (COUNT_MOVED)
        if (__double_as_longlong(inverse) != __double_as_longlong(value[r])) atomicAdd(rec + 4, 1ull);
}

// One lane per diode, once the loop has ended: v, i(v) and g(v) of the final x
__global__ __launch_bounds__(TTB) void k_newton_outputs(int64_t nd, const int32_t *__restrict__ rows,
                                                        const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                        const double *__restrict__ isat, const double *__restrict__ nvt,
                                                        double gmin, const double *__restrict__ x, double *__restrict__ vout,
                                                        double *__restrict__ iout, double *__restrict__ gout) {
    const int64_t d = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (d >= nd) return;
    const int32_t r = rows[d];
    const double v = lead(x, a[r]) - lead(x, b[r]);
    double g, i;
    diode_model(v, isat[d], nvt[d], gmin, &g, &i);
    vout[d] = v;
    iout[d] = i;
    gout[d] = g;
}

// value[rows[d]] = fill: what the companion rows hold after a linearisation that overflowed
__global__ __launch_bounds__(TTB) void k_newton_fill(int64_t nd, const int32_t *__restrict__ rows, double fill,
                                                     double *__restrict__ value) {
    const int64_t d = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (d < nd) value[rows[d]] = fill;
}

// ---- the transports (transistor_lanes.h) ----
// bad[0] |= 1 for a junction index outside [0, nd) (nothing else of that transport is looked at), |= 2 for a GM row that
// is not of type GM, |= 4 for two rows that do not share their a, b, |= 8 for c, d that are not the leads of the
// junction's row, |= 16 for an i_s that is not > 0 and finite
__global__ __launch_bounds__(TTB) void k_transport_check(int64_t nt, int64_t nd, const int32_t *__restrict__ gm,
                                                         const int32_t *__restrict__ jn, const int32_t *__restrict__ rows,
                                                         const uint8_t *__restrict__ type, const int32_t *__restrict__ a,
                                                         const int32_t *__restrict__ b, const int32_t *__restrict__ c,
                                                         const int32_t *__restrict__ d, const double *__restrict__ is,
                                                         int32_t *__restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (t >= nt) return;
    if (!(is[t] > 0.0 && is[t] < INFINITY)) atomicOr(bad, 16);
    const int32_t rf = gm[2 * t], rr = gm[2 * t + 1];
    if (type[rf] != NODAL_T_GM || type[rr] != NODAL_T_GM) atomicOr(bad, 2);
    if (a[rf] != a[rr] || b[rf] != b[rr]) atomicOr(bad, 4);
    for (int q = 0; q < 2; ++q) {
        const int32_t j = jn[2 * t + q], r = gm[2 * t + q];
        if (j < 0 || j >= nd) {
            atomicOr(bad, 1);
            continue;
        }
        const int32_t rj = rows[j];
        if (c[r] != a[rj] || d[r] != b[rj]) atomicOr(bad, 8);
    }
}

// One lane per transport: the companion model at the junctions' limited voltages.  flag: set by a gmf or gmr that is not
// finite (an overflow of the iteration).
__global__ __launch_bounds__(TTB) void k_transport_linearise(int64_t nt, const int32_t *__restrict__ gm,
                                                             const int32_t *__restrict__ jn, const double *__restrict__ is,
                                                             const double *__restrict__ nvt, const double *__restrict__ vh,
                                                             double *__restrict__ value, double *__restrict__ hist,
                                                             double *__restrict__ gmf_k, double *__restrict__ gmr_k,
                                                             double *__restrict__ it_k, int32_t *__restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (t >= nt) return;
    const int32_t jf = jn[2 * t], jr = jn[2 * t + 1];
    const double vhf = vh[jf], vhr = vh[jr];
    double gmf, gmr, it;
    transport_model(vhf, vhr, is[t], nvt[jf], nvt[jr], &gmf, &gmr, &it);
    value[gm[2 * t]] = gmf;
    value[gm[2 * t + 1]] = -gmr;
    hist[t] = transport_history(vhf, vhr, gmf, gmr, it);
    gmf_k[t] = gmf;
    gmr_k[t] = gmr;
    it_k[t] = it;
    if (!(fabs(gmf) < INFINITY && fabs(gmr) < INFINITY)) atomicOr(flag, 1);
}

// the raw voltage of junction j at x
__device__ __forceinline__ double junction_voltage(int32_t j, const int32_t *__restrict__ rows, const int32_t *__restrict__ a,
                                                   const int32_t *__restrict__ b, const double *__restrict__ x) {
    const int32_t r = rows[j];
    return lead(x, a[r]) - lead(x, b[r]);
}

// One lane per transport after the solve: its test against the linearisation this x was solved with; rec_failed counts
// the transports that fail (an integer atomicAdd)
__global__ __launch_bounds__(TTB) void k_transport_update(int64_t nt, const int32_t *__restrict__ jn,
                                                          const int32_t *__restrict__ rows, const int32_t *__restrict__ a,
                                                          const int32_t *__restrict__ b, const double *__restrict__ is,
                                                          const double *__restrict__ nvt, double reltol, double abstol,
                                                          const double *__restrict__ x, const double *__restrict__ vh,
                                                          const double *__restrict__ gmf_k, const double *__restrict__ gmr_k,
                                                          const double *__restrict__ it_k,
                                                          unsigned long long *__restrict__ rec_failed) {
    const int64_t t = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (t >= nt) return;
    const int32_t jf = jn[2 * t], jr = jn[2 * t + 1];
    const double vf = junction_voltage(jf, rows, a, b, x), vr = junction_voltage(jr, rows, a, b, x);
    const bool ok = transport_test(vf, vr, vh[jf], vh[jr], is[t], nvt[jf], nvt[jr], gmf_k[t], gmr_k[t], it_k[t], reltol, abstol);
    if (!ok) atomicAdd(rec_failed, 1ull);
}

// One lane per transport, once the loop has ended: iT, gmf and gmr at the raw junction voltages of the final x
__global__ __launch_bounds__(TTB) void k_transport_outputs(int64_t nt, const int32_t *__restrict__ jn,
                                                           const int32_t *__restrict__ rows, const int32_t *__restrict__ a,
                                                           const int32_t *__restrict__ b, const double *__restrict__ is,
                                                           const double *__restrict__ nvt, const double *__restrict__ x,
                                                           double *__restrict__ it_out, double *__restrict__ gmf_out,
                                                           double *__restrict__ gmr_out) {
    const int64_t t = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (t >= nt) return;
    const int32_t jf = jn[2 * t], jr = jn[2 * t + 1];
    const double vf = junction_voltage(jf, rows, a, b, x), vr = junction_voltage(jr, rows, a, b, x);
    transport_model(vf, vr, is[t], nvt[jf], nvt[jr], gmf_out + t, gmr_out + t, it_out + t);
}

// value[both GM rows of t] = fill
__global__ __launch_bounds__(TTB) void k_transport_fill(int64_t nt, const int32_t *__restrict__ gm, double fill,
                                                        double *__restrict__ value) {
    const int64_t q = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (q < 2 * nt) value[gm[q]] = fill;
}

}  // namespace

// ---- the call's diodes on the device (ctx.h) ----
int DiodeSet::prepare(nodal_ctx *h, const char *what, int64_t count, const int64_t *rows, const double *isat, const double *nvt,
                      double gmin_, DevBuf &spec, DevBuf &list_none, DevBuf &list_node, DevBuf &list_ptr, DevBuf &list_con,
                      size_t more_words, size_t more_doubles, int32_t **words, double **doubles) {
    hipStream_t st = h->stream;
    auto fail = [&](const char *text) { return nodal_fail(h, NODAL_E_INVALID, (std::string(what) + text).c_str()); };
    nd = count;
    nent = 0;
    gmin = gmin_;
    node = &list_node;
    ptr = &list_ptr;
    con = &list_con;
    for (int64_t i = 0; i < nd; ++i)
        if (rows[i] < 0 || rows[i] >= h->ncomp) return fail("diode row out of range");
    if (nd > 0 && h->K == 0) return fail("diodes on a network without nodes");
    if (h->n == 0) return NODAL_OK;
    const size_t row_words = ((size_t)nd + 15) & ~(size_t)15, own_words = (more_words + 15) & ~(size_t)15;
    NODAL_HIP_TRY(h, spec.reserve((row_words + own_words + 16) * 4 + ((size_t)nd * 5 + more_doubles) * 8 + 64));
    rows_dev = spec.as<int32_t>();
    *words = rows_dev + row_words;
    int32_t *bad_dev = *words + own_words;
    isat_dev = reinterpret_cast<double *>(bad_dev + 16);
    nvt_dev = isat_dev + nd;
    hist = nvt_dev + nd;
    gk = hist + nd;
    ik = gk + nd;
    *doubles = ik + nd;
    if (nd == 0) return NODAL_OK;
    std::vector<int32_t> r32((size_t)nd);
    for (int64_t i = 0; i < nd; ++i) r32[(size_t)i] = (int32_t)rows[i];
    NODAL_HIP_TRY(h, hipMemcpyAsync(rows_dev, r32.data(), (size_t)nd * 4, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(isat_dev, isat, (size_t)nd * 8, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(nvt_dev, nvt, (size_t)nd * 8, hipMemcpyHostToDevice, st));
    int32_t bad = 0;
    NODAL_HIP_TRY(h, hipMemsetAsync(bad_dev, 0, 4, st));
    k_newton_check<<<groups_of(nd, TTB), TTB, 0, st>>>(nd, rows_dev, h->type.as<uint8_t>(), isat_dev, nvt_dev, bad_dev);
    NODAL_HIP_TRY(h, hipGetLastError());
    NODAL_TRY(nodal_read_words(h, &bad, bad_dev, 4));  // (waits: the copies above are done too, r32 may end)
    if (bad & 1) return fail("a diode row that is not a resistor (R)");
    if (bad & 2) return fail("i_sat and n_vt must be positive and finite");
    int64_t ncon = 0;
    return grp::build_lists(h, DiodeLeads{rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(), nd}, (int64_t)h->K, &nent, &ncon,
                            list_none, list_node, list_ptr, list_con, nullptr, nullptr);
}

int DiodeSet::start(nodal_ctx *h, const double *x, double *vh) const {
    if (nd == 0) return NODAL_OK;
    k_newton_start<<<groups_of(nd, TTB), TTB, 0, h->stream>>>(nd, rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(), x, vh);
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

int DiodeSet::linearise(nodal_ctx *h, const double *vh, double *value) const {
    if (nd == 0) return NODAL_OK;
    k_newton_linearise<<<groups_of(nd, TTB), TTB, 0, h->stream>>>(nd, rows_dev, isat_dev, nvt_dev, gmin, vh, value, hist, gk, ik);
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

int DiodeSet::fill(nodal_ctx *h, double v, double *column) const {
    if (nd == 0) return NODAL_OK;
    k_newton_fill<<<groups_of(nd, TTB), TTB, 0, h->stream>>>(nd, rows_dev, v, column);
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

int DiodeSet::add_currents(nodal_ctx *h, double *rhs) const {
    return signed_list_add(h, nent, node->as<int32_t>(), ptr->as<int32_t>(), con->as<uint32_t>(), hist, rhs);
}

int DiodeSet::linearise_and_assemble(nodal_ctx *h, const double *vh, bool *overflowed, double *ms_stamp,
                                     const TransportSet *transports) const {
    double *value = const_cast<double *>(assembled_values(h));
    NODAL_TRY(linearise(h, vh, value));
    if (transports) NODAL_TRY(transports->linearise(h, *this, vh, value));
    const auto t0 = std::chrono::steady_clock::now();
    const int sn = stamp_numeric(h, h->member, nullptr);
    *ms_stamp += ms_since(t0);
    *overflowed = sn == NODAL_E_ZERO_RESISTANCE;  // (g overflowed: 1 / g == 0)
    if (transports && (sn == NODAL_OK || *overflowed)) {  // (a gmf or gmr that is not finite; the stream has drained)
        int32_t flag = 0;
        NODAL_TRY(nodal_read_words(h, &flag, transports->flag_dev + 1, 4));
        if (flag) *overflowed = true;
    }
    if (!*overflowed) return sn;
    NODAL_TRY(fill(h, 1.0, value));
    if (transports) NODAL_TRY(transports->fill(h, 0.0, value));
    return stamp_numeric(h, h->member, nullptr);
}

// ---- the call's transports on the device (ctx.h) ----
int TransportSet::prepare(nodal_ctx *h, const char *what, const DiodeSet &D, int64_t count, const int64_t *gm_rows,
                          const int32_t *junction, const double *i_s, DevBuf &spec, DevBuf &list_none, DevBuf &list_node,
                          DevBuf &list_ptr, DevBuf &list_con, size_t more_doubles, double **doubles) {
    hipStream_t st = h->stream;
    auto fail = [&](const char *text) { return nodal_fail(h, NODAL_E_INVALID, (std::string(what) + text).c_str()); };
    nt = count;
    nent = 0;
    node = &list_node;
    ptr = &list_ptr;
    con = &list_con;
    for (int64_t i = 0; i < 2 * nt; ++i)
        if (gm_rows[i] < 0 || gm_rows[i] >= h->ncomp) return fail("transport row out of range");
    const size_t pair_words = (2 * (size_t)nt + 15) & ~(size_t)15;
    NODAL_HIP_TRY(h, spec.reserve((2 * pair_words + 16) * 4 + ((size_t)nt * 5 + more_doubles) * 8 + 64));
    gm_dev = spec.as<int32_t>();
    jn_dev = gm_dev + pair_words;
    flag_dev = jn_dev + pair_words;
    is_dev = reinterpret_cast<double *>(flag_dev + 16);
    hist = is_dev + nt;
    gmf = hist + nt;
    gmr = gmf + nt;
    it = gmr + nt;
    *doubles = it + nt;
    std::vector<int32_t> r32(2 * (size_t)nt);
    for (int64_t i = 0; i < 2 * nt; ++i) r32[(size_t)i] = (int32_t)gm_rows[i];
    NODAL_HIP_TRY(h, hipMemcpyAsync(gm_dev, r32.data(), 2 * (size_t)nt * 4, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(jn_dev, junction, 2 * (size_t)nt * 4, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(is_dev, i_s, (size_t)nt * 8, hipMemcpyHostToDevice, st));
    int32_t bad = 0;
    NODAL_HIP_TRY(h, hipMemsetAsync(flag_dev, 0, 8, st));
    k_transport_check<<<groups_of(nt, TTB), TTB, 0, st>>>(nt, D.nd, gm_dev, jn_dev, D.rows_dev, h->type.as<uint8_t>(),
                                                          h->a.as<int32_t>(), h->b.as<int32_t>(), h->c.as<int32_t>(),
                                                          h->d.as<int32_t>(), is_dev, flag_dev);
    NODAL_HIP_TRY(h, hipGetLastError());
    NODAL_TRY(nodal_read_words(h, &bad, flag_dev, 4));  // (waits: the copies above are done too, r32 may end)
    if (bad & 1) return fail("a junction index outside the diodes");
    if (bad & 2) return fail("a transport row that is not a transconductance (GM)");
    if (bad & 4) return fail("the two rows of a transport must share their leads a, b");
    if (bad & 8) return fail("a transport row whose control leads c, d are not its junction's leads");
    if (bad & 16) return fail("i_s must be positive and finite");
    int64_t ncon = 0;
    return grp::build_lists(h, TransportLeads{gm_dev, h->a.as<int32_t>(), h->b.as<int32_t>(), nt}, (int64_t)h->K, &nent, &ncon,
                            list_none, list_node, list_ptr, list_con, nullptr, nullptr);
}

int TransportSet::linearise(nodal_ctx *h, const DiodeSet &D, const double *vh, double *value) const {
    NODAL_HIP_TRY(h, hipMemsetAsync(flag_dev + 1, 0, 4, h->stream));
    k_transport_linearise<<<groups_of(nt, TTB), TTB, 0, h->stream>>>(nt, gm_dev, jn_dev, is_dev, D.nvt_dev, vh, value, hist, gmf,
                                                                     gmr, it, flag_dev + 1);
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

int TransportSet::fill(nodal_ctx *h, double v, double *column) const {
    k_transport_fill<<<groups_of(2 * nt, TTB), TTB, 0, h->stream>>>(nt, gm_dev, v, column);
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

int TransportSet::add_currents(nodal_ctx *h, double *rhs) const {
    return signed_list_add(h, nent, node->as<int32_t>(), ptr->as<int32_t>(), con->as<uint32_t>(), hist, rhs);
}

// ---- one Newton iteration (ctx.h) ----
int newton_iteration(nodal_ctx *h, const DiodeSet &D, TransientSolver &ts, bool dense, bool assemble, bool count_moved,
                     const double *vh_now, double *vh_next, double *rhs, double *xk, unsigned long long *rec, double reltol,
                     double vntol, double abstol, double *iterate_host, double *ms_matrix, double *ms_symbolic, NewtonStep *step,
                     const TransportSet *T) {
    const int64_t n = h->n, nd = D.nd;
    hipStream_t st = h->stream;
    *step = NewtonStep();
    double ms_stamp = 0.0, ms_begin = 0.0, ms_step = 0.0;
    if (assemble) {
        bool overflowed = false;
        NODAL_TRY(D.linearise_and_assemble(h, vh_now, &overflowed, &ms_stamp, T));
        if (overflowed) {
            step->outcome = NEWTON_OVERFLOWED;
            return NODAL_OK;
        }
    } else {  // (the value column gets the bits it holds; J, g_k and i_k are this iteration's)
        NODAL_TRY(D.linearise(h, vh_now, const_cast<double *>(assembled_values(h))));
    }
    NODAL_TRY(D.add_currents(h, rhs));
    if (T) NODAL_TRY(T->add_currents(h, rhs));
    // the route and its matrix work: anew where the matrix moved, kept where numeric_epoch stands
    bool dead = false;
    NODAL_TRY(transient_solver_begin(h, ts, dense, 1, &dead, &ms_begin));
    if (ts.route == TR_ROUTE_LU && ms_begin > 0.0) *ms_symbolic += slu_analysis_ms(h);
    if (dead) {
        *ms_matrix += ms_stamp + ms_begin;
        step->outcome = NEWTON_DEAD;
        return NODAL_OK;
    }
    int32_t inf = 0;
    double resid = 0.0;  // where the solver judged on the host
    NODAL_TRY(transient_solver_step(h, ts, rhs, xk, &inf, &step->it, &resid, &step->judged, &ms_step));
    *ms_matrix += ms_stamp + ms_begin + ms_step;
    if (ts.route == TR_ROUTE_MG && ts.mg_setup && !ts.direct && !sagg_refreshed(h)) *ms_symbolic += ms_step;
    if (inf > 0) {
        step->outcome = NEWTON_SINGULAR;
        return NODAL_OK;
    }
    // (a multigrid step handed on, or a sparse LU step redone: the sparse direct solve)
    step->route = ts.route == TR_ROUTE_DENSE ? 0 : (ts.direct || (ts.route == TR_ROUTE_LU && !step->judged)) ? 3
                  : ts.route == TR_ROUTE_LU ? 1 : 2;
    if (!step->judged) NODAL_HIP_TRY(h, hipMemcpyAsync(rec + 3, ts.norms + 4 * SLU_MULTI, 8, hipMemcpyDeviceToDevice, st));
    if (nd > 0) {
        const auto update = count_moved ? k_newton_update<true> : k_newton_update<false>;
        update<<<groups_of(nd, TTB), TTB, 0, st>>>(nd, D.rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(), D.isat_dev, D.nvt_dev,
                                                  D.gmin, reltol, vntol, abstol, xk, vh_now, D.gk, D.ik, vh_next, rec,
                                                  assembled_values(h));
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    if (T) {
        k_transport_update<<<groups_of(T->nt, TTB), TTB, 0, st>>>(T->nt, T->jn_dev, D.rows_dev, h->a.as<int32_t>(),
                                                                  h->b.as<int32_t>(), T->is_dev, D.nvt_dev, reltol, abstol, xk,
                                                                  vh_now, T->gmf, T->gmr, T->it, rec + NEWTON_REC_TRANSPORTS);
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    if (iterate_host) NODAL_HIP_TRY(h, hipMemcpyAsync(iterate_host, xk, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    NODAL_TRY(nodal_read_words(h, step->words, rec, sizeof step->words));  // (the iteration's one look besides the solver's)
    memcpy(&step->dvmax, &step->words[2], 8);
    memcpy(&step->scaled, &step->words[3], 8);
    if (step->judged) step->scaled = resid;
    step->outcome = !(std::isfinite(step->dvmax) && std::isfinite(step->scaled)) ? NEWTON_NOT_FINITE  // (an iterate that overflowed)
                    : step->words[0] == 0 && step->words[NEWTON_REC_TRANSPORTS] == 0 ? NEWTON_CONVERGED
                                                                                 : NEWTON_GO_ON;
    return NODAL_OK;
}

int newton_run(nodal_ctx *h, bool dense, int64_t nd, const int64_t *diode_rows, const double *isat, const double *nvt,
               double gmin, int32_t nsrc, const double *x0, int32_t max_iter, double reltol, double vntol, double abstol,
               const NewtonOutputs &out, double *ms_matrix, double *ms_symbolic, const NewtonTransports *tr) {
    const int64_t n = h->n, nt = tr ? tr->nt : 0;
    const int rw = out.record_words;
    hipStream_t st = h->stream;
    const double nan = __builtin_nan("");
    *ms_matrix = *ms_symbolic = 0.0;
    *out.iterations = 0;
    *out.converged = 0;
    h->have_x = false;
    h->last_iterations = 0;
    for (int32_t k = 0; k < max_iter; ++k) {
        if (out.info) out.info[k] = 0;
        if (out.iters) out.iters[k] = 0;
        if (out.route) out.route[k] = -1;
        if (out.record)
            for (int q = 0; q < rw; ++q) out.record[(size_t)rw * k + q] = 0.0;
    }

    // ---- once per call: the diodes, the buffers ----
    const bool keep_vh = out.vh != nullptr;
    const size_t vh_slots = keep_vh ? (size_t)max_iter + 1 : 2;
    // tr_spec behind the diodes: v, i, g of the answer [nd] each | the limited voltages [vh_slots][nd] | the records
    // [max_iter][5]
    DiodeSet D;
    int32_t *no_words = nullptr;
    double *ans = nullptr;
    NODAL_TRY(D.prepare(h, "newton: ", nd, diode_rows, isat, nvt, gmin, h->tr_spec, h->tr_none, h->tr_node, h->tr_ptr, h->tr_con, 0,
                        (size_t)nd * (3 + vh_slots) + NEWTON_REC_WORDS * (size_t)max_iter, &no_words, &ans));
    // nb_spec behind the transports: iT, gmf, gmr of the answer [nt] each
    TransportSet TS;
    double *tans = nullptr;
    if (nt > 0 && n > 0)
        NODAL_TRY(TS.prepare(h, "newton: ", D, nt, tr->gm_rows, tr->junction, tr->i_s, h->nb_spec, h->nb_none, h->nb_node,
                             h->nb_ptr, h->nb_con, (size_t)nt * 3, &tans));
    const TransportSet *T = nt > 0 && n > 0 ? &TS : nullptr;
    if (n == 0) {  // (nothing to solve: one iteration that moves nothing)
        *out.iterations = 1;
        *out.converged = 1;
        return NODAL_OK;
    }
    double *vh_dev = ans + 3 * nd;
    unsigned long long *rec_dev = reinterpret_cast<unsigned long long *>(vh_dev + vh_slots * (size_t)nd);
    auto vh_at = [&](int32_t k) { return vh_dev + (keep_vh ? (size_t)k : (size_t)(k & 1)) * (size_t)nd; };
    // tr_vec: the iterate | right-hand side | defect | correction | the judge's norms
    NODAL_HIP_TRY(h, h->tr_vec.reserve((size_t)4 * n * 8 + 5 * SLU_MULTI * 8 + 256));
    double *xk = h->tr_vec.as<double>(), *bvec = xk + n, *rvec = bvec + n, *dvec = rvec + n, *norms = dvec + n;
    if (x0) NODAL_HIP_TRY(h, hipMemcpyAsync(xk, x0, (size_t)n * 8, hipMemcpyHostToDevice, st));
    else NODAL_HIP_TRY(h, hipMemsetAsync(xk, 0, (size_t)n * 8, st));
    NODAL_HIP_TRY(h, hipMemsetAsync(rec_dev, 0, NEWTON_REC_WORDS * (size_t)max_iter * 8, st));
    NODAL_TRY(D.start(h, xk, vh_at(0)));
    NODAL_WAIT_STREAM(h, st);  // (x0 is the caller's)

    // ---- the iterations ----
    bool dead = false, overflow = false;
    int32_t done = 0;
    for (int32_t k = 0; k < max_iter; ++k) {
        NODAL_HIP_TRY(h, hipMemsetAsync(bvec, 0, (size_t)n * 8, st));
        NODAL_TRY(stamp_rhs_multi(h, h->sw_slot.as<int32_t>(), h->sw_vals.as<double>(), nsrc, 1, bvec, 1, 0));
        // the route and its matrix work, anew: the matrix moved (without diodes it does not: what the handle kept serves)
        TransientSolver ts;
        ts.s = h;
        ts.lu_epoch = &h->tr_lu_epoch;
        ts.rvec = rvec;
        ts.dvec = dvec;
        ts.norms = norms;
        NewtonStep s;
        done = k + 1;
        NODAL_TRY(newton_iteration(h, D, ts, dense, nd > 0, false, vh_at(k), vh_at(k + 1), bvec, xk,
                                   rec_dev + NEWTON_REC_WORDS * (size_t)k, reltol, vntol, abstol,
                                   out.iterates ? out.iterates + (size_t)k * n : nullptr, ms_matrix, ms_symbolic, &s, T));
        if (s.outcome == NEWTON_SINGULAR && dense)
            return nodal_fail(h, NODAL_E_SINGULAR, "singular matrix: a zero pivot or a floating sub-network");
        overflow = s.outcome == NEWTON_OVERFLOWED;
        dead = s.outcome == NEWTON_DEAD || s.outcome == NEWTON_SINGULAR;
        if (!s.solved()) break;
        if (out.iters) out.iters[k] = s.it;
        h->last_iterations = s.it;
        if (out.route) out.route[k] = s.route;
        if (out.record) {
            double *row = out.record + (size_t)rw * k;
            row[0] = (double)s.words[0];
            row[1] = (double)s.words[1];
            row[2] = s.dvmax;
            row[3] = s.scaled;
            if (rw > 4) row[4] = (double)s.words[NEWTON_REC_TRANSPORTS];
        }
        if (s.outcome == NEWTON_CONVERGED) *out.converged = 1;
        if (s.outcome != NEWTON_GO_ON) break;
    }
    *out.iterations = done;

    // ---- after the last iteration ----
    const bool lost = dead || overflow;  // no state to report
    if (lost && done >= 1) {
        if (out.info) out.info[done - 1] = dead ? 1 : 0;
        if (out.record)
            for (int q = 0; q < rw; ++q) out.record[(size_t)rw * (done - 1) + q] = nan;
        if (out.iterates)
            for (int64_t i = 0; i < n; ++i) out.iterates[(size_t)(done - 1) * n + i] = nan;
    }
    if (nd > 0 && !lost && (out.v || out.i || out.g)) {
        k_newton_outputs<<<groups_of(nd, TTB), TTB, 0, st>>>(nd, D.rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(), D.isat_dev,
                                                            D.nvt_dev, gmin, xk, ans, ans + nd, ans + 2 * nd);
        NODAL_HIP_TRY(h, hipGetLastError());
        if (out.v) NODAL_HIP_TRY(h, hipMemcpyAsync(out.v, ans, (size_t)nd * 8, hipMemcpyDeviceToHost, st));
        if (out.i) NODAL_HIP_TRY(h, hipMemcpyAsync(out.i, ans + nd, (size_t)nd * 8, hipMemcpyDeviceToHost, st));
        if (out.g) NODAL_HIP_TRY(h, hipMemcpyAsync(out.g, ans + 2 * nd, (size_t)nd * 8, hipMemcpyDeviceToHost, st));
    }
    if (T && !lost && (tr->it || tr->gmf || tr->gmr)) {
        k_transport_outputs<<<groups_of(nt, TTB), TTB, 0, st>>>(nt, T->jn_dev, D.rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(),
                                                                T->is_dev, D.nvt_dev, xk, tans, tans + nt, tans + 2 * nt);
        NODAL_HIP_TRY(h, hipGetLastError());
        if (tr->it) NODAL_HIP_TRY(h, hipMemcpyAsync(tr->it, tans, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
        if (tr->gmf) NODAL_HIP_TRY(h, hipMemcpyAsync(tr->gmf, tans + nt, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
        if (tr->gmr) NODAL_HIP_TRY(h, hipMemcpyAsync(tr->gmr, tans + 2 * nt, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
    }
    if (out.x && !lost) NODAL_HIP_TRY(h, hipMemcpyAsync(out.x, xk, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    // vh_0 .. vh_r, r the iterations whose update ran (a dead or overflowed iteration formed none)
    const int32_t vh_rows = lost ? (done > 0 ? done : 1) : done + 1;
    if (keep_vh && nd > 0) {
        NODAL_HIP_TRY(h, hipMemcpyAsync(out.vh, vh_dev, (size_t)vh_rows * nd * 8, hipMemcpyDeviceToHost, st));
    }
    NODAL_WAIT_STREAM(h, st);
    if (keep_vh)
        for (size_t t = (size_t)vh_rows * nd; t < ((size_t)max_iter + 1) * nd; ++t) out.vh[t] = nan;
    if (lost) {
        if (out.x)
            for (int64_t i = 0; i < n; ++i) out.x[i] = nan;
        for (double *p : {out.v, out.i, out.g})
            if (p)
                for (int64_t d = 0; d < nd; ++d) p[d] = nan;
        if (tr)
            for (double *p : {tr->it, tr->gmf, tr->gmr})
                if (p)
                    for (int64_t t = 0; t < nt; ++t) p[t] = nan;
    }
    return NODAL_OK;
}
