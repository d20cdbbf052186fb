// Nonlinear transient analysis: diodes in a network stepped in time, Newton's method inside every time step.
//
// Replaces a host loop around nodal_newton_dc that downloads x, rebuilds the history currents in numpy, uploads a value
// column, assembles and solves once per Newton iteration per step.
//
// The handle holds the circuit with one companion R row per capacitor, then per inductor, then per diode.  The steps are
// transient_run's (transient.hip): its right-hand side `base_k` -- the sources in force at t_k plus the capacitors' and
// inductors' history currents -- is formed ONCE per step and held fixed, and where a linear step calls
// transient_solver_step, a step with diodes calls TransientDiodes::step below: on the handle's stream
//     k_newton_start        once per step: vh^0 = v of x_{k-1}                                              (newton.hip)
// and then per Newton iteration j
//     k_newton_linearise    one lane per diode: g, i at vh^j; 1 / g into the value column, J = g vh - i    (newton.hip)
//     stamp_numeric         G from the value column, the symbolic phase kept -- SKIPPED, with all the matrix work behind
//                           it, when no diode's 1 / g moved (below)
//     a copy                rhs = base_k (device to device)
//     k_signed_list_add     one lane per node with diodes: +-J of its diodes in list order, no atomics   (transient.hip)
//     the solve             transient_solver_begin / transient_solver_step, the route chosen as nodal_newton_dc does
//     k_tnl_update          one lane per diode: raw v from the new x, SPICE's junction limiting and the convergence test
//                           (diode_lanes.h, nodal_newton_dc's), then 1 / g of the NEXT linearisation, compared bit for
//                           bit with the value column; into the iteration's record three integer counts (atomicAdd) and
//                           the largest |v - vh| (atomicMax on the bits of a non-negative double): no floating-point
//                           sums, a repeated call gives the same bits
// and ONE read of the record's five words, the scaled residual among them: the host waits of an iteration are those of
// newton_run -- the assembly's status words (when it ran), what the solver looks at, the record.  After convergence
// transient_run goes on as after a linear solve: the inductor lane (once per step), probes, envelope, the ring; then
//     k_tnl_probe           row k of the probed diodes' v and i(v)
// Launches of this file's own per iteration: three (linearise, list add, update) and one copy, besides stamp_numeric's
// and the solver's; per step one more (k_newton_start), one for the diode probes when asked for, and one memset of the
// record ring every 64 iterations.
//
// Reuse.  Where every junction is reverse-biased i_sat exp(v / n_vt) / n_vt lies below half an ulp of gmin, g == gmin and
// 1 / g has the bits G was assembled from: the matrix did not move.  The update lane counts the diodes whose next 1 / g
// differs from the value column (record word 4); zero means that the next iteration -- of this step or, when the step
// has converged and no diode was limited, the first of the next, whose vh^0 = v is then that lane's vh' -- launches
// k_newton_linearise (which writes the same bits again) and neither stamp_numeric nor anything behind it:
// numeric_epoch stays, and with it the factors or the hierarchy, as in a linear step.  The first iteration of a call
// always assembles, as does the one after a converged iteration that limited a diode.  NODAL_TNL_REUSE=0 assembles in
// every iteration.
#include "diode_lanes.h"
#include "group.h"
#include "table_rows.h"

#include <cmath>

namespace {

constexpr int TTB = 256;
constexpr int REC_WORDS = 5;   // failed, limited, bits of max |v - vh|, scaled residual, diodes whose 1 / g moved
constexpr int REC_RING = 64;   // records zeroed together

__global__ __launch_bounds__(TTB) void k_tnl_update(int64_t nd, const int32_t *__restrict__ rows,
                                                    const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                    const double *__restrict__ isat, const double *__restrict__ nvt,
                                                    double gmin, double reltol, double vntol, double abstol,
                                                    const double *__restrict__ x, const double *__restrict__ vh,
                                                    const double *__restrict__ gk, const double *__restrict__ ik,
                                                    const double *__restrict__ value, double *__restrict__ vh_next,
                                                    unsigned long long *__restrict__ rec) {
    const int64_t d = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (d >= nd) return;
    const int32_t r = rows[d];
    const double v = lead(x, a[r]) - lead(x, b[r]);
    const double is = isat[d], nv = nvt[d];
    bool limited, ok;
    double dv;
    const double next = diode_limit_and_test(v, vh[d], is, nv, gmin, reltol, vntol, abstol, gk[d], ik[d], &limited, &ok, &dv);
    vh_next[d] = next;
    double g, i;
    diode_model(next, is, nv, gmin, &g, &i);  // (k_newton_linearise's g at vh': the same statements, the same bits)
    const double inverse = 1.0 / g;
    if (!ok) atomicAdd(rec, 1ull);
    if (limited) atomicAdd(rec + 1, 1ull);
    atomicMax(rec + 2, magnitude_bits(dv));
    if (__double_as_longlong(inverse) != __double_as_longlong(value[r])) atomicAdd(rec + 4, 1ull);
}

// vout[q], iout[q] = v and i(v) of diode index[q] at x
__global__ __launch_bounds__(TTB) void k_tnl_probe(int32_t np, const int32_t *__restrict__ index, const int32_t *__restrict__ rows,
                                                   const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                   const double *__restrict__ isat, const double *__restrict__ nvt, double gmin,
                                                   const double *__restrict__ x, double *__restrict__ vout,
                                                   double *__restrict__ iout) {
    const int32_t q = blockIdx.x * TTB + threadIdx.x;
    if (q >= np) return;
    const int32_t d = index[q], r = rows[d];
    const double v = lead(x, a[r]) - lead(x, b[r]);
    double g, i;
    diode_model(v, isat[d], nvt[d], gmin, &g, &i);
    vout[q] = v;
    iout[q] = i;
}

}  // namespace

int TransientDiodes::prepare(nodal_ctx *h, int32_t steps, const double *x0_dev) {
    const int64_t n = h->n;
    hipStream_t st = h->stream;
    reuse = knob::TNL_REUSE.now();
    moved = true;
    slot = 0;
    rec_at = 0;
    ms_matrix = ms_symbolic = 0.0;
    for (int32_t k = 0; k < steps; ++k) {
        if (newton_out) newton_out[k] = 0;
        if (updates_out) updates_out[k] = 0;
    }
    const size_t row_words = ((size_t)nd + 15) & ~(size_t)15, probe_words = ((size_t)ndprobe + 15) & ~(size_t)15;
    const size_t prow = (size_t)(steps + 1) * ndprobe;
    // tn_spec: diode rows | probed diodes | bad flag (16 words) | i_sat, n_vt, J, g_k, i_k [nd] each | the limited voltages
    // [2][nd] | the iteration's right-hand side [n] | probed v, i(v) [steps + 1][ndprobe] each | the records [64][5]
    NODAL_HIP_TRY(h, h->tn_spec.reserve((row_words + probe_words + 16) * 4 +
                                        ((size_t)nd * 7 + (size_t)n + 2 * prow + REC_RING * REC_WORDS) * 8 + 64));
    rows_dev = h->tn_spec.as<int32_t>();
    pidx_dev = rows_dev + row_words;
    bad_dev = pidx_dev + probe_words;
    isat_dev = reinterpret_cast<double *>(bad_dev + 16);
    nvt_dev = isat_dev + nd;
    hist = nvt_dev + nd;
    gk = hist + nd;
    ik = gk + nd;
    vh = ik + nd;
    rhs = vh + 2 * nd;
    pv_dev = rhs + n;
    pi_dev = pv_dev + prow;
    rec_dev = reinterpret_cast<unsigned long long *>(pi_dev + prow);
    std::vector<int32_t> r32((size_t)nd);
    for (int64_t i = 0; i < nd; ++i) r32[(size_t)i] = (int32_t)rows[i];
    NODAL_HIP_TRY(h, hipMemcpyAsync(rows_dev, r32.data(), (size_t)nd * 4, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(isat_dev, isat, (size_t)nd * 8, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(nvt_dev, nvt, (size_t)nd * 8, hipMemcpyHostToDevice, st));
    if (ndprobe > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(pidx_dev, dprobe_index, (size_t)ndprobe * 4, hipMemcpyHostToDevice, st));
    // (the verdict's wait: the copies above are done too, r32 may end)
    NODAL_TRY(newton_check_diodes(h, nd, rows_dev, isat_dev, nvt_dev, bad_dev, "transient: a diode row that is not a resistor (R)",
                                  "transient: i_sat and n_vt must be positive and finite"));
    int64_t ncon = 0;
    NODAL_TRY(grp::build_lists(h, DiodeLeads{rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(), nd}, (int64_t)h->K, &nent, &ncon,
                               h->tn_none, h->tn_node, h->tn_ptr, h->tn_con, nullptr, nullptr));
    if (ndprobe > 0) {  // row 0, from x0
        k_tnl_probe<<<groups_of(ndprobe, TTB), TTB, 0, st>>>(ndprobe, pidx_dev, rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(),
                                                            isat_dev, nvt_dev, gmin, x0_dev, pv_dev, pi_dev);
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    // (a call without a step reports the start's own junction voltages)
    if (steps == 0) NODAL_TRY(newton_launch_start(h, nd, rows_dev, x0_dev, vh));
    return NODAL_OK;
}

int TransientDiodes::step(nodal_ctx *h, TransientSolver &ts, bool dense, int32_t k, const double *xp, const double *base,
                          double *xk, int32_t *inf_out, int32_t *it_out, double *resid_host, bool *judged_out) {
    const int64_t n = h->n;
    hipStream_t st = h->stream;
    double *value = const_cast<double *>(assembled_values(h));
    *inf_out = 2;  // until an iteration converges
    *it_out = 0;
    *judged_out = false;
    NODAL_TRY(newton_launch_start(h, nd, rows_dev, xp, vh + (size_t)slot * nd));
    int32_t done = 0, updates = 0;
    double worst = 0.0;  // the largest scaled residual of the step's linear solves: what the step reports
    for (int32_t j = 0; j < max_iter; ++j) {
        double *vh_now = vh + (size_t)slot * nd, *vh_next = vh + (size_t)(slot ^ 1) * nd;
        double ms_stamp = 0.0, ms_begin = 0.0, ms_step = 0.0;
        NODAL_TRY(newton_launch_linearise(h, nd, rows_dev, isat_dev, nvt_dev, gmin, vh_now, value, hist, gk, ik));
        done = j + 1;
        if (moved || !reuse) {
            const auto t0 = std::chrono::steady_clock::now();
            const int sn = stamp_numeric(h, h->member, nullptr);
            ms_stamp = ms_since(t0);
            if (sn == NODAL_E_ZERO_RESISTANCE) {  // (g overflowed: 1 / g == 0) the value column is made legal again
                NODAL_TRY(newton_launch_fill(h, nd, rows_dev, 1.0, value));
                NODAL_TRY(stamp_numeric(h, h->member, nullptr));
                moved = true;
                break;
            }
            NODAL_TRY(sn);
            ++updates;
        }
        if (rec_at % REC_RING == 0)  // (every earlier record has been read: each read waits)
            NODAL_HIP_TRY(h, hipMemsetAsync(rec_dev, 0, (size_t)REC_RING * REC_WORDS * 8, st));
        unsigned long long *rec = rec_dev + (size_t)(rec_at++ % REC_RING) * REC_WORDS;
        NODAL_HIP_TRY(h, hipMemcpyAsync(rhs, base, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
        NODAL_TRY(signed_list_add(h, nent, h->tn_node.as<int32_t>(), h->tn_ptr.as<int32_t>(), h->tn_con.as<uint32_t>(), hist, rhs));
        // the route and its matrix work: anew where the matrix moved, kept where numeric_epoch stands
        bool dead = false;
        NODAL_TRY(transient_solver_begin(h, ts, dense, 1, &dead, &ms_begin));
        if (ts.route == TR_ROUTE_LU && ms_begin > 0.0) ms_symbolic += slu_analysis_ms(h);
        if (dead) {
            ms_matrix += ms_stamp + ms_begin;
            *inf_out = 1;
            break;
        }
        int32_t inf = 0, it = 0;
        bool judged = false;
        NODAL_TRY(transient_solver_step(h, ts, rhs, xk, &inf, &it, resid_host, &judged, &ms_step));
        ms_matrix += ms_stamp + ms_begin + ms_step;
        if (ts.route == TR_ROUTE_MG && ts.mg_setup && !ts.direct && !sagg_refreshed(h)) ms_symbolic += ms_step;
        if (inf > 0) {
            *inf_out = 1;
            break;
        }
        *it_out = it;
        if (!judged) NODAL_HIP_TRY(h, hipMemcpyAsync(rec + 3, ts.norms + 4 * SLU_MULTI, 8, hipMemcpyDeviceToDevice, st));
        k_tnl_update<<<groups_of(nd, TTB), TTB, 0, st>>>(nd, rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(), isat_dev, nvt_dev,
                                                        gmin, reltol, vntol, abstol, xk, vh_now, gk, ik, value, vh_next, rec);
        NODAL_HIP_TRY(h, hipGetLastError());
        unsigned long long words[REC_WORDS];
        NODAL_TRY(nodal_read_words(h, words, rec, sizeof words));  // (the iteration's one look besides the solver's)
        slot ^= 1;
        double dvmax, scaled;
        memcpy(&dvmax, &words[2], 8);
        memcpy(&scaled, &words[3], 8);
        if (judged) scaled = *resid_host;
        worst = scaled > worst || std::isnan(scaled) ? scaled : worst;
        moved = words[4] != 0;
        if (!(std::isfinite(dvmax) && std::isfinite(scaled))) {  // (an iterate that overflowed: not converged)
            moved = true;
            break;
        }
        if (words[0] == 0) {
            // the next step linearises at v of this x: the lane's vh' unless the limiter changed it
            if (words[1] != 0) moved = true;
            *inf_out = 0;
            break;
        }
    }
    *resid_host = worst;
    *judged_out = true;  // (on the host already)
    if (newton_out) newton_out[k - 1] = done;
    if (updates_out) updates_out[k - 1] = updates;
    return NODAL_OK;
}

int TransientDiodes::after_step(nodal_ctx *h, int32_t k, const double *xk) {
    if (ndprobe > 0) {
        k_tnl_probe<<<groups_of(ndprobe, TTB), TTB, 0, h->stream>>>(ndprobe, pidx_dev, rows_dev, h->a.as<int32_t>(),
                                                                   h->b.as<int32_t>(), isat_dev, nvt_dev, gmin, xk,
                                                                   pv_dev + (size_t)k * ndprobe, pi_dev + (size_t)k * ndprobe);
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    return NODAL_OK;
}

int TransientDiodes::finish(nodal_ctx *h, int32_t steps) {
    hipStream_t st = h->stream;
    const size_t prow = (size_t)(steps + 1) * ndprobe;
    if (dv_out && prow > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(dv_out, pv_dev, prow * 8, hipMemcpyDeviceToHost, st));
    if (di_out && prow > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(di_out, pi_dev, prow * 8, hipMemcpyDeviceToHost, st));
    if (vh_final_out) NODAL_HIP_TRY(h, hipMemcpyAsync(vh_final_out, vh + (size_t)slot * nd, (size_t)nd * 8, hipMemcpyDeviceToHost, st));
    return NODAL_OK;
}

void TransientDiodes::finish_host(int32_t steps, int32_t first_dead) {
    const double nan = __builtin_nan("");
    for (int32_t k = first_dead; k <= steps; ++k)
        for (double *p : {dv_out, di_out})
            if (p)
                for (int32_t q = 0; q < ndprobe; ++q) p[(size_t)k * ndprobe + q] = nan;
    if (vh_final_out && first_dead <= steps)
        for (int64_t d = 0; d < nd; ++d) vh_final_out[d] = nan;
}
