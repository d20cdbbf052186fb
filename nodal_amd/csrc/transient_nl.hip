// Nonlinear transient analysis: diodes in a network stepped in time, Newton's method inside every time step.
//
// Replaces a host loop around nodal_newton_dc that downloads x, rebuilds the history currents in numpy, uploads a value
// column, assembles and solves once per Newton iteration per step.
//
// The handle holds the circuit with one companion R row per capacitor, then per inductor, then per diode.  The steps are
// transient_run's (transient.hip): its right-hand side `base_k` -- the sources in force at t_k plus the capacitors' and
// inductors' history currents -- is formed ONCE per step and held fixed, and where a linear step calls
// transient_solver_step, a step with diodes calls TransientDiodes::step below: on the handle's stream k_newton_start once
// per step (vh^0 = v of x_{k-1}) and then per Newton iteration j a copy rhs = base_k (device to device) and
// newton_iteration (newton.hip, whose header describes each launch) with the update lane's COUNT_MOVED instantiation and
// `assemble` false -- stamp_numeric SKIPPED, with all the matrix work behind it -- when no diode's 1 / g moved (below).
// After convergence transient_run goes on as after a linear solve: the inductor lane (once per step), probes, envelope,
// the ring; then
//     k_tnl_probe           row k of the probed diodes' v and i(v)
// Launches per iteration besides stamp_numeric's and the solver's: three (linearise, list add, update) and one copy; per
// step one more (k_newton_start), one for the diode probes when asked for, and one memset of the record ring every 64
// iterations.
//
// Reuse.  Where every junction is reverse-biased i_sat exp(v / n_vt) / n_vt lies below half an ulp of gmin, g == gmin and
// 1 / g has the bits G was assembled from: the matrix did not move.  The update lane counts the diodes whose next 1 / g
// differs from the value column (record word 4); zero means that the next iteration -- of this step or, when the step
// has converged and no diode was limited, the first of the next, whose vh^0 = v is then that lane's vh' -- launches
// k_newton_linearise (which writes the same bits again) and neither stamp_numeric nor anything behind it:
// numeric_epoch stays, and with it the factors or the hierarchy, as in a linear step.  The first iteration of a call
// always assembles, as does the one after a converged iteration that limited a diode.  NODAL_TNL_REUSE=0 assembles in
// every iteration.
//
// Bipolar transistors (nodal_transient_nl_bjt).  The call's transports are a TransportSet (ctx.h, newton.hip) prepared once
// per call behind the DiodeSet, on buffers of its own (tb_*: the operating point's nb_* may be held by the same handle);
// their two junctions each are plain members of the diodes.  Every iteration hands the set to newton_iteration, which
// runs k_transport_linearise, the second k_signed_list_add and k_transport_update (newton.hip's header); a step has
// converged when no diode and no transport fails.  base_k, k_newton_start and the inductor lane stay once per step.
// After a step, beside k_tnl_probe,
//     k_tnl_transport_probe row k of the probed transports' raw v_f, v_r and of i_f, i_r (the junctions' i(v), gmin
//                           included) and iT at them
// NO reuse with transports: gmf = i_s exp(v_f / n_f) / n_f carries no gmin floor, so its bits move whenever a junction
// voltage moves; a bit-comparison rule would almost never fire and could not be tested deterministically.  A call with
// at least one transport therefore assembles in every Newton iteration (`moved` stays true, updates == iterations), and
// newton_iteration's `assemble == false` branch is never reached with a set.  Without transports nothing changes.
#include "transistor_lanes.h"

#include <cmath>

namespace {

constexpr int REC_RING = 64;  // records zeroed together

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

// One lane per probed transport, kind-agnostic like every transport lane: the raw voltages of its two junction rows at
// x, the junctions' currents by diode_model (with gmin) and iT by transport_model; vout[q][2] = v_f, v_r and
// iout[q][3] = i_f, i_r, iT.  The terminal currents are the caller's sums.
__global__ __launch_bounds__(TTB) void k_tnl_transport_probe(int32_t np, int64_t nt, const int32_t *__restrict__ index,
                                                             const int32_t *__restrict__ jn, const int32_t *__restrict__ rows,
                                                             const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                             const double *__restrict__ isat, const double *__restrict__ nvt,
                                                             const double *__restrict__ is, double gmin,
                                                             const double *__restrict__ x, double *__restrict__ vout,
                                                             double *__restrict__ iout) {
    const int32_t q = blockIdx.x * TTB + threadIdx.x;
    if (q >= np) return;
    const int32_t t = index[q];
    if (t < 0 || t >= nt) return;  // (the entry has refused such a probe)
    const int32_t jf = jn[2 * t], jr = jn[2 * t + 1];
    const int32_t rf = rows[jf], rr = rows[jr];
    const double vf = lead(x, a[rf]) - lead(x, b[rf]);
    const double vr = lead(x, a[rr]) - lead(x, b[rr]);
    double g, i_f, i_r, gmf, gmr, it;
    diode_model(vf, isat[jf], nvt[jf], gmin, &g, &i_f);
    diode_model(vr, isat[jr], nvt[jr], gmin, &g, &i_r);
    transport_model(vf, vr, is[t], nvt[jf], nvt[jr], &gmf, &gmr, &it);
    vout[2 * q] = vf;
    vout[2 * q + 1] = vr;
    iout[3 * q] = i_f;
    iout[3 * q + 1] = i_r;
    iout[3 * q + 2] = it;
}

}  // namespace

int TransientDiodes::prepare(nodal_ctx *h, int32_t steps, const double *x0_dev) {
    reuse = knob::TNL_REUSE.now();
    moved = true;
    slot = 0;
    rec_at = 0;
    ms_matrix = ms_symbolic = 0.0;
    for (int32_t k = 0; k < steps; ++k) {
        if (newton_out) newton_out[k] = 0;
        if (updates_out) updates_out[k] = 0;
    }
    const size_t prow = (size_t)(steps + 1) * ndprobe;
    // tn_spec behind the diodes: the probed diodes (int32) | the limited voltages [2][nd] | the iteration's right-hand
    // side [n] | probed v, i(v) [steps + 1][ndprobe] each | the records [64][5]
    NODAL_TRY(set.prepare(h, "transient: ", nd, rows, isat, nvt, gmin, h->tn_spec, h->tn_none, h->tn_node, h->tn_ptr, h->tn_con,
                          (size_t)ndprobe, (size_t)nd * 2 + (size_t)h->n + 2 * prow + REC_RING * NEWTON_REC_WORDS, &pidx_dev, &vh));
    rhs = vh + 2 * nd;
    pv_dev = rhs + h->n;
    pi_dev = pv_dev + prow;
    rec_dev = reinterpret_cast<unsigned long long *>(pi_dev + prow);
    if (ndprobe > 0)
        NODAL_HIP_TRY(h, hipMemcpyAsync(pidx_dev, dprobe_index, (size_t)ndprobe * 4, hipMemcpyHostToDevice, h->stream));
    if (nt > 0) {
        // tb_spec behind the transports: probed v_f, v_r [steps + 1][ntprobe][2] | probed i_f, i_r, iT
        // [steps + 1][ntprobe][3] | the probed transports (int32)
        const size_t trow = (size_t)(steps + 1) * ntprobe;
        NODAL_TRY(tset.prepare(h, "transient: ", set, nt, gm_rows, junction, i_s, h->tb_spec, h->tb_none, h->tb_node, h->tb_ptr,
                               h->tb_con, 5 * trow + ((size_t)ntprobe + 1) / 2, &tpv_dev));
        tpi_dev = tpv_dev + 2 * trow;
        tpidx_dev = reinterpret_cast<int32_t *>(tpi_dev + 3 * trow);
        if (ntprobe > 0)
            NODAL_HIP_TRY(h, hipMemcpyAsync(tpidx_dev, tprobe_index, (size_t)ntprobe * 4, hipMemcpyHostToDevice, h->stream));
    }
    NODAL_TRY(after_step(h, 0, x0_dev));  // (row 0 of the probes, from x0)
    // (a call without a step reports the start's own junction voltages)
    if (steps == 0) NODAL_TRY(set.start(h, x0_dev, vh));
    return NODAL_OK;
}

// What the step keeps to itself around newton_iteration (newton.hip): base_k copied anew per iteration, the solver that
// persists across iterations and steps, moved / reuse, the ring of records, the step's worst residual and its verdict.
int TransientDiodes::step(nodal_ctx *h, TransientSolver &ts, bool dense, int32_t k, const double *xp, const double *base,
                          double *xk, int32_t *inf_out, int32_t *it_out, double *resid_host, bool *judged_out) {
    hipStream_t st = h->stream;
    *inf_out = 2;  // until an iteration converges
    *it_out = 0;
    NODAL_TRY(set.start(h, xp, vh + (size_t)slot * nd));
    int32_t done = 0, updates = 0;
    double worst = 0.0;  // the largest scaled residual of the step's linear solves: what the step reports
    for (int32_t j = 0; j < max_iter; ++j) {
        double *vh_now = vh + (size_t)slot * nd, *vh_next = vh + (size_t)(slot ^ 1) * nd;
        if (rec_at % REC_RING == 0)  // (every earlier record has been read: each read waits)
            NODAL_HIP_TRY(h, hipMemsetAsync(rec_dev, 0, (size_t)REC_RING * NEWTON_REC_WORDS * 8, st));
        unsigned long long *rec = rec_dev + (size_t)(rec_at++ % REC_RING) * NEWTON_REC_WORDS;
        NODAL_HIP_TRY(h, hipMemcpyAsync(rhs, base, (size_t)h->n * 8, hipMemcpyDeviceToDevice, st));
        const TransportSet *T = transports();
        const bool assemble = moved || !reuse;  // (with transports `moved` stays true: the header comment)
        NewtonStep s;
        done = j + 1;
        NODAL_TRY(newton_iteration(h, set, ts, dense, assemble, true, vh_now, vh_next, rhs, xk, rec, reltol, vntol, abstol, nullptr,
                                   &ms_matrix, &ms_symbolic, &s, T));
        if (s.outcome == NEWTON_OVERFLOWED) {  // (the value column was made legal again)
            moved = true;
            if (T) ++updates;  // (it did assemble: updates == iterations throughout)
            break;
        }
        if (assemble) ++updates;
        if (!s.solved()) {
            *inf_out = 1;
            break;
        }
        *it_out = s.it;
        slot ^= 1;
        worst = s.scaled > worst || std::isnan(s.scaled) ? s.scaled : worst;
        moved = s.words[4] != 0 || s.outcome == NEWTON_NOT_FINITE;
        if (s.outcome == NEWTON_CONVERGED) {
            // the next step linearises at v of this x: the lane's vh' unless the limiter changed it
            if (s.words[1] != 0) moved = true;
            *inf_out = 0;
        }
        if (T) moved = true;
        if (s.outcome != NEWTON_GO_ON) break;
    }
    *resid_host = worst;
    *judged_out = true;  // (on the host already)
    if (newton_out) newton_out[k - 1] = done;
    if (updates_out) updates_out[k - 1] = updates;
    return NODAL_OK;
}

int TransientDiodes::after_step(nodal_ctx *h, int32_t k, const double *xk) {
    if (ndprobe > 0) {
        k_tnl_probe<<<groups_of(ndprobe, TTB), TTB, 0, h->stream>>>(ndprobe, pidx_dev, set.rows_dev, h->a.as<int32_t>(),
                                                                   h->b.as<int32_t>(), set.isat_dev, set.nvt_dev, gmin, xk,
                                                                   pv_dev + (size_t)k * ndprobe, pi_dev + (size_t)k * ndprobe);
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    if (nt > 0 && ntprobe > 0) {
        k_tnl_transport_probe<<<groups_of(ntprobe, TTB), TTB, 0, h->stream>>>(
            ntprobe, nt, tpidx_dev, tset.jn_dev, set.rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(), set.isat_dev, set.nvt_dev,
            tset.is_dev, gmin, xk, tpv_dev + (size_t)k * ntprobe * 2, tpi_dev + (size_t)k * ntprobe * 3);
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    return NODAL_OK;
}

int TransientDiodes::finish(nodal_ctx *h, int32_t steps) {
    hipStream_t st = h->stream;
    const size_t prow = (size_t)(steps + 1) * ndprobe;
    if (dv_out && prow > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(dv_out, pv_dev, prow * 8, hipMemcpyDeviceToHost, st));
    if (di_out && prow > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(di_out, pi_dev, prow * 8, hipMemcpyDeviceToHost, st));
    const size_t trow = nt > 0 ? (size_t)(steps + 1) * ntprobe : 0;
    if (tv_out && trow > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(tv_out, tpv_dev, 2 * trow * 8, hipMemcpyDeviceToHost, st));
    if (ti_out && trow > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(ti_out, tpi_dev, 3 * trow * 8, hipMemcpyDeviceToHost, st));
    // (all nd words, the transistors' junctions among them)
    if (vh_final_out) NODAL_HIP_TRY(h, hipMemcpyAsync(vh_final_out, vh + (size_t)slot * nd, (size_t)nd * 8, hipMemcpyDeviceToHost, st));
    return NODAL_OK;
}

void TransientDiodes::finish_host(int32_t steps, int32_t first_dead) {
    const double nan = __builtin_nan("");
    for (int32_t k = first_dead; k <= steps; ++k)
        for (double *p : {dv_out, di_out})
            if (p)
                for (int32_t q = 0; q < ndprobe; ++q) p[(size_t)k * ndprobe + q] = nan;
    for (int32_t k = first_dead; k <= steps && nt > 0; ++k) {
        if (tv_out)
            for (int32_t q = 0; q < 2 * ntprobe; ++q) tv_out[(size_t)k * ntprobe * 2 + q] = nan;
        if (ti_out)
            for (int32_t q = 0; q < 3 * ntprobe; ++q) ti_out[(size_t)k * ntprobe * 3 + q] = nan;
    }
    if (vh_final_out && first_dead <= steps)
        for (int64_t d = 0; d < nd; ++d) vh_final_out[d] = nan;
}
