// Transient analysis: capacitors stepped in time, every step a solve with the SAME matrix.
//
// Replaces a host loop of rebuild and solve per time step (with the reference: a new netlist with companion rows, a new
// `Circuit` and a `.solve()` for every t_k, reference nodal/nodal.py:306-336).
//
// The handle holds the circuit with one extra R row per capacitor, the companion conductance g = C / h (backward Euler)
// or 2 C / h (trapezoidal rule): the table's value of that row is 1 / g, the existing assembly stamped it, and nothing
// about G changes from step to step.  What changes is the right-hand side: the sources' values in force at t_k plus, per
// capacitor, the history current J_k injected into lead a and drawn from lead b,
//     Euler:        J_k = g v_{k-1}
//     trapezoidal:  J_k = 2 g v_{k-1} - J_{k-1},  J_0 = g v_0   (the capacitor currents are zero at t_0: a DC point)
// with v = x(a) - x(b) of the previous solution.  A step is, on the handle's stream,
//     k_transient_history   one lane per capacitor: J_k from x_{k-1}, one state word per capacitor
//     stamp_rhs_multi       the sources of step k into a zeroed vector (one column)
//     k_signed_list_add       one lane per node with capacitors: +-J of its capacitors in list order, no atomics
//     the solve             multigrid (the hierarchy of step 1), sparse LU (factored once) or the dense panel (n <= 64)
//     the judgement         the block judge of multi_rhs_solve on one column
//     k_transient_probe     row k of the waveforms
//     k_transient_envelope  per node compare-and-update with the step index (when asked for)
//     k_transient_inductor  one lane per inductor (nodal_transient_rlc): i_k from x_k, and the history current J_{k+1}
//     k_transient_current_probe  row k of the inductor currents asked for
// and every keep_every-th step one device-to-device copy into a staging ring.  Waveforms, envelope and residuals come
// down once, after the last step.
//
// The solve and its matrix work are transient_solver_begin / transient_solver_step: transient_gradient.hip runs the same
// steps backwards, on this handle or on the child that holds G^T.  With NODAL_OPT_TRANSIENT_TAPE a backward-Euler run
// writes x_k into row k of tr_tape instead of the two alternating vectors and leaves the tape for that sweep.
//
// Inductors (nodal_transient_rlc) are companion R rows too, g = h / L (Euler) or h / (2 L) (trapezoidal), behind the
// capacitors' in the row list, the history array and the node lists, so k_signed_list_add serves both.  What differs is
// the state: the inductor's current i (positive from lead a to lead b through the element),
//     Euler:        i_k = i_{k-1} + g v_k,              J_k = -i_{k-1}
//     trapezoidal:  i_k = i_{k-1} + g (v_k + v_{k-1}),  J_k = -(i_{k-1} + g v_{k-1})
// so that i_k = -J_k + g v_k in both: the lane finishes i_k and forms J_{k+1} from x_k alone, AFTER the solve, where a
// capacitor's lane forms J_k from x_{k-1} before it.
//
// Diodes (nodal_transient_nl) change none of the above: transient_run with a TransientDiodes forms the same right-hand
// side once per step, hands the solve to TransientDiodes::step (transient_nl.hip: Newton's method around
// transient_solver_begin / transient_solver_step) and goes on with the inductor lane, probes, envelope and ring once the
// step has converged.  Without one (nodal_transient, nodal_transient_rlc) the launches are what they were.
#include "group.h"
#include "table_rows.h"


namespace {

constexpr int TTB = 256;
constexpr int RING = 8;  // kept solutions staged on the device before they go down in one copy

// grouping enumerator (group.h): capacitor i touches node a (slot 0: +J) and node b (slot 1: -J); one column, so a
// node's capacitors form ONE entry whose run lists capacitor << 3 | slot in ascending (capacitor, slot) order
struct CapLeads {
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

// bad[0] |= 1 for a capacitor (or inductor) row that is not a resistor
__global__ __launch_bounds__(TTB) void k_transient_check(int64_t ncap, const int32_t *__restrict__ rows,
                                                         const uint8_t *__restrict__ type, int32_t *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (i < ncap && type[rows[i]] != NODAL_T_R) atomicOr(bad, 1);
}

// One lane per capacitor: the history current of the step that follows x.  trapezoidal == 0: J = g v (also the start
// value of the trapezoidal recurrence); else J = 2 g v - J.
__global__ __launch_bounds__(TTB) void k_transient_history(int64_t ncap, int trapezoidal, const int32_t *__restrict__ rows,
                                                           const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                           const double *__restrict__ value, const double *__restrict__ x,
                                                           double *__restrict__ hist) {
    const int64_t i = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (i >= ncap) return;
    const int32_t r = rows[i];
    const double g = 1.0 / value[r];
    const double v = lead(x, a[r]) - lead(x, b[r]);
    hist[i] = trapezoidal ? 2.0 * g * v - hist[i] : g * v;
}

// One lane per inductor, before the first step: the state i_0 and J_1 = -i_0 (Euler) or -(i_0 + g v_0) (trapezoidal).
__global__ __launch_bounds__(TTB) void k_transient_inductor_start(int64_t nind, int trapezoidal, const int32_t *__restrict__ rows,
                                                                  const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                                  const double *__restrict__ value, const double *__restrict__ x0,
                                                                  const double *__restrict__ i0, double *__restrict__ cur,
                                                                  double *__restrict__ hist) {
    const int64_t j = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (j >= nind) return;
    const int32_t r = rows[j];
    const double i = i0[j];
    cur[j] = i;
    const double g = 1.0 / value[r];
    hist[j] = trapezoidal ? -(i + g * (lead(x0, a[r]) - lead(x0, b[r]))) : -i;
}

// One lane per inductor, after the solve of step k: i_k = -J_k + g v_k, then J_{k+1} = -i_k (Euler) or -(i_k + g v_k).
__global__ __launch_bounds__(TTB) void k_transient_inductor(int64_t nind, int trapezoidal, const int32_t *__restrict__ rows,
                                                            const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                            const double *__restrict__ value, const double *__restrict__ x,
                                                            double *__restrict__ cur, double *__restrict__ hist) {
    const int64_t j = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (j >= nind) return;
    const int32_t r = rows[j];
    const double g = 1.0 / value[r];
    const double gv = g * (lead(x, a[r]) - lead(x, b[r]));
    const double i = gv - hist[j];
    cur[j] = i;
    hist[j] = trapezoidal ? -(i + gv) : -i;
}

// out[q] = the current of inductor index[q]
__global__ __launch_bounds__(TTB) void k_transient_current_probe(int32_t ncur, const int32_t *__restrict__ index,
                                                                 const double *__restrict__ cur, double *__restrict__ out) {
    const int32_t q = blockIdx.x * TTB + threadIdx.x;
    if (q < ncur) out[q] = cur[index[q]];
}

// One lane per entry of a group.h node list: out[node] += the signed values of the node's contributions, src[item] for
// slot 0 and -src[item] for any other, in list order -- the +-J of a node's capacitors and then of its inductors, the
// +-w of a node's probes.  The lane is the only writer of its node's row.
__global__ __launch_bounds__(TTB) void k_signed_list_add(int64_t nent, const int32_t *__restrict__ node,
                                                         const int32_t *__restrict__ cptr, const uint32_t *__restrict__ contrib,
                                                         const double *__restrict__ src, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (e >= nent) return;
    const int32_t row = node[e];
    double acc = out[row];
    for (int32_t p = cptr[e]; p < cptr[e + 1]; ++p) {
        const uint32_t u = contrib[p];
        const double v = src[u >> 3];
        acc += (u & 7u) ? -v : v;
    }
    out[row] = acc;
}

// out[p] = x(a_p) - x(b_p); a probe between a node and itself reads +0.0 whatever x holds
__global__ __launch_bounds__(TTB) void k_transient_probe(int32_t nprobe, const int32_t *__restrict__ pa,
                                                         const int32_t *__restrict__ pb, const double *__restrict__ x,
                                                         double *__restrict__ out) {
    const int32_t p = blockIdx.x * TTB + threadIdx.x;
    if (p >= nprobe) return;
    out[p] = pa[p] == pb[p] ? 0.0 : lead(x, pa[p]) - lead(x, pb[p]);
}

// per node: the lowest and highest potential so far and the step that attained it first (strict comparisons: among
// exact ties the lowest step stays).  first: no step has been taken in yet.
__global__ __launch_bounds__(TTB) void k_transient_envelope(int32_t K, int32_t step, int first, const double *__restrict__ x,
                                                            double *__restrict__ pmin, int32_t *__restrict__ pmin_step,
                                                            double *__restrict__ pmax, int32_t *__restrict__ pmax_step) {
    const int32_t i = blockIdx.x * TTB + threadIdx.x;
    if (i >= K) return;
    const double v = x[i];
    if (first || v < pmin[i]) {
        pmin[i] = v;
        pmin_step[i] = step;
    }
    if (first || v > pmax[i]) {
        pmax[i] = v;
        pmax_step[i] = step;
    }
}

// the refinement step of the sparse LU route: r = b - G x, then x += d
__global__ __launch_bounds__(TTB) void k_transient_defect(int64_t n, const int32_t *__restrict__ indptr,
                                                          const int32_t *__restrict__ indices, const double *__restrict__ data,
                                                          const double *__restrict__ x, const double *__restrict__ b,
                                                          double *__restrict__ r) {
    const int64_t i = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (i >= n) return;
    double acc = b[i];
    for (int32_t q = indptr[i]; q < indptr[i + 1]; ++q) acc = fma(-data[q], x[indices[q]], acc);
    r[i] = acc;
}
__global__ __launch_bounds__(TTB) void k_transient_correct(int64_t n, const double *__restrict__ d, double *__restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * TTB + threadIdx.x;
    if (i < n) x[i] += d[i];
}

}  // namespace

int signed_list_add(nodal_ctx *h, int64_t nent, const int32_t *node, const int32_t *cptr, const uint32_t *contrib,
                    const double *src, double *out) {
    if (nent > 0) k_signed_list_add<<<groups_of(nent, TTB), TTB, 0, h->stream>>>(nent, node, cptr, contrib, src, out);
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

int transient_add_history(nodal_ctx *h, int64_t ncap, int method, const int32_t *rows_dev, int64_t nent, const double *x_prev,
                          double *hist, double *rhs) {
    hipStream_t st = h->stream;
    if (ncap > 0)  // (0: inductors alone, whose words of hist are formed after each solve)
        k_transient_history<<<groups_of(ncap, TTB), TTB, 0, st>>>(ncap, method, rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(),
                                                                 assembled_values(h), x_prev, hist);
    return signed_list_add(h, nent, h->tr_node.as<int32_t>(), h->tr_ptr.as<int32_t>(), h->tr_con.as<uint32_t>(), hist, rhs);
}

int transient_solver_begin(nodal_ctx *h, TransientSolver &ts, bool dense, int32_t steps, bool *dead, double *ms_matrix) {
    nodal_ctx *s = ts.s;
    const int64_t n = h->n;
    hipStream_t st = h->stream;  // (s shares it: one ordered timeline)
    const bool passive = s == h && h->B == 0 && h->passive_network;  // (a child holds G^T of a network that is not)
    const int64_t multigrid_min = 4096;  // multi_rhs_solve's bound for passive systems
    ts.route = (n <= 64 || ts.force_dense) ? TR_ROUTE_DENSE : (passive && n > multigrid_min) ? TR_ROUTE_MG : TR_ROUTE_LU;
    ts.direct = ts.all_direct = ts.mg_setup = false;
    ts.first = true;
    ts.bar = knob::MULTI_BAR.now();
    if (ts.route == TR_ROUTE_DENSE) {
        NODAL_HIP_TRY(h, s->dense.reserve((size_t)dense_lda(n) * (size_t)(n + 1) * 8 + 64));
    } else if (ts.route == TR_ROUTE_LU && steps > 0) {
        if (*ts.lu_epoch != h->numeric_epoch || nodal_poison_level() >= 2) {  // (NODAL_POISON=2 poisons the factors)
            const auto t0 = std::chrono::steady_clock::now();
            int32_t inf = 0;
            NODAL_TRY(nodal_lift_error(h, s, slu_factor(s, &inf)));
            NODAL_WAIT_STREAM(h, st);
            *ms_matrix = ms_since(t0);
            if (inf > 0) {
                if (dense) return nodal_fail(h, NODAL_E_SINGULAR, "singular matrix: a zero pivot or a floating sub-network");
                *dead = true;
            } else {
                *ts.lu_epoch = h->numeric_epoch;
            }
        }
        ts.all_direct = !*dead && slu_perturbed(s) > 0;
    } else if (ts.route == TR_ROUTE_MG) {
        ts.mg_setup = !(h->tr_mg_epoch == h->numeric_epoch && sagg_ready(h, n)) || nodal_poison_level() >= 2;
    }
    return NODAL_OK;
}

int transient_solver_step(nodal_ctx *h, TransientSolver &ts, const double *bvec, double *xk, int32_t *inf_out,
                          int32_t *it_out, double *resid_host, bool *judged_out, double *ms_matrix) {
    nodal_ctx *s = ts.s;
    const int64_t n = h->n, lda = dense_lda(n);
    hipStream_t st = h->stream;
    int32_t inf = 0, it = 0;
    double rs = 0.0;
    bool judged = false;  // *resid_host is written already
    if (ts.route == TR_ROUTE_DENSE) {
        // (the tiny matrix is factored anew: a panel launch)
        if (s->csr_only) NODAL_TRY(nodal_lift_error(h, s, csr_to_dense(s, s->dense.as<double>(), lda)));
        else NODAL_TRY(stamp_to_dense(h, h->dense.as<double>(), lda, true));
        NODAL_HIP_TRY(h, hipMemcpyAsync(s->dense.as<double>() + n * lda, bvec, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
        NODAL_TRY(nodal_lift_error(h, s, dense_factor_solve_multi(s, 1, xk, n, &inf)));
    } else if (ts.route == TR_ROUTE_MG) {  // (s == h)
        const auto t0 = std::chrono::steady_clock::now();
        const bool setup = ts.first && ts.mg_setup;
        if (!ts.direct) {
            const int sv = amg_fcg_solve_rhs(h, bvec, setup, &inf, &it, &rs);  // (writes h->x)
            if (sv == -2) {
                inf = 1;  // a floating island: every step is singular
            } else if (sv == NODAL_OK) {
                NODAL_HIP_TRY(h, hipMemcpyAsync(xk, h->x.as<double>(), (size_t)n * 8, hipMemcpyDeviceToDevice, st));
                if (setup) h->tr_mg_epoch = h->numeric_epoch;
            } else if (sv < 0) {
                ts.direct = true;
                h->tr_mg_epoch = 0;  // (the hierarchy was given up and invalidated)
            } else {
                return sv;
            }
        }
        if (ts.direct) NODAL_TRY(sparse_direct_solve(h, bvec, xk, &inf, &it, &rs));
        if (setup) *ms_matrix = ms_since(t0);
    } else {
        bool redo = ts.all_direct;
        if (!ts.all_direct) {
            NODAL_TRY(nodal_lift_error(h, s, slu_apply(s, bvec, xk)));
            k_transient_defect<<<groups_of(n, TTB), TTB, 0, st>>>(n, s->indptr.as<int32_t>(), s->indices.as<int32_t>(),
                                                                 s->data.as<double>(), xk, bvec, ts.rvec);
            NODAL_HIP_TRY(h, hipGetLastError());
            NODAL_TRY(nodal_lift_error(h, s, slu_apply(s, ts.rvec, ts.dvec)));
            k_transient_correct<<<groups_of(n, TTB), TTB, 0, st>>>(n, ts.dvec, xk);
            NODAL_HIP_TRY(h, hipGetLastError());
            NODAL_TRY(nodal_lift_error(h, s, csr_judge_block(s, xk, bvec, 1, 0, 1, ts.norms)));
            NODAL_TRY(nodal_read_words(h, resid_host, ts.norms + 4 * SLU_MULTI, 8));
            judged = true;
            it = 1;
            redo = !(*resid_host <= ts.bar);
        }
        if (redo) {
            judged = false;
            NODAL_TRY(nodal_lift_error(h, s, sparse_direct_solve(s, bvec, xk, &inf, &it, &rs)));
            if (!ts.all_direct && inf == 0) {  // (the direct solve may have factored anew, with another pivot bar)
                int32_t inf2 = 0;
                NODAL_TRY(nodal_lift_error(h, s, slu_factor(s, &inf2)));
                ts.all_direct = inf2 > 0 || slu_perturbed(s) > 0;
                if (ts.all_direct) *ts.lu_epoch = 0;
            }
        }
    }
    ts.first = false;
    *inf_out = inf;
    *it_out = it;
    *judged_out = judged;
    if (inf == 0 && !judged) NODAL_TRY(nodal_lift_error(h, s, csr_judge_block(s, xk, bvec, 1, 0, 1, ts.norms)));
    return NODAL_OK;
}

int transient_run(nodal_ctx *h, bool dense, int32_t steps, int32_t method, int64_t ncap, const int64_t *cap_rows,
                  int32_t nsrc, const double *x0, int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b,
                  double *wave_out, int32_t keep_every, double *x_out, double *pot_min, int32_t *pot_min_step,
                  double *pot_max, int32_t *pot_max_step, double *resid_out, int32_t *info_out, int32_t *iters_out,
                  double *ms_matrix, const TransientInductors *inductors, TransientDiodes *diodes) {
    const int64_t n = h->n;
    const TransientInductors none;
    const TransientInductors &ind = inductors ? *inductors : none;
    const int64_t nind = ind.nind, nitems = ncap + nind;
    const int32_t ncur = ind.ncur;
    const int32_t K = h->K;
    hipStream_t st = h->stream;
    const double nan = __builtin_nan("");
    *ms_matrix = 0.0;
    const bool want_env = pot_min || pot_min_step || pot_max || pot_max_step;
    const int32_t nkeep = (keep_every > 0 && x_out) ? steps / keep_every : 0;
    std::vector<double> resid_own(resid_out ? 0 : (size_t)steps);
    std::vector<int32_t> info_own(info_out ? 0 : (size_t)steps), iters_own(iters_out ? 0 : (size_t)steps);
    double *resid = resid_out ? resid_out : resid_own.data();
    int32_t *info = info_out ? info_out : info_own.data(), *iters = iters_out ? iters_out : iters_own.data();
    for (int32_t k = 0; k < steps; ++k) {
        info[k] = iters[k] = 0;
        resid[k] = 0.0;
    }
    h->have_x = false;
    h->last_iterations = 0;
    // NODAL_OPT_TRANSIENT_TAPE: the states stay on the handle for nodal_transient_gradient (backward Euler only)
    const bool record = h->transient_tape && method == 0 && nind == 0 && !diodes;  // (no adjoint with inductors or diodes: no tape)
    auto keep_tape = [&](int64_t nent_caps) {
        h->tape_valid = true;
        h->tape_epoch = h->numeric_epoch;
        h->tape_steps = steps;
        h->tape_nsrc = nsrc;
        h->tape_ncap = ncap;
        h->tape_nent = nent_caps;
    };
    if (n == 0) {  // (every lead is ground: nothing moves)
        if (nind > 0) return nodal_fail(h, NODAL_E_INVALID, "transient: inductors on a network without nodes");
        if (wave_out)
            for (int64_t t = 0; t < (int64_t)(steps + 1) * nprobe; ++t) wave_out[t] = 0.0;
        if (record) keep_tape(0);
        return NODAL_OK;
    }

    // ---- once per call: capacitor rows and probes up, the node lists, the buffers ----
    for (int64_t i = 0; i < ncap; ++i)
        if (cap_rows[i] < 0 || cap_rows[i] >= h->ncomp) return nodal_fail(h, NODAL_E_INVALID, "transient: capacitor row out of range");
    for (int64_t j = 0; j < nind; ++j)
        if (ind.rows[j] < 0 || ind.rows[j] >= h->ncomp) return nodal_fail(h, NODAL_E_INVALID, "transient: inductor row out of range");
    for (int32_t q = 0; q < ncur; ++q)
        if (ind.cur_index[q] < 0 || ind.cur_index[q] >= nind)
            return nodal_fail(h, NODAL_E_INVALID, "transient: current probe outside the inductors");
    for (int32_t p = 0; p < nprobe; ++p)
        if (probe_a[p] < -1 || probe_a[p] >= K || probe_b[p] < -1 || probe_b[p] >= K)
            return nodal_fail(h, NODAL_E_INVALID, "transient: probe node out of range");
    const size_t cap_words = ((size_t)nitems + 15) & ~(size_t)15, probe_words = ((size_t)nprobe + 15) & ~(size_t)15;
    // tr_spec: cap rows, inductor rows | probe a | probe b | bad flag (16 words) | history [ncap + nind] doubles
    NODAL_HIP_TRY(h, h->tr_spec.reserve((cap_words + 2 * probe_words + 16) * 4 + (size_t)nitems * 8 + 64));
    int32_t *rows_dev = h->tr_spec.as<int32_t>(), *pa_dev = rows_dev + cap_words, *pb_dev = pa_dev + probe_words,
            *bad_dev = pb_dev + probe_words;
    double *hist = reinterpret_cast<double *>(bad_dev + 16);
    int64_t nent = 0, ncon = 0;
    if (nitems > 0) {
        if (K == 0)
            return nodal_fail(h, NODAL_E_INVALID, ncap > 0 ? "transient: capacitors on a network without nodes"
                                                           : "transient: inductors on a network without nodes");
        std::vector<int32_t> r32((size_t)nitems);
        for (int64_t i = 0; i < ncap; ++i) r32[(size_t)i] = (int32_t)cap_rows[i];
        for (int64_t j = 0; j < nind; ++j) r32[(size_t)(ncap + j)] = (int32_t)ind.rows[j];
        NODAL_HIP_TRY(h, hipMemcpyAsync(rows_dev, r32.data(), (size_t)nitems * 4, hipMemcpyHostToDevice, st));
        const struct { int64_t at, count; const char *message; } kinds[2] = {
            {0, ncap, "transient: a capacitor row that is not a resistor (R)"},
            {ncap, nind, "transient: an inductor row that is not a resistor (R)"}};
        for (const auto &kind : kinds) {
            if (kind.count == 0) continue;
            int32_t bad = 0;
            NODAL_HIP_TRY(h, hipMemsetAsync(bad_dev, 0, 4, st));
            k_transient_check<<<groups_of(kind.count, TTB), TTB, 0, st>>>(kind.count, rows_dev + kind.at, h->type.as<uint8_t>(),
                                                                       bad_dev);
            NODAL_HIP_TRY(h, hipGetLastError());
            NODAL_TRY(nodal_read_words(h, &bad, bad_dev, 4));  // (waits: the copy above is done too)
            if (bad) return nodal_fail(h, NODAL_E_INVALID, kind.message);
        }
        NODAL_TRY(grp::build_lists(h, CapLeads{rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(), nitems}, (int64_t)K, &nent,
                                   &ncon, h->tr_none, h->tr_node, h->tr_ptr, h->tr_con, nullptr, nullptr));
    }
    if (nprobe > 0) {
        NODAL_HIP_TRY(h, hipMemcpyAsync(pa_dev, probe_a, (size_t)nprobe * 4, hipMemcpyHostToDevice, st));
        NODAL_HIP_TRY(h, hipMemcpyAsync(pb_dev, probe_b, (size_t)nprobe * 4, hipMemcpyHostToDevice, st));
    }
    // tr_ind: the inductor currents [nind] | i_0 as passed [nind] | current rows [steps + 1][ncur] | probed inductors [ncur]
    const size_t cur_words = (size_t)(steps + 1) * ncur;
    double *icur = nullptr, *i0_dev = nullptr, *cur_dev = nullptr;
    int32_t *cidx_dev = nullptr;
    if (nind > 0) {
        NODAL_HIP_TRY(h, h->tr_ind.reserve((2 * (size_t)nind + cur_words) * 8 + ((size_t)ncur + 16) * 4 + 64));
        icur = h->tr_ind.as<double>();
        i0_dev = icur + nind;
        cur_dev = i0_dev + nind;
        cidx_dev = reinterpret_cast<int32_t *>(cur_dev + cur_words);
        if (ind.i0) NODAL_HIP_TRY(h, hipMemcpyAsync(i0_dev, ind.i0, (size_t)nind * 8, hipMemcpyHostToDevice, st));
        else NODAL_HIP_TRY(h, hipMemsetAsync(i0_dev, 0, (size_t)nind * 8, st));
        if (ncur > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(cidx_dev, ind.cur_index, (size_t)ncur * 4, hipMemcpyHostToDevice, st));
    }
    // tr_vec: two solutions | right-hand side | defect | correction | the judge's norms
    NODAL_HIP_TRY(h, h->tr_vec.reserve((size_t)5 * n * 8 + 5 * SLU_MULTI * 8 + 256));
    double *xv[2] = {h->tr_vec.as<double>(), h->tr_vec.as<double>() + n};
    double *bvec = xv[1] + n, *rvec = bvec + n, *dvec = rvec + n, *norms = dvec + n;
    // recording: x_k is written straight into row k of the tape instead (the same kernels, other addresses), and the
    // swept rows are set aside beside it (sw_rows is the next sweep's)
    double *tape = nullptr;
    if (record) {
        NODAL_HIP_TRY(h, h->tr_tape.reserve((size_t)(steps + 1) * n * 8 + 64));
        tape = h->tr_tape.as<double>();
        NODAL_HIP_TRY(h, h->tr_tsrc.reserve((size_t)(nsrc + 16) * 4));
        if (nsrc > 0)
            NODAL_HIP_TRY(h, hipMemcpyAsync(h->tr_tsrc.p, h->sw_rows.p, (size_t)nsrc * 4, hipMemcpyDeviceToDevice, st));
    }
    auto state = [&](int32_t k) { return tape ? tape + (int64_t)k * n : xv[k & 1]; };
    // tr_out: waveforms [steps + 1][nprobe] | residuals [steps] | envelope min, max [K] each | their steps [K] each
    const size_t wave_words = (size_t)(steps + 1) * nprobe, env_words = want_env ? (size_t)K : 0;
    NODAL_HIP_TRY(h, h->tr_out.reserve((wave_words + (size_t)steps + 3 * env_words + 2) * 8 + 64));
    double *wave_dev = h->tr_out.as<double>(), *resid_dev = wave_dev + wave_words, *pmin_dev = resid_dev + steps,
           *pmax_dev = pmin_dev + env_words;
    int32_t *pmin_step_dev = reinterpret_cast<int32_t *>(pmax_dev + env_words), *pmax_step_dev = pmin_step_dev + env_words;
    if (want_env) NODAL_HIP_TRY(h, hipMemsetAsync(pmin_dev, 0xFF, 3 * env_words * 8, st));  // (NaN and -1 until a step is taken in)
    double *ring = nullptr;
    if (nkeep > 0) {
        NODAL_HIP_TRY(h, h->tr_ring.reserve((size_t)std::min<int32_t>(RING, nkeep) * n * 8 + 64));
        ring = h->tr_ring.as<double>();
    }
    NODAL_HIP_TRY(h, hipMemcpyAsync(state(0), x0, (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (nprobe > 0) {
        k_transient_probe<<<groups_of(nprobe, TTB), TTB, 0, st>>>(nprobe, pa_dev, pb_dev, state(0), wave_dev);
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    const double *value = assembled_values(h);
    if (ncap > 0 && method == 1) {  // J_0 = g v_0
        k_transient_history<<<groups_of(ncap, TTB), TTB, 0, st>>>(ncap, 0, rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(), value,
                                                                 state(0), hist);
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    if (nind > 0) {  // i_0 and J_1, row 0 of the currents
        k_transient_inductor_start<<<groups_of(nind, TTB), TTB, 0, st>>>(nind, method, rows_dev + ncap, h->a.as<int32_t>(),
                                                                        h->b.as<int32_t>(), value, state(0), i0_dev, icur, hist + ncap);
        if (ncur > 0) k_transient_current_probe<<<groups_of(ncur, TTB), TTB, 0, st>>>(ncur, cidx_dev, icur, cur_dev);
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    if (diodes) NODAL_TRY(diodes->prepare(h, steps, state(0)));
    NODAL_WAIT_STREAM(h, st);  // (x0, i0 and the probes are the caller's, r32 ends here)

    // ---- the route and its matrix work ----
    TransientSolver ts;
    ts.s = h;
    ts.lu_epoch = &h->tr_lu_epoch;
    ts.rvec = rvec;
    ts.dvec = dvec;
    ts.norms = norms;
    bool dead = steps == 0;   // a singular verdict: no step from there on has a state to start from
    if (!diodes) NODAL_TRY(transient_solver_begin(h, ts, dense, steps, &dead, ms_matrix));  // (with diodes: every iteration)

    // ---- the steps ----
    int32_t first_dead = dead ? 1 : steps + 1;
    int32_t dead_info = 1;  // what the steps without a state report: 1 singular, 2 Newton's method did not converge
    std::vector<uint8_t> on_host((size_t)steps, 0);  // the step's residual was read back already (the sparse LU route)
    bool env_first = true;
    int32_t ring_fill = 0, ring_base = 0;  // kept solutions in the ring, and the index of the first of them
    auto flush_ring = [&]() -> int {
        if (ring_fill == 0) return NODAL_OK;
        NODAL_HIP_TRY(h, hipMemcpyAsync(x_out + (int64_t)ring_base * n, ring, (size_t)ring_fill * n * 8,
                                        hipMemcpyDeviceToHost, st));
        NODAL_WAIT_STREAM(h, st);  // (the ring is written again by the steps that follow)
        ring_base += ring_fill;
        ring_fill = 0;
        return NODAL_OK;
    };
    for (int32_t k = 1; k <= steps && !dead; ++k) {
        const double *xp = state(k - 1);
        double *xk = state(k);
        // the right-hand side: the sources in force at t_k, then the capacitors' history currents
        NODAL_HIP_TRY(h, hipMemsetAsync(bvec, 0, (size_t)n * 8, st));
        NODAL_TRY(stamp_rhs_multi(h, h->sw_slot.as<int32_t>(), h->sw_vals.as<double>() + (int64_t)(k - 1) * nsrc, nsrc, 1,
                                  bvec, 1, 0));
        if (nitems > 0) NODAL_TRY(transient_add_history(h, ncap, method, rows_dev, nent, xp, hist, bvec));
        // the solve
        int32_t inf = 0, it = 0;
        bool judged = false;  // resid[k - 1] is on the host already
        if (diodes) NODAL_TRY(diodes->step(h, ts, dense, k, xp, bvec, xk, &inf, &it, &resid[k - 1], &judged));
        else NODAL_TRY(transient_solver_step(h, ts, bvec, xk, &inf, &it, &resid[k - 1], &judged, ms_matrix));
        if (inf > 0) {
            if (dense && inf == 1) return nodal_fail(h, NODAL_E_SINGULAR, "singular matrix: a zero pivot or a floating sub-network");
            dead = true;
            first_dead = k;
            dead_info = inf;
            break;
        }
        iters[k - 1] = it;
        h->last_iterations = it;
        on_host[(size_t)k - 1] = judged;
        if (!judged)
            NODAL_HIP_TRY(h, hipMemcpyAsync(resid_dev + (k - 1), norms + 4 * SLU_MULTI, 8, hipMemcpyDeviceToDevice, st));
        if (nind > 0) {  // i_k and J_{k+1}
            k_transient_inductor<<<groups_of(nind, TTB), TTB, 0, st>>>(nind, method, rows_dev + ncap, h->a.as<int32_t>(),
                                                                      h->b.as<int32_t>(), value, xk, icur, hist + ncap);
            if (ncur > 0)
                k_transient_current_probe<<<groups_of(ncur, TTB), TTB, 0, st>>>(ncur, cidx_dev, icur, cur_dev + (size_t)k * ncur);
        }
        // what the caller asked for of x_k
        if (nprobe > 0) k_transient_probe<<<groups_of(nprobe, TTB), TTB, 0, st>>>(nprobe, pa_dev, pb_dev, xk, wave_dev + (size_t)k * nprobe);
        if (want_env && K > 0) {
            k_transient_envelope<<<groups_of(K, TTB), TTB, 0, st>>>(K, k, env_first ? 1 : 0, xk, pmin_dev, pmin_step_dev, pmax_dev,
                                                                   pmax_step_dev);
            env_first = false;
        }
        NODAL_HIP_TRY(h, hipGetLastError());
        if (diodes) NODAL_TRY(diodes->after_step(h, k, xk));
        if (nkeep > 0 && k % keep_every == 0) {
            NODAL_HIP_TRY(h, hipMemcpyAsync(ring + (size_t)ring_fill * n, xk, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
            if (++ring_fill == std::min<int32_t>(RING, nkeep)) NODAL_TRY(flush_ring());
        }
    }
    NODAL_TRY(flush_ring());

    // ---- after the last step: everything else comes down once ----
    std::vector<double> resid_dn((size_t)steps);
    if (wave_out && wave_words > 0)
        NODAL_HIP_TRY(h, hipMemcpyAsync(wave_out, wave_dev, wave_words * 8, hipMemcpyDeviceToHost, st));
    if (ind.cur_out && cur_words > 0)
        NODAL_HIP_TRY(h, hipMemcpyAsync(ind.cur_out, cur_dev, cur_words * 8, hipMemcpyDeviceToHost, st));
    if (ind.i_final_out && nind > 0)
        NODAL_HIP_TRY(h, hipMemcpyAsync(ind.i_final_out, icur, (size_t)nind * 8, hipMemcpyDeviceToHost, st));
    if (steps > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(resid_dn.data(), resid_dev, (size_t)steps * 8, hipMemcpyDeviceToHost, st));
    if (want_env && K > 0) {
        if (pot_min) NODAL_HIP_TRY(h, hipMemcpyAsync(pot_min, pmin_dev, (size_t)K * 8, hipMemcpyDeviceToHost, st));
        if (pot_max) NODAL_HIP_TRY(h, hipMemcpyAsync(pot_max, pmax_dev, (size_t)K * 8, hipMemcpyDeviceToHost, st));
        if (pot_min_step) NODAL_HIP_TRY(h, hipMemcpyAsync(pot_min_step, pmin_step_dev, (size_t)K * 4, hipMemcpyDeviceToHost, st));
        if (pot_max_step) NODAL_HIP_TRY(h, hipMemcpyAsync(pot_max_step, pmax_step_dev, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    }
    if (diodes) NODAL_TRY(diodes->finish(h, steps));
    NODAL_WAIT_STREAM(h, st);
    if (diodes) diodes->finish_host(steps, first_dead);
    for (int32_t k = 1; k < first_dead && k <= steps; ++k)
        if (!on_host[(size_t)k - 1]) resid[k - 1] = resid_dn[(size_t)k - 1];
    // the steps without a state: info 1, NaN wherever they were to land
    for (int32_t k = first_dead; k <= steps; ++k) {
        info[k - 1] = dead_info;
        iters[k - 1] = 0;
        resid[k - 1] = nan;
        if (wave_out)
            for (int32_t p = 0; p < nprobe; ++p) wave_out[(size_t)k * nprobe + p] = nan;
        if (nkeep > 0 && k % keep_every == 0)
            for (int64_t i = 0; i < n; ++i) x_out[(int64_t)(k / keep_every - 1) * n + i] = nan;
        if (ind.cur_out)
            for (int32_t q = 0; q < ncur; ++q) ind.cur_out[(size_t)k * ncur + q] = nan;
    }
    if (ind.i_final_out && first_dead <= steps)
        for (int64_t j = 0; j < nind; ++j) ind.i_final_out[j] = nan;
    if (record && first_dead == steps + 1) keep_tape(nent);
    return NODAL_OK;
}
