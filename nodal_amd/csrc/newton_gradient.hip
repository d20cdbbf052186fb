// Gradients through the operating point: the adjoint of the Newton solve of newton.hip.
//
// Replaces finite differences over whole Newton runs (two runs per parameter; with the reference each run is itself a
// host loop of rebuild and solve per iteration, reference nodal/nodal.py:306-336), and the host loop of download x, scipy
// transpose solve and numpy formulas.
//
// At the operating point F(x, p) = G(p) x + S i(S^T x; theta) - A(p) = 0, S the [n x nd] incidence of the diodes (+1 at
// the anode, -1 at the cathode, ground dropped), i(v) = i_sat (exp(v / n_vt) - 1) + gmin v.  With c = dL/dx the implicit
// function theorem gives
//     J^T lambda = c,   J = dF/dx = G + S diag(g(v)) S^T  at v = S^T x,   dL/dp = -lambda^T dF/dp
// and J is exactly the matrix nodal_newton_dc assembles, linearised at the answer itself instead of at the last limited
// voltages (those are one step behind: with default tolerances the difference shows in the fourth digit of a gradient).
// So the call is, on the handle's stream, the DiodeSet's lanes (ctx.h; newton.hip's header describes each launch)
//     start, linearise_and_assemble
//                           v = x(a) - x(b) per diode, 1 / g(v) into the value column, J_hist = g v - i(v), G assembled
//     stamp_rhs_multi, add_currents, the block judge on one column
//                           the right-hand side of a Newton iteration at x; because the linearisation is at x the scaled
//                           residual of x against it is the nonlinear KCL defect G x + S i(v) - A: *op_resid_out
//     the solve             transient_solver_begin / transient_solver_step on adjoint_context(h): the handle itself when
//                           B == 0 and the network is passive, the transposed child otherwise; nodal_newton_dc's routes
//     k_gradient_block, k_gradient_cross
//                           every table row's s_i(lambda, x) (table_rows.h), one column
//     k_newton_fill         +0.0 into the companion rows of the result: their table value is the device's own
//     k_opgrad_diodes       one lane per diode, D = lambda(a) - lambda(b), e = exp(v / n_vt):
//                               d/di_sat = -D (e - 1)     d/dn_vt = D i_sat e v / n_vt^2     the gmin term -D v
//                           the gmin terms summed per wavefront and per workgroup in a fixed order
//     k_opgrad_total        the workgroups' partial sums in a fixed order: d/dgmin
//     k_gradient_sources    lambda(a) - lambda(b) of an A row, lambda(K + k) of an E row
// No floating-point atomics: a repeated call gives the same bits.
#include "diode_lanes.h"

#include <cmath>

namespace {

constexpr int OTB = 256;
constexpr int OWAVES = OTB / 64;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // (lane 0 holds the sum)
}

// One lane per diode.  Every product is a statement of its own (the library is built with -ffp-contract=on), and the
// exponential is diode_model's: e = exp(v / n_vt), the current's e - 1.0 -- the derivative of the current the forward
// pass computes.  A diode with both leads on one node gets three zeros.  partials[blockIdx.x]: the workgroup's gmin terms,
// lanes summed per wavefront by shuffles, the wavefronts one after the other.
__global__ __launch_bounds__(OTB) void k_opgrad_diodes(int64_t nd, const int32_t *__restrict__ rows,
                                                       const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                       const double *__restrict__ isat, const double *__restrict__ nvt,
                                                       const double *__restrict__ v, const double *__restrict__ lam,
                                                       double *__restrict__ grad_isat, double *__restrict__ grad_nvt,
                                                       double *__restrict__ partials) {
    __shared__ double red[OWAVES];
    const int64_t d = (int64_t)blockIdx.x * OTB + threadIdx.x;
    double term = 0.0;
    if (d < nd) {
        const int32_t r = rows[d];
        const int32_t ia = a[r], ib = b[r];
        double gs = 0.0, gn = 0.0;
        if (ia != ib) {
            const double D = lead(lam, ia) - lead(lam, ib);
            const double vd = v[d], nv = nvt[d];
            const double e = exp(vd / nv);
            const double em = e - 1.0;
            const double dem = D * em;
            const double ie = isat[d] * e;
            const double die = D * ie;
            const double num = die * vd;
            const double nv2 = nv * nv;
            const double dv = D * vd;
            gs = -dem;
            gn = num / nv2;
            term = -dv;
        }
        grad_isat[d] = gs;
        grad_nvt[d] = gn;
    }
    term = wave_sum(term);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
#pragma unroll
        for (int w = 1; w < OWAVES; ++w) t += red[w];
        partials[blockIdx.x] = t;
    }
}

// The fixed-order second pass (k_power_totals of branch.hip on one column): thread t adds the partials t, t + 256, ... one
// after the other, then the 256 threads are summed as above.
__global__ __launch_bounds__(OTB) void k_opgrad_total(int64_t groups, const double *__restrict__ partials,
                                                      double *__restrict__ out) {
    __shared__ double red[OWAVES];
    double s = 0.0;
    for (int64_t g = threadIdx.x; g < groups; g += OTB) s += partials[g];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
#pragma unroll
        for (int w = 1; w < OWAVES; ++w) t += red[w];
        out[0] = t;
    }
}

void fill(double *p, int64_t count, double v) {
    if (p)
        for (int64_t i = 0; i < count; ++i) p[i] = v;
}

}  // namespace

int newton_gradient_run(nodal_ctx *h, bool dense, int64_t nd, const int64_t *diode_rows, const double *isat, const double *nvt,
                        double gmin, int32_t nsrc, const double *x, const double *cotangent, const NewtonGradientOutputs &out,
                        double *ms_matrix, double *ms_symbolic) {
    const int64_t n = h->n, ncomp = h->ncomp;
    hipStream_t st = h->stream;
    const double nan = __builtin_nan("");
    *ms_matrix = *ms_symbolic = 0.0;
    *out.info = 0;
    fill(out.grad, ncomp, 0.0);
    fill(out.grad_isat, nd, 0.0);
    fill(out.grad_nvt, nd, 0.0);
    fill(out.grad_gmin, 1, 0.0);
    fill(out.grad_sources, nsrc, 0.0);
    fill(out.adjoint, n, 0.0);
    fill(out.resid, 1, 0.0);
    fill(out.op_resid, 1, 0.0);
    h->have_x = false;
    h->last_iterations = 0;
    // ---- the diodes (rows and parameters up, the node list), the buffers ----
    const int64_t groups = groups_of(nd, OTB);
    // tr_spec behind the diodes: v, d/di_sat, d/dn_vt [nd] each | the workgroups' gmin sums | d/dgmin, the operating
    // point's residual, the adjoint solve's
    DiodeSet D;
    int32_t *no_words = nullptr;
    double *v = nullptr;
    NODAL_TRY(D.prepare(h, "operating-point gradient: ", nd, diode_rows, isat, nvt, gmin, h->tr_spec, h->tr_none, h->tr_node,
                        h->tr_ptr, h->tr_con, 0, (size_t)nd * 3 + (size_t)groups + 4, &no_words, &v));
    if (n == 0) return NODAL_OK;  // (every lead is ground: nothing depends on anything)
    double *gis = v + nd, *gnv = gis + nd, *partials = gnv + nd, *words = partials + groups;
    // tr_vec: x | right-hand side | defect | correction | cotangent | lambda | the judge's norms
    NODAL_HIP_TRY(h, h->tr_vec.reserve((size_t)6 * n * 8 + 5 * SLU_MULTI * 8 + 256));
    double *xk = h->tr_vec.as<double>(), *bvec = xk + n, *rvec = bvec + n, *dvec = rvec + n, *cvec = dvec + n, *lam = cvec + n,
           *norms = lam + n;
    // gr_acc: the table rows' terms [ncomp] | the sources' [nsrc]
    const size_t acc_words = ((size_t)ncomp + 1) & ~(size_t)1;
    NODAL_HIP_TRY(h, h->gr_acc.reserve((acc_words + (size_t)nsrc) * 8 + 64));
    double *grad_dev = h->gr_acc.as<double>(), *gsrc_dev = grad_dev + acc_words;
    NODAL_HIP_TRY(h, hipMemcpyAsync(xk, x, (size_t)n * 8, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(cvec, cotangent, (size_t)n * 8, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemsetAsync(words, 0, 3 * 8, st));
    NODAL_HIP_TRY(h, hipMemsetAsync(grad_dev, 0, acc_words * 8, st));
    NODAL_TRY(D.start(h, xk, v));
    NODAL_WAIT_STREAM(h, st);  // (x and the cotangent are the caller's)

    // ---- J at x itself, and what x leaves of the nonlinear equations ----
    double ms_stamp = 0.0, ms_begin = 0.0, ms_step = 0.0;
    bool overflow = false;
    // (without diodes the matrix does not move: what the handle kept of it serves)
    if (nd > 0) NODAL_TRY(D.linearise_and_assemble(h, v, &overflow, &ms_stamp));
    bool dead = false;
    int32_t inf = 0, it = 0;
    double resid = 0.0;
    bool judged = false;  // resid is on the host already
    if (!overflow) {
        NODAL_HIP_TRY(h, hipMemsetAsync(bvec, 0, (size_t)n * 8, st));
        NODAL_TRY(stamp_rhs_multi(h, h->sw_slot.as<int32_t>(), h->sw_vals.as<double>(), nsrc, 1, bvec, 1, 0));
        NODAL_TRY(D.add_currents(h, bvec));
        NODAL_TRY(csr_judge_block(h, xk, bvec, 1, 0, 1, norms));
        NODAL_HIP_TRY(h, hipMemcpyAsync(words + 1, norms + 4 * SLU_MULTI, 8, hipMemcpyDeviceToDevice, st));

        // ---- J^T lambda = c: h's own matrix where it is symmetric, the transposed child otherwise ----
        NODAL_TRY(sens_cross_list(h));
        TransientSolver ts;
        NODAL_TRY(adjoint_context(h, &ts.s));
        ts.lu_epoch = ts.s == h ? &h->tr_lu_epoch : &h->tg_lu_epoch;
        ts.rvec = rvec;
        ts.dvec = dvec;
        ts.norms = norms;
        NODAL_TRY(transient_solver_begin(h, ts, dense, 1, &dead, &ms_begin));
        if (ts.route == TR_ROUTE_LU && ms_begin > 0.0) *ms_symbolic += slu_analysis_ms(ts.s);
        if (!dead) {
            NODAL_TRY(transient_solver_step(h, ts, cvec, lam, &inf, &it, &resid, &judged, &ms_step));
            if (ts.route == TR_ROUTE_MG && ts.mg_setup && !ts.direct && !sagg_refreshed(h)) *ms_symbolic += ms_step;
            if (inf > 0) {
                if (dense) return nodal_fail(h, NODAL_E_SINGULAR, "singular matrix: a zero pivot or a floating sub-network");
                dead = true;
            }
        }
        h->last_iterations = it;
    }
    *ms_matrix = ms_stamp + ms_begin + ms_step;
    const bool lost = dead || overflow;

    // ---- the formulas, and everything comes down once ----
    if (!lost) {
        if (!judged) NODAL_HIP_TRY(h, hipMemcpyAsync(words + 2, norms + 4 * SLU_MULTI, 8, hipMemcpyDeviceToDevice, st));
        if (ncomp > 0) {
            NODAL_TRY(grad_launch_table(h, 1, lam, 1, 0, xk, 1, 0, grad_dev));
            NODAL_TRY(D.fill(h, 0.0, grad_dev));
            NODAL_HIP_TRY(h, hipMemcpyAsync(out.grad, grad_dev, (size_t)ncomp * 8, hipMemcpyDeviceToHost, st));
        }
        if (nd > 0) {
            k_opgrad_diodes<<<(unsigned)groups, OTB, 0, st>>>(nd, D.rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(), D.isat_dev,
                                                             D.nvt_dev, v, lam, gis, gnv, partials);
            k_opgrad_total<<<1, OTB, 0, st>>>(groups, partials, words);
            NODAL_HIP_TRY(h, hipGetLastError());
            if (out.grad_isat) NODAL_HIP_TRY(h, hipMemcpyAsync(out.grad_isat, gis, (size_t)nd * 8, hipMemcpyDeviceToHost, st));
            if (out.grad_nvt) NODAL_HIP_TRY(h, hipMemcpyAsync(out.grad_nvt, gnv, (size_t)nd * 8, hipMemcpyDeviceToHost, st));
        }
        if (nsrc > 0 && out.grad_sources) {
            NODAL_TRY(grad_launch_sources(h, 1, nsrc, h->sw_rows.as<int32_t>(), lam, 1, 0, gsrc_dev));
            NODAL_HIP_TRY(h, hipMemcpyAsync(out.grad_sources, gsrc_dev, (size_t)nsrc * 8, hipMemcpyDeviceToHost, st));
        }
        if (out.adjoint) NODAL_HIP_TRY(h, hipMemcpyAsync(out.adjoint, lam, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    }
    double down[3] = {0.0, 0.0, 0.0};
    NODAL_TRY(nodal_read_words(h, down, words, 24));  // (waits: the copies above are done too)
    if (lost) {
        // a singular J: NaN in everything it feeds; a g that overflowed has no J at all
        *out.info = dead ? 1 : 0;
        fill(out.grad, ncomp, nan);
        fill(out.grad_isat, nd, nan);
        fill(out.grad_nvt, nd, nan);
        fill(out.grad_gmin, 1, nan);
        fill(out.grad_sources, nsrc, nan);
        fill(out.adjoint, n, nan);
        fill(out.resid, 1, nan);
        if (out.op_resid) *out.op_resid = overflow ? nan : down[1];
        return NODAL_OK;
    }
    if (out.grad_gmin) *out.grad_gmin = down[0];
    if (out.op_resid) *out.op_resid = down[1];
    if (out.resid) *out.resid = judged ? resid : down[2];
    return NODAL_OK;
}
