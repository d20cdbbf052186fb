// Gradients through time: the adjoint of the backward-Euler transient analysis.
//
// Replaces finite differences over whole transient runs (two runs per component; with the reference each run is itself a
// host loop of rebuild and solve per step, reference nodal/nodal.py:306-336).
//
// Forward (transient.hip), M the handle's G with its companion rows r_i = h / C_i, g = 1 / r, S the [n x ncap] incidence
// of the capacitors (+1 at lead a, -1 at lead b, ground dropped):
//     M x_k = A_k + S (g o S^T x_{k-1}),   k = 1 .. steps
// The loss reads the probe waveforms; the caller hands over w[k][p] = dL / d wave[k][p], k = 0 .. steps, which makes
// c_k = sum_p w[k][p] (e(a_p) - e(b_p)).  Backward, with lambda_{steps+1} = 0:
//     M^T lambda_k = c_k + S (g o S^T lambda_{k+1}),   k = steps .. 1
// -- the forward step with lambda in the role of x, so k_transient_history (method 0) and k_signed_list_add serve
// unchanged, and the solve is the forward run's (transient_solver_step) on h itself when M is symmetric (B == 0 and
// passive: the kept hierarchy or factors serve as they are) and on the child that holds M^T otherwise (factored once,
// kept under tg_lu_epoch).  The results:
//     grad[i]              = sum_k s_i(lambda_k, x_k)                    every row that is not a companion row
//     grad[cap row i]      = sum_k (lambda_k(a) - lambda_k(b)) ((x_k(a) - x_k(b)) - (x_{k-1}(a) - x_{k-1}(b))) / r_i^2
//     grad_sources[k-1][j] = s_{rows[j]}(lambda_k)
//     grad_x0              = c_0 + S (g o S^T lambda_1)
// s_i the per-row formula of table_rows.h (row_term), which the companion rows' history term shares (resistor_term).
// A step is, on the handle's stream,
//     k_signed_list_add     one lane per node with probes: +-w of its probes in list order into the zeroed vector
//     k_transient_history   from lambda_{k+1} (skipped at k == steps: it is zero)
//     k_signed_list_add     the history currents (transient_add_history)
//     the solve, the judgement
// and the finished lambda_k of up to sixteen consecutive steps stay in a [16][n] block, row k - k_lo.  Once per block:
//     k_gradient_block      members y = 0 .. cols - 1 are the steps k_hi - y: lam walks the block backwards (cs = -n), x
//     k_gradient_cross      walks the tape backwards from row k_hi (xcs = -n)
//     k_tgrad_caps          one lane per capacitor: the history term, behind what k_gradient_block left at its row
//     k_gradient_sources    rows k_lo - 1 .. k_hi - 1 of the [steps][nsrc] buffer (the block forwards: no sum, no order)
// so the sum over the steps is one fixed sequence: descending k, block by block, per block the sixteen table terms and
// then the sixteen history terms.  No floating-point atomics, every row has one writer.
#include "group.h"
#include "table_rows.h"

namespace {

constexpr int GTB = 256;
constexpr int GCOLS = 16;  // steps to a block (SLU_MULTI: the width of the table kernels)

// grouping enumerator (group.h): probe p touches node a (slot 0: +w) and node b (slot 1: -w); a probe between a node
// and itself touches nothing.  One column, so a node's probes form ONE entry whose run lists probe << 3 | slot in
// ascending (probe, slot) order
struct ProbeLeads {
    static constexpr int SLOTS = 2;
    const int32_t *a, *b;
    int64_t nitems;
    template <class F>
    __device__ void for_each(int64_t i, F f) const {
        const int ia = a[i], ib = b[i];
        if (ia == ib) return;
        if (ia >= 0) f(0, ia, 0);
        if (ib >= 0) f(1, ib, 0);
    }
};

// One lane per capacitor: the companion row's record is loaded once, then for the steps k = k_hi - y, y = 0 .. cols - 1,
// -(lambda_k(a) - lambda_k(b)) (x_{k-1}(a) - x_{k-1}(b)) / r^2 is added onto grad[row].  lam_hi: lambda_{k_hi}, the
// earlier steps n doubles below each; x_hi: x_{k_hi - 1}, likewise.  The lane is the row's only writer.
__global__ __launch_bounds__(GTB) void k_tgrad_caps(int64_t ncap, int cols, int64_t n, const int32_t *__restrict__ rows,
                                                    const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                    const double *__restrict__ value, const double *__restrict__ lam_hi,
                                                    const double *__restrict__ x_hi, double *__restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (i >= ncap) return;
    const int32_t r = rows[i];
    const RowTerm t = resistor_term(r, value, a, b);
    double acc = grad[r];
    for (int y = 0; y < cols; ++y) {
        const double *lam = lam_hi - (int64_t)y * n, *x = x_hi - (int64_t)y * n;
        const double D = lead(lam, t.j1) - lead(lam, t.j2);
        const double w = (lead(x, t.p1) - lead(x, t.p2)) / t.den;
        acc -= D * w;
    }
    grad[r] = acc;
}

int run(nodal_ctx *h, bool dense, int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b, const double *wave_cot,
        double *grad_out, double *grad_sources_out, double *grad_x0_out, double *adjoint_out, double *resid,
        int32_t *info, double *ms_matrix) {
    const int64_t n = h->n, ncomp = h->ncomp, ncap = h->tape_ncap, nent = h->tape_nent;
    const int32_t K = h->K, steps = h->tape_steps, nsrc = h->tape_nsrc;
    hipStream_t st = h->stream;
    const double nan = __builtin_nan("");

    // ---- once per call: probes and cotangents up, the probes' node lists, the buffers ----
    NODAL_TRY(sens_cross_list(h));
    const size_t probe_words = ((size_t)nprobe + 15) & ~(size_t)15, cot_words = (size_t)(steps + 1) * nprobe;
    NODAL_HIP_TRY(h, h->tg_spec.reserve(2 * probe_words * 4 + 64));
    int32_t *pa_dev = h->tg_spec.as<int32_t>(), *pb_dev = pa_dev + probe_words;
    // tg_vec: sixteen adjoints | the one before them | right-hand side | defect | correction | grad_x0 | norms | history
    NODAL_HIP_TRY(h, h->tg_vec.reserve(((size_t)(GCOLS + 5) * n + 5 * SLU_MULTI + (size_t)ncap) * 8 + 256));
    double *blk = h->tg_vec.as<double>(), *lprev = blk + (size_t)GCOLS * n, *bvec = lprev + n, *rvec = bvec + n,
           *dvec = rvec + n, *gx0 = dvec + n, *norms = gx0 + n, *hist = norms + 5 * SLU_MULTI;
    // tg_out: the sums [ncomp] | source derivatives [steps][nsrc] | residuals [steps] | cotangents [steps + 1][nprobe]
    const size_t acc_words = ((size_t)ncomp + 1) & ~(size_t)1, src_words = (size_t)steps * nsrc;
    NODAL_HIP_TRY(h, h->tg_out.reserve((acc_words + src_words + (size_t)steps + cot_words) * 8 + 64));
    double *grad_dev = h->tg_out.as<double>(), *gsrc_dev = grad_dev + acc_words, *resid_dev = gsrc_dev + src_words,
           *cot_dev = resid_dev + steps;
    NODAL_HIP_TRY(h, hipMemsetAsync(grad_dev, 0, acc_words * 8, st));
    int64_t pent = 0, pcon = 0;  // entries and contributions of the probes' node list
    bool any = false;
    for (int32_t p = 0; p < nprobe; ++p) any = any || (probe_a[p] != probe_b[p]);  // (two distinct leads: one is a node)
    if (any) {
        NODAL_HIP_TRY(h, hipMemcpyAsync(pa_dev, probe_a, (size_t)nprobe * 4, hipMemcpyHostToDevice, st));
        NODAL_HIP_TRY(h, hipMemcpyAsync(pb_dev, probe_b, (size_t)nprobe * 4, hipMemcpyHostToDevice, st));
        NODAL_HIP_TRY(h, hipMemcpyAsync(cot_dev, wave_cot, cot_words * 8, hipMemcpyHostToDevice, st));
        NODAL_TRY(grp::build_lists(h, ProbeLeads{pa_dev, pb_dev, nprobe}, (int64_t)K, &pent, &pcon, h->tg_none, h->tg_node,
                                   h->tg_ptr, h->tg_con, nullptr, nullptr));
    }
    const int32_t *rows_dev = h->tr_spec.as<int32_t>();  // the recorded call's capacitor rows
    const double *tape = h->tr_tape.as<double>();
    const double *value = assembled_values(h);
    // c_k into the zeroed vector, then the history of `next` (null: none)
    auto right_hand_side = [&](int32_t k, const double *next, double *out) -> int {
        NODAL_HIP_TRY(h, hipMemsetAsync(out, 0, (size_t)n * 8, st));
        // (+-w of a node's probes in list order, w row k of the cotangents)
        NODAL_TRY(signed_list_add(h, pent, h->tg_node.as<int32_t>(), h->tg_ptr.as<int32_t>(), h->tg_con.as<uint32_t>(),
                                  cot_dev + (size_t)k * nprobe, out));
        if (next && ncap > 0) NODAL_TRY(transient_add_history(h, ncap, 0, rows_dev, nent, next, hist, out));
        return NODAL_OK;
    };

    // ---- the matrix: h's own where it is symmetric, the transposed child otherwise ----
    TransientSolver ts;
    NODAL_TRY(adjoint_context(h, &ts.s));
    ts.lu_epoch = ts.s == h ? &h->tr_lu_epoch : &h->tg_lu_epoch;
    ts.rvec = rvec;
    ts.dvec = dvec;
    ts.norms = norms;
    bool dead = false;
    NODAL_TRY(transient_solver_begin(h, ts, dense, steps, &dead, ms_matrix));

    // ---- the steps, backwards ----
    int32_t first_dead = dead ? steps : 0;  // the highest step without an adjoint: it and every lower one (0: none)
    std::vector<uint8_t> on_host((size_t)steps, 0);
    // the finished adjoints of steps k_from .. k_to of the block that starts at k_lo: their source derivatives, and down
    auto hand_down = [&](int32_t k_from, int32_t k_to, int32_t k_lo) -> int {
        const int cols = k_to - k_from + 1;
        if (cols <= 0) return NODAL_OK;
        const double *rows = blk + (size_t)(k_from - k_lo) * n;
        if (nsrc > 0 && grad_sources_out)
            NODAL_TRY(grad_launch_sources(h, cols, nsrc, h->tr_tsrc.as<int32_t>(), rows, 1, n,
                                          gsrc_dev + (size_t)(k_from - 1) * nsrc));
        if (adjoint_out) {
            NODAL_HIP_TRY(h, hipMemcpyAsync(adjoint_out + (int64_t)(k_from - 1) * n, rows, (size_t)cols * n * 8,
                                            hipMemcpyDeviceToHost, st));
            NODAL_WAIT_STREAM(h, st);  // (the block is written again by the steps that follow)
        }
        return NODAL_OK;
    };
    for (int32_t k_hi = steps; k_hi >= 1 && first_dead == 0;) {
        const int32_t k_lo = k_hi - GCOLS + 1 > 1 ? k_hi - GCOLS + 1 : 1;
        const int cols = k_hi - k_lo + 1;
        for (int32_t k = k_hi; k >= k_lo; --k) {
            double *lk = blk + (size_t)(k - k_lo) * n;
            const double *next = k == steps ? nullptr : k == k_hi ? lprev : lk + n;
            NODAL_TRY(right_hand_side(k, next, bvec));
            int32_t inf = 0, it = 0;
            bool judged = false;
            NODAL_TRY(transient_solver_step(h, ts, bvec, lk, &inf, &it, &resid[k - 1], &judged, ms_matrix));
            if (inf > 0) {
                if (dense) return nodal_fail(h, NODAL_E_SINGULAR, "singular matrix: a zero pivot or a floating sub-network");
                first_dead = k;
                break;
            }
            on_host[(size_t)k - 1] = judged;
            if (!judged)
                NODAL_HIP_TRY(h, hipMemcpyAsync(resid_dev + (k - 1), norms + 4 * SLU_MULTI, 8, hipMemcpyDeviceToDevice, st));
        }
        if (first_dead > 0) {
            NODAL_TRY(hand_down(first_dead + 1, k_hi, k_lo));
            break;
        }
        if (ncomp > 0) {
            const double *lam_hi = blk + (size_t)(cols - 1) * n;
            NODAL_TRY(grad_launch_table(h, cols, lam_hi, 1, -n, tape + (size_t)k_hi * n, 1, -n, grad_dev));
            if (ncap > 0) {
                k_tgrad_caps<<<groups_of(ncap, GTB), GTB, 0, st>>>(ncap, cols, n, rows_dev, h->a.as<int32_t>(), h->b.as<int32_t>(),
                                                                  value, lam_hi, tape + (size_t)(k_hi - 1) * n, grad_dev);
                NODAL_HIP_TRY(h, hipGetLastError());
            }
        }
        if (k_lo > 1) NODAL_HIP_TRY(h, hipMemcpyAsync(lprev, blk, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
        NODAL_TRY(hand_down(k_lo, k_hi, k_lo));
        k_hi = k_lo - 1;
    }

    // ---- after k = 1: dL/dx_0, and everything comes down once ----
    std::vector<double> resid_dn((size_t)steps);
    if (first_dead == 0) {
        NODAL_TRY(right_hand_side(0, steps > 0 ? blk : nullptr, gx0));  // (the last block starts at k = 1)
        if (grad_x0_out) NODAL_HIP_TRY(h, hipMemcpyAsync(grad_x0_out, gx0, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        if (ncomp > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(grad_out, grad_dev, (size_t)ncomp * 8, hipMemcpyDeviceToHost, st));
    }
    if (src_words > 0 && grad_sources_out)
        NODAL_HIP_TRY(h, hipMemcpyAsync(grad_sources_out, gsrc_dev, src_words * 8, hipMemcpyDeviceToHost, st));
    if (steps > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(resid_dn.data(), resid_dev, (size_t)steps * 8, hipMemcpyDeviceToHost, st));
    NODAL_WAIT_STREAM(h, st);
    for (int32_t k = first_dead + 1; k <= steps; ++k)
        if (!on_host[(size_t)k - 1]) resid[k - 1] = resid_dn[(size_t)k - 1];
    // the steps without an adjoint: info 1, NaN wherever they were to land -- and the sum is not defined without them
    for (int32_t k = 1; k <= first_dead; ++k) {
        info[k - 1] = 1;
        resid[k - 1] = nan;
        if (grad_sources_out)
            for (int32_t j = 0; j < nsrc; ++j) grad_sources_out[(size_t)(k - 1) * nsrc + j] = nan;
        if (adjoint_out)
            for (int64_t i = 0; i < n; ++i) adjoint_out[(int64_t)(k - 1) * n + i] = nan;
    }
    if (first_dead > 0) {
        for (int64_t i = 0; i < ncomp; ++i) grad_out[i] = nan;
        if (grad_x0_out)
            for (int64_t i = 0; i < n; ++i) grad_x0_out[i] = nan;
    }
    return NODAL_OK;
}

}  // namespace

int tgrad_run(nodal_ctx *h, bool dense, int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b,
              const double *wave_cot, double *grad_out, double *grad_sources_out, double *grad_x0_out, double *adjoint_out,
              double *resid_out, int32_t *info_out, double *ms_matrix) {
    const int32_t steps = h->tape_steps;
    *ms_matrix = 0.0;
    for (int32_t p = 0; p < nprobe; ++p)
        if (probe_a[p] < -1 || probe_a[p] >= h->K || probe_b[p] < -1 || probe_b[p] >= h->K)
            return nodal_fail(h, NODAL_E_INVALID, "transient gradient: probe node out of range");
    std::vector<double> resid_own(resid_out ? 0 : (size_t)steps);
    double *resid = resid_out ? resid_out : resid_own.data();
    for (int32_t k = 0; k < steps; ++k) {
        info_out[k] = 0;
        resid[k] = 0.0;
    }
    for (int64_t i = 0; i < h->ncomp; ++i) grad_out[i] = 0.0;
    if (h->n == 0) {  // (every lead is ground: nothing depends on anything)
        if (grad_sources_out)
            for (int64_t t = 0; t < (int64_t)steps * h->tape_nsrc; ++t) grad_sources_out[t] = 0.0;
        return NODAL_OK;
    }
    // the handle is left as it was found: a solution it holds is set aside (the multigrid route writes h->x)
    HandleKeeper keep;
    NODAL_TRY(keep.save(h, h->have_x));
    int status = keep.restore(h, run(h, dense, nprobe, probe_a, probe_b, wave_cot, grad_out, grad_sources_out, grad_x0_out,
                                     adjoint_out, resid, info_out, ms_matrix), "transient gradient");
    const int w = nodal_wait_stream(h, h->stream, NODAL_SITE);
    if (status == NODAL_OK) status = w;
    return status;
}
