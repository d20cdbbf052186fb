// Gradients through frequency: the adjoint of the AC analysis.  The derivative of a real scalar loss of the probe phasors
// with respect to EVERY table value, every capacitance and inductance and every driven amplitude, from one forward and one
// adjoint solve per frequency.
//
// Replaces central differences of nodal_ac_sweep: two sweeps per component, 4 10^6 sweeps on grid(1000).
//
// A(w) = G + j B(w) exactly as ac.hip defines it.  The forward system is A x_f = s, s from the driven rows with amplitudes
// alpha_j, every other independent source off; probe p reads W[f][p] = x_f(a_p) - x_f(b_p).  The caller passes the
// cotangent
//     g[f][p] = dL/dRe W[f][p] + j dL/dIm W[f][p]          so that dL = Re(sum conj(g) dW)
// and nothing else is conjugated anywhere.  The adjoint system is
//     c_f = sum_p conj(g[f][p]) (e(a_p) - e(b_p))            (added in probe order; a_p == b_p adds nothing)
//     A(w_f)^T y_f = c_f                                      (the plain transpose, as noise.hip has it)
// and dL = sum_f Re(y_f^T (ds - dA x_f)).  With X, L the complex x_f, y_f (+0.0 at a ground lead) and D, U the lead
// differences row_term names (table_rows.h, the one statement of leads and denominators; the complex evaluation stands
// next to it there):
//     table row R, value v      Re(D U) / v^2, plus for every CCVS / CCCS row j it drives
//                               Re(L(m_j) v_j (X(c_j) - X(d_j))) / v^2, in table order           (k_acgrad_cross)
//     VCVS (VCCS) row           Re(L(m) U)
//     CCVS, CCCS row            -Re(L(m) U) / Rd
//     A, E row, no term         exactly +0.0: the small-signal excitation never reads the table value
//     capacitor C on (a, b)     w Im(D U)
//     inductor L on (a, b)      Im(D U) / (w L^2)
//     amplitude of driven row j conj(D_j), D_j = L(a) - L(b) for an A row and L(m) for an E row
// The doubled real matrix of A^T is not the transpose of the doubled real matrix of A (that would be the conjugate
// transpose): ac_child(h, true, ...) builds the right one from h->adjoint.  On a symmetric G (no branch rows, every
// R > 0) A^T = A and h->ac serves both solves.
//
// A frequency is, on the handle's stream,
//     k_ac_values       the child's values (ac.hip), of both children when G is not symmetric
//     the solves        ac_block_frequency (ac_ports.hip).  Symmetric G: s and c_f are two columns of one block through
//                       ONE numeric factorisation.  Otherwise one column on h->ac and one on h->ac_t, two factorisations.
//                       The columns are built by k_acgrad_load (s) and k_acgrad_rhs (c_f, one lane walking the probes in
//                       order), and a finished block is copied out by k_acgrad_take into x_f and y_f, 2n each -- the
//                       second solve of a non-symmetric network overwrites the block of the first
//     k_acgrad_probe    row f of the forward phasors
//     k_acgrad_rows     one lane per table row: type, value and leads read once, the term added onto grad[i]
//     k_acgrad_cross    one lane per driving resistor: its group's cross terms added in table order
//     k_acgrad_react    one lane per reactive element, added onto grad_react[q]
//     k_acgrad_sources  one lane per driven row: row f of the source terms
// grad[i] is the sum over the frequencies in ascending index: the lane that owns the row loads, adds and stores.  No
// floating-point atomics anywhere: a repeated call gives the same bits.  Phasors, source terms and residuals come down
// once after the last frequency, the gradients once.  The handle itself -- solution, table, G, A, tape, hierarchy,
// factors, the kept work of the other small-signal analyses -- is only read.
#include "ac_sweep.h"

namespace {

constexpr int GTB = 256;  // lanes of a workgroup: four waves

// column `at` of a zeroed block gets s: element (i, y) at out[i * rs + at]
__global__ __launch_bounds__(GTB) void k_acgrad_load(int64_t n2, const double *__restrict__ s, double *__restrict__ out,
                                                     int64_t rs, int64_t at) {
    const int64_t i = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (i < n2) out[i * rs + at] += s[i];
}

// column `at` of a zeroed block gets c_f: one lane walks the probes in order (P is small, and probes may share a node)
__global__ __launch_bounds__(64) void k_acgrad_rhs(int32_t nprobe, const int32_t *__restrict__ pa, const int32_t *__restrict__ pb,
                                                   const double *__restrict__ cot, double *__restrict__ out, int64_t rs,
                                                   int64_t at) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int32_t p = 0; p < nprobe; ++p) {
        const int32_t a = pa[p], b = pb[p];
        if (a == b) continue;
        const double gr = cot[2 * (int64_t)p], gi = cot[2 * (int64_t)p + 1];  // conj(g) = gr - j gi
        if (a >= 0) {
            out[2 * (int64_t)a * rs + at] += gr;
            out[(2 * (int64_t)a + 1) * rs + at] -= gi;
        }
        if (b >= 0) {
            out[2 * (int64_t)b * rs + at] -= gr;
            out[(2 * (int64_t)b + 1) * rs + at] += gi;
        }
    }
}

// dst[i] = column `at` of a finished block
__global__ __launch_bounds__(GTB) void k_acgrad_take(int64_t n2, const double *__restrict__ x, int64_t rs, int64_t at,
                                                     double *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (i < n2) dst[i] = x[i * rs + at];
}

// out[p] = x(a_p) - x(b_p) as (re, im); a probe between a node and itself reads +0.0 whatever x holds (k_ac_probe's rule)
__global__ __launch_bounds__(GTB) void k_acgrad_probe(int32_t nprobe, const int32_t *__restrict__ pa, const int32_t *__restrict__ pb,
                                                      const double *__restrict__ x, double2 *__restrict__ out) {
    const int32_t p = blockIdx.x * GTB + threadIdx.x;
    if (p >= nprobe) return;
    Phasor w = {0.0, 0.0};
    if (pa[p] != pb[p]) w = phasor_diff(x, pa[p], pb[p]);
    out[p] = make_double2(w.re, w.im);
}

// One lane per table row: the row's term of this frequency onto grad[i].  The row is this lane's alone.
__global__ __launch_bounds__(GTB) void k_acgrad_rows(int64_t ncomp, int32_t K, const uint8_t *__restrict__ type,
                                                     const double *__restrict__ value, const int32_t *__restrict__ a,
                                                     const int32_t *__restrict__ b, const int32_t *__restrict__ c,
                                                     const int32_t *__restrict__ d, const int32_t *__restrict__ drv,
                                                     const int32_t *__restrict__ k, const double *__restrict__ x,
                                                     const double *__restrict__ y, double *__restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (i >= ncomp) return;
    const RowTerm r = row_term(i, K, type, value, a, b, c, d, drv, k);
    const double term = row_term_complex(r, x, y);
    grad[i] = grad[i] + term;
}

// One lane per distinct driving resistor g: the rows of its group rows[gptr[g] .. gptr[g + 1]) in table order, each with a
// statement of its own, onto what k_acgrad_rows left at the driver.
__global__ __launch_bounds__(GTB) void k_acgrad_cross(int64_t ndrivers, int32_t K, const int32_t *__restrict__ drivers,
                                                      const int32_t *__restrict__ gptr, const int32_t *__restrict__ rows,
                                                      const uint8_t *__restrict__ type, const double *__restrict__ value,
                                                      const int32_t *__restrict__ c, const int32_t *__restrict__ d,
                                                      const int32_t *__restrict__ k, const double *__restrict__ x,
                                                      const double *__restrict__ y, double *__restrict__ grad) {
    const int64_t g = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (g >= ndrivers) return;
    const int32_t i = drivers[g];
    if (type[i] != NODAL_T_R) return;  // (the front end admits no other driver; another one has no term)
    const double v = value[i];
    double acc = grad[i];
    for (int32_t q = gptr[g]; q < gptr[g + 1]; ++q) {
        const double term = cross_term_complex(rows[q], K, v, value, c, d, k, y, x);
        acc += term;
    }
    grad[i] = acc;
}

// One lane per reactive element q on (a, b): w Im(D U) for a capacitor, Im(D U) / (w L^2) for an inductor, onto grad[q]
__global__ __launch_bounds__(GTB) void k_acgrad_react(int64_t nreact, double omega, const uint8_t *__restrict__ kind,
                                                      const double *__restrict__ value, const int32_t *__restrict__ a,
                                                      const int32_t *__restrict__ b, const double *__restrict__ x,
                                                      const double *__restrict__ y, double *__restrict__ grad) {
    const int64_t q = (int64_t)blockIdx.x * GTB + threadIdx.x;
    if (q >= nreact) return;
    const int32_t la = a[q], lb = b[q];
    const double im = im_product(phasor_diff(y, la, lb), phasor_diff(x, la, lb));
    const double v = value[q];
    const double term = kind[q] == 0 ? omega * im : im / (omega * v * v);
    grad[q] = grad[q] + term;
}

// One lane per driven row j: conj(D_j) as (re, im), D_j = L(a) - L(b) for an A row, L(m) for an E row
__global__ __launch_bounds__(GTB) void k_acgrad_sources(int32_t nsrc, int32_t K, const int32_t *__restrict__ rows,
                                                        const uint8_t *__restrict__ type, const int32_t *__restrict__ a,
                                                        const int32_t *__restrict__ b, const int32_t *__restrict__ k,
                                                        const double *__restrict__ y, double2 *__restrict__ out) {
    const int32_t j = blockIdx.x * GTB + threadIdx.x;
    if (j >= nsrc) return;
    const int32_t i = rows[j];
    Phasor dj = {0.0, 0.0};
    if (type[i] == NODAL_T_A) dj = phasor_diff(y, a[i], b[i]);
    else if (k[i] >= 0) dj = phasor_diff(y, K + k[i], -1);
    out[j] = make_double2(dj.re, 0.0 - dj.im);
}

// the block loop's client: column `first` + m of the call is the forward system's (0) or the adjoint system's (1); a
// finished column is copied out into x_f or y_f
struct AcGradClient final : MultiRhsClient {
    nodal_ctx *h;
    int64_t n2;
    int first = 0;
    const double *svec = nullptr;  // device, [2n]
    int32_t nprobe = 0;
    const int32_t *pa = nullptr, *pb = nullptr;  // device, [nprobe]
    const double *cot = nullptr;                 // device, the cotangents of the frequency at hand, [nprobe][2]
    double *xk = nullptr, *yk = nullptr;         // device, [2n] each
    AcGradClient(nodal_ctx *h_, int64_t n2_) : h(h_), n2(n2_) {
        wants_rows = false;
        max_cols = 2;
    }
    bool inside(int32_t m0, int cols) const { return cols >= 1 && m0 >= 0 && first + m0 + cols <= 2; }
    int build(int32_t m0, int cols, double *out, int64_t rs, int64_t cs) override {
        if (!inside(m0, cols)) return nodal_fail(h, NODAL_E_INVALID, "ac gradient: a block outside the call's two columns");
        for (int y = 0; y < cols; ++y) {
            const int64_t at = (int64_t)y * cs;
            if (first + m0 + y == 0) k_acgrad_load<<<groups_of(n2, GTB), GTB, 0, h->stream>>>(n2, svec, out, rs, at);
            else k_acgrad_rhs<<<1, 64, 0, h->stream>>>(nprobe, pa, pb, cot, out, rs, at);
        }
        NODAL_HIP_TRY(h, hipGetLastError());
        return NODAL_OK;
    }
    int hand_over(int32_t m0, int cols, const double *x, int64_t rs, int64_t cs, const double *) override {
        if (!inside(m0, cols)) return nodal_fail(h, NODAL_E_INVALID, "ac gradient: a block outside the call's two columns");
        for (int y = 0; y < cols; ++y)
            k_acgrad_take<<<groups_of(n2, GTB), GTB, 0, h->stream>>>(n2, x, rs, (int64_t)y * cs, first + m0 + y == 0 ? xk : yk);
        NODAL_HIP_TRY(h, hipGetLastError());
        return NODAL_OK;
    }
    void all_singular(int32_t) override {}  // (ac_gradient_run fills the frequency's rows from info)
};

}  // namespace

int ac_gradient_run(nodal_ctx *h, bool dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
                    const double *value, const int32_t *lead_a, const int32_t *lead_b, int32_t nsrc, const int64_t *src_rows,
                    const double *src_re, const double *src_im, int32_t nprobe, const int32_t *probe_a,
                    const int32_t *probe_b, const double *wave_cot, double *wave_out, double *grad_out,
                    double *grad_react_out, double *grad_sources_out, int32_t keep_every, double *adjoint_out,
                    double *resid_out, int32_t *info_out, int64_t *work_out, double *ms_analysis, double *ms_factor) {
    const int64_t n = h->n, n2 = 2 * n, ncomp = h->ncomp;
    const int32_t K = h->K;
    hipStream_t st = h->stream;
    const double nan = __builtin_nan("");
    *ms_analysis = *ms_factor = 0.0;
    int64_t work[3] = {0, 0, 0};
    if (work_out) work_out[0] = work_out[1] = work_out[2] = 0;

    // ---- the arguments ----
    NODAL_TRY(ac_check_arguments(h, "ac gradient: ", nfreq, omega, nreact, kind, value, lead_a, lead_b));
    NODAL_TRY(ac_check_pairs(h, "ac gradient: ", "probe node", nprobe, probe_a, probe_b));
    const size_t wave_words = (size_t)nfreq * nprobe * 2, src_words = (size_t)nfreq * nsrc * 2;
    for (size_t t = 0; t < wave_words; ++t)
        if (!(wave_cot[t] - wave_cot[t] == 0.0)) return nodal_fail(h, NODAL_E_INVALID, "ac gradient: a cotangent that is not finite");
    NODAL_TRY(ac_sources_check(h, "ac gradient: ", "source row", nsrc, src_rows, src_re, src_im));  // (waits)

    const int32_t nkeep = (keep_every > 0 && adjoint_out) ? nfreq / keep_every : 0;
    AcLedger ledger(h, nfreq, 2, resid_out, info_out);
    // (what a call without frequencies, probes or unknowns leaves: nothing depends on anything)
    if (grad_out)
        for (int64_t i = 0; i < ncomp; ++i) grad_out[i] = 0.0;
    if (grad_react_out)
        for (int64_t q = 0; q < nreact; ++q) grad_react_out[q] = 0.0;
    if (nfreq == 0 || nprobe == 0 || n == 0) {
        if (wave_out)
            for (size_t t = 0; t < wave_words; ++t) wave_out[t] = 0.0;
        if (grad_sources_out)
            for (size_t t = 0; t < src_words; ++t) grad_sources_out[t] = 0.0;
        for (size_t t = 0; t < (size_t)nkeep * n2; ++t) adjoint_out[t] = 0.0;
        return NODAL_OK;
    }

    // ---- once per call: the children, the elements, probes and cotangents up, the right-hand side, the buffers ----
    nodal_ctx *s = nullptr;
    NODAL_TRY(adjoint_context(h, &s));
    const bool transposed = s != h;  // (G is not symmetric: the adjoint system has a child of its own)
    nodal_ctx *cf = nullptr, *ct = nullptr;
    double ms_f = 0.0, ms_t = 0.0;
    NODAL_TRY(ac_child(h, false, nreact, kind, lead_a, lead_b, &ms_f, &cf));
    if (transposed) NODAL_TRY(ac_child(h, true, nreact, kind, lead_a, lead_b, &ms_t, &ct));
    *ms_analysis = ms_f + ms_t;
    NODAL_TRY(sens_cross_list(h));
    AcSpec spec;  // the elements with their leads; probe a, probe b; the cotangents [nfreq][nprobe][2]
    NODAL_TRY(ac_upload_spec(h, nreact, kind, value, lead_a, lead_b, {{probe_a, (size_t)nprobe}, {probe_b, (size_t)nprobe}}, wave_cot,
                             wave_words, &spec));
    const double *val_dev = spec.value, *cot_dev = spec.extra;
    const uint8_t *kind_dev = spec.kind;
    const int32_t *ea_dev = spec.lead_a, *eb_dev = spec.lead_b, *pa_dev = spec.list[0], *pb_dev = spec.list[1];
    // ag_vec: the forward right-hand side | x_f | y_f (2n each)
    NODAL_HIP_TRY(h, h->ag_vec.reserve((size_t)3 * n2 * 8 + 64));
    double *svec = h->ag_vec.as<double>(), *xk = svec + n2, *yk = xk + n2;
    // ag_out: phasors [nfreq][nprobe][2] | source terms [nfreq][nsrc][2] | residuals [nfreq][2] | grad [ncomp] | grad_react [nreact]
    const size_t out_words = wave_words + src_words + (size_t)2 * nfreq + (size_t)ncomp + (size_t)nreact;
    NODAL_HIP_TRY(h, h->ag_out.reserve(out_words * 8 + 64));
    double *wave_dev = h->ag_out.as<double>(), *gsrc_dev = wave_dev + wave_words, *resid_dev = gsrc_dev + src_words,
           *grad_dev = resid_dev + 2 * (size_t)nfreq, *greact_dev = grad_dev + ncomp;
    ledger.resid_dev = resid_dev;
    NODAL_HIP_TRY(h, hipMemsetAsync(wave_dev, 0, out_words * 8, st));
    NODAL_TRY(ac_sources_stamp(h, nsrc, svec));
    NODAL_WAIT_STREAM(h, st);  // (the elements, probes and cotangents are the caller's)

    AcGradClient client(h, n2);
    client.svec = svec;
    client.nprobe = nprobe;
    client.pa = pa_dev;
    client.pb = pb_dev;
    client.xk = xk;
    client.yk = yk;

    const uint8_t *type_dev = h->type.as<uint8_t>();
    const double *value_dev = assembled_values(h);
    const int32_t *a_dev = h->a.as<int32_t>(), *b_dev = h->b.as<int32_t>(), *c_dev = h->c.as<int32_t>(),
                  *d_dev = h->d.as<int32_t>(), *drv_dev = h->drv.as<int32_t>(), *k_dev = h->k.as<int32_t>();
    const int32_t *rows_dev = h->sw_rows.as<int32_t>();  // (ac_sources_check left the driven rows there)

    // ---- the frequencies ----
    double *resid = ledger.resid;
    uint8_t *on_host = ledger.on_host.data();
    for (int32_t f = 0; f < nfreq; ++f) {
        const double w = omega[f];
        const size_t at = (size_t)2 * f;
        client.cot = cot_dev + (size_t)f * nprobe * 2;
        NODAL_TRY(ac_child_values(h, false, w, kind_dev, val_dev));
        if (transposed) NODAL_TRY(ac_child_values(h, true, w, kind_dev, val_dev));
        bool dead = false;
        client.first = 0;
        if (!transposed) {  // A^T = A: s and c_f through one factorisation
            NODAL_TRY(ac_block_frequency(h, cf, dense, 2, client, resid + at, on_host + at, resid_dev + at, &dead, work,
                                         ms_analysis, ms_factor));
        } else {
            NODAL_TRY(ac_block_frequency(h, cf, dense, 1, client, resid + at, on_host + at, resid_dev + at, &dead, work,
                                         ms_analysis, ms_factor));
            if (!dead) {
                client.first = 1;
                NODAL_TRY(ac_block_frequency(h, ct, dense, 1, client, resid + at + 1, on_host + at + 1, resid_dev + at + 1,
                                             &dead, work, ms_analysis, ms_factor));
            }
        }
        if (dead) {  // (and the sums over the frequencies are void: below)
            ledger.mark_dead(f);
            continue;
        }
        // the table pass on the finished (x_f, y_f)
        k_acgrad_probe<<<groups_of(nprobe, GTB), GTB, 0, st>>>(nprobe, pa_dev, pb_dev, xk,
                                                              reinterpret_cast<double2 *>(wave_dev) + (size_t)f * nprobe);
        if (ncomp > 0)
            k_acgrad_rows<<<groups_of(ncomp, GTB), GTB, 0, st>>>(ncomp, K, type_dev, value_dev, a_dev, b_dev, c_dev, d_dev, drv_dev,
                                                                k_dev, xk, yk, grad_dev);
        if (h->sn_ncross > 0) {
            const int32_t *drivers = h->sn_cross.as<int32_t>(), *gptr = drivers + h->sn_ndrivers, *rows = gptr + h->sn_ndrivers + 1;
            k_acgrad_cross<<<groups_of(h->sn_ndrivers, GTB), GTB, 0, st>>>(h->sn_ndrivers, K, drivers, gptr, rows, type_dev, value_dev,
                                                                          c_dev, d_dev, k_dev, xk, yk, grad_dev);
        }
        if (nreact > 0)
            k_acgrad_react<<<groups_of(nreact, GTB), GTB, 0, st>>>(nreact, w, kind_dev, val_dev, ea_dev, eb_dev, xk, yk, greact_dev);
        if (nsrc > 0)
            k_acgrad_sources<<<groups_of(nsrc, GTB), GTB, 0, st>>>(nsrc, K, rows_dev, type_dev, a_dev, b_dev, k_dev, yk,
                                                                  reinterpret_cast<double2 *>(gsrc_dev) + (size_t)f * nsrc);
        NODAL_HIP_TRY(h, hipGetLastError());
        if (nkeep > 0 && (f + 1) % keep_every == 0) {
            NODAL_HIP_TRY(h, hipMemcpyAsync(adjoint_out + (size_t)((f + 1) / keep_every - 1) * n2, yk, (size_t)n2 * 8,
                                            hipMemcpyDeviceToHost, st));
            NODAL_WAIT_STREAM(h, st);  // (y_f is written again by the frequencies that follow)
        }
    }

    // ---- after the last frequency: everything else comes down once ----
    if (wave_out) NODAL_HIP_TRY(h, hipMemcpyAsync(wave_out, wave_dev, wave_words * 8, hipMemcpyDeviceToHost, st));
    if (grad_sources_out && src_words > 0)
        NODAL_HIP_TRY(h, hipMemcpyAsync(grad_sources_out, gsrc_dev, src_words * 8, hipMemcpyDeviceToHost, st));
    if (grad_out && ncomp > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(grad_out, grad_dev, (size_t)ncomp * 8, hipMemcpyDeviceToHost, st));
    if (grad_react_out && nreact > 0)
        NODAL_HIP_TRY(h, hipMemcpyAsync(grad_react_out, greact_dev, (size_t)nreact * 8, hipMemcpyDeviceToHost, st));
    NODAL_TRY(ledger.finish([&](int32_t f) {
        if (wave_out) std::fill_n(wave_out + (size_t)f * nprobe * 2, 2 * (size_t)nprobe, nan);
        if (grad_sources_out) std::fill_n(grad_sources_out + (size_t)f * nsrc * 2, 2 * (size_t)nsrc, nan);
        if (nkeep > 0 && (f + 1) % keep_every == 0) std::fill_n(adjoint_out + (size_t)((f + 1) / keep_every - 1) * n2, (size_t)n2, nan);
    }));
    if (ledger.any_dead()) {  // (a sum over a list with a hole in it is none: the transient gradient's convention)
        if (grad_out)
            for (int64_t i = 0; i < ncomp; ++i) grad_out[i] = nan;
        if (grad_react_out)
            for (int64_t q = 0; q < nreact; ++q) grad_react_out[q] = nan;
    }
    if (work_out)
        for (int t = 0; t < 3; ++t) work_out[t] = work[t];
    return NODAL_OK;
}
