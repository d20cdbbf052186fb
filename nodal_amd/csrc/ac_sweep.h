// What the four small-signal analyses -- ac.hip, noise.hip, ac_ports.hip, ac_gradient.hip -- share around their loops
// over the frequencies: the child with the matrix, the argument checks, the upload of the call's reactive elements, the
// ledger of residuals and singular frequencies, and the per-frequency block solve.  The functions are defined in ac.hip
// (the child, the checks, the upload) and ac_ports.hip (the block solve).
#pragma once

#include "table_rows.h"

// ---- the child (ac.hip) ----
// `transposed` picks the child: false h->ac, built from h's own pattern and values (G), true h->ac_t, built from
// h->adjoint's (G^T; the caller has brought it up to date) -- B is symmetric, so the stamps are the same.
// the child, its pattern and maps rebuilt when the parent's structure or the reactive leads move; *ms_pattern is written
// only then
int ac_child(nodal_ctx *h, bool transposed, int64_t nreact, const uint8_t *kind, const int32_t *lead_a,
             const int32_t *lead_b, double *ms_pattern, nodal_ctx **child);
// the child's values at omega (k_ac_values) from the device copies of the elements' kinds and values
int ac_child_values(nodal_ctx *h, bool transposed, double omega, const uint8_t *kind_dev, const double *value_dev);

// ---- the arguments (ac.hip) ----
// the arguments that name frequencies and reactive elements; `what` begins the error texts ("ac sweep: ")
int ac_check_arguments(nodal_ctx *h, const char *what, int32_t nfreq, const double *omega, int64_t nreact,
                       const uint8_t *kind, const double *value, const int32_t *lead_a, const int32_t *lead_b);
// every lead of the pairs (a[i], b[i]) is ground (-1) or a node below K, else E_INVALID: `what` + `noun` + " out of range"
int ac_check_pairs(nodal_ctx *h, const char *what, const char *noun, int64_t count, const int32_t *a, const int32_t *b);
// the small-signal right-hand side: the named rows checked and uploaded (waits), then -- every other independent source
// off -- the members (re, im) of the source stamp written interleaved into the zeroed bvec [2n]
int ac_sources_check(nodal_ctx *h, const char *what, const char *row, int32_t nsrc, const int64_t *src_rows, const double *src_re,
                     const double *src_im);
int ac_sources_stamp(nodal_ctx *h, int32_t nsrc, double *bvec);

// ---- the call's reactive elements on the device (ac.hip) ----
// h->ac_spec, every part rounded up to sixteen words:
//     values [nreact] doubles | extra doubles | leads a | leads b (when asked for) | the int32 lists in turn | kinds (bytes)
// Every call uploads anew, so the four analyses share the one buffer.  The copies go values, leads, kinds, extra doubles,
// lists, an empty part none; the caller waits for the stream before its arrays may go.
using AcIntList = std::pair<const int32_t *, size_t>;  // host, count
struct AcSpec {
    double *value = nullptr, *extra = nullptr;
    uint8_t *kind = nullptr;
    int32_t *lead_a = nullptr, *lead_b = nullptr, *list[3] = {nullptr, nullptr, nullptr};
};
// lead_a, lead_b: null for an analysis whose kernels never read the elements' leads.  lists: at most three (probes,
// ports, outputs, probed elements).  extra: the gradient's cotangents.
int ac_upload_spec(nodal_ctx *h, int64_t nreact, const uint8_t *kind, const double *value, const int32_t *lead_a,
                   const int32_t *lead_b, std::initializer_list<AcIntList> lists, const double *extra, size_t nextra,
                   AcSpec *spec);

// peak2[i] = sqrt(peak2[i]), i < K: the peaks are compared as |x|^2 and rooted once, after the last frequency
int ac_peak_root(nodal_ctx *h, int32_t K, double *peak2);

// a numeric factorisation on the child c took ms_f host milliseconds, the symbolic analysis it may have had to do
// included: that part goes to *ms_analysis, the rest to *ms_factor
static inline void ac_add_factor_time(nodal_ctx *c, double ms_f, double *ms_analysis, double *ms_factor) {
    const double ms_a = slu_analysis_ms(c);
    *ms_analysis += ms_a;
    *ms_factor += ms_f > ms_a ? ms_f - ms_a : 0.0;
}

// ---- residuals and singular frequencies ----
// The ONE statement of the convention for a frequency whose matrix is singular (or whose solve fails) inside a sweep:
// that frequency alone is dead -- info[f] = 1, NaN in its residuals and in its rows of every per-frequency output --
// and the frequencies after it are solved as usual.  (What a dead frequency does to a sum over the frequencies is the
// analysis's own business: any_dead().)
// `per` cells per frequency: 1 for the sweep, the outputs of noise, the ports, 2 for the gradient.  A cell's scaled
// residual is either read back during the loop (the sparse LU route: resid[cell] written, on_host[cell] = 1) or copied
// on the device to resid_dev[cell], a strip of the analysis's own output buffer, and comes down in finish().
struct AcLedger {
    nodal_ctx *h;
    int32_t nfreq;
    size_t per;
    std::vector<double> resid_own;
    std::vector<int32_t> info_own;
    std::vector<uint8_t> on_host;
    double *resid;               // host, [nfreq][per]: the caller's, or resid_own
    int32_t *info;               // host, [nfreq]
    double *resid_dev = nullptr;  // device, [nfreq][per]: set by the analysis once its buffer is laid out
    // zeroes info and resid: what a call that returns before its first frequency leaves
    AcLedger(nodal_ctx *h_, int32_t nfreq_, size_t per_, double *resid_out, int32_t *info_out)
        : h(h_), nfreq(nfreq_), per(per_), resid_own(resid_out ? 0 : (size_t)nfreq_ * per_), info_own(info_out ? 0 : (size_t)nfreq_),
          on_host((size_t)nfreq_ * per_, 0), resid(resid_out ? resid_out : resid_own.data()),
          info(info_out ? info_out : info_own.data()) {
        std::fill(info, info + nfreq, 0);
        std::fill(resid, resid + (size_t)nfreq * per, 0.0);
    }
    void mark_dead(int32_t f) { info[f] = 1; }
    bool any_dead() const { return std::find(info, info + nfreq, 1) != info + nfreq; }
    // after the last frequency, behind the analysis's own copies down: the strip comes down, the stream is waited for,
    // and every dead frequency gets NaN residuals and dead_rows(f), which fills the analysis's own rows of f with NaN
    template <class DeadRows>
    int finish(DeadRows &&dead_rows) {
        const size_t cells = (size_t)nfreq * per;
        std::vector<double> down(cells);
        NODAL_HIP_TRY(h, hipMemcpyAsync(down.data(), resid_dev, cells * 8, hipMemcpyDeviceToHost, h->stream));
        NODAL_WAIT_STREAM(h, h->stream);
        for (size_t cell = 0; cell < cells; ++cell) {
            if (info[cell / per] != 0) resid[cell] = __builtin_nan("");
            else if (!on_host[cell]) resid[cell] = down[cell];
        }
        for (int32_t f = 0; f < nfreq; ++f)
            if (info[f] != 0) dead_rows(f);
        return NODAL_OK;
    }
};

// ---- every column of one frequency (ac_ports.hip) ----
// On the child c (2n unknowns) whose values ac_child_values has just written.  client.build adds the right-hand sides of
// columns m0 .. m0 + cols - 1 into a zeroed block, client.hand_over takes the finished ones in groups of at most sixteen
// (never as rows: wants_rows is not looked at; nothing waits), both with element (row, y) at [row * rs + y * cs] -- the
// interleaved block (16, 1), or the rows of the dense and redo routes (1, 2n).  *dead: singular at this frequency,
// whatever was handed over is void.  work [3]: numeric factorisations, applications of the sparse factors to a block,
// columns redone alone -- added to.  Buffers: h->ap_vec, h->ap_rows.
// The dense panel (2n <= 64, or `dense` at any size, which makes a singular matrix an error): the columns are extra
// right-hand sides of one factorisation per 512, built `build_cols` per call of client.build (the sweep's clients take
// sixteen, noise's kernel any number) and judged in groups of sixteen, whose scaled residuals go to resid_dev [count].
int ac_block_dense(nodal_ctx *h, nodal_ctx *c, bool dense, int32_t count, int32_t build_cols, MultiRhsClient &client,
                   double *resid_dev, bool *dead, int64_t *work);
// The whole block loop: the dense panel above where it applies, else the sparse LU factored once and applied to blocks
// of sixteen, which leaves every column's scaled residual at resid_host [count] (on_host[q] = 1).  ms_analysis,
// ms_factor: added to, as ac_run's.
int ac_block_frequency(nodal_ctx *h, nodal_ctx *c, bool dense, int32_t count, MultiRhsClient &client, double *resid_host,
                       uint8_t *on_host, double *resid_dev, bool *dead, int64_t *work, double *ms_analysis, double *ms_factor);
