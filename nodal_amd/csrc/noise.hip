// Noise analysis: the thermal-noise density at chosen outputs of an RLC network over a list of frequencies, and which
// resistors put it there.
//
// Replaces one AC solve per resistor and frequency (a unit current through the resistor, read at the output): 2 10^6
// solves per frequency on grid(1000).  With A(w) = G + j B(w) exactly as ac.hip defines it, output p = (oa, ob) has the
// adjoint phasor y_p,
//     A(w)^T y_p = e(oa) - e(ob)                       (the plain transpose, nothing is conjugated)
// and a table row k of type R with assembled value R_k > 0 and leads (a, b), a != b, contributes
//     c_k(f, p) = 4 k_B T / R_k |y_p(a) - y_p(b)|^2    V^2 / Hz
// -- every other row exactly +0.0 --, S_out(f, p) = sum_k c_k, and a named input source has the gain H(f, p) = y_p^T s,
// s the right-hand side of the table with that source at amplitude 1 and every other independent source off.  No
// forward solution is needed.
//
// The transposed system: adjoint_context gives the context that holds G^T -- the handle itself when G is symmetric, and
// then A^T = A, so the analysis runs on h->ac and shares its pattern and symbolic analysis with the AC sweep; otherwise
// h->adjoint, from whose pattern and values ac_child builds a second child, h->ac_t (B is symmetric: the same stamps).
// A frequency is, on the handle's stream,
//     k_ac_values     the child's values (ac.hip)
//     the solves      ONE numeric factorisation whatever the number of outputs.  Dense panel (2n <= 64, or `dense` at
//                     any size): ac_block_dense (ac_sweep.h), the outputs are the right-hand-side columns of one
//                     dense_factor_solve_multi, up to 512 at a time, judged in blocks of sixteen.  Otherwise the sparse
//                     LU factored anew on the kept analysis (transient_solver_begin), and per output two substitutions,
//                     one refinement step, the judgement, and the sparse direct solve for an output above the bar
//                     (transient_solver_step)
// and per block of sixteen outputs, whose adjoints lie as rows [16][2n],
//     k_noise_rows    one lane per table row: type, value and leads read once, then the block's outputs in turn: c_k, its
//                     weighted sum onto C_k(p) when contributions are asked for (the row is this lane's alone: a plain
//                     store), and the sum of c_k over the workgroup in a fixed order -- a wave64 shuffle tree, then LDS
//                     across the four waves -- one partial per output and workgroup
//     k_noise_fold    the partials summed in a fixed order into S_out(f, p)
//     k_noise_gain    the products y_p(i) s(i) reduced the same way, folded into H(f, p)
// No floating-point atomics anywhere: a repeated call gives the same bits.  Densities, gains and residuals come down
// once, after the last frequency, the integrated contributions [nout][ncomp] once; the [nfreq][nout][ncomp] array never
// exists.  The handle itself -- solution, table, G, A, tape, hierarchy, factors, the AC child's kept work -- is only read.
#include "ac_sweep.h"

namespace {

constexpr int NTB = 256;            // lanes of a workgroup: four waves
constexpr int NWAVES = NTB / 64;
constexpr int NCOLS = SLU_MULTI;    // outputs of a block
constexpr int DENSE_CHUNK = 512;    // right-hand-side columns of one dense factorisation
constexpr double BOLTZMANN = 1.380649e-23;  // J / K, the exact SI value

// the sum of v over the wave in a fixed order; lane 0 holds it
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// column y of a zeroed block: +1 at the real part of oa, -1 at that of ob, ground dropped (oa == ob: zeros)
__global__ __launch_bounds__(64) void k_noise_rhs(int cols, const int32_t *__restrict__ oa, const int32_t *__restrict__ ob,
                                                  double *__restrict__ out, int64_t cs) {
    const int y = blockIdx.x * 64 + threadIdx.x;
    if (y >= cols) return;
    const int32_t a = oa[y], b = ob[y];
    if (a == b) return;
    if (a >= 0) out[(int64_t)y * cs + 2 * (int64_t)a] = 1.0;
    if (b >= 0) out[(int64_t)y * cs + 2 * (int64_t)b] = -1.0;
}

// One lane per table row.  y: the block's adjoints as rows [cols][n2], interleaved (re, im).  contrib (may be null):
// C_k of the block's first output, rows of ncomp.  part [cols][gridDim.x].
__global__ __launch_bounds__(NTB) void k_noise_rows(int64_t ncomp, int cols, const uint8_t *__restrict__ type,
                                                    const double *__restrict__ value, const int32_t *__restrict__ a,
                                                    const int32_t *__restrict__ b, const double *__restrict__ y, int64_t n2,
                                                    double kt4, double weight, double *__restrict__ contrib,
                                                    double *__restrict__ part) {
    __shared__ double red[NCOLS][NWAVES];
    const int64_t i = (int64_t)blockIdx.x * NTB + threadIdx.x;
    const bool in = i < ncomp;
    int32_t la = -1, lb = -1;
    double scale = 0.0;
    bool noisy = false;
    if (in && type[i] == NODAL_T_R) {
        const double r = value[i];
        la = a[i];
        lb = b[i];
        noisy = r > 0.0 && la != lb;
        if (noisy) scale = kt4 / r;
    }
    for (int c = 0; c < cols; ++c) {
        double ck = 0.0;
        if (noisy) {
            const double *yc = y + (int64_t)c * n2;
            const double re = lead(yc, la, 2, 0) - lead(yc, lb, 2, 0), im = lead(yc, la, 2, 1) - lead(yc, lb, 2, 1);
            const double m = re * re + im * im;
            ck = scale * m;
        }
        if (contrib && in) {
            double *at = contrib + (int64_t)c * ncomp + i;
            *at = *at + weight * ck;
        }
        const double s = wave_sum(ck);
        if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < cols) {
        double s = red[threadIdx.x][0];
        for (int w = 1; w < NWAVES; ++w) s += red[threadIdx.x][w];
        part[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = s;
    }
}

// One lane per unknown: (y_c(i) s(i)) as (re, im), reduced like k_noise_rows.  part [cols][2][gridDim.x].
__global__ __launch_bounds__(NTB) void k_noise_gain(int64_t n, int cols, const double *__restrict__ y, int64_t n2,
                                                    const double *__restrict__ s, double *__restrict__ part) {
    __shared__ double red[2 * NCOLS][NWAVES];
    const int64_t i = (int64_t)blockIdx.x * NTB + threadIdx.x;
    double sr = 0.0, si = 0.0;
    if (i < n) {
        sr = s[2 * i];
        si = s[2 * i + 1];
    }
    const bool live = sr != 0.0 || si != 0.0;  // (s has a few entries: the others read nothing of y)
    for (int c = 0; c < cols; ++c) {
        double pr = 0.0, pi = 0.0;
        if (live) {
            const double yr = y[(int64_t)c * n2 + 2 * i], yi = y[(int64_t)c * n2 + 2 * i + 1];
            pr = yr * sr - yi * si;
            pi = yr * si + yi * sr;
        }
        const double tr = wave_sum(pr), ti = wave_sum(pi);
        if ((threadIdx.x & 63) == 0) {
            red[2 * c][threadIdx.x >> 6] = tr;
            red[2 * c + 1][threadIdx.x >> 6] = ti;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * cols) {
        double t = red[threadIdx.x][0];
        for (int w = 1; w < NWAVES; ++w) t += red[threadIdx.x][w];
        part[(int64_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

// out[t] = the sum of part[t][0 .. ngroups) in a fixed order: one wave per t, lane l takes l, l + 64, ..., then the tree
__global__ __launch_bounds__(64) void k_noise_fold(int64_t ngroups, const double *__restrict__ part, double *__restrict__ out) {
    const double *p = part + (int64_t)blockIdx.x * ngroups;
    double acc = 0.0;
    for (int64_t g = threadIdx.x; g < ngroups; g += 64) acc += p[g];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// the block loop's client: the columns are the outputs' unit differences, a finished block of up to sixteen adjoints
// goes through the table pass, the fold and the gain of frequency f
struct NoiseClient final : MultiRhsClient {
    nodal_ctx *h;
    int64_t n, ncomp;
    int32_t nout, f = 0;  // the frequency at hand
    const int32_t *oa, *ob;  // device, [nout]
    double kt4;
    const double *weight = nullptr;  // host, [nfreq]; null: no contributions
    const double *svec = nullptr;    // device, the input's right-hand side [2n]; null: no gains
    double *part, *dens, *gain, *contrib;  // device: the partial sums, [nfreq][nout], [nfreq][nout][2], [nout][ncomp]
    NoiseClient(nodal_ctx *h_, int32_t nout_, const int32_t *oa_, const int32_t *ob_)
        : h(h_), n(h_->n), ncomp(h_->ncomp), nout(nout_), oa(oa_), ob(ob_) {
        wants_rows = false;
        max_cols = NCOLS;
    }
    // (k_noise_rhs writes rows: column y at out + y * cs, any number of them)
    int build(int32_t m0, int cols, double *out, int64_t rs, int64_t cs) override {
        if (cols < 1 || m0 < 0 || m0 + cols > nout || rs != 1)
            return nodal_fail(h, NODAL_E_INVALID, "noise: a block outside the call's columns");
        k_noise_rhs<<<groups_of(cols, 64), 64, 0, h->stream>>>(cols, oa + m0, ob + m0, out, cs);
        NODAL_HIP_TRY(h, hipGetLastError());
        return NODAL_OK;
    }
    // the table pass, the fold and the gain of outputs p0 .. p0 + cols - 1, their adjoints the rows [cols][2n] at y
    int hand_over(int32_t p0, int cols, const double *y, int64_t rs, int64_t cs, const double *) override {
        const int64_t n2 = 2 * n, row_groups = groups_of(ncomp, NTB), gain_groups = groups_of(n, NTB);
        if (cols < 1 || cols > NCOLS || p0 < 0 || p0 + cols > nout || rs != 1 || cs != n2)
            return nodal_fail(h, NODAL_E_INVALID, "noise: a block outside the call's columns");
        hipStream_t st = h->stream;
        if (ncomp > 0) {
            k_noise_rows<<<(unsigned)row_groups, NTB, 0, st>>>(ncomp, cols, h->type.as<uint8_t>(), assembled_values(h), h->a.as<int32_t>(),
                                                              h->b.as<int32_t>(), y, n2, kt4, weight ? weight[f] : 0.0,
                                                              weight ? contrib + (size_t)p0 * ncomp : nullptr, part);
            k_noise_fold<<<(unsigned)cols, 64, 0, st>>>(row_groups, part, dens + (size_t)f * nout + p0);
        }
        if (svec) {
            k_noise_gain<<<(unsigned)gain_groups, NTB, 0, st>>>(n, cols, y, n2, svec, part);
            k_noise_fold<<<(unsigned)(2 * cols), 64, 0, st>>>(gain_groups, part, gain + ((size_t)f * nout + p0) * 2);
        }
        NODAL_HIP_TRY(h, hipGetLastError());
        return NODAL_OK;
    }
    void all_singular(int32_t) override {}  // (noise_run fills the frequency's rows from info)
};

}  // namespace

int noise_run(nodal_ctx *h, bool dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
              const double *value, const int32_t *lead_a, const int32_t *lead_b, double temperature, int32_t nout,
              const int32_t *out_a, const int32_t *out_b, int64_t input_row, const double *weight, double *density_out,
              double *gain_out, double *contrib_out, double *resid_out, int32_t *info_out, double *ms_analysis,
              double *ms_factor) {
    const int64_t n = h->n, n2 = 2 * n, ncomp = h->ncomp;
    hipStream_t st = h->stream;
    const double nan = __builtin_nan("");
    *ms_analysis = *ms_factor = 0.0;

    // ---- the arguments ----
    NODAL_TRY(ac_check_arguments(h, "noise: ", nfreq, omega, nreact, kind, value, lead_a, lead_b));
    if (!(temperature > 0.0 && temperature - temperature == 0.0))
        return nodal_fail(h, NODAL_E_INVALID, "noise: a temperature that is not finite and positive");
    NODAL_TRY(ac_check_pairs(h, "noise: ", "output node", nout, out_a, out_b));
    const bool have_input = input_row >= 0;
    if (input_row < -1) return nodal_fail(h, NODAL_E_INVALID, "noise: input: source row out of range");
    if (gain_out && !have_input) return nodal_fail(h, NODAL_E_INVALID, "noise: a gain is asked for and no input source is named");
    if (contrib_out && !weight) return nodal_fail(h, NODAL_E_INVALID, "noise: contributions are asked for without weights");
    if (have_input) {
        const double one = 1.0, zero = 0.0;
        NODAL_TRY(ac_sources_check(h, "noise: input: ", "source row", 1, &input_row, &one, &zero));  // (waits)
    }
    if (nfreq == 0 || nout == 0) return NODAL_OK;

    const bool want_gain = gain_out != nullptr, want_contrib = contrib_out != nullptr && ncomp > 0;
    const size_t cells = (size_t)nfreq * nout, contrib_words = want_contrib ? (size_t)nout * ncomp : 0;
    AcLedger ledger(h, nfreq, (size_t)nout, resid_out, info_out);
    if (n == 0) {  // (no unknowns: every lead is ground, nothing is seen)
        if (density_out) std::fill_n(density_out, cells, 0.0);
        if (gain_out) std::fill_n(gain_out, 2 * cells, 0.0);
        if (contrib_out) std::fill_n(contrib_out, (size_t)nout * ncomp, 0.0);
        return NODAL_OK;
    }

    // ---- once per call: the transposed child, the elements and outputs up, the input's right-hand side, the buffers ----
    nodal_ctx *s = nullptr;
    NODAL_TRY(adjoint_context(h, &s));
    const bool transposed = s != h;
    nodal_ctx *c = nullptr;
    NODAL_TRY(ac_child(h, transposed, nreact, kind, lead_a, lead_b, ms_analysis, &c));
    AcSpec spec;  // the elements without their leads (no kernel here reads them); output a, output b
    NODAL_TRY(ac_upload_spec(h, nreact, kind, value, nullptr, nullptr, {{out_a, (size_t)nout}, {out_b, (size_t)nout}}, nullptr, 0, &spec));
    // nz_vec: the input's right-hand side (2n) and, for the sparse LU route, | defect | correction (2n each)
    // | right-hand sides [16][2n] | adjoints [16][2n] | the judge's norms
    const bool dense_route = n2 <= 64 || dense;
    NODAL_HIP_TRY(h, h->nz_vec.reserve((size_t)(3 + 2 * NCOLS) * n2 * 8 + 5 * SLU_MULTI * 8 + 256));
    double *svec = h->nz_vec.as<double>(), *rvec = svec + n2, *dvec = rvec + n2, *bblk = dvec + n2, *ys = bblk + (size_t)NCOLS * n2,
           *norms = ys + (size_t)NCOLS * n2;
    // nz_part: the workgroups' partial sums, [16][groups of the table] or [16][2][groups of the unknowns]
    const int64_t row_groups = groups_of(ncomp, NTB), gain_groups = groups_of(n, NTB);
    NODAL_HIP_TRY(h, h->nz_part.reserve((size_t)std::max<int64_t>(row_groups, 2 * gain_groups) * NCOLS * 8 + 64));
    double *part = h->nz_part.as<double>();
    // nz_out: densities [nfreq][nout] | gains [nfreq][nout][2] | residuals [nfreq][nout] | contributions [nout][ncomp]
    NODAL_HIP_TRY(h, h->nz_out.reserve((4 * cells + contrib_words + 2) * 8 + 64));
    double *dens_dev = h->nz_out.as<double>(), *gain_dev = dens_dev + cells, *resid_dev = gain_dev + 2 * cells,
           *contrib_dev = resid_dev + cells;
    ledger.resid_dev = resid_dev;
    NODAL_HIP_TRY(h, hipMemsetAsync(dens_dev, 0, (4 * cells + contrib_words) * 8, st));
    if (have_input) NODAL_TRY(ac_sources_stamp(h, 1, svec));
    NODAL_WAIT_STREAM(h, st);  // (the elements and outputs are the caller's)

    NoiseClient client(h, nout, spec.list[0], spec.list[1]);
    client.kt4 = 4.0 * BOLTZMANN * temperature;
    if (want_contrib) client.weight = weight;
    if (want_gain) client.svec = svec;
    client.part = part;
    client.dens = dens_dev;
    client.gain = gain_dev;
    client.contrib = contrib_dev;

    // ---- the frequencies ----
    uint64_t lu_epoch = 0;  // (never the child's numeric_epoch: every frequency is factored anew)
    int64_t work[3] = {0, 0, 0};  // (not reported)
    for (int32_t f = 0; f < nfreq; ++f) {
        NODAL_TRY(ac_child_values(h, transposed, omega[f], spec.kind, spec.value));
        client.f = f;
        bool dead = false;
        if (dense_route) {  // k_noise_rhs fills the panel's columns of a chunk in one launch
            NODAL_TRY(ac_block_dense(h, c, dense, nout, DENSE_CHUNK, client, resid_dev + (size_t)f * nout, &dead, work));
        } else {
            // One output at a time through transient_solver_step (two substitutions and one refinement step), not sixteen
            // through slu_apply_multi as ac_block_frequency has them: an output has the same bits alone as inside a block
            // (tests/test_gpu_noise.py).  Moving this branch onto the block apply is a change of speed and of bits, for a
            // pull request of its own.
            TransientSolver ts;
            ts.s = c;
            ts.lu_epoch = &lu_epoch;
            ts.rvec = rvec;
            ts.dvec = dvec;
            ts.norms = norms;
            double ms_f = 0.0;
            NODAL_TRY(nodal_lift_error(h, c, transient_solver_begin(c, ts, false, 1, &dead, &ms_f)));
            ac_add_factor_time(c, ms_f, ms_analysis, ms_factor);
            for (int32_t p0 = 0; p0 < nout && !dead; p0 += NCOLS) {
                const int cols = std::min<int32_t>(NCOLS, nout - p0);
                NODAL_HIP_TRY(h, hipMemsetAsync(bblk, 0, (size_t)cols * n2 * 8, st));
                NODAL_TRY(client.build(p0, cols, bblk, 1, n2));
                for (int y = 0; y < cols && !dead; ++y) {
                    const size_t cell = (size_t)f * nout + p0 + y;
                    int32_t inf = 0, it = 0;
                    bool judged = false;
                    double ms_none = 0.0;
                    NODAL_TRY(nodal_lift_error(h, c, transient_solver_step(c, ts, bblk + (size_t)y * n2, ys + (size_t)y * n2, &inf, &it,
                                                                           &ledger.resid[cell], &judged, &ms_none)));
                    if (inf > 0) {
                        dead = true;
                        break;
                    }
                    ledger.on_host[cell] = judged;
                    if (!judged) NODAL_HIP_TRY(h, hipMemcpyAsync(resid_dev + cell, norms + 4 * SLU_MULTI, 8, hipMemcpyDeviceToDevice, st));
                }
                if (!dead) NODAL_TRY(client.hand_over(p0, cols, ys, 1, n2, nullptr));
            }
        }
        if (dead) ledger.mark_dead(f);
    }

    // ---- after the last frequency: everything comes down once ----
    if (density_out) NODAL_HIP_TRY(h, hipMemcpyAsync(density_out, dens_dev, cells * 8, hipMemcpyDeviceToHost, st));
    if (gain_out) NODAL_HIP_TRY(h, hipMemcpyAsync(gain_out, gain_dev, 2 * cells * 8, hipMemcpyDeviceToHost, st));
    if (want_contrib) NODAL_HIP_TRY(h, hipMemcpyAsync(contrib_out, contrib_dev, contrib_words * 8, hipMemcpyDeviceToHost, st));
    NODAL_TRY(ledger.finish([&](int32_t f) {
        if (density_out) std::fill_n(density_out + (size_t)f * nout, (size_t)nout, nan);
        if (gain_out) std::fill_n(gain_out + (size_t)f * nout * 2, 2 * (size_t)nout, nan);
    }));
    if (ledger.any_dead() && want_contrib)  // (an integral over a list with a hole in it is none)
        std::fill_n(contrib_out, contrib_words, nan);
    return NODAL_OK;
}
