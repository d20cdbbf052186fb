// AC port analysis: the multiport impedance matrix Z(j omega) of an RLC network seen from chosen ports, over a list of
// frequencies.
//
// Replaces one nodal_ac_sweep per port -- an A source across the port has to be in the netlist already, one excitation
// per call, one numeric factorisation of the doubled system per port and frequency -- and nodal_port_matrix, which gives
// the P x P matrix at DC only and for G alone.  With A(w) = G + j B(w) exactly as ac.hip defines it, port q = (a_q, b_q)
// has the real unit injection s_q = e(a_q) - e(b_q) (zeros in the branch rows; every independent source off, the
// dependent ones in G), x_q solves
//     A(w) x_q = s_q                                  (A itself, not its transpose)
// and Z[f][p][q] = x_q(a_p) - x_q(b_p): volts at port p per ampere entering a_q and leaving b_q, the sign of ports.hip.
//
// The matrix is the child ac.hip keeps on h->ac (ac_child, ac_child_values): pattern and symbolic analysis are shared with
// the sweep in both directions.  A frequency is, on the handle's stream,
//     k_ac_values      the child's values (ac.hip)
//     the solves       ac_block_frequency below: ONE numeric factorisation whatever the number of ports.  Dense panel
//                      (2n <= 64, or `dense` at any size): the ports are the right-hand-side columns of one
//                      dense_factor_solve_multi, up to 512 at a time, judged in groups of sixteen.  Otherwise the sparse
//                      LU factored anew on the kept analysis, and per block of up to sixteen ports
//                          k_acport_rhs        the unit injections into the zeroed interleaved block
//                          slu_apply_multi     X = A^-1 B: every entry of the factors read once for sixteen columns
//                          k_acport_residual   R = B - A X
//                          slu_apply_multi     D = A^-1 R
//                          k_acport_correct    X += D
//                          csr_judge_block     the columns' scaled residuals, read back for the bar
//                      a column above knob::MULTI_BAR -- every column when the factorisation replaced pivots -- redone
//                      alone by sparse_direct_solve among its block's rows (k_acport_rows), and the factors made anew
//     k_acport_gather  the finished block read at the port nodes into the device copy of Z[f]
//     k_acport_peak    per node the largest |x_q(i)|^2 of the frequency so far and its port (when peaks are asked for),
//     k_acport_merge   and, once the frequency is known to be solved, that into the call's peaks with the frequency index
// Every kernel addresses a block as element (row, y) at [row * rs + y * cs]: the interleaved block (16, 1) and the rows of
// the redo and dense routes (1, 2n) go through the same code, as in ports.hip.  Z, the peaks and the dense routes'
// residuals come down once, after the last frequency: F P P complex numbers, not F P 2n.  No floating-point atomics: a
// repeated call gives the same bits.  The handle itself -- solution, table, G, A, tape, hierarchy, factors -- is only read.
//
// The block loop is not multi_rhs_solve's LU branch called on the child: that driver's size thresholds would send
// 2n = 290 to the dense LU, and its present callers compare bits.  ac_block_frequency takes a MultiRhsClient: the AC
// gradient hands its two columns to it, and the noise analysis its outputs to the dense part, ac_block_dense.
#include "ac_sweep.h"


namespace {

constexpr int PTB = 256;
constexpr int NCOLS = SLU_MULTI;  // ports of a block
constexpr int DENSE_CHUNK = 512;  // right-hand-side columns of one dense factorisation

// One thread per column y < cols of a zeroed block of the doubled system: the <= 2 entries of s_q, at the real parts of
// a_q and b_q.  Both adds by the same thread, in order: a == b gives exactly 0.
__global__ __launch_bounds__(64) void k_acport_rhs(int cols, const int32_t *__restrict__ ia, const int32_t *__restrict__ ib,
                                                   double *__restrict__ out, int64_t rs, int64_t cs) {
    const int y = threadIdx.x;
    if (y >= cols) return;
    double *col = out + (int64_t)y * cs;
    const int32_t a = ia[y], b = ib[y];
    if (a >= 0) col[2 * (int64_t)a * rs] += 1.0;
    if (b >= 0) col[2 * (int64_t)b * rs] -= 1.0;
}

// r = b - A x for the `cols` columns of a block: the lanes of a row share every matrix entry
__global__ __launch_bounds__(PTB) void k_acport_residual(int64_t n, int cols, const int32_t *__restrict__ indptr,
                                                         const int32_t *__restrict__ indices, const double *__restrict__ data,
                                                         const double *__restrict__ x, const double *__restrict__ b,
                                                         double *__restrict__ r, int64_t rs, int64_t cs) {
    for (int64_t t = (int64_t)blockIdx.x * PTB + threadIdx.x; t < n * NCOLS; t += (int64_t)gridDim.x * PTB) {
        const int64_t i = t / NCOLS;
        const int y = (int)(t % NCOLS);
        if (y >= cols) continue;
        const int64_t at = (int64_t)y * cs;
        double acc = b[i * rs + at];
        for (int32_t q = indptr[i]; q < indptr[i + 1]; ++q) acc = fma(-data[q], x[(int64_t)indices[q] * rs + at], acc);
        r[i * rs + at] = acc;
    }
}

// x += d for the `cols` columns of a block
__global__ __launch_bounds__(PTB) void k_acport_correct(int64_t n, int cols, const double *__restrict__ d, double *__restrict__ x,
                                                        int64_t rs, int64_t cs) {
    for (int64_t t = (int64_t)blockIdx.x * PTB + threadIdx.x; t < n * NCOLS; t += (int64_t)gridDim.x * PTB) {
        const int64_t i = t / NCOLS;
        const int y = (int)(t % NCOLS);
        if (y >= cols) continue;
        x[i * rs + (int64_t)y * cs] += d[i * rs + (int64_t)y * cs];
    }
}

// rows[y * n + i] = X(i, y), y < cols: a block as [cols][n] rows, where a column redone alone lands among its block's
__global__ __launch_bounds__(PTB) void k_acport_rows(int64_t n, int cols, const double *__restrict__ x, int64_t rs, int64_t cs,
                                                     double *__restrict__ rows) {
    for (int64_t t = (int64_t)blockIdx.x * PTB + threadIdx.x; t < n * cols; t += (int64_t)gridDim.x * PTB) {
        const int64_t y = t / n, i = t - y * n;
        rows[t] = x[i * rs + y * cs];
    }
}

// One thread per (port p, column y) of a finished block X of the doubled system:
// z[p * nports + m0 + y] = X(a_p, y) - X(b_p, y) as (re, im), a ground lead reading +0.0; exactly +0.0 when port p or
// the column's own port lies between a node and itself, whatever X holds.  (No column is ever flagged NaN here: a
// singular column makes its frequency singular, and ac_ports_run fills that frequency's rows from info.)
__global__ __launch_bounds__(PTB) void k_acport_gather(int32_t nports, int cols, int32_t m0, const int32_t *__restrict__ ia,
                                                       const int32_t *__restrict__ ib, const double *__restrict__ x,
                                                       int64_t rs, int64_t cs, double2 *__restrict__ z) {
    const int64_t t = (int64_t)blockIdx.x * PTB + threadIdx.x;
    const int64_t p = t / cols;
    const int y = (int)(t - p * cols);
    if (p >= nports) return;
    double re = 0.0, im = 0.0;
    const int32_t a = ia[p], b = ib[p];
    if (a != b && ia[m0 + y] != ib[m0 + y]) {
        const int64_t at = (int64_t)y * cs;
        const int32_t ra = a < 0 ? -1 : 2 * a, rb = b < 0 ? -1 : 2 * b;
        re = lead(x, ra, rs, at) - lead(x, rb, rs, at);
        im = lead(x, ra, rs, at + rs) - lead(x, rb, rs, at + rs);
    }
    z[p * nports + m0 + y] = make_double2(re, im);
}

// Sixteen lanes per node, lane y the (re, im) of column y of the finished block -- the `cols` valid columns only --, so
// that a wave reads 512 contiguous bytes of the interleaved block per row (one lane per node walking its row alone reads
// them 8 bytes per lane and instruction: measured at 0.5 TB/s).  The sixteen are folded by xor shuffles with the larger
// |x|^2 winning and, among exact ties, the lower port: what columns ascending under a strict comparison give, whatever the
// order of the fold.  Lane 0 then updates the frequency's peak under the same strict comparison (blocks ascending).
// first: nothing of this frequency has been taken in yet.
__global__ __launch_bounds__(PTB) void k_acport_peak(int32_t K, int cols, int32_t m0, int first, const double *__restrict__ x,
                                                     int64_t rs, int64_t cs, double *__restrict__ peak2,
                                                     int32_t *__restrict__ peak_port) {
    const int64_t t = (int64_t)blockIdx.x * PTB + threadIdx.x;
    const int64_t i = t / NCOLS;
    const int y = (int)(t % NCOLS);
    double m = -1.0;  // (below every |x|^2: a lane without a column never wins, and lane 0 always has one)
    if (i < K && y < cols) {
        const double re = x[2 * i * rs + (int64_t)y * cs], im = x[(2 * i + 1) * rs + (int64_t)y * cs];
        m = re * re + im * im;
    }
    int32_t port = m0 + y;
    for (int off = 1; off < NCOLS; off <<= 1) {  // (every lane of the wave takes part: nothing has returned)
        const double om = __shfl_xor(m, off, 64);
        const int32_t op = __shfl_xor(port, off, 64);
        if (om > m || (om == m && op < port)) {
            m = om;
            port = op;
        }
    }
    if (i < K && y == 0 && (first || m > peak2[i])) {
        peak2[i] = m;
        peak_port[i] = port;
    }
}

// the peaks of a solved frequency into the call's: frequencies ascending, a strict comparison (among exact ties the
// lowest frequency stays, and within it the lowest port).  first: no frequency has been taken in yet.
__global__ __launch_bounds__(PTB) void k_acport_merge(int32_t K, int32_t freq, int first, const double *__restrict__ fpeak2,
                                                      const int32_t *__restrict__ fport, double *__restrict__ peak2,
                                                      int32_t *__restrict__ peak_port, int32_t *__restrict__ peak_freq) {
    const int32_t i = blockIdx.x * PTB + threadIdx.x;
    if (i >= K) return;
    const double m = fpeak2[i];
    if (first || m > peak2[i]) {
        peak2[i] = m;
        peak_port[i] = fport[i];
        peak_freq[i] = freq;
    }
}

// the block loop's client: the columns are the ports' unit injections, a finished block is read at the port nodes and,
// when peaks are asked for, taken into the frequency's peaks
struct AcPortClient final : MultiRhsClient {
    nodal_ctx *h;
    int32_t nports, K;
    const int32_t *ia, *ib;     // device, [nports]
    double2 *z = nullptr;       // device, Z of the frequency at hand, [nports][nports]
    double *fpeak2 = nullptr;   // device, [K]; null: no peaks
    int32_t *fport = nullptr;
    bool first = true;          // nothing of the frequency at hand has been taken into the peaks yet
    AcPortClient(nodal_ctx *h_, int32_t nports_, int32_t K_, const int32_t *ia_, const int32_t *ib_)
        : h(h_), nports(nports_), K(K_), ia(ia_), ib(ib_) {
        wants_rows = false;
        max_cols = NCOLS;
    }
    int build(int32_t m0, int cols, double *out, int64_t rs, int64_t cs) override {
        if (cols < 1 || cols > NCOLS || m0 < 0 || m0 + cols > nports)
            return nodal_fail(h, NODAL_E_INVALID, "ac ports: 1 to 16 columns of the call per launch");
        k_acport_rhs<<<1, 64, 0, h->stream>>>(cols, ia + m0, ib + m0, out, rs, cs);
        NODAL_HIP_TRY(h, hipGetLastError());
        return NODAL_OK;
    }
    int hand_over(int32_t m0, int cols, const double *x, int64_t rs, int64_t cs, const double *) override {
        if (cols < 1 || cols > NCOLS || m0 < 0 || m0 + cols > nports)
            return nodal_fail(h, NODAL_E_INVALID, "ac ports: a block outside the call's columns");
        k_acport_gather<<<groups_of((int64_t)nports * cols, PTB), PTB, 0, h->stream>>>(nports, cols, m0, ia, ib, x, rs, cs, z);
        if (fpeak2) {
            k_acport_peak<<<groups_of((int64_t)K * NCOLS, PTB), PTB, 0, h->stream>>>(K, cols, m0, first ? 1 : 0, x, rs, cs, fpeak2, fport);
            first = false;
        }
        NODAL_HIP_TRY(h, hipGetLastError());
        return NODAL_OK;
    }
    void all_singular(int32_t) override {}  // (ac_ports_run fills the frequency's rows from info)
};

// The sparse LU part of the block loop, factored once for every column of the frequency.
int block_sparse(nodal_ctx *h, nodal_ctx *c, int32_t count, MultiRhsClient &client, double *resid_host, uint8_t *on_host,
                 bool *dead, int64_t *work, double *ms_analysis, double *ms_factor) {
    const int64_t n2 = c->n;
    hipStream_t st = h->stream;  // (c shares it: one ordered timeline)
    // ap_vec: the blocks B, X, R, D interleaved by row [2n][16] | one right-hand side [2n] | the norms
    const size_t blk = (size_t)n2 * NCOLS;
    NODAL_HIP_TRY(h, h->ap_vec.reserve((4 * blk + (size_t)n2) * 8 + 5 * SLU_MULTI * 8 + 256));
    double *Bil = h->ap_vec.as<double>(), *Xil = Bil + blk, *Ril = Xil + blk, *Dil = Ril + blk, *bvec = Dil + blk, *norms = bvec + n2;
    {
        const auto t0 = std::chrono::steady_clock::now();
        int32_t inf = 0;
        NODAL_TRY(nodal_lift_error(h, c, slu_factor(c, &inf)));
        NODAL_WAIT_STREAM(h, st);
        ac_add_factor_time(c, ms_since(t0), ms_analysis, ms_factor);
        ++work[0];
        if (inf > 0) {
            *dead = true;
            return NODAL_OK;
        }
    }
    bool all_direct = slu_perturbed(c) > 0;
    // the backward-error bar of the refinement, multi_rhs_solve's: below 0 every column goes through the redo
    const double bar = knob::MULTI_BAR.now();
    const unsigned gv = (unsigned)std::min<int64_t>(((int64_t)blk + PTB - 1) / PTB, 65536);
    const int32_t *indptr = c->indptr.as<int32_t>(), *indices = c->indices.as<int32_t>();
    for (int32_t m0 = 0; m0 < count; m0 += NCOLS) {
        const int cnt = std::min<int32_t>(NCOLS, count - m0);
        bool redo = all_direct;
        if (!all_direct) {
            NODAL_HIP_TRY(h, hipMemsetAsync(Bil, 0, blk * 8, st));  // (the whole block: nothing of the one before stays)
            NODAL_TRY(client.build(m0, cnt, Bil, NCOLS, 1));
            NODAL_TRY(nodal_lift_error(h, c, slu_apply_multi(c, Bil, Xil)));
            k_acport_residual<<<gv, PTB, 0, st>>>(n2, NCOLS, indptr, indices, c->data.as<double>(), Xil, Bil, Ril, NCOLS, 1);
            NODAL_HIP_TRY(h, hipGetLastError());
            NODAL_TRY(nodal_lift_error(h, c, slu_apply_multi(c, Ril, Dil)));
            k_acport_correct<<<gv, PTB, 0, st>>>(n2, NCOLS, Dil, Xil, NCOLS, 1);
            NODAL_HIP_TRY(h, hipGetLastError());
            work[1] += 2;
            NODAL_TRY(nodal_lift_error(h, c, csr_judge_block(c, Xil, Bil, NCOLS, 1, cnt, norms)));
            NODAL_TRY(nodal_read_words(h, resid_host + m0, norms + 4 * SLU_MULTI, (size_t)cnt * 8));
            for (int y = 0; y < cnt; ++y) {
                on_host[m0 + y] = 1;
                redo = redo || !(resid_host[m0 + y] <= bar);
            }
        }
        if (!redo) {  // the usual case: the block is handed over interleaved
            NODAL_TRY(client.hand_over(m0, cnt, Xil, NCOLS, 1, nullptr));
            continue;
        }
        NODAL_HIP_TRY(h, h->ap_rows.reserve(blk * 8 + 64));
        double *rows = h->ap_rows.as<double>();
        if (!all_direct) {
            k_acport_rows<<<groups_of(n2 * cnt, PTB), PTB, 0, st>>>(n2, cnt, Xil, NCOLS, 1, rows);
            NODAL_HIP_TRY(h, hipGetLastError());
        }
        for (int y = 0; y < cnt; ++y) {
            if (!all_direct && resid_host[m0 + y] <= bar) continue;
            double *xk = rows + (size_t)y * n2;
            NODAL_HIP_TRY(h, hipMemsetAsync(bvec, 0, (size_t)n2 * 8, st));
            NODAL_TRY(client.build(m0 + y, 1, bvec, 1, 0));
            int32_t inf1 = 0, it = 0;
            double rs = 0.0;
            NODAL_TRY(nodal_lift_error(h, c, sparse_direct_solve(c, bvec, xk, &inf1, &it, &rs)));
            ++work[2];
            if (inf1 > 0) {  // (singular after all: the frequency is, with every column of it)
                *dead = true;
                return NODAL_OK;
            }
            NODAL_TRY(nodal_lift_error(h, c, csr_judge_block(c, xk, bvec, 1, 0, 1, norms)));
            NODAL_TRY(nodal_read_words(h, resid_host + m0 + y, norms + 4 * SLU_MULTI, 8));
            on_host[m0 + y] = 1;
        }
        NODAL_TRY(client.hand_over(m0, cnt, rows, 1, n2, nullptr));
        if (!all_direct) {  // (the direct solve may have factored anew, with another pivot bar)
            int32_t inf = 0;
            NODAL_TRY(nodal_lift_error(h, c, slu_factor(c, &inf)));
            ++work[0];
            all_direct = inf > 0 || slu_perturbed(c) > 0;
        }
    }
    return NODAL_OK;
}

}  // namespace

int ac_block_dense(nodal_ctx *h, nodal_ctx *c, bool dense, int32_t count, int32_t build_cols, MultiRhsClient &client,
                   double *resid_dev, bool *dead, int64_t *work) {
    const int64_t n2 = c->n;
    hipStream_t st = h->stream;  // (c shares it: one ordered timeline)
    // one LU per chunk of up to 512 columns: they are extra right-hand-side columns of the augmented panel
    // ap_vec: the right-hand sides of a group, kept for the judgement [16][2n] | solutions [chunk][2n] | the norms
    const int32_t chunk = std::min<int32_t>(count, DENSE_CHUNK);
    NODAL_HIP_TRY(h, h->ap_vec.reserve((size_t)(NCOLS + chunk) * n2 * 8 + 5 * SLU_MULTI * 8 + 256));
    double *bblk = h->ap_vec.as<double>(), *xs = bblk + (size_t)NCOLS * n2, *norms = xs + (size_t)chunk * n2;
    const int64_t lda = dense_lda(n2);
    for (int32_t q0 = 0; q0 < count; q0 += chunk) {
        const int32_t width = std::min<int32_t>(chunk, count - q0);
        NODAL_HIP_TRY(h, c->dense.reserve((size_t)lda * (size_t)(n2 + width) * 8 + 64));
        NODAL_TRY(nodal_lift_error(h, c, csr_to_dense(c, c->dense.as<double>(), lda)));
        double *cols = c->dense.as<double>() + n2 * lda;
        NODAL_HIP_TRY(h, hipMemsetAsync(cols, 0, (size_t)lda * width * 8, st));
        for (int32_t g0 = 0; g0 < width; g0 += build_cols)
            NODAL_TRY(client.build(q0 + g0, std::min<int32_t>(build_cols, width - g0), cols + (int64_t)g0 * lda, 1, lda));
        int32_t inf = 0;
        NODAL_TRY(nodal_lift_error(h, c, dense_factor_solve_multi(c, width, xs, n2, &inf)));
        ++work[0];
        if (inf > 0) {
            if (dense) return nodal_fail(h, NODAL_E_SINGULAR, "singular matrix: a zero pivot or a floating sub-network");
            *dead = true;
            return NODAL_OK;
        }
        for (int32_t g0 = 0; g0 < width; g0 += NCOLS) {  // every group of sixteen is judged
            const int k = std::min<int32_t>(NCOLS, width - g0);
            const double *x = xs + (size_t)g0 * n2;
            NODAL_HIP_TRY(h, hipMemsetAsync(bblk, 0, (size_t)k * n2 * 8, st));
            NODAL_TRY(client.build(q0 + g0, k, bblk, 1, n2));
            NODAL_TRY(nodal_lift_error(h, c, csr_judge_block(c, x, bblk, 1, n2, k, norms)));
            NODAL_HIP_TRY(h, hipMemcpyAsync(resid_dev + q0 + g0, norms + 4 * SLU_MULTI, (size_t)k * 8, hipMemcpyDeviceToDevice, st));
            NODAL_TRY(client.hand_over(q0 + g0, k, x, 1, n2, nullptr));
        }
    }
    return NODAL_OK;
}

int ac_block_frequency(nodal_ctx *h, nodal_ctx *c, bool dense, int32_t count, MultiRhsClient &client, double *resid_host,
                       uint8_t *on_host, double *resid_dev, bool *dead, int64_t *work, double *ms_analysis, double *ms_factor) {
    *dead = false;
    if (count <= 0 || c->n <= 0) return NODAL_OK;
    if (c->n <= 64 || dense) return ac_block_dense(h, c, dense, count, NCOLS, client, resid_dev, dead, work);
    return block_sparse(h, c, count, client, resid_host, on_host, dead, work, ms_analysis, ms_factor);
}

int ac_ports_run(nodal_ctx *h, bool dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
                 const double *value, const int32_t *lead_a, const int32_t *lead_b, int32_t nports, const int32_t *ia,
                 const int32_t *ib, double *z_out, double *node_peak_out, int32_t *node_peak_port_out,
                 int32_t *node_peak_freq_out, double *resid_out, int32_t *info_out, int64_t *work_out, double *ms_analysis,
                 double *ms_factor) {
    const int64_t n = h->n;
    const int32_t K = h->K;
    hipStream_t st = h->stream;
    const double nan = __builtin_nan("");
    *ms_analysis = *ms_factor = 0.0;
    int64_t work[3] = {0, 0, 0};
    if (work_out) work_out[0] = work_out[1] = work_out[2] = 0;

    // ---- the arguments ----
    NODAL_TRY(ac_check_arguments(h, "ac ports: ", nfreq, omega, nreact, kind, value, lead_a, lead_b));
    NODAL_TRY(ac_check_pairs(h, "ac ports: ", "port node", nports, ia, ib));
    if (nfreq == 0 || nports == 0) return NODAL_OK;

    const size_t cells = (size_t)nfreq * nports, zwords = cells * (size_t)nports * 2;
    AcLedger ledger(h, nfreq, (size_t)nports, resid_out, info_out);
    if (n == 0) {  // (no unknowns: every lead is ground, nothing is seen)
        if (z_out)
            for (size_t t = 0; t < zwords; ++t) z_out[t] = 0.0;
        return NODAL_OK;
    }
    const bool want_peak = (node_peak_out || node_peak_port_out || node_peak_freq_out) && K > 0;

    // ---- once per call: the child, the elements and ports up, the buffers ----
    nodal_ctx *c = nullptr;
    NODAL_TRY(ac_child(h, false, nreact, kind, lead_a, lead_b, ms_analysis, &c));
    AcSpec spec;  // the elements without their leads (no kernel here reads them); port a, port b
    NODAL_TRY(ac_upload_spec(h, nreact, kind, value, nullptr, nullptr, {{ia, (size_t)nports}, {ib, (size_t)nports}}, nullptr, 0, &spec));
    const int32_t *ia_dev = spec.list[0], *ib_dev = spec.list[1];
    // ap_out: Z [nfreq][nports][nports][2] | residuals [nfreq][nports] | the frequency's peaks |x|^2 [K] | the call's [K] |
    // the frequency's ports [K] | the call's ports [K] | their frequencies [K]
    const size_t kw = want_peak ? (((size_t)K + 1) & ~(size_t)1) : 0;
    NODAL_HIP_TRY(h, h->ap_out.reserve((zwords + cells + 2 * kw) * 8 + 3 * kw * 4 + 64));
    double *z_dev = h->ap_out.as<double>(), *resid_dev = z_dev + zwords, *fpeak_dev = resid_dev + cells, *peak_dev = fpeak_dev + kw;
    ledger.resid_dev = resid_dev;
    int32_t *fport_dev = reinterpret_cast<int32_t *>(peak_dev + kw), *port_dev = fport_dev + kw, *freq_dev = port_dev + kw;
    NODAL_HIP_TRY(h, hipMemsetAsync(z_dev, 0, (zwords + cells) * 8, st));
    if (want_peak) {  // (NaN and -1 until a frequency is taken in)
        NODAL_HIP_TRY(h, hipMemsetAsync(peak_dev, 0xFF, kw * 8, st));
        NODAL_HIP_TRY(h, hipMemsetAsync(port_dev, 0xFF, 2 * kw * 4, st));
    }
    NODAL_WAIT_STREAM(h, st);  // (the elements and ports are the caller's)

    AcPortClient client(h, nports, K, ia_dev, ib_dev);
    if (want_peak) {
        client.fpeak2 = fpeak_dev;
        client.fport = fport_dev;
    }

    // ---- the frequencies ----
    bool peak_first = true;
    for (int32_t f = 0; f < nfreq; ++f) {
        NODAL_TRY(ac_child_values(h, false, omega[f], spec.kind, spec.value));
        client.z = reinterpret_cast<double2 *>(z_dev) + (size_t)f * nports * nports;
        client.first = true;
        bool dead = false;
        const size_t at = (size_t)f * nports;
        NODAL_TRY(ac_block_frequency(h, c, dense, nports, client, ledger.resid + at, ledger.on_host.data() + at, resid_dev + at,
                                     &dead, work, ms_analysis, ms_factor));
        if (dead) {
            ledger.mark_dead(f);
            continue;
        }
        if (want_peak) {
            k_acport_merge<<<groups_of(K, PTB), PTB, 0, st>>>(K, f, peak_first ? 1 : 0, fpeak_dev, fport_dev, peak_dev, port_dev, freq_dev);
            NODAL_HIP_TRY(h, hipGetLastError());
            peak_first = false;
        }
    }

    // ---- after the last frequency: everything comes down once ----
    if (want_peak && !peak_first) NODAL_TRY(ac_peak_root(h, K, peak_dev));
    if (z_out) NODAL_HIP_TRY(h, hipMemcpyAsync(z_out, z_dev, zwords * 8, hipMemcpyDeviceToHost, st));
    if (want_peak) {
        if (node_peak_out) NODAL_HIP_TRY(h, hipMemcpyAsync(node_peak_out, peak_dev, (size_t)K * 8, hipMemcpyDeviceToHost, st));
        if (node_peak_port_out) NODAL_HIP_TRY(h, hipMemcpyAsync(node_peak_port_out, port_dev, (size_t)K * 4, hipMemcpyDeviceToHost, st));
        if (node_peak_freq_out) NODAL_HIP_TRY(h, hipMemcpyAsync(node_peak_freq_out, freq_dev, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    }
    NODAL_TRY(ledger.finish([&](int32_t f) {
        if (z_out) std::fill_n(z_out + (size_t)f * nports * nports * 2, (size_t)nports * nports * 2, nan);
    }));
    if (work_out)
        for (int k = 0; k < 3; ++k) work_out[k] = work[k];
    return NODAL_OK;
}
