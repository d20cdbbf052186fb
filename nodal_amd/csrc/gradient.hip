// Loss gradients: the derivative of a scalar loss of the solution(s) with respect to the value of EVERY component.
//
// Replaces one nodal_sensitivities output per unknown the loss touches (one adjoint solve and one [ncomp] row each; the
// reference itself has nothing of the kind, nodal/nodal.py:306-336 is the solve a finite-difference loop would repeat).
//
// L = sum_m L_m(x_m) over the `count` members of a source sweep (or the single solve, count == 1), G(p) x_m = A_m(p).  The
// caller hands over c_m = dL/dx_m, a dense vector per member.  With G^T lambda_m = c_m the chain rule leaves one number
// per table row,
//     dL/dp_i = sum_m lambda_m^T (dA_m/dp_i - dG/dp_i x_m) = sum_m s_i(lambda_m, x_m),
// s_i the per-row formula at the head of sensitivity.hip without an explicit term (the loss's own dependence on p is the
// caller's).  k_gradient_block forms the sixteen terms of a block of members per row and adds them, in member order, onto
// grad[i]: the thread that owns row i is its only writer and the blocks come in member order, so the sum over the members
// is one fixed sequence of additions -- no floating-point atomics, a repeated call returns the same bits.  Nothing of
// size [count][ncomp] exists anywhere.  k_gradient_cross adds the terms a resistor gets from the CCVS / CCCS rows it
// drives (the lists of sensitivity.hip), k_gradient_sources writes member m's derivative with respect to its OWN swept
// value (the formula of an A or E row reads neither x nor the value).
//
// The transposed solves are multi_rhs_solve (sparse.hip) with the GradientClient below: its columns are the cotangents,
// brought up sixteen rows at a time and written in whatever layout the route asks for -- for the interleaved block that
// is a [16][n] -> [n][16] transposition, k_gradient_interleave -- and a finished block meets its members' solutions in the
// same layout.
#include "table_rows.h"

#include <algorithm>

namespace {

constexpr int STB = 256;
constexpr int SCOLS = 16;  // members per launch of the table kernels (SLU_MULTI)

// ---- rows -> the layout a route asks for -------------------------------------------------------------------------
// out[i * rs + y * cs] = src[y * n + i], y < cols: the dense panel's columns, [cols][n] rows, a column alone.  One
// thread per element, i fastest: with rs == 1 reads and writes are both whole lines.
__global__ __launch_bounds__(STB) void k_gradient_spread(int64_t n, int cols, const double *__restrict__ src,
                                                         double *__restrict__ out, int64_t rs, int64_t cs) {
    const int64_t t = (int64_t)blockIdx.x * STB + threadIdx.x;
    if (t >= n * cols) return;
    const int64_t y = t / n, i = t - y * n;
    out[i * rs + y * cs] = src[t];
}

// out[i * 16 + y] = src[y * stride + i] (y < cols; zeros in the other columns): [16][n] rows as the block interleaved by
// row.  One wavefront per 64 unknowns: it reads sixteen runs of 512 bytes into a 16 x 64 tile in LDS (rows padded to 65:
// the transposed reads then fall on distinct banks) and writes the tile's 8 KB, which are contiguous in `out`, 512 bytes
// per instruction -- whole lines both ways, where one strided element per thread would touch a line per element.
__global__ __launch_bounds__(64) void k_gradient_interleave(int64_t n, int cols, const double *__restrict__ src,
                                                            int64_t stride, double *__restrict__ out) {
    __shared__ double tile[SCOLS][65];
    const int lane = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 64;
    const bool in = i0 + lane < n;
#pragma unroll
    for (int y = 0; y < SCOLS; ++y) tile[y][lane] = (in && y < cols) ? src[(int64_t)y * stride + i0 + lane] : 0.0;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SCOLS; ++r) {
        const int e = r * 64 + lane, i = e >> 4, y = e & 15;
        if (i0 + i < n) out[(i0 + i) * SCOLS + y] = tile[y][i];
    }
}

// ---- the table kernels ---------------------------------------------------------------------------------------------
// One thread per table row for the whole block of members: the row's record is decoded once (row_term, table_rows.h),
// then per member y the term D_y * w_y with D = L(j1) - L(j2) and w = u / den, u = X(p1) - X(p2), or 1 for a row that
// does not read x -- added one after the other, in member order, onto grad[i].
// IL: lam and x are interleaved by row, element (j, y) at [j * 16 + y] -- the sixteen L (or X) of a lead are one
// 128-byte line, fetched as eight 16-byte loads; otherwise element (j, y) at lam[j * rs + y * cs] / x[j * xrs + y * xcs].
template <bool IL>
__global__ __launch_bounds__(STB) void k_gradient_block(int64_t ncomp, int32_t K, int cols,
                                                        const uint8_t *__restrict__ type,
                                                        const double *__restrict__ value,
                                                        const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                        const int32_t *__restrict__ c, const int32_t *__restrict__ d,
                                                        const int32_t *__restrict__ drv, const int32_t *__restrict__ k,
                                                        const double *__restrict__ lam, int64_t rs, int64_t cs,
                                                        const double *__restrict__ x, int64_t xrs, int64_t xcs,
                                                        double *__restrict__ grad) {
    const int64_t i = (int64_t)blockIdx.x * STB + threadIdx.x;
    if (i >= ncomp) return;
    const RowTerm r = row_term(i, K, type, value, a, b, c, d, drv, k);
    if (r.none) return;  // (its sum stays the zero it started from)
    const int32_t j1 = r.j1, j2 = r.j2, p1 = r.p1, p2 = r.p2;
    const bool reads_x = r.reads_x;
    const double den = r.den;  // w = u / den
    double acc = grad[i];
    if constexpr (IL) {
        const double2 *l1 = reinterpret_cast<const double2 *>(lam + (int64_t)(j1 < 0 ? 0 : j1) * SCOLS);
        const double2 *l2 = reinterpret_cast<const double2 *>(lam + (int64_t)(j2 < 0 ? 0 : j2) * SCOLS);
        const double2 *x1 = reinterpret_cast<const double2 *>(x + (int64_t)(p1 < 0 ? 0 : p1) * SCOLS);
        const double2 *x2 = reinterpret_cast<const double2 *>(x + (int64_t)(p2 < 0 ? 0 : p2) * SCOLS);
        const double2 zero = make_double2(0.0, 0.0);
#pragma unroll
        for (int y = 0; y < SCOLS; y += 2) {
            const double2 la = j1 >= 0 ? l1[y >> 1] : zero, lb = j2 >= 0 ? l2[y >> 1] : zero;
            double w0 = 1.0, w1 = 1.0;
            if (reads_x) {
                const double2 xa = p1 >= 0 ? x1[y >> 1] : zero, xb = p2 >= 0 ? x2[y >> 1] : zero;
                w0 = (xa.x - xb.x) / den;
                w1 = (xa.y - xb.y) / den;
            }
            if (y < cols) acc += (la.x - lb.x) * w0;
            if (y + 1 < cols) acc += (la.y - lb.y) * w1;
        }
    } else {
        // (the dense panel's columns, a column solved alone: no line to share, the members one after the other)
#pragma unroll 2
        for (int y = 0; y < cols; ++y) {
            const double D = lead(lam, j1, rs, (int64_t)y * cs) - lead(lam, j2, rs, (int64_t)y * cs);
            double w = 1.0;
            if (reads_x) w = (lead(x, p1, xrs, (int64_t)y * xcs) - lead(x, p2, xrs, (int64_t)y * xcs)) / den;
            acc += D * w;
        }
    }
    grad[i] = acc;
}

// The cross terms of the resistors that drive CCVS / CCCS rows.  One thread per distinct driver g: over the block's
// members in order, and for each over the rows of its group rows[gptr[g] .. gptr[g + 1]) in table order, onto what
// k_gradient_block left at the driver.
__global__ __launch_bounds__(STB) void k_gradient_cross(int64_t ndrivers, int32_t K, int cols,
                                                        const int32_t *__restrict__ drivers,
                                                        const int32_t *__restrict__ gptr,
                                                        const int32_t *__restrict__ rows,
                                                        const uint8_t *__restrict__ type,
                                                        const double *__restrict__ value,
                                                        const int32_t *__restrict__ c, const int32_t *__restrict__ d,
                                                        const int32_t *__restrict__ k, const double *__restrict__ lam,
                                                        int64_t rs, int64_t cs, const double *__restrict__ x, int64_t xrs,
                                                        int64_t xcs, double *__restrict__ grad) {
    const int64_t g = (int64_t)blockIdx.x * STB + threadIdx.x;
    if (g >= ndrivers) return;
    const int32_t i = drivers[g];
    if (type[i] != NODAL_T_R) return;  // (the front end admits no other driver; another one has no term)
    const double v = value[i];
    double acc = grad[i];
    for (int y = 0; y < cols; ++y)
        for (int32_t q = gptr[g]; q < gptr[g + 1]; ++q) {
            const double term =
                cross_term(rows[q], K, v, value, c, d, k, lam, rs, (int64_t)y * cs, x, xrs, (int64_t)y * xcs);
            acc += term;
        }
    grad[i] = acc;
}

// One thread per (member y of the block, swept row j): out[y * nsrc + j] = L(a) - L(b) of an A row, L(m) of an E row.
__global__ __launch_bounds__(STB) void k_gradient_sources(int cols, int32_t nsrc, int32_t K,
                                                          const int32_t *__restrict__ swept,
                                                          const uint8_t *__restrict__ type,
                                                          const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                          const int32_t *__restrict__ k, const double *__restrict__ lam,
                                                          int64_t rs, int64_t cs, double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * STB + threadIdx.x;
    if (t >= (int64_t)cols * nsrc) return;
    const int64_t y = t / nsrc;
    const int32_t i = swept[t - y * nsrc];
    double s = 0.0;
    if (type[i] == NODAL_T_A) s = lead(lam, a[i], rs, y * cs) - lead(lam, b[i], rs, y * cs);
    else if (k[i] >= 0) s = lam[((int64_t)K + k[i]) * rs + y * cs];
    out[t] = s;
}

// the driver's client: the columns are the members' cotangents, a finished block goes through the table kernels
struct GradientClient final : MultiRhsClient {
    nodal_ctx *h;
    int32_t count, nsrc;
    const double *x_host, *cot_host;  // x_host null: the single solve's solution, set aside in sn_x
    const int32_t *swept_dev;
    double *grad_dev, *gsrc_dev;
    double *gsrc_out, *adjoint_out;
    int32_t staged_m0 = 0, staged_cols = 0;  // the cotangent rows gr_cot holds
    GradientClient(nodal_ctx *h_) : h(h_) { max_cols = SCOLS; }

    // [16][n] rows -> element (row, y) at out[row * rs + y * cs]
    int layout(const double *src, int64_t stride, int cols, double *out, int64_t rs, int64_t cs) {
        const int64_t n = h->n;
        if (rs == SCOLS && cs == 1) {
            k_gradient_interleave<<<(unsigned)((n + 63) / 64), 64, 0, h->stream>>>(n, cols, src, stride, out);
        } else {
            if (stride != n) return nodal_fail(h, NODAL_E_INVALID, "gradient: rows of another stride");
            k_gradient_spread<<<groups_of(n * cols, STB), STB, 0, h->stream>>>(n, cols, src, out, rs, cs);
        }
        NODAL_HIP_TRY(h, hipGetLastError());
        return NODAL_OK;
    }
    int build(int32_t m0, int cols, double *out, int64_t rs, int64_t cs) override {
        const int64_t n = h->n;
        if (cols < 1 || cols > SCOLS || m0 < 0 || m0 + cols > count)
            return nodal_fail(h, NODAL_E_INVALID, "gradient: 1 to 16 columns per launch");
        // (a route may ask for the same columns again: the dense route folds twice, a redone column is one of its block's)
        if (m0 < staged_m0 || m0 + cols > staged_m0 + staged_cols) {
            NODAL_HIP_TRY(h, hipMemcpyAsync(h->gr_cot.p, cot_host + (int64_t)m0 * n, (size_t)cols * n * 8,
                                            hipMemcpyHostToDevice, h->stream));
            staged_m0 = m0;
            staged_cols = cols;
        }
        return layout(h->gr_cot.as<double>() + (int64_t)(m0 - staged_m0) * n, n, cols, out, rs, cs);
    }
    int hand_over(int32_t m0, int cols, const double *lam, int64_t rs, int64_t cs, const double *rows) override {
        const int64_t n = h->n, ncomp = h->ncomp;
        hipStream_t st = h->stream;
        if (cols < 1 || cols > SCOLS || m0 < 0 || m0 + cols > count)
            return nodal_fail(h, NODAL_E_INVALID, "gradient: 1 to 16 columns per block");
        if (rows && adjoint_out)
            NODAL_HIP_TRY(h, hipMemcpyAsync(adjoint_out + (int64_t)m0 * n, rows, (size_t)cols * n * 8, hipMemcpyDeviceToHost, st));
        if (ncomp > 0) {
            // the members' solutions in the layout of lam: the staging rows serve directly unless it is interleaved
            const bool il = rs == SCOLS && cs == 1;
            const double *x = h->sn_x.as<double>();
            int64_t xrs = 1, xcs = 0;
            if (x_host) {
                NODAL_HIP_TRY(h, hipMemcpyAsync(h->gr_x.p, x_host + (int64_t)m0 * n, (size_t)cols * n * 8,
                                                hipMemcpyHostToDevice, st));
                x = h->gr_x.as<double>();
                xcs = n;
            }
            if (il) {
                double *xil = h->gr_x.as<double>() + (int64_t)SCOLS * n;
                NODAL_TRY(layout(x, n, cols, xil, SCOLS, 1));
                x = xil;
                xrs = SCOLS;
                xcs = 1;
            }
            NODAL_TRY(grad_launch_table(h, cols, lam, rs, cs, x, xrs, xcs, grad_dev));
            if (nsrc > 0 && gsrc_out) {
                NODAL_TRY(grad_launch_sources(h, cols, nsrc, swept_dev, lam, rs, cs, gsrc_dev));
                NODAL_HIP_TRY(h, hipMemcpyAsync(gsrc_out + (int64_t)m0 * nsrc, gsrc_dev, (size_t)cols * nsrc * 8,
                                                hipMemcpyDeviceToHost, st));
            }
            NODAL_HIP_TRY(h, hipGetLastError());
        }
        NODAL_WAIT_STREAM(h, st);
        return NODAL_OK;
    }
    void all_singular(int32_t cnt) override {
        const double nan = __builtin_nan("");
        if (gsrc_out)
            for (int64_t t = 0; t < (int64_t)cnt * nsrc; ++t) gsrc_out[t] = nan;
        if (adjoint_out)
            for (int64_t t = 0; t < (int64_t)cnt * h->n; ++t) adjoint_out[t] = nan;
    }
};

}  // namespace

int grad_launch_table(nodal_ctx *h, int cols, const double *lam, int64_t rs, int64_t cs, const double *x, int64_t xrs,
                      int64_t xcs, double *grad_dev) {
    const int64_t ncomp = h->ncomp;
    hipStream_t st = h->stream;
    const bool il = rs == SCOLS && cs == 1;
    const double *value = assembled_values(h);
    auto launch = il ? k_gradient_block<true> : k_gradient_block<false>;
    launch<<<groups_of(ncomp, STB), STB, 0, st>>>(ncomp, h->K, cols, h->type.as<uint8_t>(), value, h->a.as<int32_t>(),
                                                  h->b.as<int32_t>(), h->c.as<int32_t>(), h->d.as<int32_t>(),
                                                  h->drv.as<int32_t>(), h->k.as<int32_t>(), lam, rs, cs, x, xrs, xcs,
                                                  grad_dev);
    if (h->sn_ncross > 0) {
        const int32_t *drivers = h->sn_cross.as<int32_t>(), *gptr = drivers + h->sn_ndrivers,
                      *grows = gptr + h->sn_ndrivers + 1;
        k_gradient_cross<<<groups_of(h->sn_ndrivers, STB), STB, 0, st>>>(
            h->sn_ndrivers, h->K, cols, drivers, gptr, grows, h->type.as<uint8_t>(), value, h->c.as<int32_t>(),
            h->d.as<int32_t>(), h->k.as<int32_t>(), lam, rs, cs, x, xrs, xcs, grad_dev);
    }
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

int grad_launch_sources(nodal_ctx *h, int cols, int32_t nsrc, const int32_t *swept_dev, const double *lam, int64_t rs,
                        int64_t cs, double *out) {
    k_gradient_sources<<<groups_of((int64_t)cols * nsrc, STB), STB, 0, h->stream>>>(
        cols, nsrc, h->K, swept_dev, h->type.as<uint8_t>(), h->a.as<int32_t>(), h->b.as<int32_t>(), h->k.as<int32_t>(), lam,
        rs, cs, out);
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

int grad_run(nodal_ctx *h, bool dense, int32_t count, const double *x, const double *cotangent, int32_t nsrc,
             const int64_t *rows, double *grad_out, double *grad_sources_out, double *adjoint_out, double *resid_out,
             int32_t *info_out) {
    const int64_t n = h->n, ncomp = h->ncomp;
    hipStream_t st = h->stream;
    // the swept rows: in range here, independent sources and each named once on the device (one read-back)
    const int32_t pad = (nsrc + 15) & ~15;
    NODAL_HIP_TRY(h, h->gr_spec.reserve((size_t)(pad + 16 + ncomp) * 4 + 64));
    int32_t *swept_dev = h->gr_spec.as<int32_t>();
    if (nsrc > 0)
        NODAL_TRY(sweep_check_rows(h, "gradient: ", "swept row", nsrc, rows, swept_dev, swept_dev + pad + 16,
                                   swept_dev + pad));
    for (int64_t i = 0; i < ncomp; ++i) grad_out[i] = 0.0;
    if (count == 0) return NODAL_OK;
    if (n == 0) {  // (every lead is ground: nothing depends on anything)
        if (grad_sources_out)
            for (int64_t t = 0; t < (int64_t)count * nsrc; ++t) grad_sources_out[t] = 0.0;
        for (int32_t m = 0; m < count; ++m) {
            info_out[m] = 0;
            if (resid_out) resid_out[m] = 0.0;
        }
        return NODAL_OK;
    }
    // the handle is left as it was found.  A solution it holds is set aside: the table kernels read it when the caller
    // brings none, and the multigrid route writes h->x
    HandleKeeper keep;
    NODAL_TRY(keep.save(h, h->have_x));
    NODAL_TRY(sens_cross_list(h));
    const size_t acc_words = ((size_t)ncomp + 1) & ~(size_t)1;
    NODAL_HIP_TRY(h, h->gr_acc.reserve((acc_words + (size_t)SCOLS * nsrc) * 8 + 64));
    NODAL_HIP_TRY(h, h->gr_cot.reserve((size_t)SCOLS * n * 8 + 64));
    NODAL_HIP_TRY(h, h->gr_x.reserve((size_t)2 * SCOLS * n * 8 + 64));
    NODAL_HIP_TRY(h, hipMemsetAsync(h->gr_acc.p, 0, acc_words * 8, st));

    GradientClient client(h);
    client.wants_rows = adjoint_out != nullptr;
    client.count = count;
    client.nsrc = nsrc;
    client.x_host = x;
    client.cot_host = cotangent;
    client.swept_dev = swept_dev;
    client.grad_dev = h->gr_acc.as<double>();
    client.gsrc_dev = client.grad_dev + acc_words;
    client.gsrc_out = grad_sources_out;
    client.adjoint_out = adjoint_out;

    nodal_ctx *s = nullptr;
    NODAL_TRY(adjoint_context(h, &s));
    int status = keep.restore(h, multi_rhs_solve(h, s, dense, count, resid_out, info_out, client), "gradient");
    if (status == NODAL_OK) {
        // the sum is not defined with a member missing
        bool missing = false;
        for (int32_t m = 0; m < count; ++m) missing = missing || info_out[m] > 0;
        if (missing) {
            for (int64_t i = 0; i < ncomp; ++i) grad_out[i] = __builtin_nan("");
        } else if (ncomp > 0 &&
                   hipMemcpyAsync(grad_out, client.grad_dev, (size_t)ncomp * 8, hipMemcpyDeviceToHost, st) != hipSuccess) {
            status = nodal_fail(h, NODAL_E_HIP, "gradient: could not bring the sum down");
        }
    }
    const int w = nodal_wait_stream(h, st, NODAL_SITE);
    if (status == NODAL_OK) status = w;
    return status;
}
