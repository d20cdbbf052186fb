// Multiport Thevenin / Norton equivalents: what the network looks like from chosen ports.
//
// Replaces a loop of equivalent_resistance over node pairs (reference nodal/equiv.py:31-61: one deepcopy + Circuit + solve
// per pair, resistive networks only, the diagonal number R(a, b) alone); the reference has no equivalent of an active
// network and no coupling between ports.
//
// A port q is an ordered pair of nodes (a_q, b_q), either may be ground (-1, potential +0.0).  With G the assembled
// matrix (n = K + B unknowns) and s_q = e(a_q) - e(b_q) (zeros in the B branch rows), x_q solves G x_q = s_q -- G itself,
// not its transpose; the independent sources are off, the dependent ones live in G -- and
//     Z[p][q] = x_q[a_p] - x_q[b_p]         volts at port p per ampere entering a_q and leaving b_q
//     V_oc[p] = x[a_p] - x[b_p]             for the solution x of the last single solve
// so that v = V_oc + Z i for any external currents i.  A port with a_q == b_q has an all-zero column and row.
//
// The solves are multi_rhs_solve's (sparse.hip), as the source sweep's, with the PortClient below: k_port_rhs builds a
// block of right-hand sides where a sweep folds its members' sources, and k_port_gather reads a finished block at the
// port nodes into Z on the device where a sweep's rows would go down to the host.
// Z comes down once, P x P numbers instead of P x n.  No floating-point atomics: a repeated call returns the same bits.
#include "table_rows.h"

namespace {

constexpr int PTB = 256;
constexpr int PORT_CHUNK = 512;  // columns one hand-over brings at most (the dense route's chunk)

// One thread per column y < cols of a zeroed block, element (row, y) at out[row * rs + y * cs]: the <= 2 entries of s_q.
// Both adds by the same thread, in order: a == b gives exactly 0.
__global__ __launch_bounds__(64) void k_port_rhs(int cols, const int32_t *__restrict__ ia, const int32_t *__restrict__ ib,
                                                 double *__restrict__ out, int64_t rs, int64_t cs) {
    const int y = threadIdx.x;
    if (y >= cols) return;
    double *col = out + (int64_t)y * cs;
    const int32_t a = ia[y], b = ib[y];
    if (a >= 0) col[(int64_t)a * rs] += 1.0;
    if (b >= 0) col[(int64_t)b * rs] -= 1.0;
}

// the columns of one hand-over whose member is flagged singular, one bit each
struct PortFlags { uint32_t word[PORT_CHUNK / 32]; };

// One thread per (port p, column y) of a finished block X, element (row, y) at x[row * rs + y * cs]:
// out[p * ld + m0 + y] = X(a_p, y) - X(b_p, y), a ground lead reading +0.0; NaN in every row of a flagged column.
__global__ __launch_bounds__(PTB) void k_port_gather(int32_t nports, int cols, int32_t m0, const int32_t *__restrict__ ia,
                                                     const int32_t *__restrict__ ib, const double *__restrict__ x,
                                                     int64_t rs, int64_t cs, PortFlags bad, double *__restrict__ out,
                                                     int64_t ld) {
    const int64_t t = (int64_t)blockIdx.x * PTB + threadIdx.x;
    const int64_t p = t / cols;
    const int y = (int)(t - p * cols);
    if (p >= nports || y >= cols) return;
    double v;
    if ((bad.word[y >> 5] >> (y & 31)) & 1u) {
        v = __builtin_nan("");
    } else {
        const int32_t a = ia[p], b = ib[p];
        const double *col = x + (int64_t)y * cs;
        const double xa = a >= 0 ? col[(int64_t)a * rs] : 0.0;
        const double xb = b >= 0 ? col[(int64_t)b * rs] : 0.0;
        v = xa - xb;
    }
    out[p * ld + m0 + y] = v;
}

}  // namespace

int port_rhs_block(nodal_ctx *h, const PortCall *call, int32_t m0, int cols, double *out, int64_t rs, int64_t cs) {
    if (cols < 1 || cols > SLU_MULTI || m0 < 0 || m0 + cols > call->nports)
        return nodal_fail(h, NODAL_E_INVALID, "port rhs: 1 to 16 columns of the call per launch");
    k_port_rhs<<<1, 64, 0, h->stream>>>(cols, call->ia + m0, call->ib + m0, out, rs, cs);
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

int port_gather_block(nodal_ctx *h, const PortCall *call, int32_t m0, int cols, const double *rows,
                      const int32_t *info) {
    if (cols < 1 || cols > PORT_CHUNK || m0 < 0 || m0 + cols > call->nports)
        return nodal_fail(h, NODAL_E_INVALID, "port gather: a block outside the call's columns");
    PortFlags bad = {};
    for (int y = 0; y < cols; ++y)
        if (info[m0 + y] > 0) bad.word[y >> 5] |= 1u << (y & 31);
    const int64_t P = call->nports;
    k_port_gather<<<groups_of(P * cols, PTB), PTB, 0, h->stream>>>(call->nports, cols, m0, call->ia, call->ib, rows, 1, h->n, bad,
                                                                  call->z, P);
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

namespace {
// the driver's client: the columns are the ports' unit injections, a finished block is read at the port nodes
struct PortClient final : MultiRhsClient {
    nodal_ctx *h;
    const PortCall *call;
    const int32_t *info;  // the driver's flags (host), settled for a block by the time it is handed over
    PortClient(nodal_ctx *h_, const PortCall *call_, const int32_t *info_) : h(h_), call(call_), info(info_) {
        max_cols = PORT_CHUNK;
    }
    int build(int32_t m0, int cols, double *out, int64_t rs, int64_t cs) override {
        return port_rhs_block(h, call, m0, cols, out, rs, cs);
    }
    int hand_over(int32_t m0, int cols, const double *, int64_t, int64_t, const double *rows) override {
        NODAL_TRY(port_gather_block(h, call, m0, cols, rows, info));
        NODAL_WAIT_STREAM(h, h->stream);
        return NODAL_OK;
    }
    void all_singular(int32_t) override {}  // (port_run fills the columns of Z from info)
};
}  // namespace

int port_run(nodal_ctx *h, bool dense, int32_t nports, const int32_t *ia, const int32_t *ib, double *z_out,
             double *voc_out, double *resid_out, int32_t *info_out) {
    const int64_t n = h->n, P = nports;
    hipStream_t st = h->stream;
    for (int32_t q = 0; q < nports; ++q)
        if (ia[q] < -1 || ia[q] >= h->K || ib[q] < -1 || ib[q] >= h->K)
            return nodal_fail(h, NODAL_E_INVALID, "port matrix: node index out of range");
    if (n == 0) {  // (every lead is ground)
        for (int64_t t = 0; t < P * P; ++t) z_out[t] = 0.0;
        for (int32_t q = 0; q < nports; ++q) {
            info_out[q] = 0;
            if (voc_out) voc_out[q] = 0.0;
            if (resid_out) resid_out[q] = 0.0;
        }
        return NODAL_OK;
    }
    // the ports (ia | ib as int32 [P] each, padded to a double), then Z [P][P] and V_oc [P]
    const size_t words = ((size_t)2 * P + 1) & ~(size_t)1;
    NODAL_HIP_TRY(h, h->pt_buf.reserve(words * 4 + (size_t)(P * P + P) * 8 + 64));
    int32_t *ia_dev = h->pt_buf.as<int32_t>(), *ib_dev = ia_dev + P;
    double *z_dev = reinterpret_cast<double *>(ia_dev + words), *voc_dev = z_dev + P * P;
    NODAL_HIP_TRY(h, hipMemcpyAsync(ia_dev, ia, (size_t)P * 4, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(ib_dev, ib, (size_t)P * 4, hipMemcpyHostToDevice, st));
    // the handle is left as it was found: the single solve's solution is set aside (the multigrid route writes h->x)
    // and V_oc read from the copy
    HandleKeeper keep;
    NODAL_TRY(keep.save(h, h->have_x));
    if (voc_out) {
        k_port_gather<<<groups_of(P, PTB), PTB, 0, st>>>(nports, 1, 0, ia_dev, ib_dev, h->sn_x.as<double>(), 1, n, PortFlags{},
                                                        voc_dev, 1);
        NODAL_HIP_TRY(h, hipGetLastError());
        NODAL_HIP_TRY(h, hipMemcpyAsync(voc_out, voc_dev, (size_t)P * 8, hipMemcpyDeviceToHost, st));
    }
    NODAL_WAIT_STREAM(h, st);  // (the copies up read the caller's arrays)

    PortCall call;
    call.nports = nports;
    call.ia = ia_dev;
    call.ib = ib_dev;
    call.z = z_dev;
    PortClient client(h, &call, info_out);
    int status = keep.restore(h, multi_rhs_solve(h, h, dense, nports, resid_out, info_out, client), "port matrix");
    if (status == NODAL_OK && hipMemcpyAsync(z_out, z_dev, (size_t)(P * P) * 8, hipMemcpyDeviceToHost, st) != hipSuccess)
        status = nodal_fail(h, NODAL_E_HIP, "port matrix: could not bring Z down");
    const int w = nodal_wait_stream(h, st, NODAL_SITE);
    if (status == NODAL_OK) status = w;
    if (status != NODAL_OK) return status;
    // a member the sweep declared singular without handing it over (a floating island, a singular G: every member)
    const double nan = __builtin_nan("");
    for (int32_t q = 0; q < nports; ++q)
        if (info_out[q] > 0)
            for (int64_t p = 0; p < P; ++p) z_out[p * P + q] = nan;
    return NODAL_OK;
}
