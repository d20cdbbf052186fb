// Branch quantities of a solution: what flows through every component, what it absorbs, and -- for a source sweep --
// the worst case over the members, without the members' solutions leaving HBM.
//
// Replaces a Python loop over Solution.result after Circuit.solve (reference nodal/nodal.py:313-336 returns the
// potentials and the branch unknowns only; the current of a resistor is (e_a - e_b) / R, gathered per component).
//
// Per table row i, e(-1) = +0.0 for the ground lead, K = nums["kcl"]:
//   voltage = e(a) - e(b)                                  one subtraction
//   current = voltage / value        R                     one division (not a product with 1 / value); flows a -> b
//           = value (or the member's swept value)   A      flows b -> a inside the component, into node a
//           = x[K + k]               E, VCVS, CCVS, CCCS   the branch unknown; same direction as A
//   power   = voltage * current      R;   -(voltage * current) otherwise: what the component absorbs
// The product is formed from the stored current in a statement of its own, so that -ffp-contract=on cannot fuse it
// into the sums.  The sums have a fixed shape -- shuffles inside a wavefront, the four wavefronts of a workgroup in
// order, then k_power_totals over the workgroups' partials in a fixed order -- and use no floating-point atomics: a run
// repeats bit for bit.
//
// Envelopes: one thread owns one table row (one node) for the whole sweep and the blocks of a sweep follow each other on
// the handle's stream, so the running maximum is a plain read-modify-write.  It starts as NaN / -1 and is replaced on
// !(m <= best): the first member that counts always wins, and among exact ties the lowest index stays.
#include "table_rows.h"

namespace {

constexpr int BTB = 256;           // threads per workgroup: four wavefronts
constexpr int BWAVES = BTB / 64;
constexpr int BCOLS = 16;          // members per launch of the envelope kernels (SLU_MULTI)

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;  // (lane 0 holds the sum)
}

// lead potentials and the current of one row from one solution vector
struct RowEntry {
    int type;
    double value;
    int32_t a, b, k;
};

__device__ __forceinline__ double row_current(const RowEntry &r, double v, double source_value,
                                              const double *__restrict__ x, int32_t K) {
    if (r.type == NODAL_T_R) return v / r.value;
    if (r.type == NODAL_T_A) return source_value;
    if (r.k >= 0) return x[(int64_t)K + r.k];
    return 0.0;  // (the internal transconductance rows of a presolved table own no branch)
}

__device__ __forceinline__ double row_power(int type, double v, double cur) {
    double p = v * cur;
    if (type != NODAL_T_R) p = -p;
    return p;
}

// One thread per table row.  voltage / current / power may each be null; partials[blockIdx.x * 2 + {0, 1}] = the
// workgroup's power sums over its R rows / its other rows.
__global__ __launch_bounds__(BTB) void k_branch_single(int64_t ncomp, int32_t K, const uint8_t *__restrict__ type,
                                                       const double *__restrict__ value, const int32_t *__restrict__ a,
                                                       const int32_t *__restrict__ b, const int32_t *__restrict__ k,
                                                       const double *__restrict__ x, double *__restrict__ voltage,
                                                       double *__restrict__ current, double *__restrict__ power,
                                                       double *__restrict__ partials) {
    __shared__ double red[BWAVES][2];
    const int64_t i = (int64_t)blockIdx.x * BTB + threadIdx.x;
    double pr = 0.0, ps = 0.0;
    if (i < ncomp) {
        const RowEntry r{type[i], value[i], a[i], b[i], k[i]};
        const double v = lead(x, r.a) - lead(x, r.b);
        const double cur = row_current(r, v, r.value, x, K);
        const double p = row_power(r.type, v, cur);
        if (voltage) voltage[i] = v;
        if (current) current[i] = cur;
        if (power) power[i] = p;
        if (r.type == NODAL_T_R) pr = p;
        else ps = p;
    }
    pr = wave_sum(pr);
    ps = wave_sum(ps);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave][0] = pr;
        red[wave][1] = ps;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < BWAVES; ++w) s += red[w][threadIdx.x];
        partials[(int64_t)blockIdx.x * 2 + threadIdx.x] = s;
    }
}

// One thread per table row, members y < cols of the block rows[y * n + .] (members m0 + y of the sweep).  A member
// whose bit of `mask` is clear is left out of the envelope.  partials[(blockIdx.x * 16 + y) * 2 + {0, 1}] as above,
// per member (left-out members too: the caller overwrites their totals).
__global__ __launch_bounds__(BTB) void k_branch_envelope(int64_t ncomp, int32_t K, int64_t n, int cols, uint32_t mask,
                                                         int32_t m0, const uint8_t *__restrict__ type,
                                                         const double *__restrict__ value, const int32_t *__restrict__ a,
                                                         const int32_t *__restrict__ b, const int32_t *__restrict__ k,
                                                         const int32_t *__restrict__ slot,
                                                         const double *__restrict__ swept, int32_t nsrc,
                                                         const double *__restrict__ rows,
                                                         double *__restrict__ absmax, int32_t *__restrict__ member,
                                                         double *__restrict__ partials) {
    __shared__ double red[BWAVES][BCOLS][2];
    const int64_t i = (int64_t)blockIdx.x * BTB + threadIdx.x;
    const bool live = i < ncomp;
    RowEntry r{NODAL_T_A, 0.0, -1, -1, -1};
    int32_t sl = -1;
    double best = 0.0;
    int32_t who = -1;
    if (live) {
        r = RowEntry{type[i], value[i], a[i], b[i], k[i]};
        sl = slot[i];
        best = absmax[i];
        who = member[i];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int y = 0; y < BCOLS; ++y) {
        double pr = 0.0, ps = 0.0;
        if (live && y < cols) {
            const double *__restrict__ x = rows + (int64_t)y * n;
            const double v = lead(x, r.a) - lead(x, r.b);
            const double src = sl >= 0 ? swept[(int64_t)y * nsrc + sl] : r.value;
            const double cur = row_current(r, v, src, x, K);
            const double p = row_power(r.type, v, cur);
            if (r.type == NODAL_T_R) pr = p;
            else ps = p;
            const double m = fabs(cur);
            if (((mask >> y) & 1u) && !(m <= best)) {
                best = m;
                who = m0 + y;
            }
        }
        pr = wave_sum(pr);
        ps = wave_sum(ps);
        if (lane == 0) {
            red[wave][y][0] = pr;
            red[wave][y][1] = ps;
        }
    }
    if (live) {
        absmax[i] = best;
        member[i] = who;
    }
    __syncthreads();
    if (threadIdx.x < BCOLS * 2) {
        const int y = threadIdx.x >> 1, w2 = threadIdx.x & 1;
        double s = red[0][y][w2];
#pragma unroll
        for (int w = 1; w < BWAVES; ++w) s += red[w][y][w2];
        partials[(int64_t)blockIdx.x * (BCOLS * 2) + threadIdx.x] = s;
    }
}

// One thread per node j < K over the same block: running minimum / maximum of the potential and their members.
__global__ __launch_bounds__(BTB) void k_node_envelope(int32_t K, int64_t n, int cols, uint32_t mask, int32_t m0,
                                                       const double *__restrict__ rows, double *__restrict__ pmin,
                                                       int32_t *__restrict__ pmin_member, double *__restrict__ pmax,
                                                       int32_t *__restrict__ pmax_member) {
    const int64_t j = (int64_t)blockIdx.x * BTB + threadIdx.x;
    if (j >= K) return;
    double lo = pmin[j], hi = pmax[j];
    int32_t lom = pmin_member[j], him = pmax_member[j];
#pragma unroll
    for (int y = 0; y < BCOLS; ++y) {
        if (y >= cols || !((mask >> y) & 1u)) continue;
        const double v = rows[(int64_t)y * n + j];
        if (!(v >= lo)) {
            lo = v;
            lom = m0 + y;
        }
        if (!(v <= hi)) {
            hi = v;
            him = m0 + y;
        }
    }
    pmin[j] = lo;
    pmin_member[j] = lom;
    pmax[j] = hi;
    pmax_member[j] = him;
}

// The fixed-order second pass: out[j] = sum over workgroups g of partials[g * stride + j], j = blockIdx.x < stride.
// Thread t adds the partials t, t + 256, ... one after the other, then the 256 threads are summed as above.
__global__ __launch_bounds__(BTB) void k_power_totals(int64_t groups, int stride, const double *__restrict__ partials,
                                                      double *__restrict__ out) {
    __shared__ double red[BWAVES];
    const int j = blockIdx.x;
    double s = 0.0;
    for (int64_t g = threadIdx.x; g < groups; g += BTB) s += partials[g * stride + j];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = red[0];
#pragma unroll
        for (int w = 1; w < BWAVES; ++w) t += red[w];
        out[j] = t;
    }
}

}  // namespace

// voltage / current / power [ncomp] and totals2 = {dissipated, absorbed_by_sources} of the solution in h->x, to the
// host; each may be null
int branch_single(nodal_ctx *h, double *voltage, double *current, double *power, double *totals2) {
    const int64_t ncomp = h->ncomp;
    if (totals2) totals2[0] = totals2[1] = 0.0;
    if (ncomp == 0) return NODAL_OK;
    hipStream_t st = h->stream;
    const int64_t groups = groups_of(ncomp, BTB);
    double *out[3] = {voltage, current, power};
    int wanted = 0;
    for (double *p : out) wanted += p ? 1 : 0;
    NODAL_HIP_TRY(h, h->br_out.reserve((size_t)wanted * ncomp * 8 + 64));
    NODAL_HIP_TRY(h, h->br_part.reserve((size_t)groups * 2 * 8 + 2 * 8 + 64));
    double *dev[3] = {nullptr, nullptr, nullptr};
    for (int q = 0, at = 0; q < 3; ++q)
        if (out[q]) dev[q] = h->br_out.as<double>() + (int64_t)(at++) * ncomp;
    double *partials = h->br_part.as<double>(), *totals = partials + groups * 2;
    k_branch_single<<<(unsigned)groups, BTB, 0, st>>>(ncomp, h->K, h->type.as<uint8_t>(), assembled_values(h),
                                                     h->a.as<int32_t>(), h->b.as<int32_t>(), h->k.as<int32_t>(),
                                                     h->x.as<double>(), dev[0], dev[1], dev[2], partials);
    k_power_totals<<<2, BTB, 0, st>>>(groups, 2, partials, totals);
    NODAL_HIP_TRY(h, hipGetLastError());
    for (int q = 0; q < 3; ++q)
        if (out[q]) NODAL_HIP_TRY(h, hipMemcpyAsync(out[q], dev[q], (size_t)ncomp * 8, hipMemcpyDeviceToHost, st));
    if (totals2) return nodal_read_words(h, totals2, totals, 16);  // (waits: the copies above are done too)
    NODAL_WAIT_STREAM(h, st);
    return NODAL_OK;
}

// ---- sweep envelopes: begin (buffers, NaN / -1), one call per handed-over block, finish (to the host) ----

int branch_sweep_begin(nodal_ctx *h, BranchSweep *env, int32_t count) {
    const int64_t ncomp = h->ncomp, K = h->K;
    const int64_t groups = groups_of(ncomp, BTB);
    // doubles first (absmax [ncomp], min [K], max [K]), then their members as int32
    const size_t doubles = (size_t)(ncomp + 2 * K), bytes = doubles * 8 + doubles * 4;
    NODAL_HIP_TRY(h, h->br_env.reserve(bytes + 64));
    NODAL_HIP_TRY(h, h->br_part.reserve((size_t)groups * BCOLS * 2 * 8 + 64));
    NODAL_HIP_TRY(h, h->br_tot.reserve((size_t)count * 2 * 8 + 64));
    env->absmax = h->br_env.as<double>();
    env->pmin = env->absmax + ncomp;
    env->pmax = env->pmin + K;
    env->absmax_member = reinterpret_cast<int32_t *>(env->pmax + K);
    env->pmin_member = env->absmax_member + ncomp;
    env->pmax_member = env->pmin_member + K;
    env->partials = h->br_part.as<double>();
    env->totals = h->br_tot.as<double>();
    // 0xFF bytes: NaN as doubles, -1 as integers
    if (bytes) NODAL_HIP_TRY(h, hipMemsetAsync(h->br_env.p, 0xFF, bytes, h->stream));
    if (count > 0) NODAL_HIP_TRY(h, hipMemsetAsync(env->totals, 0xFF, (size_t)count * 2 * 8, h->stream));
    return NODAL_OK;
}

// members m0 .. m0 + cols - 1, final rows [cols][n] on the device; info: the sweep's flags (host), all settled
int branch_sweep_block(nodal_ctx *h, const BranchSweep *env, int32_t m0, int cols, const double *rows,
                       const int32_t *info, const double *swept_dev, const int32_t *slot_dev, int32_t nsrc) {
    const int64_t ncomp = h->ncomp, n = h->n;
    const int64_t groups = groups_of(ncomp, BTB);
    hipStream_t st = h->stream;
    for (int g0 = 0; g0 < cols; g0 += BCOLS) {
        const int c = cols - g0 < BCOLS ? cols - g0 : BCOLS;
        uint32_t mask = 0;
        for (int y = 0; y < c; ++y)
            if (info[m0 + g0 + y] == 0) mask |= 1u << y;
        if (!mask) continue;  // (nothing of this group counts: its totals stay NaN)
        const double *blk = rows + (int64_t)g0 * n;
        if (ncomp > 0) {
            k_branch_envelope<<<(unsigned)groups, BTB, 0, st>>>(
                ncomp, h->K, n, c, mask, m0 + g0, h->type.as<uint8_t>(), assembled_values(h), h->a.as<int32_t>(),
                h->b.as<int32_t>(), h->k.as<int32_t>(), slot_dev, swept_dev + (int64_t)(m0 + g0) * nsrc, nsrc, blk,
                env->absmax, env->absmax_member, env->partials);
            k_power_totals<<<c * 2, BTB, 0, st>>>(groups, BCOLS * 2, env->partials, env->totals + (int64_t)(m0 + g0) * 2);
        }
        if (h->K > 0)
            k_node_envelope<<<(unsigned)((h->K + BTB - 1) / BTB), BTB, 0, st>>>(h->K, n, c, mask, m0 + g0, blk, env->pmin,
                                                                               env->pmin_member, env->pmax,
                                                                               env->pmax_member);
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    return NODAL_OK;
}

// the envelope to the caller's arrays (each may be null); members with info > 0 get NaN totals.  With every member
// left out nothing of the device's is used: NaN and -1 throughout.
int branch_sweep_finish(nodal_ctx *h, const BranchSweep *env, int32_t count, const int32_t *info) {
    const int64_t ncomp = h->ncomp, K = h->K;
    hipStream_t st = h->stream;
    const double nan = __builtin_nan("");
    bool any = false;
    for (int32_t m = 0; m < count; ++m) any = any || info[m] == 0;
    struct { void *dst; const void *src; size_t items, size; } copies[] = {
        {env->out_absmax, env->absmax, (size_t)ncomp, 8}, {env->out_absmax_member, env->absmax_member, (size_t)ncomp, 4},
        {env->out_pmin, env->pmin, (size_t)K, 8},         {env->out_pmin_member, env->pmin_member, (size_t)K, 4},
        {env->out_pmax, env->pmax, (size_t)K, 8},         {env->out_pmax_member, env->pmax_member, (size_t)K, 4},
        {env->out_power, env->totals, (size_t)count * 2, 8}};
    for (const auto &c : copies) {
        if (!c.dst || !c.items) continue;
        if (any) {
            NODAL_HIP_TRY(h, hipMemcpyAsync(c.dst, c.src, c.items * c.size, hipMemcpyDeviceToHost, st));
        } else if (c.size == 8) {
            for (size_t t = 0; t < c.items; ++t) static_cast<double *>(c.dst)[t] = nan;
        } else {
            for (size_t t = 0; t < c.items; ++t) static_cast<int32_t *>(c.dst)[t] = -1;
        }
    }
    NODAL_WAIT_STREAM(h, st);
    if (env->out_power)
        for (int32_t m = 0; m < count; ++m)
            if (info[m] != 0) env->out_power[2 * m] = env->out_power[2 * m + 1] = nan;
    return NODAL_OK;
}
