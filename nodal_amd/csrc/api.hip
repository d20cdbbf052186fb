// extern "C" entry points of libnodal_hip.so (see include/nodal_hip.h).
#include <stdlib.h>
#include <string.h>

#include "ctx.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

int dense_prepare(nodal_ctx *h);  // sparse.hip
int pair_read_host(nodal_ctx *h, const double *x, int32_t ia, int32_t ib, double *out);  // sparse.hip
int nodal_upload_internal(nodal_ctx *h, int64_t ncomp, const uint8_t *type, const double *value,
                          const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d,
                          const int32_t *drv, const int32_t *k, int32_t K, int32_t B);

// Host threads inside an API call right now, process-wide (nested calls of one thread count once).  A solve that
// has the device to itself spreads independent pieces over streams of its own (the multigrid setup's second stream,
// the direct route's lanes); with several solves in flight -- one context and host thread each -- the extra queues
// only get in each other's way (four contexts with two streams each: 232 -> 178 circuits/s), and the solves overlap
// anyway.
static std::atomic<int> g_calls_in_flight{0};
static thread_local int t_call_depth = 0;
int nodal_calls_in_flight() { return g_calls_in_flight.load(std::memory_order_relaxed); }
// Handles alive in the process.  (The runtime spreads a process's streams over a handful of hardware queues: a second
// stream per handle makes the main streams of four handles share queues -- four solves in flight, symbolic phases
// kept: 232 -> 181 circuits/s even with the extra streams idle, and a stream created while another handle's extra
// stream exists keeps its shared queue after that one is gone.  Hence extra streams are an OPTION of the handle.)
static std::atomic<int> g_live_handles{0};
int nodal_live_handles() { return g_live_handles.load(std::memory_order_relaxed); }
bool nodal_extra_streams_ok(const nodal_ctx *ctx) {  // the handle was told it is alone (NODAL_OPT_EXTRA_STREAMS) and no other call runs
    const nodal_ctx *h = ctx->stream_owner ? ctx->stream_owner : ctx;
    return h->extra_streams && nodal_calls_in_flight() <= 1;
}

namespace {

// selects the handle's device for the duration of an API call and gives the calling
// thread its own current device back afterwards
struct DeviceGuard {
    int prev = -1;
    FillStreamScope fill;
    explicit DeviceGuard(nodal_ctx *h) : fill(h->stream) {
        if (t_call_depth++ == 0) g_calls_in_flight.fetch_add(1, std::memory_order_relaxed);
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != h->device) (void)hipSetDevice(h->device);
        else prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
        if (--t_call_depth == 0) g_calls_in_flight.fetch_sub(1, std::memory_order_relaxed);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

template <class T>
int upload(nodal_ctx *h, DevBuf &buf, const T *src, int64_t count) {
    NODAL_HIP_TRY(h, buf.reserve((size_t)count * sizeof(T) + 16));
    if (count > 0)
        NODAL_HIP_TRY(h, hipMemcpyAsync(buf.p, src, (size_t)count * sizeof(T),
                                        hipMemcpyHostToDevice, h->stream));
    return NODAL_OK;
}

// Range check of the uploaded table ON THE DEVICE (a kernel must never see an out-of-range node; the
// host loop that did this walked 2e6 rows x 8 columns on one thread: half of the upload time of the
// 1e6-node grid).  *bad = first offending row (~0 if none).
__global__ __launch_bounds__(256) void validate_table(int64_t ncomp, int32_t K, int32_t B,
                                                      const uint8_t *__restrict__ type, const int32_t *__restrict__ a,
                                                      const int32_t *__restrict__ b, const int32_t *__restrict__ c,
                                                      const int32_t *__restrict__ d, const int32_t *__restrict__ drv,
                                                      const int32_t *__restrict__ k, unsigned long long *__restrict__ bad) {
    unsigned sources = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ncomp; i += (int64_t)gridDim.x * 256) {
        const uint8_t t = type[i];
        const bool branch = t >= NODAL_T_E && t <= NODAL_T_CCCS;
        const int32_t ci = c ? c[i] : -1, di = d ? d[i] : -1, ri = drv ? drv[i] : -1, ki = k ? k[i] : -1;
        // (a plain table -- no c / d / drv / k columns -- can only hold resistors and current sources: any other
        // row would stamp nothing, silently)
        const bool plain_ok = c != nullptr || t == NODAL_T_R || t == NODAL_T_A;
        const bool ok = t <= NODAL_T_GM && plain_ok && a[i] >= -1 && a[i] < K && b[i] >= -1 && b[i] < K && ci >= -1 &&
                        ci < K && di >= -1 && di < K && ri >= -1 && ri < ncomp && ki >= -1 && ki < B &&
                        (branch == (ki >= 0));
        if (!ok) atomicMin(bad, (unsigned long long)i);
        sources += (t == NODAL_T_A || t == NODAL_T_E) ? 1u : 0u;
    }
    // how many components stamp the right-hand side (bad[1]): lets the symbolic phase group a handful of rhs
    // stamps with two launches instead of thirteen.  One atomic per workgroup that has any.
    __shared__ unsigned wsum[4];
    for (int off = 32; off > 0; off >>= 1) sources += __shfl_down(sources, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sources;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (tot) atomicAdd(bad + 1, (unsigned long long)tot);
    }
}

// rec: (row, c, d, drv, k) of the rows that read those columns (packed by the host: nodal_upload_internal)
__global__ __launch_bounds__(256) void place_dependent_rows(int64_t count, const int32_t *__restrict__ rec, int64_t ncomp,
                                                            int32_t *__restrict__ c, int32_t *__restrict__ d,
                                                            int32_t *__restrict__ drv, int32_t *__restrict__ k) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= count) return;
    const int32_t row = rec[5 * q];
    if (row < 0 || row >= ncomp) return;
    c[row] = rec[5 * q + 1];
    d[row] = rec[5 * q + 2];
    drv[row] = rec[5 * q + 3];
    k[row] = rec[5 * q + 4];
}

double elapsed(nodal_ctx *h, int a, int b) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev[a], h->ev[b]) != hipSuccess) return 0.0;
    return ms;
}

}  // namespace

extern "C" {

const char *nodal_version(void) { return "nodal_hip 0.1 gfx950"; }

int nodal_create(int device_id, nodal_handle *out) {
    if (!out) return NODAL_E_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count)
        return NODAL_E_HIP;
    nodal_ctx *h = new nodal_ctx();
    h->device = device_id;
    // main stream: highest priority -- it carries the latency-critical chains (LU panel
    // factorisation, multigrid cycles)
    int lo = 0, hi = 0;  // least / greatest priority
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (const char *e = knob::STREAM_PRIORITY.now())  // "normal": the default priority instead of the highest
        if (e[0] == 'n') hi = 0;
    if (hipSetDevice(device_id) != hipSuccess ||
        hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, hi) != hipSuccess) {
        delete h;
        return NODAL_E_HIP;
    }
    for (auto &e : h->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            delete h;
            return NODAL_E_HIP;
        }
    if (const auto v = knob::DENSE_BLOCKINV.now()) h->dense_blockinv = *v != 0;
    if (const auto v = knob::GJ_SCALAR.now()) h->gj_scalar = *v;
    if (const auto v = knob::GEPP_PANEL.now()) h->gepp_panel = *v != 0;
    if (const auto v = knob::PRESOLVE.now()) h->use_presolve = *v != 0;  // 0: branch equations stay in the system
    if (const auto v = knob::EXTRA_STREAMS.now()) h->extra_streams = *v != 0;
    g_live_handles.fetch_add(1, std::memory_order_relaxed);
    *out = h;
    return NODAL_OK;
}

}  // extern "C"


void *nodal_pinned(nodal_ctx *ctx) {
    nodal_ctx *h = ctx->stream_owner ? ctx->stream_owner : ctx;
    if (!h->pinned && hipHostMalloc(&h->pinned, NODAL_PINNED_BYTES, hipHostMallocDefault) != hipSuccess) {
        h->pinned = nullptr;
        (void)hipGetLastError();
    }
    return h->pinned;
}

void *nodal_pinned_arena(nodal_ctx *ctx, size_t bytes) {
    nodal_ctx *h = ctx->stream_owner ? ctx->stream_owner : ctx;
    if (bytes <= h->arena_bytes) return h->arena;
    if (h->arena) (void)hipHostFree(h->arena);
    h->arena = nullptr;
    h->arena_bytes = 0;
    const size_t want = bytes + (bytes >> 2) + 4096;
    if (hipHostMalloc(&h->arena, want, hipHostMallocDefault) != hipSuccess) {
        h->arena = nullptr;
        (void)hipGetLastError();
        return nullptr;
    }
    h->arena_bytes = want;
    return h->arena;
}

int nodal_read_words(nodal_ctx *h, void *dst, const void *dev_src, size_t bytes) {
    void *pin = bytes <= NODAL_PINNED_BYTES ? nodal_pinned(h) : nullptr;
    NODAL_HIP_TRY(h, hipMemcpyAsync(pin ? pin : dst, dev_src, bytes, hipMemcpyDeviceToHost, h->stream));
    NODAL_WAIT_STREAM(h, h->stream);
    if (pin) memcpy(dst, pin, bytes);
    return NODAL_OK;
}

int nodal_ensure_aux_streams(nodal_ctx *ctx) {
    nodal_ctx *h = ctx->stream_owner ? ctx->stream_owner : ctx;
    if (!h->stream2 || !h->stream3) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(h->device);
        int lo = 0, hi = 0;  // least / greatest priority
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        int status = NODAL_OK;
        // second stream for the dense LU's trailing updates (lookahead).  It is confined to
        // 224 of the 256 CUs: the panel chain on the main stream is a sequence of small
        // latency-bound kernels and must always find idle CUs, otherwise every one of its
        // ~1300 launches queues behind 58-us GEMM workgroups.  (If the CU mask is refused,
        // fall back to a low-priority stream.)
        if (!h->stream2) {
            uint32_t mask[8];
            int reserve = knob::PANEL_CUS.now();  // CUs kept free for the main stream
            if (reserve < 0) reserve = 0;
            if (reserve > 224) reserve = 224;
            for (int i = 0; i < 8; ++i) mask[i] = 0xFFFFFFFFu;
            for (int cu = 0; cu < reserve; ++cu) mask[cu / 32] &= ~(1u << (cu % 32));
            if (hipExtStreamCreateWithCUMask(&h->stream2, 8, mask) != hipSuccess) {
                h->stream2 = nullptr;
                (void)hipGetLastError();
            }
            if (!h->stream2 && hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, lo) != hipSuccess) status = NODAL_E_HIP;
        }
        if (status == NODAL_OK && !h->stream3 &&
            hipStreamCreateWithPriority(&h->stream3, hipStreamNonBlocking, lo) != hipSuccess) status = NODAL_E_HIP;
        for (auto &e : h->ev_la)
            if (status == NODAL_OK && !e &&
                hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess) status = NODAL_E_HIP;
        for (auto &e : h->ev_bi)
            if (status == NODAL_OK && !e &&
                hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventReleaseToDevice) != hipSuccess) status = NODAL_E_HIP;
        if (prev >= 0) (void)hipSetDevice(prev);
        if (status != NODAL_OK) return nodal_fail(ctx, status, "could not create the dense paths' streams");
    }
    if (ctx != h) {
        ctx->stream2 = h->stream2;
        ctx->stream3 = h->stream3;
        for (int i = 0; i < 2; ++i) ctx->ev_la[i] = h->ev_la[i];
        for (int i = 0; i < 6; ++i) ctx->ev_bi[i] = h->ev_bi[i];
    }
    return NODAL_OK;
}

void nodal_free_buffers(nodal_ctx *h) {
    amg_destroy(h);
    sagg_destroy(h);
    slu_destroy(h);
    presolve_free_plan(h);
    nodal_free_block_child(h);
    sens_free_child(h);
    ac_free_child(h);
    if (h->reduced) {
        nodal_free_buffers(h->reduced);
        delete h->reduced;
        h->reduced = nullptr;
    }
    if (h->lowdeg) {
        nodal_free_buffers(h->lowdeg);
        delete h->lowdeg;
        h->lowdeg = nullptr;
    }
    DevBuf *bufs[] = {&h->type, &h->value, &h->a, &h->b, &h->c, &h->d, &h->drv, &h->k,
                      &h->values_batch, &h->indptr, &h->indices, &h->rowidx, &h->cptr,
                      &h->contrib, &h->rhs_row, &h->rhs_cptr, &h->rhs_contrib, &h->diag_pos,
                      &h->data, &h->rhs, &h->status, &h->x, &h->dense, &h->piv, &h->work,
                      &h->work2, &h->work3, &h->solver, &h->krylov, &h->gn_indptr, &h->gn_indices,
                      &h->gn_rowidx, &h->gn_data, &h->gn_diag, &h->schur, &h->ps_buf, &h->ps_newidx,
                      &h->ps_hits, &h->ps_stage, &h->grounded, &h->ld_newidx, &h->ld_work, &h->batch_scale, &h->rhs_none,
                      &h->sw_rows, &h->sw_slot, &h->sw_vals, &h->sw_blk, &h->br_out, &h->br_part, &h->br_tot,
                      &h->br_env, &h->sn_x, &h->sn_spec, &h->sn_out, &h->sn_cross, &h->sn_perm, &h->pt_buf,
                      &h->gr_cot, &h->gr_x, &h->gr_spec, &h->gr_acc,
                      &h->tr_spec, &h->tr_none, &h->tr_node, &h->tr_ptr, &h->tr_con, &h->tr_vec, &h->tr_out, &h->tr_ring,
                      &h->tr_ind, &h->tn_spec, &h->tn_none, &h->tn_node, &h->tn_ptr, &h->tn_con,
                      &h->nb_spec, &h->nb_none, &h->nb_node, &h->nb_ptr, &h->nb_con,
                      &h->tb_spec, &h->tb_none, &h->tb_node, &h->tb_ptr, &h->tb_con,
                      &h->tr_tape, &h->tr_tsrc, &h->tg_vec, &h->tg_out, &h->tg_spec, &h->tg_none, &h->tg_node, &h->tg_ptr,
                      &h->tg_con,
                      &h->ac_gsrc, &h->ac_ptr, &h->ac_con, &h->ac_spec, &h->ac_vec, &h->ac_out, &h->ac_ring,
                      &h->ac_t_gsrc, &h->ac_t_ptr, &h->ac_t_con, &h->nz_vec, &h->nz_part, &h->nz_out,
                      &h->ap_vec, &h->ap_rows, &h->ap_out, &h->ag_vec, &h->ag_out,
                      &h->dbg_resid, &h->dbg_apply, &h->dbg_lowdeg};
    for (DevBuf *b : bufs) b->release();
    for (auto &e : h->evpool) (void)hipEventDestroy(e);
    h->evpool.clear();
}

// NODAL_POISON=2: every buffer that carries nothing from one solve to the next -- the solution, the dense
// panel, the scratch and Krylov areas -- becomes 0xFF bytes (NaNs / -1) in this context and its child
// contexts, in order on the handle's stream: the state a pooled handle is in after a singular solve of a
// larger system.  A kernel that reads a slot of these before writing it shows up as a NaN or a fault.
void nodal_poison_scratch(nodal_ctx *h) {
    if (nodal_poison_level() < 2 || !h) return;
    DevBuf *bufs[] = {&h->x, &h->dense, &h->piv, &h->work, &h->work2, &h->work3, &h->solver, &h->krylov,
                      &h->ld_work, &h->schur, &h->batch_x, &h->batch_scale, &h->rhs_none, &h->sw_blk};
    for (DevBuf *b : bufs) b->poison(h->stream);
    slu_poison(h);
    nodal_poison_scratch(h->reduced);
    nodal_poison_scratch(h->lowdeg);
    nodal_poison_scratch(h->blocksys);
    nodal_poison_scratch(h->adjoint);
    nodal_poison_scratch(h->ac);
    nodal_poison_scratch(h->ac_t);
}

void nodal_nan_probe(nodal_ctx *h, const double *dev, int64_t n, const char *tag) {
    static const bool on = knob::NANCHECK.now();
    if (!on || !dev || n <= 0) return;
    std::vector<double> host((size_t)n);
    if (nodal_wait_stream(h, h->stream, NODAL_SITE) != NODAL_OK ||
        hipMemcpyAsync(host.data(), dev, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        nodal_wait_stream(h, h->stream, NODAL_SITE) != NODAL_OK) {
        fprintf(stderr, "[nancheck] %s: copy failed\n", tag);
        return;
    }
    int64_t bad = 0, first = -1;
    for (int64_t i = 0; i < n; ++i)
        if (!(host[i] - host[i] == 0.0)) {
            if (first < 0) first = i;
            ++bad;
        }
    fprintf(stderr, "[nancheck] %s: %lld of %lld not finite (first at %lld)\n", tag, (long long)bad, (long long)n,
            (long long)first);
}

extern "C" {

int nodal_destroy(nodal_handle h) {
    if (!h) return NODAL_OK;
    DeviceGuard g(h);
    // (bounded like every other wait: a handle whose device work never ends is leaked, not freed under running kernels)
    bool drained = !h->hung && nodal_wait_stream(h, h->stream, NODAL_SITE) == NODAL_OK;
    if (drained && h->stream2) drained = nodal_wait_stream(h, h->stream2, NODAL_SITE) == NODAL_OK;
    if (drained && h->stream3) drained = nodal_wait_stream(h, h->stream3, NODAL_SITE) == NODAL_OK;
    if (!drained) {
        fprintf(stderr, "[nodal] nodal_destroy: the handle's streams did not drain (%s): its device memory is leaked\n",
                h->err.c_str());
        g_live_handles.fetch_sub(1, std::memory_order_relaxed);
        return NODAL_E_HIP;
    }
    nodal_free_buffers(h);
    for (auto &e : h->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : h->ev_la)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : h->ev_bi)
        if (e) (void)hipEventDestroy(e);
    if (h->stream3) (void)hipStreamDestroy(h->stream3);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    if (h->pinned) (void)hipHostFree(h->pinned);
    if (h->arena) (void)hipHostFree(h->arena);
    delete h;
    g_live_handles.fetch_sub(1, std::memory_order_relaxed);
    return NODAL_OK;
}

const char *nodal_last_error(nodal_handle h) { return h ? h->err.c_str() : "null handle"; }

int nodal_upload_components(nodal_handle h, int64_t ncomp, const uint8_t *type,
                            const double *value, const int32_t *a, const int32_t *b,
                            const int32_t *c, const int32_t *d, const int32_t *drv,
                            const int32_t *k, int32_t K, int32_t B) {
    return nodal_upload_internal(h, ncomp, type, value, a, b, c, d, drv, k, K, B);
}

}  // extern "C"

int nodal_upload_internal(nodal_ctx *h, int64_t ncomp, const uint8_t *type, const double *value,
                          const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d,
                          const int32_t *drv, const int32_t *k, int32_t K, int32_t B) {
    if (!h || ncomp < 0 || K < 0 || B < 0) return NODAL_E_INVALID;
    // c, d, drv, k may be null TOGETHER when the table holds no dependent source and no branch (B == 0:
    // resistors and current sources read none of them): 16 of the 33 bytes per row stay on the host
    const bool plain = !c && !d && !drv && !k;
    if (ncomp > 0 && (!type || !value || !a || !b || (!plain && (!c || !d || !drv || !k)) || (plain && B != 0)))
        return nodal_fail(h, NODAL_E_INVALID, "null component column");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    const int64_t n = (int64_t)K + B;
    h->have_table = h->have_symbolic = h->have_numeric = h->have_x = false;
    ++h->table_epoch;
    h->batch_count = 0;
    h->ncomp = ncomp;
    h->K = K;
    h->B = B;
    h->n = n;
    h->batch = 0;
    // (an early return must not leave DMA from the caller's columns in flight: the caller may free them)
    auto fail_synced = [&](int status) {
        (void)nodal_wait_stream(h, h->stream, NODAL_SITE);
        return status;
    };
#define UPLOAD_TRY(expr)                             \
    do {                                             \
        const int _s = (expr);                       \
        if (_s != NODAL_OK) return fail_synced(_s);  \
    } while (0)
    UPLOAD_TRY(upload(h, h->type, type, ncomp));
    UPLOAD_TRY(upload(h, h->value, value, ncomp));
    UPLOAD_TRY(upload(h, h->a, a, ncomp));
    UPLOAD_TRY(upload(h, h->b, b, ncomp));
    // c, d, drv, k: -1 everywhere, then (a table with branches) the entries of the rows that use them.  Those rows
    // are few -- 3e4 of config 5's 2e6 -- and 16 of the 33 bytes per row are these four columns: the host lists the
    // dependent rows while the first four columns are on their way (threads over chunks of the type column), packs
    // their entries into the page-locked arena, one copy and one scatter kernel place them (config 5: 67 -> 35 MB up).
    {
        DevBuf *cols[] = {&h->c, &h->d, &h->drv, &h->k};
        for (DevBuf *col : cols) {
            if (col->reserve((size_t)ncomp * 4 + 16) != hipSuccess ||
                (ncomp > 0 && hipMemsetAsync(col->p, 0xFF, (size_t)ncomp * 4, h->stream) != hipSuccess))  // -1
                return fail_synced(nodal_fail(h, NODAL_E_NOMEM, "upload: could not allocate a table column"));
        }
    }
    std::vector<int64_t> branch_rows;
    if (!plain && ncomp > 0) {
        // dependent rows by chunk of the type column, in file order
        constexpr int CHUNKS = 8;
        std::vector<int64_t> found[CHUNKS];
        {
            nodal_parallel_chunks(CHUNKS, 1, ncomp >= (1 << 18) ? CHUNKS : 1, [&](int64_t c0, int64_t c1) {
                for (int64_t q = c0; q < c1; ++q) {
                    std::vector<int64_t> &out = found[q];
                    for (int64_t i = ncomp * q / CHUNKS, e = ncomp * (q + 1) / CHUNKS; i < e; ++i)
                        if (type[i] >= NODAL_T_E) out.push_back(i);
                }
            });
            int64_t total = 0;
            for (int q = 0; q < CHUNKS; ++q) total += (int64_t)found[q].size();
            struct DepRow { int32_t row, c, d, drv, k; };
            DepRow *rec = total ? static_cast<DepRow *>(nodal_pinned_arena(h, (size_t)total * sizeof(DepRow))) : nullptr;
            if (total && !rec) return fail_synced(nodal_fail(h, NODAL_E_NOMEM, "upload: no page-locked staging memory"));
            int64_t at = 0;
            branch_rows.reserve((size_t)total);
            for (int q = 0; q < CHUNKS; ++q)
                for (const int64_t i : found[q]) {
                    rec[at++] = DepRow{(int32_t)i, c[i], d[i], drv[i], k[i]};
                    if (type[i] <= NODAL_T_CCCS) branch_rows.push_back(i);
                }
            if (total) {
                if (h->ps_stage.reserve((size_t)total * sizeof(DepRow) + 64) != hipSuccess)
                    return fail_synced(nodal_fail(h, NODAL_E_NOMEM, "upload: dependent rows"));
                if (hipMemcpyAsync(h->ps_stage.p, rec, (size_t)total * sizeof(DepRow), hipMemcpyHostToDevice, h->stream) != hipSuccess)
                    return fail_synced(nodal_fail(h, NODAL_E_HIP, "upload: dependent rows"));
                place_dependent_rows<<<(unsigned)((total + 255) / 256), 256, 0, h->stream>>>(
                    total, reinterpret_cast<const int32_t *>(h->ps_stage.p), ncomp, h->c.as<int32_t>(), h->d.as<int32_t>(),
                    h->drv.as<int32_t>(), h->k.as<int32_t>());
                if (hipGetLastError() != hipSuccess) return fail_synced(nodal_fail(h, NODAL_E_HIP, "upload: dependent rows launch failed"));
            }
        }
    }
    // the range check runs on the device, behind the copies; its verdict is the one word that comes back
    if (h->status.reserve(64) != hipSuccess) return fail_synced(nodal_fail(h, NODAL_E_NOMEM, "upload: status words"));
    unsigned long long *bad_dev = h->status.as<unsigned long long>() + 4;
    unsigned long long bad[2] = {~0ull, 0ull};
    if (hipMemsetAsync(bad_dev, 0xFF, 8, h->stream) != hipSuccess || hipMemsetAsync(bad_dev + 1, 0, 8, h->stream) != hipSuccess)
        return fail_synced(nodal_fail(h, NODAL_E_HIP, "upload: could not clear the status words"));
    if (ncomp > 0) {
        const int64_t blocks = (ncomp + 255) / 256;
        validate_table<<<(unsigned)(blocks > 4096 ? 4096 : blocks), 256, 0, h->stream>>>(
            ncomp, K, B, h->type.as<uint8_t>(), h->a.as<int32_t>(), h->b.as<int32_t>(),
            plain ? nullptr : h->c.as<int32_t>(), plain ? nullptr : h->d.as<int32_t>(),
            plain ? nullptr : h->drv.as<int32_t>(), plain ? nullptr : h->k.as<int32_t>(), bad_dev);
        // (the entries of the dependent rows only: a row number that is out of range was not placed and its k stays -1,
        // which the branch-type test above reports)
        if (hipGetLastError() != hipSuccess) return fail_synced(nodal_fail(h, NODAL_E_HIP, "upload: range check launch failed"));
    }
#undef UPLOAD_TRY
    // the host's view of the table (only systems with branch equations are presolved), made while the copies run:
    // the caller's columns in place when it has promised to keep them (NODAL_OPT_BORROW_TABLE), else copies (threads)
    if (h->keep_host_table && B > 0) {
        HostTable &t = h->host;
        if (h->borrow_table) {
            t.type.borrow(type, (size_t)ncomp);
            t.value.borrow(value, (size_t)ncomp);
            t.a.borrow(a, (size_t)ncomp);
            t.b.borrow(b, (size_t)ncomp);
            t.c.borrow(c, (size_t)ncomp);
            t.d.borrow(d, (size_t)ncomp);
            t.drv.borrow(drv, (size_t)ncomp);
            t.k.borrow(k, (size_t)ncomp);
        } else {
            t.type.resize((size_t)ncomp);
            t.value.resize((size_t)ncomp);
            HostCol<int32_t> *ic[] = {&t.a, &t.b, &t.c, &t.d, &t.drv, &t.k};
            const int32_t *src[] = {a, b, c, d, drv, k};
            for (HostCol<int32_t> *col : ic) col->resize((size_t)ncomp);
            nodal_parallel_chunks(ncomp, 1 << 16, 8, [&](int64_t lo, int64_t hi) {
                memcpy(t.type.own.data() + lo, type + lo, (size_t)(hi - lo));
                memcpy(t.value.own.data() + lo, value + lo, (size_t)(hi - lo) * 8);
                for (int q = 0; q < 6; ++q) memcpy(ic[q]->own.data() + lo, src[q] + lo, (size_t)(hi - lo) * 4);
            });
        }
        t.values_batch.clear();
        t.branch_rows.swap(branch_rows);
    } else {
        h->host = HostTable();
    }
    NODAL_TRY(nodal_read_words(h, bad, bad_dev, 16));
    h->rhs_items = (int64_t)bad[1];
    if (bad[0] != ~0ull) {
        h->ncomp = 0;  // (nothing may run on this table)
        h->host = HostTable();
        return nodal_fail(h, NODAL_E_INVALID, "component table row out of range");
    }
    h->have_table = true;
    return NODAL_OK;
}

extern "C" {

int nodal_upload_values(nodal_handle h, int32_t batch, const double *values) {
    if (!h || !h->have_table || batch < 1 || !values) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    NODAL_TRY(upload(h, h->values_batch, values, (int64_t)batch * h->ncomp));
    NODAL_WAIT_STREAM(h, h->stream);
    if (h->keep_host_table && h->B > 0)
        h->host.values_batch.assign(values, values + (size_t)batch * h->ncomp);
    h->batch = batch;
    h->have_numeric = h->have_x = false;
    return NODAL_OK;
}

int nodal_assemble_symbolic(nodal_handle h) {
    if (!h) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    int s = stamp_symbolic(h);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[0] = elapsed(h, 0, 1);
    return s;
}

int nodal_assemble_numeric(nodal_handle h, int32_t member, int64_t *bad_component) {
    if (!h) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    int s = stamp_numeric(h, member, bad_component);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[1] = elapsed(h, 0, 1);
    return s;
}

int nodal_get_sizes(nodal_handle h, int64_t *n, int64_t *nnz, int64_t *ncontrib) {
    if (!h || !h->have_symbolic) return NODAL_E_INVALID;
    if (n) *n = h->n;
    if (nnz) *nnz = h->nnz;
    if (ncontrib) *ncontrib = h->ncontrib;
    return NODAL_OK;
}

int nodal_export_csr(nodal_handle h, int32_t *indptr, int32_t *indices, double *data,
                     double *rhs) {
    if (!h || !h->have_symbolic) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    hipStream_t st = h->stream;
    if (indptr)
        NODAL_HIP_TRY(h, hipMemcpyAsync(indptr, h->indptr.p, (size_t)(h->n + 1) * 4,
                                        hipMemcpyDeviceToHost, st));
    if (indices && h->nnz)
        NODAL_HIP_TRY(h, hipMemcpyAsync(indices, h->indices.p, (size_t)h->nnz * 4,
                                        hipMemcpyDeviceToHost, st));
    if (data || rhs) {
        if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "assemble_numeric not called");
        if (data && h->nnz)
            NODAL_HIP_TRY(h, hipMemcpyAsync(data, h->data.p, (size_t)h->nnz * 8,
                                            hipMemcpyDeviceToHost, st));
        if (rhs && h->n)
            NODAL_HIP_TRY(h, hipMemcpyAsync(rhs, h->rhs.p, (size_t)h->n * 8,
                                            hipMemcpyDeviceToHost, st));
    }
    NODAL_WAIT_STREAM(h, st);
    return NODAL_OK;
}

int nodal_export_dense(nodal_handle h, double *G, double *rhs) {
    if (!h || !h->have_numeric) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    const int64_t n = h->n;
    if (G && n) {
        NODAL_HIP_TRY(h, h->dense.reserve((size_t)dense_lda(n) * (size_t)(n + 1) * 8 + 64));
        NODAL_TRY(stamp_to_dense(h, h->dense.as<double>(), n, false));
        NODAL_HIP_TRY(h, hipMemcpyAsync(G, h->dense.p, (size_t)n * n * 8, hipMemcpyDeviceToHost,
                                        h->stream));
    }
    if (rhs && n)
        NODAL_HIP_TRY(h, hipMemcpyAsync(rhs, h->rhs.p, (size_t)n * 8, hipMemcpyDeviceToHost,
                                        h->stream));
    NODAL_WAIT_STREAM(h, h->stream);
    return NODAL_OK;
}

int nodal_download_x(nodal_handle h, double *x) {
    if (!h || !h->have_x || !x) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    if (h->n)
        NODAL_HIP_TRY(h, hipMemcpyAsync(x, h->x.p, (size_t)h->n * 8, hipMemcpyDeviceToHost,
                                        h->stream));
    NODAL_WAIT_STREAM(h, h->stream);
    return NODAL_OK;
}

int nodal_solve_dense(nodal_handle h, double *x, int32_t *info) {
    if (!h || !info) return NODAL_E_INVALID;
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "assemble_numeric not called");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    *info = 0;
    h->have_x = false;
    h->last_batch_block = false;
    h->last_iterations = 0;
    h->amg_levels = 0;
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    if (h->n > 0) {
        // Large systems with voltage-defined branches: eliminate those branches first
        // (presolve.hip).  If what remains is a passive network, the dense block elimination
        // solves it without pivoting; the answer is checked against the ORIGINAL equations.
        bool done = false;
        if (h->n > 512 && h->B > 0 && h->use_presolve && !h->force_pivoting && !h->passive_network) {
            int32_t it = 0;
            double rs = 0.0;
            NODAL_TRY(presolve_solve(h, &done, info, &it, &rs, true));
        }
        // Passive networks made of chains / ladders / trees: the exact elimination of nodes with
        // <= 2 neighbours (lowdeg.hip) shrinks the system before anything is formed densely
        // (ladder of 5000 sections: 1.9 ms instead of 5.7).  Grids have no such nodes: one probe
        // kernel, then the block elimination as before.
        if (!done && h->n > 1024 && h->B == 0 && h->passive_network && !h->force_pivoting) {
            int32_t it = 0;
            double rs = 0.0;
            NODAL_TRY(lowdeg_solve(h, 8, &done, info, &it, &rs));
            if (done && *info > 0) NODAL_TRY(dense_fill_nan(h, h->x.as<double>(), h->n));
        }
        if (!done) {
            *info = 0;
            NODAL_TRY(dense_prepare(h));
            NODAL_TRY(dense_factor_solve(h, info));
        }
    }
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[2] = elapsed(h, 0, 1);
    if (*info > 0) return nodal_fail(h, NODAL_E_SINGULAR, "singular matrix: a zero pivot or a floating sub-network");
    h->have_x = true;
    if (x) return nodal_download_x(h, x);
    return NODAL_OK;
}

int nodal_solve_sparse(nodal_handle h, int32_t method, double *x, int32_t *info, int32_t *iters,
                       double *resid) {
    if (!h || !info) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    int32_t it = 0;
    double rs = 0;
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    h->amg_levels = 0;
    h->last_batch_block = false;
    int s = sparse_solve(h, method, info, &it, &rs);
    h->last_iterations = it;
    h->last_relres = rs;
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[2] = elapsed(h, 0, 1);
    if (iters) *iters = it;
    if (resid) *resid = rs;
    if (s != NODAL_OK) return s;
    if (x) return nodal_download_x(h, x);
    return NODAL_OK;
}

int nodal_solve_pairs(nodal_handle h, int32_t dense, int32_t npairs, const int32_t *ia,
                      const int32_t *ib, double *resistance, int32_t *info) {
    if (!h || !info || npairs < 0 || (npairs > 0 && (!ia || !ib || !resistance)))
        return NODAL_E_INVALID;
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "assemble_numeric not called");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    *info = 0;
    const int64_t n = h->n;
    for (int32_t q = 0; q < npairs; ++q)
        if (ia[q] < -1 || ia[q] >= h->K || ib[q] < -1 || ib[q] >= h->K)
            return nodal_fail(h, NODAL_E_INVALID, "pair index out of range");
    if (npairs == 0) return NODAL_OK;
    h->have_x = false;
    NODAL_HIP_TRY(h, h->schur.reserve((size_t)npairs * 8 + 64));
    double *res = h->schur.as<double>();
    if (n == 0) {
        for (int32_t q = 0; q < npairs; ++q) resistance[q] = 0.0;
        return NODAL_OK;
    }
    bool reduced = false;
    if (n > 1024 && h->B == 0 && h->passive_network && !h->force_pivoting) {
        // chains / ladders / trees: exact elimination of the low-degree nodes per pair (lowdeg.hip)
        NODAL_TRY(lowdeg_solve_pairs(h, npairs, ia, ib, res, &reduced, info));
        if (reduced && *info > 0) {
            if (dense) return nodal_fail(h, NODAL_E_SINGULAR, "singular matrix: a floating sub-network");
            for (int32_t q = 0; q < npairs; ++q) resistance[q] = __builtin_nan("");
            return NODAL_OK;
        }
    }
    if (reduced) {
        // results are in `res`
    } else if (dense || n <= 64 || (!(h->B == 0 && h->passive_network) && n <= 8192)) {
        // (a non-passive network above 8192 unknowns on the sparse switch: one sparse LU, sparse_solve_pairs)
        // one LU for up to CHUNK pairs: they are extra right-hand-side columns
        const int32_t CHUNK = 512;
        for (int32_t q0 = 0; q0 < npairs; q0 += CHUNK) {
            const int32_t m = npairs - q0 < CHUNK ? npairs - q0 : CHUNK;
            NODAL_TRY(dense_prepare_pairs(h, m, ia + q0, ib + q0));
            NODAL_HIP_TRY(h, h->solver.reserve((size_t)n * m * 8 + 64));
            NODAL_TRY(dense_factor_solve_multi(h, m, h->solver.as<double>(), n, info));
            if (*info > 0) {
                if (dense) return nodal_fail(h, NODAL_E_SINGULAR, "singular matrix: exact zero pivot");
                for (int32_t q = 0; q < npairs; ++q) resistance[q] = __builtin_nan("");
                return NODAL_OK;
            }
            for (int32_t q = 0; q < m; ++q)
                NODAL_TRY(pair_read_host(h, h->solver.as<double>() + (int64_t)q * n, ia[q0 + q],
                                         ib[q0 + q], res + q0 + q));
        }
    } else {
        NODAL_TRY(sparse_solve_pairs(h, npairs, ia, ib, res, info));
        if (*info > 0) {
            for (int32_t q = 0; q < npairs; ++q) resistance[q] = __builtin_nan("");
            return NODAL_OK;
        }
    }
    NODAL_HIP_TRY(h, hipMemcpyAsync(resistance, res, (size_t)npairs * 8, hipMemcpyDeviceToHost,
                                    h->stream));
    NODAL_WAIT_STREAM(h, h->stream);
    return NODAL_OK;
}

}  // extern "C"

int sweep_check_rows(nodal_ctx *h, const char *prefix, const char *row, int32_t nsrc, const int64_t *rows,
                     int32_t *rows_dev, int32_t *slot_dev, int32_t *bad_dev) {
    const std::string the = std::string(prefix) + row, a = std::string(prefix) + "a " + row;
    std::vector<int32_t> r32((size_t)nsrc + 1);
    for (int32_t j = 0; j < nsrc; ++j) {
        if (rows[j] < 0 || rows[j] >= h->ncomp) return nodal_fail(h, NODAL_E_INVALID, (the + " out of range").c_str());
        r32[j] = (int32_t)rows[j];
    }
    if (nsrc > 0)
        NODAL_HIP_TRY(h, hipMemcpyAsync(rows_dev, r32.data(), (size_t)nsrc * 4, hipMemcpyHostToDevice, h->stream));
    NODAL_TRY(stamp_sweep_slots(h, rows_dev, nsrc, slot_dev, bad_dev));
    int32_t bad = 0;
    NODAL_TRY(nodal_read_words(h, &bad, bad_dev, 4));  // (waits: the host copies before it are done too)
    if (bad & 1)
        return nodal_fail(h, NODAL_E_INVALID, (a + " that is not an independent source (A or E)").c_str());
    if (bad & 2) return nodal_fail(h, NODAL_E_INVALID, (a + " named twice").c_str());
    return NODAL_OK;
}

namespace {
// Arguments of a source sweep: values uploaded, and the rows through sweep_check_rows into sw_rows and sw_slot
int sweep_prepare(nodal_ctx *h, int32_t count, int32_t nsrc, const int64_t *rows, const double *values) {
    if (count < 0 || nsrc < 0 || (nsrc > 0 && !rows) || (count > 0 && nsrc > 0 && !values))
        return nodal_fail(h, NODAL_E_INVALID, "source sweep: bad count, rows or values");
    if (!h->have_numeric || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "assemble_numeric not called");
    NODAL_HIP_TRY(h, h->sw_rows.reserve((size_t)(nsrc + 16) * 4));
    NODAL_HIP_TRY(h, h->sw_slot.reserve((size_t)h->ncomp * 4 + 64));
    NODAL_HIP_TRY(h, h->sw_vals.reserve((size_t)count * nsrc * 8 + 64));
    if ((int64_t)count * nsrc > 0)
        NODAL_HIP_TRY(h, hipMemcpyAsync(h->sw_vals.p, values, (size_t)count * nsrc * 8, hipMemcpyHostToDevice, h->stream));
    int32_t *rows_dev = h->sw_rows.as<int32_t>();
    return sweep_check_rows(h, "source sweep: ", "row", nsrc, rows, rows_dev, h->sw_slot.as<int32_t>(),
                            rows_dev + ((nsrc + 15) & ~15));
}

// multi_rhs_solve's client for a source sweep: the columns are the members' folded sources, a finished block feeds the
// envelope (branch.hip, when one is kept) and goes down to the caller as rows
struct SweepClient final : MultiRhsClient {
    nodal_ctx *h;
    int32_t nsrc;
    const double *swept;
    const int32_t *slot;
    double *x_out;        // host, [count][n]; may be null
    const int32_t *info;  // the driver's flags (host), settled for a block by the time it is handed over
    const BranchSweep *env;
    SweepClient(nodal_ctx *h_, int32_t nsrc_, double *x_out_, const int32_t *info_, const BranchSweep *env_)
        : h(h_), nsrc(nsrc_), swept(h_->sw_vals.as<double>()), slot(h_->sw_slot.as<int32_t>()), x_out(x_out_),
          info(info_), env(env_) {}
    int build(int32_t m0, int cols, double *out, int64_t rs, int64_t cs) override {
        return stamp_rhs_multi(h, slot, swept + (int64_t)m0 * nsrc, nsrc, cols, out, rs, cs);
    }
    int hand_over(int32_t m0, int cols, const double *, int64_t, int64_t, const double *rows) override {
        const int64_t n = h->n;
        if (env) NODAL_TRY(branch_sweep_block(h, env, m0, cols, rows, info, swept, slot, nsrc));
        if (x_out)
            NODAL_HIP_TRY(h, hipMemcpyAsync(x_out + (int64_t)m0 * n, rows, (size_t)cols * n * 8, hipMemcpyDeviceToHost,
                                            h->stream));
        NODAL_WAIT_STREAM(h, h->stream);
        return NODAL_OK;
    }
    void all_singular(int32_t count) override {
        if (x_out)
            for (int64_t t = 0; t < (int64_t)count * h->n; ++t) x_out[t] = __builtin_nan("");
    }
};
}  // namespace

extern "C" {

int nodal_solve_sources(nodal_handle h, int32_t dense, int32_t count, int32_t nsrc, const int64_t *rows,
                        const double *values, double *x_out, double *resid_out, int32_t *info_out) {
    return nodal_solve_sources_branches(h, dense, count, nsrc, rows, values, x_out, resid_out, info_out, nullptr, nullptr,
                                        nullptr, nullptr, nullptr, nullptr, nullptr);
}

int nodal_solve_sources_branches(nodal_handle h, int32_t dense, int32_t count, int32_t nsrc, const int64_t *rows,
                                 const double *values, double *x_out, double *resid_out, int32_t *info_out,
                                 double *current_absmax, int32_t *current_member, double *potential_min,
                                 int32_t *potential_min_member, double *potential_max, int32_t *potential_max_member,
                                 double *power_out) {
    if (!h || (count > 0 && !info_out)) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    NODAL_TRY(sweep_prepare(h, count, nsrc, rows, values));
    BranchSweep env;
    env.out_absmax = current_absmax;
    env.out_absmax_member = current_member;
    env.out_pmin = potential_min;
    env.out_pmin_member = potential_min_member;
    env.out_pmax = potential_max;
    env.out_pmax_member = potential_max_member;
    env.out_power = power_out;
    const bool want_env = current_absmax || current_member || potential_min || potential_min_member || potential_max ||
                          potential_max_member || power_out;
    if (count == 0) return want_env ? branch_sweep_finish(h, &env, 0, info_out) : NODAL_OK;  // (NaN and -1 throughout)
    h->amg_levels = 0;
    h->last_batch_block = false;
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    if (want_env) NODAL_TRY(branch_sweep_begin(h, &env, count));
    SweepClient client(h, nsrc, x_out, info_out, want_env ? &env : nullptr);
    int s = multi_rhs_solve(h, h, dense != 0, count, resid_out, info_out, client);
    if (s == NODAL_OK && want_env) s = branch_sweep_finish(h, &env, count, info_out);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[2] = elapsed(h, 0, 1);
    return s;
}

int nodal_branches(nodal_handle h, double *voltage, double *current, double *power, double *totals2) {
    if (!h) return NODAL_E_INVALID;
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "branches: no component table on the handle");
    if (!h->have_numeric || !h->have_x) return nodal_fail(h, NODAL_E_INVALID, "branches: no solution on the handle");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    return branch_single(h, voltage, current, power, totals2);
}

int nodal_sensitivities(nodal_handle h, int32_t dense, int32_t count, const int32_t *kind, const int32_t *p,
                        const int32_t *q2, double *sens_out, double *value_out, double *adjoint_out,
                        double *resid_out, int32_t *info_out) {
    if (!h || count < 0 || (count > 0 && (!kind || !p || !q2 || !sens_out || !info_out))) return NODAL_E_INVALID;
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "sensitivities: no component table on the handle");
    if (!h->have_numeric || !h->have_x) return nodal_fail(h, NODAL_E_INVALID, "sensitivities: no solution on the handle");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    if (count == 0) return NODAL_OK;
    return sens_run(h, dense != 0, count, kind, p, q2, sens_out, value_out, adjoint_out, resid_out, info_out);
}

int nodal_gradient(nodal_handle h, int32_t dense, int32_t count, const double *x, const double *cotangent, int32_t nsrc,
                   const int64_t *rows, double *grad_out, double *grad_sources_out, double *adjoint_out,
                   double *resid_out, int32_t *info_out) {
    if (!h || count < 0 || nsrc < 0 || (nsrc > 0 && !rows) || (count > 0 && (!cotangent || !info_out))) return NODAL_E_INVALID;
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "gradient: no component table on the handle");
    if (h->ncomp > 0 && !grad_out) return nodal_fail(h, NODAL_E_INVALID, "gradient: no array for the result");
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "gradient: assemble_numeric not called");
    if (!x && !h->have_x) return nodal_fail(h, NODAL_E_INVALID, "gradient: no solution on the handle");
    if (!x && (count != 1 || nsrc != 0))
        return nodal_fail(h, NODAL_E_INVALID, "gradient: the solution on the handle serves one member without swept sources");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    return grad_run(h, dense != 0, count, x, cotangent, nsrc, rows, grad_out, grad_sources_out, adjoint_out, resid_out,
                    info_out);
}

int nodal_transient(nodal_handle h, int32_t dense, int32_t steps, int32_t method, int64_t ncap, const int64_t *cap_rows,
                    int32_t nsrc, const int64_t *src_rows, const double *src_values, const double *x0, int32_t nprobe,
                    const int32_t *probe_a, const int32_t *probe_b, double *wave_out, int32_t keep_every, double *x_out,
                    double *pot_min, int32_t *pot_min_step, double *pot_max, int32_t *pot_max_step, double *resid_out,
                    int32_t *info_out, int32_t *iters_out) {
    return nodal_transient_rlc(h, dense, steps, method, ncap, cap_rows, nsrc, src_rows, src_values, x0, nprobe, probe_a,
                               probe_b, wave_out, keep_every, x_out, pot_min, pot_min_step, pot_max, pot_max_step, resid_out,
                               info_out, iters_out, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr);
}

int nodal_transient_rlc(nodal_handle h, int32_t dense, int32_t steps, int32_t method, int64_t ncap, const int64_t *cap_rows,
                        int32_t nsrc, const int64_t *src_rows, const double *src_values, const double *x0, int32_t nprobe,
                        const int32_t *probe_a, const int32_t *probe_b, double *wave_out, int32_t keep_every, double *x_out,
                        double *pot_min, int32_t *pot_min_step, double *pot_max, int32_t *pot_max_step, double *resid_out,
                        int32_t *info_out, int32_t *iters_out, int64_t nind, const int64_t *ind_rows, const double *i0,
                        int32_t ncur, const int32_t *cur_index, double *cur_out, double *i_final_out) {
    if (!h || nind < 0 || (nind > 0 && !ind_rows) || ncur < 0 || (ncur > 0 && (!cur_index || nind == 0))) return NODAL_E_INVALID;
    if (!h || steps < 0 || (method != 0 && method != 1) || ncap < 0 || (ncap > 0 && !cap_rows) || nprobe < 0 ||
        (nprobe > 0 && (!probe_a || !probe_b)) || keep_every < 0)
        return NODAL_E_INVALID;
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "transient: no component table on the handle");
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "transient: assemble_numeric not called");
    if (h->n > 0 && !x0) return nodal_fail(h, NODAL_E_INVALID, "transient: no initial state");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    h->tape_valid = false;  // (whatever an earlier call recorded: this one replaces it, if it records)
    NODAL_TRY(sweep_prepare(h, steps, nsrc, src_rows, src_values));
    h->amg_levels = 0;
    h->last_batch_block = false;
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    double ms_matrix = 0.0;
    TransientInductors ind;
    ind.nind = nind;
    ind.rows = ind_rows;
    ind.i0 = i0;
    ind.ncur = ncur;
    ind.cur_index = cur_index;
    ind.cur_out = cur_out;
    ind.i_final_out = i_final_out;
    const int s = transient_run(h, dense != 0, steps, method, ncap, cap_rows, nsrc, x0, nprobe, probe_a, probe_b, wave_out,
                                keep_every, x_out, pot_min, pot_min_step, pot_max, pot_max_step, resid_out, info_out,
                                iters_out, &ms_matrix, nind > 0 ? &ind : nullptr);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[0] = ms_matrix;
    h->ms[1] = 0.0;
    h->ms[2] = elapsed(h, 0, 1);
    return s;
}

int nodal_transient_nl(nodal_handle h, int32_t dense, int32_t steps, int32_t method, int64_t ncap, const int64_t *cap_rows,
                       int32_t nsrc, const int64_t *src_rows, const double *src_values, const double *x0, int32_t nprobe,
                       const int32_t *probe_a, const int32_t *probe_b, double *wave_out, int32_t keep_every, double *x_out,
                       double *pot_min, int32_t *pot_min_step, double *pot_max, int32_t *pot_max_step, double *resid_out,
                       int32_t *info_out, int32_t *iters_out, int64_t nind, const int64_t *ind_rows, const double *i0,
                       int32_t ncur, const int32_t *cur_index, double *cur_out, double *i_final_out, int64_t ndiode,
                       const int64_t *diode_rows, const double *i_sat, const double *n_vt, double gmin, int32_t max_iter,
                       double reltol, double vntol, double abstol, int32_t ndprobe, const int32_t *dprobe_index,
                       int32_t *newton_out, int32_t *updates_out, double *dv_out, double *di_out, double *vh_final_out) {
    return nodal_transient_nl_bjt(h, dense, steps, method, ncap, cap_rows, nsrc, src_rows, src_values, x0, nprobe, probe_a,
                                  probe_b, wave_out, keep_every, x_out, pot_min, pot_min_step, pot_max, pot_max_step,
                                  resid_out, info_out, iters_out, nind, ind_rows, i0, ncur, cur_index, cur_out, i_final_out,
                                  ndiode, diode_rows, i_sat, n_vt, gmin, max_iter, reltol, vntol, abstol, ndprobe,
                                  dprobe_index, newton_out, updates_out, dv_out, di_out, vh_final_out, 0, nullptr, nullptr,
                                  nullptr, 0, nullptr, nullptr, nullptr);
}

int nodal_transient_nl_bjt(nodal_handle h, int32_t dense, int32_t steps, int32_t method, int64_t ncap, const int64_t *cap_rows,
                           int32_t nsrc, const int64_t *src_rows, const double *src_values, const double *x0, int32_t nprobe,
                           const int32_t *probe_a, const int32_t *probe_b, double *wave_out, int32_t keep_every, double *x_out,
                           double *pot_min, int32_t *pot_min_step, double *pot_max, int32_t *pot_max_step, double *resid_out,
                           int32_t *info_out, int32_t *iters_out, int64_t nind, const int64_t *ind_rows, const double *i0,
                           int32_t ncur, const int32_t *cur_index, double *cur_out, double *i_final_out, int64_t ndiode,
                           const int64_t *diode_rows, const double *i_sat, const double *n_vt, double gmin, int32_t max_iter,
                           double reltol, double vntol, double abstol, int32_t ndprobe, const int32_t *dprobe_index,
                           int32_t *newton_out, int32_t *updates_out, double *dv_out, double *di_out, double *vh_final_out,
                           int64_t ntr, const int64_t *gm_rows, const int32_t *junction, const double *i_s, int32_t ntprobe,
                           const int32_t *tprobe_index, double *tv_out, double *ti_out) {
    if (!h || nind < 0 || (nind > 0 && !ind_rows) || ncur < 0 || (ncur > 0 && (!cur_index || nind == 0))) return NODAL_E_INVALID;
    if (steps < 0 || (method != 0 && method != 1) || ncap < 0 || (ncap > 0 && !cap_rows) || nprobe < 0 ||
        (nprobe > 0 && (!probe_a || !probe_b)) || keep_every < 0)
        return NODAL_E_INVALID;
    if (ndiode < 0 || (ndiode > 0 && (!diode_rows || !i_sat || !n_vt)) || max_iter < 1 || ndprobe < 0 ||
        (ndprobe > 0 && (!dprobe_index || ndiode == 0)))
        return NODAL_E_INVALID;
    if (ntr < 0 || (ntr > 0 && (!gm_rows || !junction || !i_s)) || ntprobe < 0 || (ntprobe > 0 && (!tprobe_index || ntr == 0)))
        return NODAL_E_INVALID;
    if (!(gmin >= 0.0 && reltol >= 0.0 && vntol >= 0.0 && abstol >= 0.0) || std::isinf(gmin) || std::isinf(reltol) ||
        std::isinf(vntol) || std::isinf(abstol))
        return nodal_fail(h, NODAL_E_INVALID, "transient: gmin and the tolerances must be finite and not negative");
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "transient: no component table on the handle");
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "transient: assemble_numeric not called");
    if (h->n > 0 && !x0) return nodal_fail(h, NODAL_E_INVALID, "transient: no initial state");
    if (ndiode > 0 && h->K == 0) return nodal_fail(h, NODAL_E_INVALID, "transient: diodes on a network without nodes");
    for (int64_t i = 0; i < ndiode; ++i)
        if (diode_rows[i] < 0 || diode_rows[i] >= h->ncomp) return nodal_fail(h, NODAL_E_INVALID, "transient: diode row out of range");
    for (int32_t q = 0; q < ndprobe; ++q)
        if (dprobe_index[q] < 0 || dprobe_index[q] >= ndiode)
            return nodal_fail(h, NODAL_E_INVALID, "transient: diode probe outside the diodes");
    // (the transports' other cases are TransportSet::prepare's; these two it would not see, or see too late)
    for (int64_t i = 0; i < 2 * ntr; ++i)
        if (junction[i] < 0 || junction[i] >= ndiode)
            return nodal_fail(h, NODAL_E_INVALID, "transient: a junction index outside the diodes");
    for (int32_t q = 0; q < ntprobe; ++q)
        if (tprobe_index[q] < 0 || tprobe_index[q] >= ntr)
            return nodal_fail(h, NODAL_E_INVALID, "transient: transistor probe outside the transports");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    h->tape_valid = false;  // (no tape with diodes, and whatever an earlier call recorded is written over)
    NODAL_TRY(sweep_prepare(h, steps, nsrc, src_rows, src_values));
    h->amg_levels = 0;
    h->last_batch_block = false;
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    double ms_matrix = 0.0;
    TransientInductors ind;
    ind.nind = nind;
    ind.rows = ind_rows;
    ind.i0 = i0;
    ind.ncur = ncur;
    ind.cur_index = cur_index;
    ind.cur_out = cur_out;
    ind.i_final_out = i_final_out;
    TransientDiodes dio;
    dio.nd = ndiode;
    dio.rows = diode_rows;
    dio.isat = i_sat;
    dio.nvt = n_vt;
    dio.gmin = gmin;
    dio.reltol = reltol;
    dio.vntol = vntol;
    dio.abstol = abstol;
    dio.max_iter = max_iter;
    dio.ndprobe = ndprobe;
    dio.dprobe_index = dprobe_index;
    dio.newton_out = newton_out;
    dio.updates_out = updates_out;
    dio.dv_out = dv_out;
    dio.di_out = di_out;
    dio.vh_final_out = vh_final_out;
    dio.nt = ntr;  // (ntr > 0 has ndiode >= 1: the junctions are diodes)
    dio.gm_rows = gm_rows;
    dio.junction = junction;
    dio.i_s = i_s;
    dio.ntprobe = ntprobe;
    dio.tprobe_index = tprobe_index;
    dio.tv_out = tv_out;
    dio.ti_out = ti_out;
    const bool nonlinear = ndiode > 0 && h->n > 0;  // (without diodes: nodal_transient_rlc's launches, one iteration a step)
    std::vector<int32_t> info_own(info_out || !newton_out ? 0 : (size_t)steps);
    int32_t *info = info_out ? info_out : info_own.data();
    const int s = transient_run(h, dense != 0, steps, method, ncap, cap_rows, nsrc, x0, nprobe, probe_a, probe_b, wave_out,
                                keep_every, x_out, pot_min, pot_min_step, pot_max, pot_max_step, resid_out,
                                nonlinear ? info_out : info, iters_out, &ms_matrix, nind > 0 ? &ind : nullptr,
                                nonlinear ? &dio : nullptr);
    if (!nonlinear && s == NODAL_OK)
        for (int32_t k = 0; k < steps; ++k) {
            if (newton_out) newton_out[k] = info[k] == 0 ? 1 : 0;
            if (updates_out) updates_out[k] = 0;
        }
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[0] = nonlinear ? dio.ms_matrix : ms_matrix;
    h->ms[1] = nonlinear ? dio.ms_symbolic : 0.0;
    h->ms[2] = elapsed(h, 0, 1);
    return s;
}

// nodal_newton_dc and nodal_newton_dc_bjt: `tr` null for the first, whose record has four words a row
static int newton_dc_entry(nodal_handle h, int32_t dense, int64_t ndiode, const int64_t *diode_rows, const double *i_sat,
                           const double *n_vt, double gmin, int32_t nsrc, const int64_t *src_rows, const double *src_values,
                           const double *x0, int32_t max_iter, double reltol, double vntol, double abstol, double *x_out,
                           double *v_out, double *i_out, double *g_out, double *iterates_out, double *vh_out,
                           double *record_out, int32_t *info_out, int32_t *iters_out, int32_t *route_out,
                           int32_t *iterations, int32_t *converged, const NewtonTransports *tr) {
    if (!h || ndiode < 0 || (ndiode > 0 && (!diode_rows || !i_sat || !n_vt)) || max_iter < 1 || !iterations || !converged)
        return NODAL_E_INVALID;
    if (!(gmin >= 0.0 && reltol >= 0.0 && vntol >= 0.0 && abstol >= 0.0) || std::isinf(gmin) || std::isinf(reltol) ||
        std::isinf(vntol) || std::isinf(abstol))
        return nodal_fail(h, NODAL_E_INVALID, "newton: gmin and the tolerances must be finite and not negative");
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "newton: no component table on the handle");
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "newton: assemble_numeric not called");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    h->tape_valid = false;  // (the node lists and the state buffers of a recorded transient are written over)
    NODAL_TRY(sweep_prepare(h, 1, nsrc, src_rows, src_values));
    h->amg_levels = 0;
    h->last_batch_block = false;
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    double ms_matrix = 0.0, ms_symbolic = 0.0;
    NewtonOutputs out;
    out.x = x_out;
    out.v = v_out;
    out.i = i_out;
    out.g = g_out;
    out.iterates = iterates_out;
    out.vh = vh_out;
    out.record = record_out;
    out.info = info_out;
    out.iters = iters_out;
    out.route = route_out;
    out.iterations = iterations;
    out.converged = converged;
    out.record_words = tr ? 5 : 4;
    const int s = newton_run(h, dense != 0, ndiode, diode_rows, i_sat, n_vt, gmin, nsrc, x0, max_iter, reltol, vntol, abstol,
                             out, &ms_matrix, &ms_symbolic, tr);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[0] = ms_matrix;
    h->ms[1] = ms_symbolic;
    h->ms[2] = elapsed(h, 0, 1);
    return s;
}

int nodal_newton_dc(nodal_handle h, int32_t dense, int64_t ndiode, const int64_t *diode_rows, const double *i_sat,
                    const double *n_vt, double gmin, int32_t nsrc, const int64_t *src_rows, const double *src_values,
                    const double *x0, int32_t max_iter, double reltol, double vntol, double abstol, double *x_out,
                    double *v_out, double *i_out, double *g_out, double *iterates_out, double *vh_out, double *record_out,
                    int32_t *info_out, int32_t *iters_out, int32_t *route_out, int32_t *iterations, int32_t *converged) {
    return newton_dc_entry(h, dense, ndiode, diode_rows, i_sat, n_vt, gmin, nsrc, src_rows, src_values, x0, max_iter, reltol,
                           vntol, abstol, x_out, v_out, i_out, g_out, iterates_out, vh_out, record_out, info_out, iters_out,
                           route_out, iterations, converged, nullptr);
}

int nodal_newton_dc_bjt(nodal_handle h, int32_t dense, int64_t ndiode, const int64_t *diode_rows, const double *i_sat,
                        const double *n_vt, double gmin, int32_t nsrc, const int64_t *src_rows, const double *src_values,
                        const double *x0, int32_t max_iter, double reltol, double vntol, double abstol, int64_t ntr,
                        const int64_t *gm_rows, const int32_t *junction, const double *i_s, double *x_out, double *v_out,
                        double *i_out, double *g_out, double *it_out, double *gmf_out, double *gmr_out, double *iterates_out,
                        double *vh_out, double *record_out, int32_t *info_out, int32_t *iters_out, int32_t *route_out,
                        int32_t *iterations, int32_t *converged) {
    if (!h || ntr < 0 || (ntr > 0 && (!gm_rows || !junction || !i_s))) return NODAL_E_INVALID;
    NewtonTransports tr;
    tr.nt = ntr;
    tr.gm_rows = gm_rows;
    tr.junction = junction;
    tr.i_s = i_s;
    tr.it = it_out;
    tr.gmf = gmf_out;
    tr.gmr = gmr_out;
    return newton_dc_entry(h, dense, ndiode, diode_rows, i_sat, n_vt, gmin, nsrc, src_rows, src_values, x0, max_iter, reltol,
                           vntol, abstol, x_out, v_out, i_out, g_out, iterates_out, vh_out, record_out, info_out, iters_out,
                           route_out, iterations, converged, &tr);
}

int nodal_newton_gradient(nodal_handle h, int32_t dense, int64_t ndiode, const int64_t *diode_rows, const double *i_sat,
                          const double *n_vt, double gmin, int32_t nsrc, const int64_t *src_rows, const double *src_values,
                          const double *x, const double *cotangent, double *grad_out, double *grad_isat_out,
                          double *grad_nvt_out, double *grad_gmin_out, double *grad_sources_out, double *adjoint_out,
                          double *resid_out, double *op_resid_out, int32_t *info_out) {
    if (!h || ndiode < 0 || (ndiode > 0 && (!diode_rows || !i_sat || !n_vt)) || !info_out) return NODAL_E_INVALID;
    if (!(gmin >= 0.0) || std::isinf(gmin))
        return nodal_fail(h, NODAL_E_INVALID, "operating-point gradient: gmin must be finite and not negative");
    if (!h->have_table || h->csr_only)
        return nodal_fail(h, NODAL_E_INVALID, "operating-point gradient: no component table on the handle");
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "operating-point gradient: assemble_numeric not called");
    if (h->ncomp > 0 && !grad_out) return nodal_fail(h, NODAL_E_INVALID, "operating-point gradient: no array for the result");
    if (h->n > 0 && (!x || !cotangent))
        return nodal_fail(h, NODAL_E_INVALID, "operating-point gradient: no operating point or no cotangent");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    h->tape_valid = false;  // (the node lists and the state buffers of a recorded transient are written over)
    NODAL_TRY(sweep_prepare(h, 1, nsrc, src_rows, src_values));
    h->amg_levels = 0;
    h->last_batch_block = false;
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    double ms_matrix = 0.0, ms_symbolic = 0.0;
    NewtonGradientOutputs out;
    out.grad = grad_out;
    out.grad_isat = grad_isat_out;
    out.grad_nvt = grad_nvt_out;
    out.grad_gmin = grad_gmin_out;
    out.grad_sources = grad_sources_out;
    out.adjoint = adjoint_out;
    out.resid = resid_out;
    out.op_resid = op_resid_out;
    out.info = info_out;
    const int s = newton_gradient_run(h, dense != 0, ndiode, diode_rows, i_sat, n_vt, gmin, nsrc, x, cotangent, out, &ms_matrix,
                                      &ms_symbolic);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[0] = ms_matrix;
    h->ms[1] = ms_symbolic;
    h->ms[2] = elapsed(h, 0, 1);
    return s;
}

int nodal_transient_gradient(nodal_handle h, int32_t dense, int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b,
                             const double *wave_cot, double *grad_out, double *grad_sources_out, double *grad_x0_out,
                             double *adjoint_out, double *resid_out, int32_t *info_out) {
    if (!h || nprobe < 0 || (nprobe > 0 && (!probe_a || !probe_b || !wave_cot))) return NODAL_E_INVALID;
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "transient gradient: no component table on the handle");
    if (!h->have_numeric || !h->tape_valid || h->tape_epoch != h->numeric_epoch)
        return nodal_fail(h, NODAL_E_INVALID, "transient gradient: no recorded transient on the handle");
    if ((h->ncomp > 0 && !grad_out) || (h->tape_steps > 0 && !info_out))
        return nodal_fail(h, NODAL_E_INVALID, "transient gradient: no array for the result");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    double ms_matrix = 0.0;
    const int s = tgrad_run(h, dense != 0, nprobe, probe_a, probe_b, wave_cot, grad_out, grad_sources_out, grad_x0_out,
                            adjoint_out, resid_out, info_out, &ms_matrix);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[0] = ms_matrix;
    h->ms[1] = 0.0;
    h->ms[2] = elapsed(h, 0, 1);
    return s;
}

int nodal_ac_sweep(nodal_handle h, int32_t dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
                   const double *value, const int32_t *lead_a, const int32_t *lead_b, int32_t nsrc, const int64_t *src_rows,
                   const double *src_re, const double *src_im, int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b,
                   double *wave_out, int32_t ncur, const int32_t *cur_index, double *cur_out, int32_t keep_every, double *x_out,
                   double *peak_out, int32_t *peak_freq_out, double *resid_out, int32_t *info_out) {
    if (!h || nreact < 0 || (nreact > 0 && (!kind || !value || !lead_a || !lead_b)) || nsrc < 0 ||
        (nsrc > 0 && (!src_rows || !src_re || !src_im)) || nprobe < 0 || (nprobe > 0 && (!probe_a || !probe_b)) || ncur < 0 ||
        (ncur > 0 && !cur_index) || keep_every < 0)
        return NODAL_E_INVALID;
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "ac sweep: no component table on the handle");
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "ac sweep: assemble_numeric not called");
    if (nfreq < 0 || (nfreq > 0 && !omega)) return nodal_fail(h, NODAL_E_INVALID, "ac sweep: a negative number of frequencies");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    double ms_analysis = 0.0, ms_factor = 0.0;
    const int s = ac_run(h, dense != 0, nfreq, omega, nreact, kind, value, lead_a, lead_b, nsrc, src_rows, src_re, src_im, nprobe,
                         probe_a, probe_b, wave_out, ncur, cur_index, cur_out, keep_every, x_out, peak_out, peak_freq_out,
                         resid_out, info_out, &ms_analysis, &ms_factor);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[0] = ms_analysis;
    h->ms[1] = ms_factor;
    h->ms[2] = elapsed(h, 0, 1);
    return s;
}

int nodal_ac_noise(nodal_handle h, int32_t dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
                   const double *value, const int32_t *lead_a, const int32_t *lead_b, double temperature, int32_t nout,
                   const int32_t *out_a, const int32_t *out_b, int64_t input_row, const double *weight, double *density_out,
                   double *gain_out, double *contrib_out, double *resid_out, int32_t *info_out) {
    if (!h || nreact < 0 || (nreact > 0 && (!kind || !value || !lead_a || !lead_b)) || nout < 0 ||
        (nout > 0 && (!out_a || !out_b)))
        return NODAL_E_INVALID;
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "noise: no component table on the handle");
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "noise: assemble_numeric not called");
    if (nfreq < 0 || (nfreq > 0 && !omega)) return nodal_fail(h, NODAL_E_INVALID, "noise: a negative number of frequencies");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    double ms_analysis = 0.0, ms_factor = 0.0;
    const int s = noise_run(h, dense != 0, nfreq, omega, nreact, kind, value, lead_a, lead_b, temperature, nout, out_a, out_b,
                            input_row, weight, density_out, gain_out, contrib_out, resid_out, info_out, &ms_analysis, &ms_factor);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[0] = ms_analysis;
    h->ms[1] = ms_factor;
    h->ms[2] = elapsed(h, 0, 1);
    return s;
}

int nodal_ac_ports(nodal_handle h, int32_t dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
                   const double *value, const int32_t *lead_a, const int32_t *lead_b, int32_t nports, const int32_t *ia,
                   const int32_t *ib, double *z_out, double *node_peak_out, int32_t *node_peak_port_out,
                   int32_t *node_peak_freq_out, double *resid_out, int32_t *info_out, int64_t *work_out) {
    if (!h || nreact < 0 || (nreact > 0 && (!kind || !value || !lead_a || !lead_b))) return NODAL_E_INVALID;
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "ac ports: no component table on the handle");
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "ac ports: assemble_numeric not called");
    if (nfreq < 0 || (nfreq > 0 && !omega)) return nodal_fail(h, NODAL_E_INVALID, "ac ports: a negative number of frequencies");
    if (nports < 0 || (nports > 0 && (!ia || !ib))) return nodal_fail(h, NODAL_E_INVALID, "ac ports: a negative number of ports");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    double ms_analysis = 0.0, ms_factor = 0.0;
    const int s = ac_ports_run(h, dense != 0, nfreq, omega, nreact, kind, value, lead_a, lead_b, nports, ia, ib, z_out,
                               node_peak_out, node_peak_port_out, node_peak_freq_out, resid_out, info_out, work_out,
                               &ms_analysis, &ms_factor);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[0] = ms_analysis;
    h->ms[1] = ms_factor;
    h->ms[2] = elapsed(h, 0, 1);
    return s;
}

int nodal_ac_gradient(nodal_handle h, int32_t dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
                      const double *value, const int32_t *lead_a, const int32_t *lead_b, int32_t nsrc, const int64_t *src_rows,
                      const double *src_re, const double *src_im, int32_t nprobe, const int32_t *probe_a,
                      const int32_t *probe_b, const double *wave_cot, double *wave_out, double *grad_out,
                      double *grad_react_out, double *grad_sources_out, int32_t keep_every, double *adjoint_out,
                      double *resid_out, int32_t *info_out, int64_t *work_out) {
    if (!h || nreact < 0 || (nreact > 0 && (!kind || !value || !lead_a || !lead_b)) || nsrc < 0 ||
        (nsrc > 0 && (!src_rows || !src_re || !src_im)) || nprobe < 0 || (nprobe > 0 && (!probe_a || !probe_b)) || keep_every < 0)
        return NODAL_E_INVALID;
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "ac gradient: no component table on the handle");
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "ac gradient: assemble_numeric not called");
    if (nfreq < 0 || (nfreq > 0 && !omega)) return nodal_fail(h, NODAL_E_INVALID, "ac gradient: a negative number of frequencies");
    if (nfreq > 0 && nprobe > 0 && !wave_cot) return nodal_fail(h, NODAL_E_INVALID, "ac gradient: no cotangents");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    nodal_poison_scratch(h);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    double ms_analysis = 0.0, ms_factor = 0.0;
    const int s = ac_gradient_run(h, dense != 0, nfreq, omega, nreact, kind, value, lead_a, lead_b, nsrc, src_rows, src_re,
                                  src_im, nprobe, probe_a, probe_b, wave_cot, wave_out, grad_out, grad_react_out,
                                  grad_sources_out, keep_every, adjoint_out, resid_out, info_out, work_out, &ms_analysis,
                                  &ms_factor);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[0] = ms_analysis;
    h->ms[1] = ms_factor;
    h->ms[2] = elapsed(h, 0, 1);
    return s;
}

int nodal_port_matrix(nodal_handle h, int32_t dense, int32_t nports, const int32_t *ia, const int32_t *ib, double *z_out,
                      double *voc_out, double *resid_out, int32_t *info_out) {
    if (!h || nports < 0 || (nports > 0 && (!ia || !ib || !z_out || !info_out))) return NODAL_E_INVALID;
    if (!h->have_table || h->csr_only) return nodal_fail(h, NODAL_E_INVALID, "port matrix: no component table on the handle");
    if (!h->have_numeric) return nodal_fail(h, NODAL_E_INVALID, "port matrix: assemble_numeric not called");
    if (voc_out && !h->have_x) return nodal_fail(h, NODAL_E_INVALID, "port matrix: no solution on the handle");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    if (nports == 0) return NODAL_OK;
    return port_run(h, dense != 0, nports, ia, ib, z_out, voc_out, resid_out, info_out);
}

int nodal_debug_sources_rhs(nodal_handle h, int32_t count, int32_t nsrc, const int64_t *rows, const double *values,
                            double *rhs_out) {
    if (!h || (count > 0 && !rhs_out)) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    NODAL_TRY(sweep_prepare(h, count, nsrc, rows, values));
    SweepClient client(h, nsrc, rhs_out, nullptr, nullptr);
    return sparse_sources_rhs(h, count, client);
}

int nodal_debug_residual(nodal_handle h, int32_t transposed, int32_t cols, int32_t layout, const double *x,
                         const double *b, double *scaled_out, double *norms_out) {
    if (!h) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return sparse_debug_residual(h, transposed != 0, cols, layout, x, b, scaled_out, norms_out);
}

int nodal_debug_direct_apply(nodal_handle h, int32_t transposed, int32_t cols, const double *r, double *z,
                             int64_t *perturbed_out, int32_t *info_out) {
    if (!h) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return sparse_debug_direct_apply(h, transposed != 0, cols, r, z, perturbed_out, info_out);
}

int nodal_debug_hierarchy_info(nodal_handle h, int32_t *nlev, int64_t *ints, double *reals) {
    if (!h || !nlev || !ints || !reals) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return sagg_debug_info(h, nlev, ints, reals);
}

int nodal_debug_hierarchy_array(nodal_handle h, int32_t level, int32_t which, void *dst, int64_t capacity_bytes,
                                int64_t *bytes_out) {
    if (!h || !bytes_out) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return sagg_debug_array(h, level, which, dst, capacity_bytes, bytes_out);
}

int nodal_debug_cycle_apply(nodal_handle h, int32_t mode, const double *r, const double *u, const double *frozen,
                            double *z, double *dots_out, int32_t *params_out) {
    if (!h || !r || !z) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return sagg_debug_cycle_apply(h, mode, r, u, frozen, z, dots_out, params_out);
}

int nodal_debug_amg_info(nodal_handle h, int32_t *nlev, int64_t *ints, int64_t *words, double *reals, int64_t *tail) {
    if (!h || !nlev || !ints || !words || !reals || !tail) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return amg_debug_info(h, nlev, ints, words, reals, tail);
}

int nodal_debug_amg_array(nodal_handle h, int32_t level, int32_t which, void *dst, int64_t capacity_bytes,
                          int64_t *bytes_out) {
    if (!h || !bytes_out) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return amg_debug_array(h, level, which, dst, capacity_bytes, bytes_out);
}

int nodal_debug_amg_apply(nodal_handle h, int32_t level, const double *r, double *z, int32_t *params_out) {
    if (!h || !r || !z) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return amg_debug_apply(h, level, r, z, params_out);
}

int nodal_debug_fgmres_cycle(nodal_handle h, int32_t system, int32_t precond, int32_t window, int32_t max_cols,
                             double rel_tol, int64_t n, const double *b, double *x_out, double *V_out, double *Z_out, double *gst_out,
                             double *y_out, double *norms_out, int64_t *params_out) {
    if (!h) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return general_debug_cycle(h, system, precond, window, max_cols, rel_tol, n, b, x_out, V_out, Z_out, gst_out, y_out,
                               norms_out, params_out);
}

int nodal_debug_general_array(nodal_handle h, int32_t which, void *dst, int64_t capacity_bytes, int64_t *bytes_out) {
    if (!h || !bytes_out) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return general_debug_array(h, which, dst, capacity_bytes, bytes_out);
}

int nodal_debug_presolve_build(nodal_handle h, int64_t *info) {
    if (!h || !info) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return presolve_debug_build(h, info);
}

int nodal_debug_presolve_array(nodal_handle h, int32_t which, void *dst, int64_t capacity_bytes, int64_t *bytes_out) {
    if (!h || !bytes_out) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return presolve_debug_array(h, which, dst, capacity_bytes, bytes_out);
}

int nodal_debug_presolve_recover(nodal_handle h, int64_t ny, const double *y, double *x_out) {
    if (!h || ny < 0 || (ny > 0 && !y) || !x_out) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return presolve_debug_recover(h, ny, y, x_out);
}

int nodal_debug_scan_u32(nodal_handle h, int64_t n, const uint32_t *in, uint32_t *out, int32_t in_place,
                         uint32_t *total_out) {
    if (!h) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return scan_debug_u32(h, n, in, out, in_place != 0, total_out);
}

int nodal_debug_lowdeg_info(nodal_handle h, int32_t *rounds, int64_t *ints) {
    if (!h || !rounds || !ints) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return lowdeg_debug_info(h, rounds, ints);
}

int nodal_debug_lowdeg_array(nodal_handle h, int32_t round, int32_t which, void *dst, int64_t capacity_bytes,
                             int64_t *bytes_out) {
    if (!h || !bytes_out) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return lowdeg_debug_array(h, round, which, dst, capacity_bytes, bytes_out);
}

int nodal_debug_floating_small(nodal_handle h, int64_t n, const int32_t *indptr, const int32_t *indices,
                               const uint8_t *grounded, int32_t *floating) {
    if (!h || n < 0 || !indptr || !floating || (n > 0 && !grounded)) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    return lowdeg_debug_floating_small(h, n, indptr, indices, grounded, floating);
}

int nodal_residual(nodal_handle h, double *scaled_residual) {
    if (!h || !scaled_residual) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    if (h->last_batch_block && h->blocksys) {  // whole block-diagonal system of the last nodal_run_batch
        const int s = sparse_residual(h->blocksys, scaled_residual);
        if (s != NODAL_OK) h->err = h->blocksys->err;
        return s;
    }
    return sparse_residual(h, scaled_residual);
}

int nodal_run(nodal_handle h, int32_t dense, int32_t member, int32_t reuse_symbolic,
              int32_t *info) {
    if (!h || !info) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    // symbolic + numeric back to back: the symbolic phase's timer is read AFTER the numeric phase has waited for its
    // status words anyway (waiting for it in between left the GPU idle for ~30 us per circuit)
    hipEvent_t ev_s0 = h->ev[2], ev_s1 = h->ev[3];  // (free until the solve records them around its dominant kernel)
    const bool do_symbolic = !(reuse_symbolic && h->have_symbolic);
    if (do_symbolic) {
        NODAL_HIP_TRY(h, hipEventRecord(ev_s0, h->stream));
        NODAL_TRY(stamp_symbolic(h));
        NODAL_HIP_TRY(h, hipEventRecord(ev_s1, h->stream));
    }
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[0], h->stream));
    const int sn = stamp_numeric(h, member, nullptr);
    NODAL_HIP_TRY(h, hipEventRecord(h->ev[1], h->stream));
    NODAL_WAIT_EVENT(h, h->ev[1], h->stream);
    h->ms[1] = elapsed(h, 0, 1);
    h->ms[0] = 0.0;  // (kept: nothing ran)
    if (do_symbolic) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev_s0, ev_s1) == hipSuccess) h->ms[0] = ms;
    }
    NODAL_TRY(sn);
    if (dense) return nodal_solve_dense(h, nullptr, info);
    return nodal_solve_sparse(h, NODAL_SPARSE_AUTO, nullptr, info, nullptr, nullptr);
}

int nodal_last_timings(nodal_handle h, double *ms3) {
    if (!h || !ms3) return NODAL_E_INVALID;
    ms3[0] = h->ms[0];
    ms3[1] = h->ms[1];
    ms3[2] = h->ms[2];
    return NODAL_OK;
}

int nodal_last_kernel_stats(nodal_handle h, double *ms_total, int64_t *launches,
                            double *alg_bytes_or_flops) {
    if (!h) return NODAL_E_INVALID;
    if (ms_total) *ms_total = h->kern_ms;
    if (launches) *launches = h->kern_launches;
    if (alg_bytes_or_flops) *alg_bytes_or_flops = h->kern_alg;
    return NODAL_OK;
}

int nodal_set_option(nodal_handle h, int32_t option, int32_t value) {
    if (!h) return NODAL_E_INVALID;
    if (option == NODAL_OPT_FORCE_PIVOTING) {
        h->force_pivoting = value != 0;
        return NODAL_OK;
    }
    if (option == NODAL_OPT_GEPP_PANEL) {
        h->gepp_panel = value != 0;
        return NODAL_OK;
    }
    if (option == NODAL_OPT_EXTRA_STREAMS) {
        h->extra_streams = value != 0;
        return NODAL_OK;
    }
    if (option == NODAL_OPT_BORROW_TABLE) {
        h->borrow_table = value != 0;
        return NODAL_OK;
    }
    if (option == NODAL_OPT_TRANSIENT_TAPE) {
        h->transient_tape = value != 0;
        return NODAL_OK;
    }
    return nodal_fail(h, NODAL_E_INVALID, "unknown option");
}

int nodal_debug_gemm(nodal_handle h, int32_t M, int32_t N, int32_t K, const double *A,
                     const double *B, double *C) {
    if (!h || M < 1 || N < 1 || K < 1 || !A || !B || !C) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    const size_t sa = (size_t)M * K * 8, sb = (size_t)K * N * 8, sc = (size_t)M * N * 8;
    NODAL_HIP_TRY(h, h->work.reserve(sa + sb + sc + 768));
    char *w = h->work.as<char>();
    double *dA = reinterpret_cast<double *>(w);
    double *dB = reinterpret_cast<double *>(w + ((sa + 255) & ~(size_t)255));
    double *dC = reinterpret_cast<double *>(w + ((sa + 255) & ~(size_t)255) + ((sb + 255) & ~(size_t)255));
    NODAL_HIP_TRY(h, hipMemcpyAsync(dA, A, sa, hipMemcpyHostToDevice, h->stream));
    NODAL_HIP_TRY(h, hipMemcpyAsync(dB, B, sb, hipMemcpyHostToDevice, h->stream));
    NODAL_HIP_TRY(h, hipMemcpyAsync(dC, C, sc, hipMemcpyHostToDevice, h->stream));
    NODAL_TRY(gemm_sub_f64(h, h->stream, dC, M, dA, M, dB, K, M, N, K));
    NODAL_HIP_TRY(h, hipMemcpyAsync(C, dC, sc, hipMemcpyDeviceToHost, h->stream));
    NODAL_WAIT_STREAM(h, h->stream);
    return NODAL_OK;
}

}  // extern "C"

// ---- testing hooks of the dense path's pieces (gemm_f64.hip, block_elim.hip, dense_lu.hip): host arrays into scratch,
// the production function, the results back.  No arithmetic here. ----
namespace {

inline size_t dbg_pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

struct DebugGemmOperands {
    const double *A, *B;
    double *C;
    int64_t lda, ldb, ldc, acols;  // acols: columns of the host image of A (K, or M for the transposed panel)
    int32_t M, N, K;
    double *dA = nullptr, *dB = nullptr, *dC = nullptr;
    size_t bytes() const { return dbg_pad((size_t)lda * acols * 8) + dbg_pad((size_t)ldb * N * 8) + dbg_pad((size_t)ldc * N * 8); }
    int up(nodal_ctx *h, char *&w) {
        dA = reinterpret_cast<double *>(w);
        w += dbg_pad((size_t)lda * acols * 8);
        dB = reinterpret_cast<double *>(w);
        w += dbg_pad((size_t)ldb * N * 8);
        dC = reinterpret_cast<double *>(w);
        w += dbg_pad((size_t)ldc * N * 8);
        NODAL_HIP_TRY(h, hipMemcpyAsync(dA, A, (size_t)lda * acols * 8, hipMemcpyHostToDevice, h->stream));
        NODAL_HIP_TRY(h, hipMemcpyAsync(dB, B, (size_t)ldb * N * 8, hipMemcpyHostToDevice, h->stream));
        NODAL_HIP_TRY(h, hipMemcpyAsync(dC, C, (size_t)ldc * N * 8, hipMemcpyHostToDevice, h->stream));
        return NODAL_OK;
    }
    int down(nodal_ctx *h) {
        NODAL_HIP_TRY(h, hipMemcpyAsync(C, dC, (size_t)ldc * N * 8, hipMemcpyDeviceToHost, h->stream));
        return NODAL_OK;
    }
};

}  // namespace

size_t dense_debug_inverse_scratch();  // block_elim.hip
int dense_debug_block_inverse(nodal_ctx *h, double *D, int64_t lda, int w, double *Q, int64_t ldq, double *scratch,
                              int32_t *dinfo, int base, int variant);

extern "C" {

int nodal_debug_gemm_ex(nodal_handle h, int32_t kind, int32_t mode, int32_t band, int32_t M, int32_t N, int32_t K,
                        const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int32_t M2,
                        int32_t N2, int32_t K2, const double *A2, int64_t lda2, const double *B2, int64_t ldb2, double *C2,
                        int64_t ldc2) {
    if (!h) return NODAL_E_INVALID;
    if (kind < 0 || kind > 2 || mode < GEMM_SUB || mode > GEMM_SETNEG || M < 1 || N < 1 || K < 1 || !A || !B || !C ||
        lda < (kind == 1 ? K : M) || ldb < K || ldc < M || (kind == 1 && mode != GEMM_SUB))
        return nodal_fail(h, NODAL_E_INVALID, "debug_gemm_ex: kind, mode, sizes or leading dimensions");
    if (kind == 2 && (M2 < 1 || N2 < 1 || K2 < 1 || !A2 || !B2 || !C2 || lda2 < M2 || ldb2 < K2 || ldc2 < M2))
        return nodal_fail(h, NODAL_E_INVALID, "debug_gemm_ex: the second problem's sizes or leading dimensions");
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    DebugGemmOperands p{A, B, C, lda, ldb, ldc, kind == 1 ? M : K, M, N, K};
    DebugGemmOperands q{A2, B2, C2, lda2, ldb2, ldc2, K2, M2, N2, K2};
    NODAL_HIP_TRY(h, h->work.reserve(p.bytes() + (kind == 2 ? q.bytes() : 0) + 256));
    char *w = h->work.as<char>();
    NODAL_TRY(p.up(h, w));
    if (kind == 2) NODAL_TRY(q.up(h, w));
    if (kind == 0) NODAL_TRY(gemm_f64(h, h->stream, mode, p.dC, ldc, p.dA, lda, p.dB, ldb, M, N, K));
    else if (kind == 1) NODAL_TRY(gemm_sub_tn_upper_f64(h, h->stream, p.dC, ldc, p.dA, lda, p.dB, ldb, M, N, K, band));
    else
        NODAL_TRY(gemm_pair_f64(h, h->stream, mode, GemmProblem{p.dC, ldc, p.dA, lda, p.dB, ldb, M, N, K},
                                GemmProblem{q.dC, ldc2, q.dA, lda2, q.dB, ldb2, M2, N2, K2}));
    NODAL_TRY(p.down(h));
    if (kind == 2) NODAL_TRY(q.down(h));
    NODAL_WAIT_STREAM(h, h->stream);
    return NODAL_OK;
}

int nodal_debug_block_inverse(nodal_handle h, int32_t w, const double *A, int64_t lda, int32_t base, int32_t variant,
                              double *Q, int64_t ldq, int32_t *dinfo_out) {
    if (!h || !A || !Q || !dinfo_out || w < 1 || lda < w || ldq < w) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    const size_t sa = dbg_pad((size_t)lda * w * 8), sq = dbg_pad((size_t)ldq * w * 8);
    const size_t st = dbg_pad(dense_debug_inverse_scratch() * 8);
    NODAL_HIP_TRY(h, h->work.reserve(sa + sq + st + 512));
    char *wk = h->work.as<char>();
    double *dA = reinterpret_cast<double *>(wk), *dQ = reinterpret_cast<double *>(wk + sa);
    double *dT = reinterpret_cast<double *>(wk + sa + sq);
    int32_t *dinfo = reinterpret_cast<int32_t *>(wk + sa + sq + st);
    NODAL_HIP_TRY(h, hipMemcpyAsync(dA, A, (size_t)lda * w * 8, hipMemcpyHostToDevice, h->stream));
    NODAL_HIP_TRY(h, hipMemcpyAsync(dQ, Q, (size_t)ldq * w * 8, hipMemcpyHostToDevice, h->stream));
    NODAL_HIP_TRY(h, hipMemsetAsync(dinfo, 0, 4, h->stream));
    NODAL_TRY(dense_debug_block_inverse(h, dA, lda, w, dQ, ldq, dT, dinfo, base, variant));
    NODAL_HIP_TRY(h, hipMemcpyAsync(Q, dQ, (size_t)ldq * w * 8, hipMemcpyDeviceToHost, h->stream));
    return nodal_read_words(h, dinfo_out, dinfo, 4);
}

int nodal_debug_dense_solve(nodal_handle h, int32_t n, int32_t nrhs, int32_t route, const double *A, const double *B,
                            double *X, int32_t *info_out, int32_t *ipiv_out) {
    if (!h || n < 1 || nrhs < 1 || route < 0 || route > 7 || !A || !B || !X || !info_out || !ipiv_out) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;
    // the dispatcher reads the system's size and route from the context: set for this call, put back on every way out
    struct Restore {
        nodal_ctx *h;
        int64_t n;
        bool passive, optimistic, pivoting;
        ~Restore() {
            h->n = n;
            h->passive_network = passive;
            h->optimistic_nopivot = optimistic;
            h->force_pivoting = pivoting;
        }
    } restore{h, h->n, h->passive_network, h->optimistic_nopivot, h->force_pivoting};
    h->n = n;
    h->passive_network = (route & 1) != 0;
    h->optimistic_nopivot = (route & 2) != 0;
    h->force_pivoting = (route & 4) != 0;
    const int64_t lda = dense_lda(n);
    const size_t panel = (size_t)lda * (size_t)(n + nrhs) * 8;
    NODAL_HIP_TRY(h, h->dense.reserve(panel + 64));
    NODAL_HIP_TRY(h, h->piv.reserve((size_t)n * 4 + 64));  // (as the dispatcher reserves it: the pointer stays)
    NODAL_HIP_TRY(h, h->dbg_apply.reserve((size_t)n * nrhs * 8 + 64));
    double *dA = h->dense.as<double>(), *dX = h->dbg_apply.as<double>();
    hipStream_t st = h->stream;
    NODAL_HIP_TRY(h, hipMemsetAsync(dA, 0xff, panel, st));  // the padding rows hold NaN: nothing may read them into a result
    NODAL_HIP_TRY(h, hipMemcpy2DAsync(dA, (size_t)lda * 8, A, (size_t)n * 8, (size_t)n * 8, (size_t)n, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpy2DAsync(dA + (int64_t)n * lda, (size_t)lda * 8, B, (size_t)n * 8, (size_t)n * 8, (size_t)nrhs,
                                      hipMemcpyHostToDevice, st));
    // routes without row interchanges never write the list: it starts as the identity (the caller's ipiv_out)
    NODAL_HIP_TRY(h, hipMemcpyAsync(h->piv.as<int32_t>(), ipiv_out, (size_t)n * 4, hipMemcpyHostToDevice, st));
    *info_out = 0;
    NODAL_TRY(dense_factor_solve_multi(h, nrhs, dX, n, info_out));
    NODAL_HIP_TRY(h, hipMemcpyAsync(X, dX, (size_t)n * nrhs * 8, hipMemcpyDeviceToHost, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(ipiv_out, h->piv.as<int32_t>(), (size_t)n * 4, hipMemcpyDeviceToHost, st));
    NODAL_WAIT_STREAM(h, st);
    return NODAL_OK;
}

}  // extern "C"

extern "C" {

int nodal_last_solve_info(nodal_handle h, int32_t *iterations, int32_t *amg_levels,
                          double *relative_residual) {
    if (!h) return NODAL_E_INVALID;
    if (iterations) *iterations = h->last_iterations;
    if (amg_levels) *amg_levels = h->amg_levels;
    if (relative_residual) *relative_residual = h->last_relres;
    return NODAL_OK;
}

int nodal_synchronize(nodal_handle h) {
    if (!h) return NODAL_E_INVALID;
    DeviceGuard g(h);
    if (h->hung) return NODAL_E_HIP;  // (a wait timed out earlier: nodal_last_error still says where)
    NODAL_WAIT_STREAM(h, h->stream);
    return NODAL_OK;
}

}  // extern "C"

// ---- pinned host memory for the component table (include/nodal_hip.h) ----
extern "C" {

int nodal_host_alloc(size_t bytes, void **out) {
    if (!out) return NODAL_E_INVALID;
    *out = nullptr;
    if (bytes == 0) return NODAL_OK;
    const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return e == hipErrorOutOfMemory ? NODAL_E_NOMEM : NODAL_E_HIP;
    }
    return NODAL_OK;
}

int nodal_host_free(void *p) {
    if (p && hipHostFree(p) != hipSuccess) {
        (void)hipGetLastError();
        return NODAL_E_HIP;
    }
    return NODAL_OK;
}

}  // extern "C"
