// Internal context of libnodal_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nodal_hip.h"
#include "knobs.h"

// A device allocation that grows on demand and is reused across calls, so the
// launch path never calls hipMalloc once sizes have settled.
// The stream of the handle whose API call is running on this thread (set by FillStreamScope at the
// entry points): a growing DevBuf zero-fills itself on it, in order with every kernel the call launches
// afterwards.  Null outside an API call: the fill then runs on the null stream and is waited for.
inline thread_local hipStream_t nodal_fill_stream = nullptr;
struct FillStreamScope {
    hipStream_t prev;
    explicit FillStreamScope(hipStream_t s) : prev(nodal_fill_stream) { nodal_fill_stream = s; }
    ~FillStreamScope() { nodal_fill_stream = prev; }
    FillStreamScope(const FillStreamScope &) = delete;
    FillStreamScope &operator=(const FillStreamScope &) = delete;
};

// 0: off; 1: growing buffers are filled with 0xFF; 2: scratch buffers too, at every solve entry
inline int nodal_poison_level() {
    static const int level = knob::POISON.now();
    return level;
}

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + (bytes >> 3) + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        // A buffer that grows starts from zeros, whatever the allocator hands back: hardening only --
        // no kernel may depend on it (NODAL_POISON shows the ones that do).
        // NODAL_POISON=1 (debugging) fills with 0xFF bytes instead -- NaNs as doubles, -1 as integers;
        // NODAL_POISON=2 also re-poisons every scratch buffer of the handle at the entry of each solve
        // (nodal_poison_scratch, api.hip): what a pooled handle looks like after somebody else's solve.
        static const bool nofill = knob::NOFILL.now();
        const bool poison = nodal_poison_level() > 0;
        if (e != hipSuccess || nofill) return e;
        if (nodal_fill_stream) return hipMemsetAsync(p, poison ? 0xFF : 0, want, nodal_fill_stream);
        // (outside an API call the fill runs on the null stream; the contexts' streams do not wait for
        // that one by themselves)
        e = hipMemset(p, poison ? 0xFF : 0, want);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        return e;
    }
    // debugging (NODAL_POISON=2): the whole allocation becomes 0xFF bytes, in order on `st`
    void poison(hipStream_t st) {
        if (p) (void)hipMemsetAsync(p, 0xFF, cap, st);
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// A column of the host table: either a copy the library owns, or (NODAL_OPT_BORROW_TABLE) the caller's own column,
// read in place.  The subset of std::vector's interface the readers use.
template <class T>
struct HostCol {
    const T *p = nullptr;
    size_t n = 0;
    std::vector<T> own;
    bool empty() const { return n == 0; }
    size_t size() const { return n; }
    const T *data() const { return p; }
    const T &operator[](size_t i) const { return p[i]; }
    T &operator[](size_t i) { return own[i]; }  // (writers: a column they resize()d themselves)
    void assign(const T *first, const T *last) {
        own.assign(first, last);
        p = own.data();
        n = own.size();
    }
    void borrow(const T *q, size_t count) {
        std::vector<T>().swap(own);
        p = q;
        n = count;
    }
    void resize(size_t count) {
        own.resize(count);
        p = own.data();
        n = count;
    }
    void clear() {
        own.clear();
        p = nullptr;
        n = 0;
    }
};

// host view of the component table (the presolve of presolve.hip works on it)
struct HostTable {
    HostCol<uint8_t> type;
    HostCol<double> value;
    HostCol<int32_t> a, b, c, d, drv, k;
    std::vector<double> values_batch;
    std::vector<int64_t> branch_rows;  // rows of the components that own a branch unknown (types E .. CCCS),
                                       // in file order: what the presolve's planning pass looks at
    mutable std::vector<int32_t> node_slot;  // K entries, all -1 between uses: the presolve's direct map from a
                                             // node to its place in a short list (lead nodes, pivots)
};

// f(lo, hi) over [0, n) in contiguous chunks on up to `max_threads` host threads (the calling one included); chunks
// of at least `min_chunk` items, one chunk = a plain call.  The loops handed to it write disjoint ranges.
template <class F>
inline void nodal_parallel_chunks(int64_t n, int64_t min_chunk, int max_threads, F f) {
    unsigned hw = std::thread::hardware_concurrency();
    if (const auto t = knob::HOST_THREADS.now()) hw = (unsigned)std::max(1, *t);
    int64_t T = hw ? (int64_t)hw : 1;
    if (T > max_threads) T = max_threads;
    if (min_chunk < 1) min_chunk = 1;
    if (T > n / min_chunk) T = n / min_chunk;
    if (T <= 1) {
        f((int64_t)0, n);
        return;
    }
    std::vector<std::thread> th;
    th.reserve((size_t)T - 1);
    for (int64_t c = 1; c < T; ++c) th.emplace_back(f, n * c / T, n * (c + 1) / T);
    f((int64_t)0, n / T);
    for (auto &t : th) t.join();
}

struct nodal_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // trailing updates of the dense LU (lookahead)
    hipEvent_t ev_la[2] = {nullptr, nullptr};
    hipStream_t stream3 = nullptr;   // bulk stream of the block-inverse elimination (all CUs)
    hipEvent_t ev_bi[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t gt_used = 0;              // GemmTimer (dense_common.h): timed launches, their flops
    double gt_flops = 0.0;
    bool hung = false;               // a bounded wait ran out (wait.hip): nothing more may run on this handle
    bool optimistic_nopivot = false; // dense: block elimination although not passive (caller verifies the answer)
    int gj_scalar = 0;               // NODAL_GJ_SCALAR=1: scalar Gauss-Jordan, 2: rank-4 MFMA steps; default rank-16
    bool dense_blockinv = true;      // passive dense systems: block elimination (NODAL_DENSE_BLOCKINV=0: LU)
    std::string err;

    // ---- component table (HBM, structure of arrays) ----
    int64_t ncomp = 0;
    int32_t K = 0, B = 0;
    int64_t n = 0;
    DevBuf type, value, a, b, c, d, drv, k;
    DevBuf values_batch;  // [batch][ncomp] doubles
    int32_t batch = 0;
    bool have_table = false;
    uint64_t table_epoch = 1;      // bumped by every upload_components (topology identity)
    // value sweeps as one block-diagonal system (batch.hip): child context + [count][n] results
    nodal_ctx *blocksys = nullptr;
    uint64_t block_epoch = 0;      // (child) table_epoch of the parent its table was replicated from
    DevBuf batch_x;
    DevBuf batch_scale;            // per-member right-hand-side scales of the last block solve (batch.hip)
    int32_t batch_count = 0;
    bool last_batch_block = false;  // the last solve was a block-diagonal batch (nodal_residual looks at it)
    hipEvent_t ev_batch[4] = {nullptr, nullptr, nullptr, nullptr};  // phase timing of nodal_run_batch
    HostTable host;
    bool keep_host_table = true;
    bool borrow_table = false;       // NODAL_OPT_BORROW_TABLE: the caller's columns stay valid until the next upload
    int32_t member = 0;            // batch member of the last numeric assembly
    nodal_ctx *reduced = nullptr;  // presolved (branch-free) system, see presolve.hip
    uint64_t reduced_key = 0;      // (on the reduced context) fingerprint of the topology its symbolic lists belong to
    bool owns_streams = true;
    nodal_ctx *stream_owner = nullptr;  // (child contexts) the context whose streams and events this one borrows
    void *pinned = nullptr;             // small page-locked scratch for read-backs of a few words (nodal_pinned)
    void *arena = nullptr;              // page-locked staging area that grows on demand (nodal_pinned_arena)
    size_t arena_bytes = 0;
    bool use_presolve = true;
    bool use_graphs = false;       // hipGraph replay of the FCG iteration: measured no gain (kernels are not host-bound)
    DevBuf ps_buf, ps_newidx, ps_hits, ps_stage;
    // source sweeps (nodal_solve_sources, sparse.hip): swept rows, their slot map, the members' values, the
    // right-hand-side / solution blocks
    DevBuf sw_rows, sw_slot, sw_vals, sw_blk;
    // branch quantities (branch.hip): voltage / current / power on their way to the host, the workgroups' power
    // partials (+ the two totals of a single solution), a sweep's totals [count][2], a sweep's envelope arrays
    DevBuf br_out, br_part, br_tot, br_env;
    // adjoint sensitivities (sensitivity.hip): the solution set aside during the call, the outputs' specification and
    // values, one block of results on its way to the host, the CCVS / CCCS rows grouped by their driving resistor
    // (kept per table_epoch); the child context holding G^T as CSR (networks that are not passive), the parent
    // struct_epoch its pattern was transposed from and the permutation that gathers its values from `data`
    DevBuf sn_x, sn_spec, sn_out, sn_cross, sn_perm;
    // loss gradients (gradient.hip): sixteen cotangent rows on their way up ([16][n]), sixteen solution rows and the
    // same block interleaved ([16][n] + [n][16]), the swept rows with their slot map, the sum [ncomp] and one block of
    // source derivatives [16][nsrc]
    DevBuf gr_cot, gr_x, gr_spec, gr_acc;
    uint64_t sn_cross_epoch = 0;
    int64_t sn_ndrivers = 0, sn_ncross = 0;
    nodal_ctx *adjoint = nullptr;
    uint64_t adjoint_epoch = 0;
    // multiport equivalents (ports.hip): the ports' nodes, Z [P][P] and V_oc [P] until they go down (the solution set
    // aside during the call borrows sn_x)
    DevBuf pt_buf;
    // transient analysis (transient.hip): the capacitor rows, probes and per-capacitor history words; the node ->
    // incident-capacitor lists (entries' nodes, their runs, capacitor << 3 | lead); the two solutions, the step's
    // right-hand side, the refinement's vectors and the judge's norms; waveforms, envelope and residuals until they go
    // down; the staging ring of kept solutions
    DevBuf tr_spec, tr_none, tr_node, tr_ptr, tr_con, tr_vec, tr_out, tr_ring;
    // ... with inductors (nodal_transient_rlc): their currents, i_0, the probed currents' rows until they go down and the
    // probed inductors' indices
    DevBuf tr_ind;
    // ... with diodes (nodal_transient_nl, transient_nl.hip): the diode rows, parameters, linearisations, limited voltages,
    // records, the iteration's right-hand side and the probed diodes' rows until they go down; the node -> incident-diode
    // lists (as tr_none .. tr_con, which stay the capacitors' and inductors')
    DevBuf tn_spec, tn_none, tn_node, tn_ptr, tn_con;
    // ... with bipolar transistors (nodal_newton_dc_bjt, newton.hip): the transports' GM rows, junctions, parameters,
    // linearisations and outputs until they go down; the node -> incident-transport lists (as tr_none .. tr_con, which
    // stay the diodes')
    DevBuf nb_spec, nb_none, nb_node, nb_ptr, nb_con;
    // ... and in the transient analysis (nodal_transient_nl_bjt, transient_nl.hip): the same for the transports of a run
    // in time, beside tn_* (the diodes', the junctions among them), with the probed transports' rows until they go down.
    // Its own: a handle may hold nb_* from an operating point as well
    DevBuf tb_spec, tb_none, tb_node, tb_ptr, tb_con;
    uint64_t numeric_epoch = 1;   // bumped by every numeric assembly (stamp_numeric): the identity of G's values
    uint64_t tr_mg_epoch = 0;     // numeric_epoch the multigrid hierarchy a transient call set up belongs to (0: none)
    uint64_t tr_lu_epoch = 0;     // ... and the sparse LU factors a transient call left
    // gradients through time (transient_gradient.hip).  NODAL_OPT_TRANSIENT_TAPE: a backward-Euler nodal_transient whose
    // every step was solved leaves x_0 .. x_steps ([steps + 1][n]) and its swept rows on the handle; the capacitor rows
    // and node lists stay where they are (tr_spec, tr_node, tr_ptr, tr_con).  The tape belongs to one numeric_epoch and
    // is void after an upload and after any later nodal_transient.
    bool transient_tape = false;
    bool tape_valid = false;
    uint64_t tape_epoch = 0;
    int32_t tape_steps = 0, tape_nsrc = 0;
    int64_t tape_ncap = 0, tape_nent = 0;  // capacitors, and the entries of their node list
    DevBuf tr_tape, tr_tsrc;
    // the backward sweep's own buffers: sixteen adjoints [16][n], the one before them, right-hand side, refinement
    // vectors, norms, the capacitors' history words, the sums and what else goes down once; the probes and cotangents;
    // the node -> incident-probe lists (as tr_none .. tr_con)
    DevBuf tg_vec, tg_out, tg_spec, tg_none, tg_node, tg_ptr, tg_con;
    uint64_t tg_lu_epoch = 0;     // numeric_epoch the sparse LU factors of the transposed child belong to (0: none)
    // AC analysis (ac.hip): the child context that holds the interleaved real form of G + j B(omega), 2n unknowns, as CSR
    // (kept per struct_epoch and reactive leads: ac_epoch, ac_key = kinds | leads a | leads b); per stored entry of the
    // child the place of G's value in `data` (-1: none), the entries' runs of reactive elements and the runs themselves
    // (element << 1 | subtract); ac_spec, the reactive elements and int32 lists of the call at hand, of whichever of the
    // four small-signal analyses (ac_upload_spec in ac_sweep.h: every call uploads anew); right-hand side, solution,
    // refinement vectors and norms; phasors, currents, residuals and peaks until they go down; the staging ring of kept
    // solutions
    nodal_ctx *ac = nullptr;
    uint64_t ac_epoch = 0;
    std::vector<int32_t> ac_key;
    DevBuf ac_gsrc, ac_ptr, ac_con, ac_spec, ac_vec, ac_out, ac_ring;
    // noise analysis (noise.hip): the child with the interleaved real form of (G + j B)^T for networks whose G is not
    // symmetric, built from the pattern and values of h->adjoint (G^T) and kept like h->ac with maps of its own (a
    // symmetric G shares h->ac); the input's right-hand side and, on the sparse LU route, refinement vectors, a block of
    // right-hand sides, one of adjoint phasors and the norms (the dense route solves in ap_vec); the workgroups' partial
    // sums; densities, gains, residuals and the integrated contributions until they go down
    nodal_ctx *ac_t = nullptr;
    uint64_t ac_t_epoch = 0;
    std::vector<int32_t> ac_t_key;
    DevBuf ac_t_gsrc, ac_t_ptr, ac_t_con, nz_vec, nz_part, nz_out;
    // AC port analysis (ac_ports.hip), on h->ac.  ap_vec and ap_rows belong to the block loop (ac_block_frequency,
    // ac_block_dense), whichever analysis calls it: the four interleaved blocks (right-hand sides, solutions, defect,
    // correction) or the dense route's right-hand sides and solutions, one vector and the judge's norms; the [16][2n]
    // rows of a block with a column redone alone (reserved when the first one is).  ap_out: Z, residuals and peaks until
    // they go down
    DevBuf ap_vec, ap_rows, ap_out;
    // AC gradient (ac_gradient.hip), on h->ac and, when G is not symmetric, h->ac_t: the forward right-hand side, x_f and
    // y_f (2n each); phasors, source terms, residuals and the two gradient sums until they go down
    DevBuf ag_vec, ag_out;
    DevBuf dbg_resid;  // testing hook nodal_debug_residual: the caller's x | b and the norms, nothing else lives here
    DevBuf dbg_apply;  // testing hooks nodal_debug_direct_apply / nodal_debug_cycle_apply: the caller's vectors during
                       // the call, nothing else lives here
    // exact elimination of nodes with <= 2 neighbours (lowdeg.hip): the reduced network is a
    // matrix-only context (no component table) that inherits the grounded-node flags
    nodal_ctx *lowdeg = nullptr;
    bool csr_only = false;
    DevBuf grounded;        // u8[n]
    DevBuf ld_newidx, ld_work;
    int ld_rounds = 0, ld_slow_rounds = 0;  // rounds that led to this context (all / those removing < 1/32)
    // The choice of the eliminated set and the pattern of the reduced matrix depend on the
    // STRUCTURE of this context's matrix only: kept while struct_epoch stands (value sweeps,
    // pair sweeps, repeated solves), so that a later round is three kernels and no read-back.
    uint64_t struct_epoch = 1;     // bumped whenever the CSR pattern of this context is rebuilt
    uint64_t ld_epoch = 0;         // struct_epoch the cached decision below belongs to
    int ld_state = 0;              // 1 too few candidates, 2 child built, 3 child built and singular (leftover)
    int ld_share = 0;              // the bar (n / share nodes) the decision was taken with
    int64_t ld_n = 0, ld_nnz = 0;
    const void *ld_rhs = nullptr;  // the right-hand side the last round read (a pair sweep swaps ps_buf in): for the testing hook
    DevBuf dbg_lowdeg;             // testing hooks nodal_debug_lowdeg_array / nodal_debug_floating_small: nothing else lives here

    // ---- symbolic assembly results ----
    bool have_symbolic = false;
    uint64_t sym_sizes_epoch = ~0ull;  // table_epoch the sizes below were read back for (stamp_symbolic); ~0: none yet
    int64_t sym_sizes[4] = {0, 0, 0, 0};  // nnz, ncontrib, nrhs, nrhs_contrib
    int sym_long_rows = -1;        // the matrix grouping of this table found rows of more than 16 stamps (1) / none (0)
    int64_t rhs_items = -1;        // components that stamp the right-hand side (counted at upload; -1: unknown)
    int64_t nnz = 0;        // matrix entries
    int64_t ncontrib = 0;   // matrix contributions
    int64_t nrhs = 0;       // rhs entries (rows with at least one contribution)
    int64_t nrhs_contrib = 0;
    DevBuf indptr;          // i32[n+1]
    DevBuf indices;         // i32[nnz]  (sorted inside each row)
    DevBuf rowidx;          // i32[nnz]  row of each entry (COO companion)
    DevBuf cptr;            // i32[nnz+1] contribution run of each entry
    DevBuf contrib;         // u32[ncontrib] comp<<3 | slot, in fold order
    DevBuf rhs_row;         // i32[nrhs]
    DevBuf rhs_cptr;        // i32[nrhs+1]
    DevBuf rhs_contrib;     // u32[nrhs_contrib]
    DevBuf rhs_none;        // scratch: the (unused) column list of the rhs grouping
    DevBuf diag_pos;        // i32[n] position of (i,i) in CSR or -1

    // ---- numeric assembly results ----
    bool have_numeric = false;
    bool force_pivoting = false;   // testing: use the tournament path even when passive
    bool gepp_panel = true;        // partial pivoting: one launch per 32-column panel (dense_lu.hip)
    bool passive_network = false;  // B == 0 and all R > 0 (set by stamp_numeric)
    DevBuf data;            // f64[nnz]
    DevBuf rhs;             // f64[n]
    DevBuf status;          // i64[4] device-side error words

    // ---- solve ----
    DevBuf x;               // f64[n]
    bool have_x = false;
    DevBuf dense;           // f64[n*n] column-major working copy for LU
    DevBuf piv;             // i32[n]
    DevBuf work;            // scratch (scans, sorts, solver vectors)
    DevBuf work2;
    DevBuf work3;           // grouping: padded scratch for hub-row sorts
    DevBuf solver;          // persistent solver vectors
    DevBuf krylov;          // FGMRES bases (sparse_general.hip)
    DevBuf gn_indptr, gn_indices, gn_rowidx, gn_data, gn_diag;  // node block of G
    DevBuf schur;           // diagonal Schur-complement approximation of the branch block
    int64_t gn_nnz = 0;     // entries of the node block the last general setup extracted
    // testing hooks nodal_debug_fgmres_cycle / nodal_debug_general_array: the `system` whose block preconditioner the
    // former set up last (-1: none) and that context's numeric_epoch then
    int32_t dbg_general_system = -1;
    uint64_t dbg_general_epoch = 0;

    // ---- timing ----
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms[3] = {0, 0, 0};
    double kern_ms = 0;
    int64_t kern_launches = 0;
    double kern_alg = 0;
    std::vector<hipEvent_t> evpool;  // HIP-event pairs around the dominant kernel

    void *amg = nullptr;  // multigrid hierarchy (amg.hip)
    void *sagg = nullptr; // smoothed-aggregation hierarchy (sagg.hip)
    int64_t sym_low_rows = -1;           // ... of the table grouped last (kept with sym_sizes)
    int64_t low_rows = -1;               // rows of two or three entries of the matrix pattern (upper bound; group.h), -1 unknown
    unsigned long long low_rows_epoch = ~0ull;  // struct_epoch it belongs to
    bool extra_streams = false;  // NODAL_OPT_EXTRA_STREAMS: the handle is used alone and may use streams of its own
    void *slu = nullptr;  // multifrontal LU of the direct route (sparse_direct.hip)
    void *ps_plan = nullptr;  // the presolve's plan, made ahead of the solve (presolve.hip: presolve_plan_ahead)
    void *ps_debug = nullptr; // testing hooks nodal_debug_presolve_*: the plan of the last build and what it reported
    bool slu_strict = false;  // refinement judged by |r| / |b| alone (the direct route's second opinion)
    int32_t last_iterations = 0;
    double last_relres = 0;
    int32_t amg_levels = 0;
    int64_t amg_min_n = 65;    // below this the sparse SPD path goes dense
};

#define NODAL_HIP_TRY(h, expr)                                                   \
    do {                                                                         \
        hipError_t _e = (expr);                                                  \
        if (_e != hipSuccess) {                                                  \
            char _buf[512];                                                      \
            snprintf(_buf, sizeof _buf, "%s failed at %s:%d: %s", #expr, __FILE__, \
                     __LINE__, hipGetErrorString(_e));                           \
            (h)->err = _buf;                                                     \
            return _e == hipErrorOutOfMemory ? NODAL_E_NOMEM : NODAL_E_HIP;      \
        }                                                                        \
    } while (0)

// ---- bounded host waits (wait.hip) ----
// Every host wait of the library: polls hipStreamQuery / hipEventQuery against NODAL_WAIT_TIMEOUT_S (default 60 s;
// 0: the runtime's blocking wait).  On a timeout: NODAL_E_HIP, nodal_last_error = the wait site + the last kernel
// enqueued on that stream, the handle marked hung.  `site` is a string literal ("file:line").
struct nodal_ctx;
int nodal_wait_stream(nodal_ctx *h, hipStream_t st, const char *site);
int nodal_wait_event(nodal_ctx *h, hipEvent_t ev, hipStream_t recorded_on, const char *site);
unsigned long long nodal_launches_noted();  // launches this thread has sent through the library's launch log
#define NODAL_STR2(x) #x
#define NODAL_STR(x) NODAL_STR2(x)
#define NODAL_SITE __FILE__ ":" NODAL_STR(__LINE__)
#define NODAL_WAIT_STREAM(h, st) NODAL_TRY(nodal_wait_stream((h), (st), NODAL_SITE))
#define NODAL_WAIT_EVENT(h, ev, st) NODAL_TRY(nodal_wait_event((h), (ev), (st), NODAL_SITE))

#define NODAL_TRY(expr)                  \
    do {                                 \
        int _s = (expr);                 \
        if (_s != NODAL_OK) return _s;   \
    } while (0)

// A section that spreads work over side streams joins them at its end; this makes the main stream wait for them on
// every OTHER way out as well (a failed call in the middle), so that no side stream keeps writing a handle's buffers
// behind the back of whatever the main stream does next.  disarm() on the normal way out, after the section's own join.
struct StreamJoinGuard {
    hipStream_t main;
    hipStream_t side[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int count = 0;
    bool armed = true;
    explicit StreamJoinGuard(hipStream_t m) : main(m) {}
    void add(hipStream_t s, hipEvent_t e) {
        if (s && e && s != main && count < 4) {
            side[count] = s;
            ev[count++] = e;
        }
    }
    void disarm() { armed = false; }
    ~StreamJoinGuard() {
        if (!armed) return;
        for (int i = 0; i < count; ++i)
            if (hipEventRecord(ev[i], side[i]) == hipSuccess) (void)hipStreamWaitEvent(main, ev[i], 0);
        (void)hipGetLastError();
    }
    StreamJoinGuard(const StreamJoinGuard &) = delete;
    StreamJoinGuard &operator=(const StreamJoinGuard &) = delete;
};

static inline int nodal_fail(nodal_ctx *h, int code, const char *msg) {
    h->err = msg;
    return code;
}

// ---- device-wide primitives (scan.hip) ----
// exclusive prefix sum of n uint32 values; out may alias in; total (optional,
// device pointer) receives the grand total.  `tmp` must hold scan_tmp_bytes(n).
size_t scan_tmp_bytes(int64_t n);
int scan_exclusive_u32(nodal_ctx *h, const uint32_t *in, uint32_t *out, int64_t n,
                       uint32_t *total_dev, void *tmp);
// testing hook (nodal_debug_scan_u32): scan_exclusive_u32 on a host array, nothing else
int scan_debug_u32(nodal_ctx *h, int64_t n, const uint32_t *in, uint32_t *out, bool in_place, uint32_t *total_out);

// ---- stamping (stamp.hip) ----
int stamp_symbolic(nodal_ctx *h);
int stamp_numeric(nodal_ctx *h, int32_t member, int64_t *bad_component);
int stamp_to_dense(nodal_ctx *h, double *G_dev, int64_t ld, bool col_major);
// source sweeps (nodal_solve_sources): slot_dev[comp] = index of comp among the swept rows, else -1 (*bad_dev: 1 a row
// that is not an A / E source, 2 a repeated row); then the right-hand sides of `cols` (<= 16) members whose swept
// values are swept_dev[y * nsrc + j], element (row, y) at out[row * rs + y * cs] (rows without a source untouched)
int stamp_sweep_slots(nodal_ctx *h, const int32_t *rows_dev, int32_t nsrc, int32_t *slot_dev, int32_t *bad_dev);
int stamp_rhs_multi(nodal_ctx *h, const int32_t *slot_dev, const double *swept_dev, int32_t nsrc, int32_t cols,
                    double *out, int64_t rs, int64_t cs);
// The swept rows of a call (api.hip): in range, narrowed and uploaded to rows_dev, stamp_sweep_slots, and the verdict read
// back (one wait) -- E_INVALID for a row out of range, one that is no A / E source, one named twice.  The texts are
// `prefix` + ["a "] + `row` + what is wrong: ("source sweep: ", "row"), ("gradient: ", "swept row").
int sweep_check_rows(nodal_ctx *h, const char *prefix, const char *row, int32_t nsrc, const int64_t *rows,
                     int32_t *rows_dev, int32_t *slot_dev, int32_t *bad_dev);
// ---- same G, many right-hand sides (multi_rhs_solve in sparse.hip) ----
// What a front end tells the one driver of source sweeps, port matrices and adjoint sensitivities.  Columns are
// addressed as element (row, y) at [row * rs + y * cs] throughout.
struct MultiRhsClient {
    bool wants_rows = true;  // hand_over gets the finished columns as [cols][n] rows as well
    int32_t max_cols = 512;  // the widest block hand_over accepts (the dense route hands a whole chunk over at 512)
    // adds the right-hand sides of columns m0 .. m0 + cols - 1 (cols <= 16) into a zeroed block
    virtual int build(int32_t m0, int cols, double *out, int64_t rs, int64_t cs) = 0;
    // takes the finished columns m0 .. m0 + cols - 1 (`rows`: the same as [cols][n] rows, null unless wants_rows): the
    // client's device work, its copies down, and the stream wait
    virtual int hand_over(int32_t m0, int cols, const double *x, int64_t rs, int64_t cs, const double *rows) = 0;
    // every column is singular: NaN into the client's own host arrays (info and resid are the driver's)
    virtual void all_singular(int32_t count) = 0;
protected:
    ~MultiRhsClient() = default;
};
// s: the context whose matrix is solved -- h itself, or the csr_only child that holds G^T
int multi_rhs_solve(nodal_ctx *h, nodal_ctx *s, bool dense, int32_t count, double *resid_out /* may be null */,
                    int32_t *info_out, MultiRhsClient &client);
// testing hook: the right-hand sides `client` builds, through the interleaved block, handed over as rows
int sparse_sources_rhs(nodal_ctx *h, int32_t count, MultiRhsClient &client);
// host milliseconds since t0
static inline double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
// a call on the solve context s: on failure its error text becomes the handle's
static inline int nodal_lift_error(nodal_ctx *h, nodal_ctx *s, int status) {
    if (status != NODAL_OK && s != h) h->err = s->err;
    return status;
}

// "The handle is left as it was found": the solution (set aside in sn_x) and what the last solve reported about itself,
// around an analysis that solves on the handle.  save before, restore after; the caller waits for the stream.
struct HandleKeeper {
    int32_t iterations = 0, levels = 0;
    double relres = 0, kern_ms = 0, kern_alg = 0;
    int64_t kern_launches = 0;
    bool copied = false;
    int save(nodal_ctx *h, bool copy_x) {
        iterations = h->last_iterations;
        levels = h->amg_levels;
        relres = h->last_relres;
        kern_ms = h->kern_ms;
        kern_alg = h->kern_alg;
        kern_launches = h->kern_launches;
        copied = copy_x;
        if (!copy_x) return NODAL_OK;
        NODAL_HIP_TRY(h, h->sn_x.reserve((size_t)h->n * 8 + 64));
        if (h->n > 0)
            NODAL_HIP_TRY(h, hipMemcpyAsync(h->sn_x.p, h->x.p, (size_t)h->n * 8, hipMemcpyDeviceToDevice, h->stream));
        return NODAL_OK;
    }
    // `what`: the analysis, as its error texts begin ("sensitivities", "port matrix")
    int restore(nodal_ctx *h, int status, const char *what) {
        h->last_iterations = iterations;
        h->amg_levels = levels;
        h->last_relres = relres;
        h->kern_ms = kern_ms;
        h->kern_alg = kern_alg;
        h->kern_launches = kern_launches;
        h->have_x = false;
        if (!copied) return status;
        if (hipMemcpyAsync(h->x.p, h->sn_x.p, (size_t)h->n * 8, hipMemcpyDeviceToDevice, h->stream) != hipSuccess) {
            if (status == NODAL_OK) {
                h->err = std::string(what) + ": could not put the solution back";
                status = NODAL_E_HIP;
            }
        } else {
            h->have_x = !h->hung;
        }
        return status;
    }
};

// ---- branch currents, power, sweep envelopes (branch.hip) ----
// the envelope of one source sweep: device arrays (branch_sweep_begin sets them) and the caller's host arrays (any null)
struct BranchSweep {
    double *absmax = nullptr, *pmin = nullptr, *pmax = nullptr, *partials = nullptr, *totals = nullptr;
    int32_t *absmax_member = nullptr, *pmin_member = nullptr, *pmax_member = nullptr;
    double *out_absmax = nullptr, *out_pmin = nullptr, *out_pmax = nullptr, *out_power = nullptr;
    int32_t *out_absmax_member = nullptr, *out_pmin_member = nullptr, *out_pmax_member = nullptr;
};
int branch_single(nodal_ctx *h, double *voltage, double *current, double *power, double *totals2);
int branch_sweep_begin(nodal_ctx *h, BranchSweep *env, int32_t count);
int branch_sweep_block(nodal_ctx *h, const BranchSweep *env, int32_t m0, int cols, const double *rows,
                       const int32_t *info, const double *swept_dev, const int32_t *slot_dev, int32_t nsrc);
int branch_sweep_finish(nodal_ctx *h, const BranchSweep *env, int32_t count, const int32_t *info);

// ---- adjoint sensitivities (sensitivity.hip; the transposed solves: multi_rhs_solve in sparse.hip) ----
// one call of nodal_sensitivities: the outputs' specification (device, [count]), the single solve's solution set aside
// (device, [n]) and the caller's host arrays
struct SensCall {
    const int32_t *kind = nullptr, *p = nullptr, *q2 = nullptr;
    const int32_t *kind_host = nullptr, *p_host = nullptr;  // the caller's own arrays
    const double *x = nullptr;
    double *sens_out = nullptr, *adjoint_out = nullptr;
};
// adds the entries of the columns c of outputs m0 .. m0 + cols - 1 (cols <= 16) into a zeroed block, element (row, y) at
// out[row * rs + y * cs]
int sens_rhs_block(nodal_ctx *h, const SensCall *call, int32_t m0, int cols, double *out, int64_t rs, int64_t cs);
// the table kernels for those outputs from their adjoints lam (same addressing), results to the host, and the wait
int sens_block(nodal_ctx *h, const SensCall *call, int32_t m0, int cols, const double *lam, int64_t rs, int64_t cs);
int sens_run(nodal_ctx *h, bool dense, int32_t count, const int32_t *kind, const int32_t *p, const int32_t *q2,
             double *sens_out, double *value_out, double *adjoint_out, double *resid_out, int32_t *info_out);
void sens_free_child(nodal_ctx *h);
// what the gradients (gradient.hip, transient_gradient.hip) share with the call above: the CCVS / CCCS rows grouped by
// their driving resistor (sn_cross, sn_ndrivers, sn_ncross; kept per table_epoch) and the child context that holds G^T
// (h->adjoint)
int sens_cross_list(nodal_ctx *h);
int sens_transposed_child(nodal_ctx *h);
// a csr_only child context of h in *slot, made on first use on h's streams, its solver options brought up to h's: what
// holds a matrix no netlist stamped (h->adjoint, h->ac); the caller sets K, B, n, nnz and the CSR arrays
nodal_ctx *csr_child(nodal_ctx *h, nodal_ctx **slot);
// *s: the context the transposed solves run on -- h itself when G is symmetric (B == 0 and passive), otherwise the
// child, brought up to date
int adjoint_context(nodal_ctx *h, nodal_ctx **s);

// ---- loss gradients (gradient.hip; the transposed solves: multi_rhs_solve in sparse.hip) ----
// one adjoint solve per member with the caller's dense cotangent, the per-row formulas summed over the members on the
// device; the arguments are those of nodal_gradient
int grad_run(nodal_ctx *h, bool dense, int32_t count, const double *x, const double *cotangent, int32_t nsrc,
             const int64_t *rows, double *grad_out, double *grad_sources_out, double *adjoint_out, double *resid_out,
             int32_t *info_out);
// the table kernels of one block of `cols` (<= 16) members, element (j, y) of lam at [j * rs + y * cs] and of x at
// [j * xrs + y * xcs] (strides may be negative): k_gradient_block and k_gradient_cross add the members' terms, in member
// order, onto grad_dev [ncomp] (sens_cross_list first); k_gradient_sources writes out[y * nsrc + j] for the swept rows
int grad_launch_table(nodal_ctx *h, int cols, const double *lam, int64_t rs, int64_t cs, const double *x, int64_t xrs,
                      int64_t xcs, double *grad_dev);
int grad_launch_sources(nodal_ctx *h, int cols, int32_t nsrc, const int32_t *swept_dev, const double *lam, int64_t rs,
                        int64_t cs, double *out);

// ---- transient analysis (transient.hip): capacitors stepped in time, one solve per step on the kept matrix work ----
// the arguments are those of nodal_transient; the source table is already on the device (sw_slot, sw_vals: api.hip's
// sweep_prepare).  ms_matrix: host milliseconds of the matrix work done once per call, 0.0 when it was kept
// inductors: nodal_transient_rlc's further arguments, nullptr for nodal_transient (the same run with nind == 0)
struct TransientInductors {
    int64_t nind = 0;
    const int64_t *rows = nullptr;   // [nind] table rows of type R, the companion resistors
    const double *i0 = nullptr;      // [nind] the currents at t_0 (nullptr: zero)
    int32_t ncur = 0;
    const int32_t *cur_index = nullptr;  // [ncur] indices into the inductors
    double *cur_out = nullptr;           // [steps + 1][ncur]
    double *i_final_out = nullptr;       // [nind]
};
int transient_run(nodal_ctx *h, bool dense, int32_t steps, int32_t method, int64_t ncap, const int64_t *cap_rows,
                  int32_t nsrc, const double *x0, int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b,
                  double *wave_out, int32_t keep_every, double *x_out, double *pot_min, int32_t *pot_min_step,
                  double *pot_max, int32_t *pot_max_step, double *resid_out, int32_t *info_out, int32_t *iters_out,
                  double *ms_matrix, const TransientInductors *inductors = nullptr, struct TransientDiodes *diodes = nullptr);
// One step's solve, shared by the forward steps and the backward sweep of transient_gradient.hip.  s: the context whose
// matrix is solved -- h itself, or the csr_only child that holds G^T (never the multigrid route); lu_epoch: where the
// numeric_epoch of s's kept LU factors is filed; rvec, dvec [n] and norms ([16][4] + [16]) are the caller's scratch.
enum { TR_ROUTE_DENSE, TR_ROUTE_LU, TR_ROUTE_MG };
struct TransientSolver {
    nodal_ctx *s = nullptr;
    uint64_t *lu_epoch = nullptr;
    double *rvec = nullptr, *dvec = nullptr, *norms = nullptr;
    int route = TR_ROUTE_DENSE;
    bool direct = false;      // multigrid route: the iteration gave up, this step and every later one by the direct solve
    bool all_direct = false;  // sparse LU route: pivots were replaced, every step by the direct solve (which judges its own)
    bool mg_setup = false, first = true;
    bool force_dense = false;  // the dense panel at any size (ac.hip with `dense`); set before transient_solver_begin
    double bar = 0.0;
};
// the route and its matrix work (the dense panel's room, the factorisation unless kept, whether the hierarchy is to be
// set up); *dead: a singular factorisation without `dense`; ms_matrix as transient_run's
int transient_solver_begin(nodal_ctx *h, TransientSolver &ts, bool dense, int32_t steps, bool *dead, double *ms_matrix);
// xk from bvec: dense panel, multigrid, or sparse LU with one refinement step, with their fall-backs to the sparse direct
// solve, and the judgement -- *judged: the scaled residual is in *resid_host already, otherwise at norms[4 * 16] on the
// device.  *inf > 0: singular, nothing was judged.
int transient_solver_step(nodal_ctx *h, TransientSolver &ts, const double *bvec, double *xk, int32_t *inf, int32_t *it,
                          double *resid_host, bool *judged, double *ms_matrix);
// out[node[e]] += the signed sum of src over entry e's contributions (a group.h node list: item << 3 | slot, slot 0 adds,
// any other subtracts), in list order, one lane per entry and no atomics; nent == 0 launches nothing
int signed_list_add(nodal_ctx *h, int64_t nent, const int32_t *node, const int32_t *cptr, const uint32_t *contrib,
                    const double *src, double *out);
// rhs += S (g o S^T x_prev), the capacitors' history currents (k_transient_history with `method`, then signed_list_add
// over the node list of the last transient_run: tr_node, tr_ptr, tr_con); hist [ncap] is scratch.  A run with inductors
// passes hist [ncap + nind] whose last nind words it formed itself (transient.hip); ncap == 0 skips the first kernel.
int transient_add_history(nodal_ctx *h, int64_t ncap, int method, const int32_t *rows_dev, int64_t nent, const double *x_prev,
                          double *hist, double *rhs);

// ---- nonlinear DC analysis (newton.hip): diodes as companion R rows, Newton's method with the lane work on the device ----
struct NewtonOutputs {           // host arrays, each may be null except iterations and converged
    double *x = nullptr;         // [n] the last iterate
    double *v = nullptr, *i = nullptr, *g = nullptr;  // [nd] of the last iterate
    double *iterates = nullptr;  // [max_iter][n]
    double *vh = nullptr;        // [max_iter + 1][nd]
    double *record = nullptr;    // [max_iter][record_words]: not converged, limited, max |v - vh|, scaled residual,
                                 // and with five words the transports that failed
    int record_words = 4;
    int32_t *info = nullptr, *iters = nullptr, *route = nullptr;  // [max_iter]
    int32_t *iterations = nullptr, *converged = nullptr;
};
// the swept sources are those of the last sweep_prepare (one setting); *ms_matrix: host ms of assembly, factorisation and
// hierarchy setup summed over the iterations, *ms_symbolic: the part of it that was an analysis or a full hierarchy setup
// tr: the transports of nodal_newton_dc_bjt (null, or nt == 0: none -- the launches and bits of a call without them)
struct NewtonTransports {
    int64_t nt = 0;
    const int64_t *gm_rows = nullptr;   // [nt][2] table rows of type GM: forward, reverse
    const int32_t *junction = nullptr;  // [nt][2] indices into the diodes: jf, jr
    const double *i_s = nullptr;        // [nt]
    double *it = nullptr, *gmf = nullptr, *gmr = nullptr;  // [nt] of the last iterate, each may be null
};
int newton_run(nodal_ctx *h, bool dense, int64_t nd, const int64_t *diode_rows, const double *isat, const double *nvt,
               double gmin, int32_t nsrc, const double *x0, int32_t max_iter, double reltol, double vntol, double abstol,
               const NewtonOutputs &out, double *ms_matrix, double *ms_symbolic, const NewtonTransports *tr = nullptr);

// ---- what the three nonlinear analyses share (newton.hip): the call's diodes on the device, one Newton iteration ----
// A spec buffer holds, every part rounded up to sixteen words,
//     diode rows [nd] int32 | the caller's further int32 words | bad flag | i_sat, n_vt, J, g_k, i_k [nd] doubles each |
//     the caller's further doubles
// and three more buffers the diodes' node list (group.h over diode_lanes.h's DiodeLeads): tr_* for nodal_newton_dc and
// nodal_newton_gradient, tn_* for nodal_transient_nl, whose capacitors' list holds tr_*.
struct TransportSet;
struct DiodeSet {
    int64_t nd = 0, nent = 0;  // diodes, entries of their node list
    double gmin = 0.0;
    int32_t *rows_dev = nullptr;
    double *isat_dev = nullptr, *nvt_dev = nullptr, *hist = nullptr, *gk = nullptr, *ik = nullptr;
    DevBuf *node = nullptr, *ptr = nullptr, *con = nullptr;
    // Once per call.  E_INVALID, the texts beginning with `what` ("newton: "): a row out of range, diodes on a network
    // without nodes; then, unless n == 0 (nothing of the set is used), the buffer carved, rows (narrowed) and parameters
    // up, and with the device's verdict (ONE wait: the uploads are done too, the host arrays may go) a row that is not an
    // R, an i_sat or n_vt that is not positive and finite; then the node list.  nd == 0 carves only.
    int prepare(nodal_ctx *h, const char *what, int64_t nd, const int64_t *rows, const double *isat, const double *nvt,
                double gmin, DevBuf &spec, DevBuf &list_none, DevBuf &list_node, DevBuf &list_ptr, DevBuf &list_con,
                size_t more_words, size_t more_doubles, int32_t **words, double **doubles);
    // the lanes (nd == 0 launches nothing): vh = x(a) - x(b); g, i at vh -- 1 / g into the diodes' rows of `value`,
    // J = g vh - i into hist, g and i into gk and ik; column[rows[d]] = v; rhs += J at the anodes, -= J at the cathodes
    int start(nodal_ctx *h, const double *x, double *vh) const;
    int linearise(nodal_ctx *h, const double *vh, double *value) const;
    int fill(nodal_ctx *h, double v, double *column) const;
    int add_currents(nodal_ctx *h, double *rhs) const;
    // linearise() into the value column the assembly reads, then stamp_numeric (its host ms added to *ms_stamp).
    // *overflowed: some g overflowed, 1 / g == 0 and the assembly said NODAL_E_ZERO_RESISTANCE -- the diodes' rows then
    // hold 1.0 and G is assembled from them, so that the handle stays usable; the call has no matrix to go on with
    // With transports: their lanes run behind the diodes' and before the assembly; a gmf or gmr that is not finite is
    // an overflow as well (ONE more read, of the transports' flag word, behind the assembly's wait), and the GM rows
    // then hold 0.0
    int linearise_and_assemble(nodal_ctx *h, const double *vh, bool *overflowed, double *ms_stamp,
                               const TransportSet *transports = nullptr) const;
};

// The call's transports on the device (transistor_lanes.h): the transport currents of bipolar transistors whose two
// junctions are members jf, jr of the DiodeSet beside it.  A spec buffer holds, every part rounded up to sixteen words,
//     GM rows [nt][2] int32 (forward, reverse) | junctions [nt][2] int32 (jf, jr) | flags (word 0: the check's verdict,
//     word 1: a linearisation that is not finite) | i_s, JT, gmf_k, gmr_k, iT_k [nt] doubles each | the caller's further
//     doubles
// and three more buffers the transports' node list (group.h over TransportLeads).  A network with transports never
// takes the multigrid route: GM rows make it non-passive.
struct TransportSet {
    int64_t nt = 0, nent = 0;  // transports, entries of their node list
    int32_t *gm_dev = nullptr, *jn_dev = nullptr, *flag_dev = nullptr;
    double *is_dev = nullptr, *hist = nullptr, *gmf = nullptr, *gmr = nullptr, *it = nullptr;
    DevBuf *node = nullptr, *ptr = nullptr, *con = nullptr;
    // Once per call, behind the DiodeSet's prepare.  E_INVALID, the texts beginning with `what`: a GM row out of range;
    // then the buffer carved, rows (narrowed), junctions and i_s up, and with the device's verdict (ONE wait) a
    // junction index outside [0, nd), a GM row that is not of type GM, two rows of a transport that do not share their
    // a, b, a row whose c, d are not the leads of the junction's row, an i_s that is not positive and finite; then the
    // node list.  nt == 0 is not prepared at all: newton_iteration takes a null set.
    int prepare(nodal_ctx *h, const char *what, const DiodeSet &diodes, int64_t nt, const int64_t *gm_rows,
                const int32_t *junction, const double *i_s, DevBuf &spec, DevBuf &list_none, DevBuf &list_node,
                DevBuf &list_ptr, DevBuf &list_con, size_t more_doubles, double **doubles);
    // the lanes: gmf, gmr, iT at (vh[jf], vh[jr]) -- gmf and -gmr into the GM rows of `value`, JT into hist, flag word 1
    // set by a gmf or gmr that is not finite (zeroed first); column[both rows of t] = v; rhs += JT at the leads a,
    // -= JT at the leads b
    int linearise(nodal_ctx *h, const DiodeSet &diodes, const double *vh, double *value) const;
    int fill(nodal_ctx *h, double v, double *column) const;
    int add_currents(nodal_ctx *h, double *rhs) const;
};

// How one Newton iteration ended; the first three have an x and a record.  NOT_FINITE: the record is not finite,
// OVERFLOWED: linearise_and_assemble's, DEAD: transient_solver_begin's verdict, SINGULAR: transient_solver_step's inf > 0
enum { NEWTON_CONVERGED, NEWTON_GO_ON, NEWTON_NOT_FINITE, NEWTON_OVERFLOWED, NEWTON_DEAD, NEWTON_SINGULAR };
// failed, limited, bits of max |v - vh|, bits of the scaled residual, 1 / g moved, transports that failed
constexpr int NEWTON_REC_WORDS = 6;
constexpr int NEWTON_REC_TRANSPORTS = 5;
struct NewtonStep {
    int outcome = NEWTON_GO_ON;
    int32_t it = 0;       // the solver's iterations
    int32_t route = -1;   // nodal_newton_dc's code: 0 dense, 1 sparse LU, 2 multigrid, 3 the sparse direct solve
    bool judged = false;  // the scaled residual was on the host before the record came down
    double dvmax = 0.0, scaled = 0.0;
    unsigned long long words[NEWTON_REC_WORDS] = {0, 0, 0, 0, 0, 0};  // the record as read
    bool solved() const { return outcome <= NEWTON_NOT_FINITE; }
};
// One iteration on h's stream: the linearisation at vh_now (and with `assemble` the assembly; false: the matrix work
// `ts` keeps still stands), rhs += the diodes' J (the caller has put the sources and any history into rhs), the route
// and the solve into xk, the update lane into vh_next and the zeroed record `rec` (count_moved: word 4 as well), the
// iterate to iterate_host if that is not null, and ONE read of the record.  The iteration's host waits: the assembly's
// status words, what the solver looks at, the record.  Without diodes: the solve and the record's residual alone.
// *ms_matrix += the host ms of assembly and solver, *ms_symbolic += the part that was an analysis or a full setup.
// `transports` (null: none, and then the launches and the bits are those of the iteration without the argument): linearised
// behind the diodes at the same vh_now, rhs += their JT behind the diodes', one lane each behind the diodes' update lane
// that counts into word NEWTON_REC_TRANSPORTS of the record; converged when no diode and no transport failed.  With
// `assemble` only.
int newton_iteration(nodal_ctx *h, const DiodeSet &diodes, TransientSolver &ts, bool dense, bool assemble, bool count_moved,
                     const double *vh_now, double *vh_next, double *rhs, double *xk, unsigned long long *rec, double reltol,
                     double vntol, double abstol, double *iterate_host, double *ms_matrix, double *ms_symbolic, NewtonStep *step,
                     const TransportSet *transports = nullptr);

// ---- gradients through the operating point (newton_gradient.hip): one transposed solve with J at the caller's x ----
struct NewtonGradientOutputs {   // host arrays, each may be null except grad (with ncomp > 0) and info
    double *grad = nullptr;                               // [ncomp], +0.0 in the diode rows
    double *grad_isat = nullptr, *grad_nvt = nullptr;     // [nd]
    double *grad_gmin = nullptr;                          // [1]
    double *grad_sources = nullptr;                       // [nsrc]
    double *adjoint = nullptr;                            // [n]
    double *resid = nullptr, *op_resid = nullptr;         // [1] each: of the adjoint solve, of x as an operating point
    int32_t *info = nullptr;                              // [1]
};
// the arguments are those of nodal_newton_gradient; the sources are those of the last sweep_prepare (one setting);
// ms_matrix and ms_symbolic as newton_run's
int newton_gradient_run(nodal_ctx *h, bool dense, int64_t nd, const int64_t *diode_rows, const double *isat, const double *nvt,
                        double gmin, int32_t nsrc, const double *x, const double *cotangent, const NewtonGradientOutputs &out,
                        double *ms_matrix, double *ms_symbolic);

// ---- nonlinear transient analysis (transient_nl.hip): Newton's method inside every step of transient_run ----
// nodal_transient_nl's further arguments, and the loop's state.  transient_run with `diodes` leaves the route and the
// matrix work to step(): prepare() once before the first step (uploads, checks, node lists, row 0 of the diode probes),
// step() in place of transient_solver_step (base: the step's sources and history currents, held fixed; *inf 0 converged,
// 1 singular, 2 not converged), after_step() once x_k stands, finish() enqueues what comes down once and finish_host()
// writes NaN where the steps from first_dead on were to land.
// With transports (nodal_transient_nl_bjt, nt > 0): a TransportSet prepared once per call behind the DiodeSet, on tb_*,
// and handed to newton_iteration in every iteration; a step has converged when no diode and no transport fails.  Such a
// call assembles in EVERY iteration (`moved` stays true, updates_out[k] == newton_out[k]): gmf = i_s exp(v_f / n_f) / n_f
// has no gmin floor, its bits move whenever a junction voltage moves, and a bit-comparison reuse rule would almost never
// fire.  So newton_iteration's `assemble == false` branch is never reached with a set.  nt == 0: nothing changes.
struct TransientDiodes {
    int64_t nd = 0;
    const int64_t *rows = nullptr;            // [nd] table rows of type R, the companion resistors
    const double *isat = nullptr, *nvt = nullptr;
    double gmin = 0.0, reltol = 0.0, vntol = 0.0, abstol = 0.0;
    int32_t max_iter = 1;
    int32_t ndprobe = 0;
    const int32_t *dprobe_index = nullptr;    // [ndprobe] indices into the diodes
    int32_t *newton_out = nullptr, *updates_out = nullptr;  // [steps]
    double *dv_out = nullptr, *di_out = nullptr;            // [steps + 1][ndprobe]
    double *vh_final_out = nullptr;                         // [nd]
    int64_t nt = 0;                            // transports (NewtonTransports' three arrays)
    const int64_t *gm_rows = nullptr;          // [nt][2]
    const int32_t *junction = nullptr;         // [nt][2]
    const double *i_s = nullptr;               // [nt]
    int32_t ntprobe = 0;
    const int32_t *tprobe_index = nullptr;     // [ntprobe] indices into the transports
    double *tv_out = nullptr, *ti_out = nullptr;  // [steps + 1][ntprobe][2]: v_f, v_r; [steps + 1][ntprobe][3]: i_f, i_r, iT
    double ms_matrix = 0.0, ms_symbolic = 0.0;  // newton_run's two sums
    // the loop's state
    bool reuse = true;        // NODAL_TNL_REUSE
    bool moved = true;        // the next linearisation's 1 / g differs from what G was assembled from (or is not known to)
    int64_t rec_at = 0;
    int32_t slot = 0;         // which of the two vh vectors the next linearisation reads
    DiodeSet set;
    int32_t *pidx_dev = nullptr;
    double *vh = nullptr, *rhs = nullptr, *pv_dev = nullptr, *pi_dev = nullptr;
    unsigned long long *rec_dev = nullptr;
    TransportSet tset;        // prepared when nt > 0
    int32_t *tpidx_dev = nullptr;
    double *tpv_dev = nullptr, *tpi_dev = nullptr;
    const TransportSet *transports() const { return nt > 0 ? &tset : nullptr; }
    int prepare(nodal_ctx *h, int32_t steps, const double *x0_dev);
    int step(nodal_ctx *h, TransientSolver &ts, bool dense, int32_t k, const double *xp, const double *base, double *xk,
             int32_t *inf, int32_t *it, double *resid_host, bool *judged);
    int after_step(nodal_ctx *h, int32_t k, const double *xk);
    int finish(nodal_ctx *h, int32_t steps);
    void finish_host(int32_t steps, int32_t first_dead);
};

// ---- gradients through time (transient_gradient.hip): the adjoint of the recorded backward-Euler run ----
// the arguments are those of nodal_transient_gradient; ms_matrix as transient_run's
int tgrad_run(nodal_ctx *h, bool dense, int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b,
              const double *wave_cot, double *grad_out, double *grad_sources_out, double *grad_x0_out, double *adjoint_out,
              double *resid_out, int32_t *info_out, double *ms_matrix);

// ---- AC analysis (ac.hip): one solve of the interleaved real form of G + j B(omega) per frequency, on the child h->ac ----
// the arguments are those of nodal_ac_sweep; ms_analysis: host milliseconds of the child's pattern and of the sparse LU's
// symbolic analysis done by this call (0.0 when both were kept), ms_factor: of the numeric factorisations, summed
int ac_run(nodal_ctx *h, bool dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
           const double *value, const int32_t *lead_a, const int32_t *lead_b, int32_t nsrc, const int64_t *src_rows,
           const double *src_re, const double *src_im, int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b,
           double *wave_out, int32_t ncur, const int32_t *cur_index, double *cur_out, int32_t keep_every, double *x_out,
           double *peak_out, int32_t *peak_freq_out, double *resid_out, int32_t *info_out, double *ms_analysis,
           double *ms_factor);
void ac_free_child(nodal_ctx *h);
// (what the other small-signal analyses share with it: ac_sweep.h)

// ---- noise analysis (noise.hip): thermal-noise spectra by the adjoint of the AC system, one factorisation per frequency ----
// the arguments are those of nodal_ac_noise; ms_analysis, ms_factor as ac_run's
int noise_run(nodal_ctx *h, bool dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
              const double *value, const int32_t *lead_a, const int32_t *lead_b, double temperature, int32_t nout,
              const int32_t *out_a, const int32_t *out_b, int64_t input_row, const double *weight, double *density_out,
              double *gain_out, double *contrib_out, double *resid_out, int32_t *info_out, double *ms_analysis,
              double *ms_factor);

// ---- AC port analysis (ac_ports.hip): the multiport Z(j omega) of an RLC network, one factorisation per frequency ----
// (the per-frequency block loop, ac_block_frequency: ac_sweep.h)
// the arguments are those of nodal_ac_ports; ms_analysis, ms_factor as ac_run's
int ac_ports_run(nodal_ctx *h, bool dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
                 const double *value, const int32_t *lead_a, const int32_t *lead_b, int32_t nports, const int32_t *ia,
                 const int32_t *ib, double *z_out, double *node_peak_out, int32_t *node_peak_port_out,
                 int32_t *node_peak_freq_out, double *resid_out, int32_t *info_out, int64_t *work_out, double *ms_analysis,
                 double *ms_factor);

// ---- AC gradient (ac_gradient.hip): the adjoint of the AC analysis, dL/d(every value) of a loss of the probe phasors ----
// the arguments are those of nodal_ac_gradient; ms_analysis, ms_factor as ac_run's
int ac_gradient_run(nodal_ctx *h, bool dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
                    const double *value, const int32_t *lead_a, const int32_t *lead_b, int32_t nsrc, const int64_t *src_rows,
                    const double *src_re, const double *src_im, int32_t nprobe, const int32_t *probe_a,
                    const int32_t *probe_b, const double *wave_cot, double *wave_out, double *grad_out,
                    double *grad_react_out, double *grad_sources_out, int32_t keep_every, double *adjoint_out,
                    double *resid_out, int32_t *info_out, int64_t *work_out, double *ms_analysis, double *ms_factor);

// ---- multiport Thevenin / Norton equivalents (ports.hip; the solves: multi_rhs_solve in sparse.hip) ----
// one call of nodal_port_matrix: the ports' nodes (device, [nports] each, -1 ground) and Z (device, [nports][nports])
struct PortCall {
    int32_t nports = 0;
    const int32_t *ia = nullptr, *ib = nullptr;
    double *z = nullptr;
};
// adds the entries of s_q = e(a_q) - e(b_q) of ports m0 .. m0 + cols - 1 (cols <= 16) into a zeroed block, element
// (row, y) at out[row * rs + y * cs]
int port_rhs_block(nodal_ctx *h, const PortCall *call, int32_t m0, int cols, double *out, int64_t rs, int64_t cs);
// z[p][m0 + y] = X(a_p, y) - X(b_p, y) for the finished rows [cols][n] of those ports (cols <= 512); a column whose
// info (host, indexed by port) is > 0 becomes NaN in every row
int port_gather_block(nodal_ctx *h, const PortCall *call, int32_t m0, int cols, const double *rows, const int32_t *info);
int port_run(nodal_ctx *h, bool dense, int32_t nports, const int32_t *ia, const int32_t *ib, double *z_out,
             double *voc_out, double *resid_out, int32_t *info_out);

// ---- fp64 MFMA GEMM (gemm_f64.hip), column-major ----
enum { GEMM_SUB = 0, GEMM_SET = 1, GEMM_SETNEG = 2 };  // C -= A B | C = A B | C = -A B
int gemm_f64(nodal_ctx *h, hipStream_t stream, int mode, double *C, int64_t ldc, const double *A,
             int64_t lda, const double *B, int64_t ldb, int64_t M, int64_t N, int64_t K);
struct GemmProblem {
    double *C; int64_t ldc;
    const double *A; int64_t lda;
    const double *B; int64_t ldb;
    int M, N, K;
};
int gemm_pair_f64(nodal_ctx *h, hipStream_t stream, int mode, const GemmProblem &p0, const GemmProblem &p1);
int gemm_sub_f64(nodal_ctx *h, hipStream_t stream, double *C, int64_t ldc, const double *A,
                 int64_t lda, const double *B, int64_t ldb, int64_t M, int64_t N, int64_t K);
// C -= At^T B for the upper triangle of a square-leading C (At: K x M panel, B: K x N, column-major)
int gemm_sub_tn_upper_f64(nodal_ctx *h, hipStream_t stream, double *C, int64_t ldc, const double *At,
                          int64_t ldat, const double *B, int64_t ldb, int64_t M, int64_t N, int64_t K, int band);

// ---- dense LU (dense_lu.hip) ----
// leading dimension of the column-major dense panel: padded so that 32-row tiles
// are aligned and columns do not alias on the HBM channels
static inline int64_t dense_lda(int64_t n) {
    int64_t l = (n + 31) & ~(int64_t)31;
    if (l < 32) l = 32;
    if (l % 1024 == 0) l += 32;
    return l;
}
int dense_factor_solve(nodal_ctx *h, int32_t *info);
int dense_fill_nan(nodal_ctx *h, double *x, int64_t n);
// block elimination with inverted diagonal blocks (block_elim.hip): factor + back substitution
int dense_block_elimination(nodal_ctx *h, double *A, int64_t n, int64_t lda, int32_t nrhs, double *xout,
                            int64_t ldx, int32_t *dinfo);
int dense_factor_solve_multi(nodal_ctx *h, int32_t nrhs, double *xout, int64_t ldx, int32_t *info);
int dense_prepare(nodal_ctx *h);
int dense_prepare_pairs(nodal_ctx *h, int32_t nrhs, const int32_t *ia, const int32_t *ib);
int sparse_solve_pairs(nodal_ctx *h, int32_t npairs, const int32_t *ia, const int32_t *ib,
                       double *res_dev, int32_t *info);
int lowdeg_solve_pairs(nodal_ctx *h, int32_t npairs, const int32_t *ia, const int32_t *ib, double *res_dev,
                       bool *done, int32_t *info);

// ---- aggregation multigrid preconditioner (amg.hip) ----
int amg_setup(nodal_ctx *h, double *flag_dev);
int amg_setup_csr(nodal_ctx *h, int64_t n, int64_t nnz, const int32_t *indptr,
                  const int32_t *indices, const int32_t *rowidx, const double *data,
                  const int32_t *diag_pos, double *flag_dev);
int amg_apply(nodal_ctx *h, const double *r, double *z);
int amg_num_levels(nodal_ctx *h);
int64_t amg_level_size(nodal_ctx *h, int level);
void amg_destroy(nodal_ctx *h);
// another solver takes the matrix (or the matrix changes): the hierarchies of h and of its reduced systems are no longer
// what the last solve preconditioned with.  Only the testing hooks below look at this.
void amg_invalidate(nodal_ctx *h);
// testing hooks (nodal_debug_amg_info / nodal_debug_amg_array / nodal_debug_amg_apply): sizes, raw device buffers and
// one application of cycle() at a level outside the tail
int amg_debug_info(nodal_ctx *h, int32_t *nlev, int64_t *ints, int64_t *words, double *reals, int64_t *tail);
int amg_debug_array(nodal_ctx *h, int32_t level, int32_t which, void *dst, int64_t capacity_bytes, int64_t *bytes_out);
int amg_debug_apply(nodal_ctx *h, int32_t level, const double *r, double *z, int32_t *params_out);
void sagg_destroy(nodal_ctx *h);
// smoothed-aggregation FCG (sagg.hip): NODAL_OK, -1 breakdown, -2 structurally singular,
// -3 declined (not this hierarchy's kind of network: use amg.hip)
int sagg_fcg_solve(nodal_ctx *h, const double *b, bool do_setup, int32_t *info, int32_t *iters, double *resid);
bool sagg_ready(nodal_ctx *h, int64_t n);  // a hierarchy for n unknowns is set up
bool sagg_refreshed(nodal_ctx *h);         // ... and its last setup kept the symbolic part: the values alone were refreshed
// up to 16 probe pairs per iteration on that hierarchy (sagg_multi.h); -1: breakdown / no convergence
int sagg_pairs_block_width();  // pairs the block iteration takes per call (sagg_multi.h: MK)
// up to 16 general right-hand sides B (interleaved by row, unused columns zero) on that hierarchy; each column stops on
// |r| <= 1e-13 |b|, an all-zero one at once with x = 0; X receives the solutions in the same layout.  -1: breakdown /
// no convergence
int sagg_fcg_solve_block(nodal_ctx *h, int32_t count, const double *B, double *X, int32_t *iters);
int sagg_fcg_solve_pairs_block(nodal_ctx *h, int32_t count, const int32_t *ia_host, const int32_t *ib_host,
                               double *res_dev, int32_t *iters);
void sagg_invalidate(nodal_ctx *h);  // the hierarchy is not to be used again until the next setup
// the same hierarchy as a preconditioner for any device CSR matrix (general: a few off-diagonals
// of either sign, not symmetric); sagg_apply: z ~= A^-1 r with one cycle
int sagg_setup_csr(nodal_ctx *h, int64_t n, int64_t nnz, const int32_t *indptr, const int32_t *indices,
                   const double *data, bool general, bool check_floating, bool *accepted, int32_t *floating);
typedef float nodal_cyc_t;  // vectors inside the multigrid cycle (csrc/sagg.hip: cyc_t)
// x0_ready: the caller's last kernel already left the cycle's start iterate w D^-1 r (sagg_x0_slot) -- the launch that
// computes it is skipped
int sagg_apply(nodal_ctx *h, const double *r, double *z, bool x0_ready = false, int it = -1);
// where a producer of r can leave the start iterate of the next sagg_apply: x0[i] = (nodal_cyc_t)(omega * dinv[i] * r[i]),
// i < n0.  false: no hierarchy.
bool sagg_x0_slot(nodal_ctx *h, const double **dinv, nodal_cyc_t **x0, int64_t *n0, double *omega);
int sagg_levels(nodal_ctx *h);
// testing hooks (nodal_debug_hierarchy_info / nodal_debug_hierarchy_array): the hierarchy's sizes and raw device buffers
int sagg_debug_info(nodal_ctx *h, int32_t *nlev, int64_t *ints, double *reals);
int sagg_debug_array(nodal_ctx *h, int32_t level, int32_t which, void *dst, int64_t capacity_bytes, int64_t *bytes_out);
// testing hook (nodal_debug_cycle_apply): one application of the hierarchy's cycle to host vectors, nothing behind it
int sagg_debug_cycle_apply(nodal_ctx *h, int32_t mode, const double *r, const double *u, const double *frozen, double *z,
                           double *dots_out, int32_t *params_out);
int sagg_spmv(nodal_ctx *h, const double *x, double *y, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);  // y = A x on the hierarchy's own (level-0, ELL) matrix
int amg_has_floating_component(nodal_ctx *h, const uint8_t *grounded0, int32_t *floating);
int csr_has_floating_component(nodal_ctx *h, const uint8_t *grounded, int32_t *floating);

// u8[n] flags: 1 where a resistor connects the node to ground (stamp.hip)
int stamp_grounded_flags(nodal_ctx *h, uint8_t *flags_dev);
// the same for any context, matrix-only ones included (lowdeg.hip)
int grounded_flags(nodal_ctx *h, uint8_t *flags_dev);
int csr_to_dense(nodal_ctx *h, double *G_dev, int64_t ld);
int csr_small_floating_check(nodal_ctx *h, int32_t *floating);
int csr_floating_check_small(nodal_ctx *h, int64_t n, const int32_t *indptr, const int32_t *indices,
                             const uint8_t *grounded, uint32_t *flag_dev);
int lowdeg_solve(nodal_ctx *h, int min_share, bool *done, int32_t *info, int32_t *iters, double *resid);
// testing hooks (nodal_debug_lowdeg_info / _array, nodal_debug_floating_small): the rounds the last solve left, one array
// of one round, and small_floating_check on a host graph -- no arithmetic of their own
int lowdeg_debug_info(nodal_ctx *h, int32_t *rounds, int64_t *ints);
int lowdeg_debug_array(nodal_ctx *h, int32_t round, int32_t which, void *dst, int64_t capacity_bytes, int64_t *bytes_out);
int lowdeg_debug_floating_small(nodal_ctx *h, int64_t n, const int32_t *indptr, const int32_t *indices,
                                const uint8_t *grounded, int32_t *floating);

// ---- sparse solvers (sparse_*.hip) ----
// the multigrid FCG of the passive route with the caller's right-hand side (writes h->x): NODAL_OK, -1 the iteration
// broke down or hit its cap, -2 a floating island (singular); do_setup false re-uses the hierarchy of an earlier call
int amg_fcg_solve_rhs(nodal_ctx *h, const double *b, bool do_setup, int32_t *info, int32_t *iters, double *resid);
int sparse_solve(nodal_ctx *h, int32_t method, int32_t *info, int32_t *iters, double *resid);
int sparse_residual(nodal_ctx *h, double *scaled);
// |G x - b|_inf / (|G|_inf |x|_inf + |b|_inf) for any device vectors x, b with the context's CSR matrix; norms5 (host, may
// be null) receives the five words residual_kernel leaves
int csr_scaled_residual(nodal_ctx *h, const double *x, const double *b, double *scaled, double *norms5 = nullptr);
// the block judge of multi_rhs_solve (sparse.hip): scaled residuals of the `cols` (<= 16) columns of x against b, element
// (i, y) at [i * rs + y * cs], with m's CSR matrix on m's stream; norms (device): [16][4] maxima, then [16] scaled
// residuals.  Nothing is read back.
int csr_judge_block(nodal_ctx *m, const double *x, const double *b, int64_t rs, int64_t cs, int cols, double *norms);
// testing hook (nodal_debug_residual): the single-vector judge (cols 0) or the block judge (cols 1 .. 16) on host vectors
int sparse_debug_residual(nodal_ctx *h, bool transposed, int32_t cols, int32_t layout, const double *x, const double *b,
                          double *scaled_out, double *norms_out);
// testing hook (nodal_debug_direct_apply): slu_factor + one slu_apply (cols 1) or slu_apply_multi (cols 16) on host vectors
int sparse_debug_direct_apply(nodal_ctx *h, bool transposed, int32_t cols, const double *r, double *z,
                              int64_t *perturbed_out, int32_t *info_out);
// testing hook (nodal_debug_fgmres_cycle): the general route's setup and ONE restart cycle on host vectors, nothing behind
// it; (nodal_debug_general_array): what that setup left, raw (sparse_general.hip)
int general_debug_cycle(nodal_ctx *h, int32_t system, int32_t precond, int32_t window, int32_t max_cols, double rel_tol,
                        int64_t n_caller, const double *b_host, double *x_out, double *V_out, double *Z_out, double *gst_out, double *y_out,
                        double *norms_out, int64_t *params_out);
int general_debug_array(nodal_ctx *h, int32_t which, void *dst, int64_t capacity_bytes, int64_t *bytes_out);
// dense_child: solve the reduced system by the dense block elimination (only if it is passive)
void presolve_plan_ahead(nodal_ctx *h);  // host-only; called by stamp_numeric while its kernels run
void presolve_free_plan(nodal_ctx *h);
int presolve_solve(nodal_ctx *h, bool *done, int32_t *info, int32_t *iters, double *resid,
                   bool dense_child = false);
// testing hooks (nodal_debug_presolve_build / _array / _recover): plan, rewrite and reduced assembly as presolve_solve
// does them, what they left, and presolve_recover on the caller's y -- no solver, no acceptance test
int presolve_debug_build(nodal_ctx *h, int64_t *info);
int presolve_debug_array(nodal_ctx *h, int32_t which, void *dst, int64_t capacity_bytes, int64_t *bytes_out);
int presolve_debug_recover(nodal_ctx *h, int64_t ny, const double *y, double *x_out);
// ---- sparse direct route (sparse_direct.hip): multifrontal LU + FGMRES refinement ----
// tiny_factor scales (and signs) the value that replaces an unusable pivot
int slu_factor(nodal_ctx *h, int32_t *info, double tiny_factor = 1.0, double tiny_threshold = 0.0);
int slu_apply(nodal_ctx *h, const double *r, double *z);
int64_t slu_perturbed(nodal_ctx *h);  // pivots the last slu_factor replaced
constexpr int SLU_MULTI = 16;         // right-hand sides of slu_apply_multi (interleaved by row: element (i, c) at [i * 16 + c])
int slu_apply_multi(nodal_ctx *h, const double *r, double *z);
bool slu_analysis_kept(nodal_ctx *h); // an analysis for the context's present pattern is at hand (no host work to factor)
double slu_analysis_ms(nodal_ctx *h); // host milliseconds the last slu_factor spent on its analysis, 0.0 when it was kept
void slu_destroy(nodal_ctx *h);
void slu_poison(nodal_ctx *h);
int sparse_direct_solve(nodal_ctx *h, const double *b, double *x, int32_t *info, int32_t *iters, double *resid);
void nodal_free_buffers(nodal_ctx *h);  // api.hip
void nodal_poison_scratch(nodal_ctx *h);  // api.hip: NODAL_POISON=2, entry of every solve
// debugging (NODAL_NANCHECK=1): waits for the stream, copies n doubles to the host and reports on stderr how
// many are not finite and where the first one sits; a no-op otherwise
void nodal_nan_probe(nodal_ctx *h, const double *dev, int64_t n, const char *tag);  // api.hip
// The dense paths' two extra streams (one CU-masked) and their events, created on first use: a handle
// that only ever solves sparse systems holds ONE hardware queue, so that four of them in flight still
// get a queue each (the runtime multiplexes streams beyond its hardware queues: erratic throughput).
int nodal_ensure_aux_streams(nodal_ctx *h);  // api.hip
int nodal_calls_in_flight();  // host threads inside an API call right now, process-wide (api.hip)
int nodal_live_handles();     // handles alive in the process (api.hip)
bool nodal_extra_streams_ok(const nodal_ctx *h);  // NODAL_OPT_EXTRA_STREAMS is set and no other call is in flight (api.hip)
// NODAL_PINNED_BYTES of page-locked host memory of the handle (child contexts use their parent's): the
// destination of every read-back of a few words -- a copy to a stack variable is staged by the runtime
// through its own pinned buffer and costs 15-20 us more.  One API call at a time per handle, and every use is
// copy, wait, read: users need not coordinate.  Null if the allocation failed (callers fall back to the stack).
constexpr size_t NODAL_PINNED_BYTES = 4096;
void *nodal_pinned(nodal_ctx *h);  // api.hip
// At least `bytes` of page-locked host memory of the handle (child contexts: their parent's), grown on demand
// and kept: the staging area of host-built tables that go up in several pieces (a copy from a std::vector is
// staged by the runtime piece by piece, 30-60 us each).  The caller owns it until it has waited for its
// copies; contents do not survive a call that grows it.  Null if the allocation failed.
void *nodal_pinned_arena(nodal_ctx *h, size_t bytes);  // api.hip
// read `bytes` (<= NODAL_PINNED_BYTES) from the device into `dst` through the pinned scratch, and wait
int nodal_read_words(nodal_ctx *h, void *dst, const void *dev_src, size_t bytes);  // api.hip
void nodal_free_block_child(nodal_ctx *h);  // batch.hip
