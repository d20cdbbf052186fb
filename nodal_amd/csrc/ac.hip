// AC analysis: the steady state of an RLC network at each of a list of frequencies, one complex solve per frequency.
//
// Replaces a transient run per frequency, long enough to settle, and an amplitude fit afterwards -- or, on the host,
// exporting G, forming G + j B with scipy and one spsolve per frequency.
//
// G (n x n, n = K + B) is the matrix of the last numeric assembly.  A capacitor C between a and b has the susceptance
// b_C = w C, an inductor L the susceptance b_L = -1 / (w L); B(w) stamps every reactive element like a conductance of
// that value (+b at (a, a) and (b, b), -b at (a, b) and (b, a), ground leads dropped).  The phasors solve
//     (G + j B) (x_r + j x_i) = s_r + j s_i
// and are computed from the real system of twice the size, interleaved by unknown (real part of unknown i at 2i, imaginary
// part at 2i + 1): entry (i, j) is the 2 x 2 block [[g, -b], [b, g]].  That matrix lives on a csr_only child context,
// h->ac, after the pattern of h->adjoint: its pattern (the union of G's and the reactive elements' node pairs, every
// entry a full block) is built on the host once per struct_epoch and set of reactive leads, together with
//     ac_gsrc   per stored entry the place of G's value in h->data, -1 where the entry carries none
//     ac_ptr    per stored entry the run of reactive elements that add to it
//     ac_con    the runs: element << 1 | subtract, capacitors ascending, then inductors ascending
// so that a later call with the same structure and leads -- other values, frequencies, sources or probes -- repeats
// neither this nor the sparse LU's symbolic analysis.  The excitation is small-signal: every independent source is off
// but the ones the caller names, which carry a complex amplitude; the right-hand side is the existing source stamp of
// two members (real parts, imaginary parts) written interleaved, once per call.  A frequency is, on the handle's stream,
//     k_ac_values    one lane per stored entry: G's value or +0.0, then the entry's susceptances in list order, no atomics
//     the solve      transient_solver_begin / transient_solver_step on the child: the dense panel (2n <= 64, or `dense`
//                    at any size), else the sparse LU factored anew on the kept analysis, two substitutions, one
//                    refinement step, the judgement, and the sparse direct solve for a frequency above the bar
//     k_ac_probe     row f of the phasors
//     k_ac_current   row f of the element currents, j b_q (x(a) - x(b))
//     k_ac_peak      per node compare-and-update of |x|^2 with the frequency index (when asked for)
// and every keep_every-th frequency one device-to-device copy into a staging ring.  Phasors, currents, peaks and residuals
// come down once, after the last frequency.  The handle itself -- solution, table, G, A, tape, hierarchy, factors -- is
// only read.
//
// The noise analysis (noise.hip) solves with the transpose of the same matrix.  What it shares is exported from here:
// ac_child takes which child it builds -- h->ac from the handle's own pattern and values, or h->ac_t from those of
// h->adjoint, which holds G^T (B is symmetric, the stamps are the same) --, ac_child_values launches k_ac_values for
// either, and ac_check_arguments / ac_sources_check / ac_sources_stamp are the argument checks and the small-signal
// right-hand side.  ac_sweep.h declares these and what else the four small-signal analyses share: the upload of a call's
// reactive elements (ac_upload_spec, below) and the ledger of residuals and singular frequencies (AcLedger).
#include "ac_sweep.h"

namespace {

constexpr int ATB = 256;
constexpr int RING = 8;  // kept solutions staged on the device before they go down in one copy

// the susceptance of a reactive element at omega: kind 0 a capacitor (farads), 1 an inductor (henries)
__device__ __forceinline__ double susceptance(uint8_t kind, double value, double omega) {
    return kind == 0 ? omega * value : -1.0 / (omega * value);
}

// One lane per stored entry of the child: G's value (or +0.0), then +-b of the entry's elements in list order.
__global__ __launch_bounds__(ATB) void k_ac_values(int64_t nnz, double omega, const int32_t *__restrict__ gsrc,
                                                   const int32_t *__restrict__ cptr, const uint32_t *__restrict__ contrib,
                                                   const uint8_t *__restrict__ kind, const double *__restrict__ value,
                                                   const double *__restrict__ g, double *__restrict__ data) {
    const int64_t e = (int64_t)blockIdx.x * ATB + threadIdx.x;
    if (e >= nnz) return;
    const int32_t q = gsrc[e];
    double acc = q >= 0 ? g[q] : 0.0;
    for (int32_t p = cptr[e]; p < cptr[e + 1]; ++p) {
        const uint32_t u = contrib[p];
        const double b = susceptance(kind[u >> 1], value[u >> 1], omega);
        acc += (u & 1u) ? -b : b;
    }
    data[e] = acc;
}

// slot[row] = off for every independent source (A, E) the caller did not name: its value is the zero at swept[off]
__global__ __launch_bounds__(ATB) void k_ac_sources_off(int64_t ncomp, const uint8_t *__restrict__ type, int32_t off,
                                                        int32_t *__restrict__ slot) {
    const int64_t i = (int64_t)blockIdx.x * ATB + threadIdx.x;
    if (i >= ncomp) return;
    if ((type[i] == NODAL_T_A || type[i] == NODAL_T_E) && slot[i] < 0) slot[i] = off;
}

// the interleaved difference x(a) - x(b), +0.0 for a ground lead
__device__ __forceinline__ void lead_phasor(const double *__restrict__ x, int32_t a, int32_t b, double &re, double &im) {
    re = lead(x, a, 2, 0) - lead(x, b, 2, 0);
    im = lead(x, a, 2, 1) - lead(x, b, 2, 1);
}

// out[p] = x(a_p) - x(b_p) as (re, im); a probe between a node and itself reads +0.0 whatever x holds
__global__ __launch_bounds__(ATB) void k_ac_probe(int32_t nprobe, const int32_t *__restrict__ pa, const int32_t *__restrict__ pb,
                                                  const double *__restrict__ x, double2 *__restrict__ out) {
    const int32_t p = blockIdx.x * ATB + threadIdx.x;
    if (p >= nprobe) return;
    double re = 0.0, im = 0.0;
    if (pa[p] != pb[p]) lead_phasor(x, pa[p], pb[p], re, im);
    out[p] = make_double2(re, im);
}

// out[t] = j b_q (x(a) - x(b)), the current from lead a to lead b through reactive element q = index[t]
__global__ __launch_bounds__(ATB) void k_ac_current(int32_t ncur, double omega, const int32_t *__restrict__ index,
                                                    const uint8_t *__restrict__ kind, const double *__restrict__ value,
                                                    const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                    const double *__restrict__ x, double2 *__restrict__ out) {
    const int32_t t = blockIdx.x * ATB + threadIdx.x;
    if (t >= ncur) return;
    const int32_t q = index[t];
    const double bq = susceptance(kind[q], value[q], omega);
    double re, im;
    lead_phasor(x, a[q], b[q], re, im);
    out[t] = make_double2(-(bq * im), bq * re);
}

// per node: the largest |x|^2 so far and the frequency that attained it first (a strict comparison: among exact ties the
// lowest index stays).  first: no frequency has been taken in yet.
__global__ __launch_bounds__(ATB) void k_ac_peak(int32_t K, int32_t freq, int first, const double *__restrict__ x,
                                                 double *__restrict__ peak2, int32_t *__restrict__ peak_freq) {
    const int32_t i = blockIdx.x * ATB + threadIdx.x;
    if (i >= K) return;
    const double re = x[2 * (int64_t)i], im = x[2 * (int64_t)i + 1];
    const double m = re * re + im * im;
    if (first || m > peak2[i]) {
        peak2[i] = m;
        peak_freq[i] = freq;
    }
}
__global__ __launch_bounds__(ATB) void k_ac_peak_root(int32_t K, double *__restrict__ peak2) {
    const int32_t i = blockIdx.x * ATB + threadIdx.x;
    if (i < K) peak2[i] = sqrt(peak2[i]);
}

// Where a child keeps itself on the handle: h->ac, from h's own pattern and values, or h->ac_t, from those of h->adjoint.
struct AcSlot {
    nodal_ctx **child, *src;
    uint64_t *epoch;
    std::vector<int32_t> *key;
    DevBuf *gsrc, *ptr, *con;
};
AcSlot ac_slot(nodal_ctx *h, bool transposed) {
    if (transposed) return {&h->ac_t, h->adjoint, &h->ac_t_epoch, &h->ac_t_key, &h->ac_t_gsrc, &h->ac_t_ptr, &h->ac_t_con};
    return {&h->ac, h, &h->ac_epoch, &h->ac_key, &h->ac_gsrc, &h->ac_ptr, &h->ac_con};
}

void free_slot(nodal_ctx *h, bool transposed) {
    const AcSlot a = ac_slot(h, transposed);
    if (!*a.child) return;
    nodal_free_buffers(*a.child);
    delete *a.child;
    *a.child = nullptr;
    *a.epoch = 0;
    a.key->clear();
}

}  // namespace

// The child context with the interleaved real form: made once, its pattern and maps rebuilt when the parent's structure
// or the reactive leads move.  order: the reactive elements, capacitors ascending, then inductors ascending.
int ac_child(nodal_ctx *h, bool transposed, int64_t nreact, const uint8_t *kind, const int32_t *lead_a, const int32_t *lead_b,
             double *ms_pattern, nodal_ctx **child) {
    const AcSlot a = ac_slot(h, transposed);
    const int64_t n = h->n, nnz = h->nnz, n2 = 2 * n;
    hipStream_t st = h->stream;
    if (n2 >= (1ll << 31) - 2) return nodal_fail(h, NODAL_E_UNSUPPORTED, "ac sweep: more than 2^30 unknowns");
    if (!a.src || a.src->n != n || a.src->nnz != nnz) return nodal_fail(h, NODAL_E_INVALID, "ac sweep: no transposed matrix on the handle");
    if (!*a.child) *a.epoch = 0;
    nodal_ctx *c = csr_child(h, a.child);
    *child = c;
    c->K = (int32_t)n2;
    c->B = 0;
    std::vector<int32_t> key((size_t)3 * nreact);
    for (int64_t q = 0; q < nreact; ++q) {
        key[(size_t)q] = kind[q];
        key[(size_t)(nreact + q)] = lead_a[q];
        key[(size_t)(2 * nreact + q)] = lead_b[q];
    }
    if (*a.epoch == h->struct_epoch && c->n == n2 && key == *a.key) return NODAL_OK;

    const auto t0 = std::chrono::steady_clock::now();
    c->have_numeric = false;
    *a.epoch = 0;
    std::vector<int32_t> indptr((size_t)n + 1), indices((size_t)nnz);
    NODAL_HIP_TRY(h, hipMemcpyAsync(indptr.data(), a.src->indptr.p, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, st));
    if (nnz > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(indices.data(), a.src->indices.p, (size_t)nnz * 4, hipMemcpyDeviceToHost, st));
    NODAL_WAIT_STREAM(h, st);
    // the reactive stamps as (row, column, place in the list order, element, subtract), sorted
    struct Stamp {
        int32_t row, col, rank, elem, sub;
    };
    std::vector<Stamp> stamps;
    stamps.reserve((size_t)4 * nreact);
    {
        int32_t rank = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int64_t q = 0; q < nreact; ++q) {
                if (kind[q] != pass) continue;
                const int32_t a = lead_a[q], b = lead_b[q], e = (int32_t)q;
                if (a >= 0) stamps.push_back({a, a, rank, e, 0});
                if (b >= 0) stamps.push_back({b, b, rank, e, 0});
                if (a >= 0 && b >= 0) {
                    stamps.push_back({a, b, rank, e, 1});
                    stamps.push_back({b, a, rank, e, 1});
                }
                ++rank;
            }
    }
    std::sort(stamps.begin(), stamps.end(), [](const Stamp &l, const Stamp &r) {
        return l.row != r.row ? l.row < r.row : l.col != r.col ? l.col < r.col : l.rank < r.rank;
    });
    // per row of G the merge of its columns with the stamps' (both ascending); a block (i, j) becomes the entries
    // (2i, 2j) g, (2i, 2j + 1) -b, (2i + 1, 2j) b, (2i + 1, 2j + 1) g
    struct Block {
        int32_t col, gq, s0, s1;  // G's entry (-1: none), the stamps [s0, s1)
    };
    std::vector<Block> blocks;
    blocks.reserve((size_t)nnz + stamps.size());
    std::vector<int64_t> bptr((size_t)n + 1, 0);
    {
        size_t s = 0;
        for (int64_t i = 0; i < n; ++i) {
            int32_t q = indptr[i];
            const int32_t qe = indptr[i + 1];
            for (;;) {
                const bool more_g = q < qe, more_s = s < stamps.size() && stamps[s].row == i;
                if (!more_g && !more_s) break;
                if (more_g && (indices[q] < 0 || indices[q] >= n))
                    return nodal_fail(h, NODAL_E_INVALID, "ac sweep: a column index out of range");
                const int32_t col = more_g && (!more_s || indices[q] <= stamps[s].col) ? indices[q] : stamps[s].col;
                Block blk{col, -1, (int32_t)s, (int32_t)s};
                if (more_g && indices[q] == col) blk.gq = q++;
                while (s < stamps.size() && stamps[s].row == i && stamps[s].col == col) ++s;
                blk.s1 = (int32_t)s;
                blocks.push_back(blk);
            }
            bptr[(size_t)i + 1] = (int64_t)blocks.size();
        }
    }
    const int64_t nblk = (int64_t)blocks.size(), nnz2 = 4 * nblk;
    if (nnz2 >= (1ll << 31) - 2) return nodal_fail(h, NODAL_E_UNSUPPORTED, "ac sweep: more than 2^31 stored entries");
    std::vector<int32_t> cind((size_t)nnz2), crow((size_t)nnz2), gsrc((size_t)nnz2), cptr((size_t)nnz2 + 1), cindptr((size_t)n2 + 1),
        diag((size_t)n2, -1);
    std::vector<uint32_t> con;
    con.reserve(2 * stamps.size());
    {
        int64_t e = 0;
        for (int64_t i = 0; i < n; ++i)
            for (int half = 0; half < 2; ++half) {
                const int32_t row = (int32_t)(2 * i + half);
                cindptr[(size_t)row] = (int32_t)e;
                for (int64_t t = bptr[(size_t)i]; t < bptr[(size_t)i + 1]; ++t) {
                    const Block &blk = blocks[(size_t)t];
                    for (int part = 0; part < 2; ++part) {
                        const int32_t col = 2 * blk.col + part;
                        cind[(size_t)e] = col;
                        crow[(size_t)e] = row;
                        cptr[(size_t)e] = (int32_t)con.size();
                        if (part == half) {  // g
                            gsrc[(size_t)e] = blk.gq;
                        } else {  // -B above the diagonal of the block, +B below it
                            gsrc[(size_t)e] = -1;
                            for (int32_t s = blk.s0; s < blk.s1; ++s)
                                con.push_back((uint32_t)stamps[(size_t)s].elem << 1 | (uint32_t)(stamps[(size_t)s].sub ^ (half == 0 ? 1 : 0)));
                        }
                        if (col == row) diag[(size_t)row] = (int32_t)e;
                        ++e;
                    }
                }
            }
        cindptr[(size_t)n2] = (int32_t)e;
        cptr[(size_t)nnz2] = (int32_t)con.size();
    }
    NODAL_HIP_TRY(h, c->indptr.reserve((size_t)(n2 + 1) * 4 + 16));
    NODAL_HIP_TRY(h, c->indices.reserve((size_t)nnz2 * 4 + 16));
    NODAL_HIP_TRY(h, c->rowidx.reserve((size_t)nnz2 * 4 + 16));
    NODAL_HIP_TRY(h, c->diag_pos.reserve((size_t)n2 * 4 + 16));
    NODAL_HIP_TRY(h, c->data.reserve((size_t)nnz2 * 8 + 16));
    NODAL_HIP_TRY(h, c->rhs.reserve((size_t)n2 * 8 + 16));
    NODAL_HIP_TRY(h, c->x.reserve((size_t)n2 * 8 + 16));
    NODAL_HIP_TRY(h, a.gsrc->reserve((size_t)nnz2 * 4 + 16));
    NODAL_HIP_TRY(h, a.ptr->reserve((size_t)(nnz2 + 1) * 4 + 16));
    NODAL_HIP_TRY(h, a.con->reserve(con.size() * 4 + 16));
    NODAL_HIP_TRY(h, hipMemcpyAsync(c->indptr.p, cindptr.data(), (size_t)(n2 + 1) * 4, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(c->diag_pos.p, diag.data(), (size_t)n2 * 4, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(a.ptr->p, cptr.data(), (size_t)(nnz2 + 1) * 4, hipMemcpyHostToDevice, st));
    if (nnz2 > 0) {
        NODAL_HIP_TRY(h, hipMemcpyAsync(c->indices.p, cind.data(), (size_t)nnz2 * 4, hipMemcpyHostToDevice, st));
        NODAL_HIP_TRY(h, hipMemcpyAsync(c->rowidx.p, crow.data(), (size_t)nnz2 * 4, hipMemcpyHostToDevice, st));
        NODAL_HIP_TRY(h, hipMemcpyAsync(a.gsrc->p, gsrc.data(), (size_t)nnz2 * 4, hipMemcpyHostToDevice, st));
    }
    if (!con.empty()) NODAL_HIP_TRY(h, hipMemcpyAsync(a.con->p, con.data(), con.size() * 4, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemsetAsync(c->rhs.p, 0, (size_t)n2 * 8, st));
    NODAL_WAIT_STREAM(h, st);  // (the copies read vectors that end here)
    c->n = n2;
    c->nnz = nnz2;
    ++c->struct_epoch;  // whatever the child had cached about its own matrix is void
    *a.epoch = h->struct_epoch;
    a.key->swap(key);
    *ms_pattern = ms_since(t0);
    return NODAL_OK;
}

void ac_free_child(nodal_ctx *h) {
    free_slot(h, false);
    free_slot(h, true);
}

int ac_child_values(nodal_ctx *h, bool transposed, double omega, const uint8_t *kind_dev, const double *value_dev) {
    const AcSlot a = ac_slot(h, transposed);
    nodal_ctx *c = *a.child;
    if (c->nnz > 0) {
        k_ac_values<<<groups_of(c->nnz, ATB), ATB, 0, h->stream>>>(c->nnz, omega, a.gsrc->as<int32_t>(), a.ptr->as<int32_t>(),
                                                                  a.con->as<uint32_t>(), kind_dev, value_dev,
                                                                  a.src->data.as<double>(), c->data.as<double>());
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    ++c->numeric_epoch;
    c->have_numeric = true;
    return NODAL_OK;
}

int ac_check_arguments(nodal_ctx *h, const char *what, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
                       const double *value, const int32_t *lead_a, const int32_t *lead_b) {
    auto finite_positive = [](double v) { return v > 0.0 && v - v == 0.0; };
    auto fail = [&](const char *text) { return nodal_fail(h, NODAL_E_INVALID, (std::string(what) + text).c_str()); };
    for (int32_t f = 0; f < nfreq; ++f)
        if (!finite_positive(omega[f])) return fail("an angular frequency that is not finite and positive");
    for (int64_t q = 0; q < nreact; ++q) {
        if (kind[q] > 1) return fail("a reactive element's kind is neither 0 (capacitor) nor 1 (inductor)");
        if (!finite_positive(value[q])) return fail("a reactive element's value is not finite and positive");
        NODAL_TRY(ac_check_pairs(h, what, "a reactive element's lead", 1, lead_a + q, lead_b + q));
        if (lead_a[q] == lead_b[q]) return fail("both leads of a reactive element on one node");
    }
    return NODAL_OK;
}

int ac_check_pairs(nodal_ctx *h, const char *what, const char *noun, int64_t count, const int32_t *a, const int32_t *b) {
    const int32_t K = h->K;
    for (int64_t i = 0; i < count; ++i)
        if (a[i] < -1 || a[i] >= K || b[i] < -1 || b[i] >= K)
            return nodal_fail(h, NODAL_E_INVALID, (std::string(what) + noun + " out of range").c_str());
    return NODAL_OK;
}

int ac_upload_spec(nodal_ctx *h, int64_t nreact, const uint8_t *kind, const double *value, const int32_t *lead_a,
                   const int32_t *lead_b, std::initializer_list<AcIntList> lists, const double *extra, size_t nextra,
                   AcSpec *spec) {
    auto rounded = [](size_t words) { return (words + 15) & ~(size_t)15; };
    auto up = [&](void *to, const void *from, size_t bytes) {
        return bytes > 0 ? hipMemcpyAsync(to, from, bytes, hipMemcpyHostToDevice, h->stream) : hipSuccess;
    };
    const size_t rw = rounded((size_t)nreact), xw = rounded(nextra);
    size_t list_words = 0;
    for (const AcIntList &l : lists) list_words += rounded(l.second);
    NODAL_HIP_TRY(h, h->ac_spec.reserve((rw + xw) * 8 + ((lead_a ? 2 * rw : 0) + list_words) * 4 + rw + 64));
    spec->value = h->ac_spec.as<double>();
    spec->extra = spec->value + rw;
    int32_t *at = reinterpret_cast<int32_t *>(spec->extra + xw);
    NODAL_HIP_TRY(h, up(spec->value, value, (size_t)nreact * 8));
    if (lead_a) {
        spec->lead_a = at;
        spec->lead_b = at + rw;
        at += 2 * rw;
        NODAL_HIP_TRY(h, up(spec->lead_a, lead_a, (size_t)nreact * 4));
        NODAL_HIP_TRY(h, up(spec->lead_b, lead_b, (size_t)nreact * 4));
    }
    spec->kind = reinterpret_cast<uint8_t *>(at + list_words);
    NODAL_HIP_TRY(h, up(spec->kind, kind, (size_t)nreact));
    NODAL_HIP_TRY(h, up(spec->extra, extra, nextra * 8));
    int k = 0;
    for (const AcIntList &l : lists) {
        spec->list[k++] = at;
        NODAL_HIP_TRY(h, up(at, l.first, l.second * 4));
        at += rounded(l.second);
    }
    return NODAL_OK;
}

int ac_peak_root(nodal_ctx *h, int32_t K, double *peak2) {
    k_ac_peak_root<<<groups_of(K, ATB), ATB, 0, h->stream>>>(K, peak2);
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

// the swept rows: the named sources' real parts, a zero, their imaginary parts, a zero -- two members of nsrc + 1 values,
// the extra one for every source that is not named (k_ac_sources_off)
int ac_sources_check(nodal_ctx *h, const char *what, const char *row, int32_t nsrc, const int64_t *src_rows, const double *src_re,
                     const double *src_im) {
    hipStream_t st = h->stream;
    NODAL_HIP_TRY(h, h->sw_rows.reserve((size_t)(nsrc + 16) * 4));
    NODAL_HIP_TRY(h, h->sw_slot.reserve((size_t)h->ncomp * 4 + 64));
    NODAL_HIP_TRY(h, h->sw_vals.reserve((size_t)2 * (nsrc + 1) * 8 + 64));
    std::vector<double> amplitudes((size_t)2 * (nsrc + 1), 0.0);
    for (int32_t j = 0; j < nsrc; ++j) {
        amplitudes[(size_t)j] = src_re[j];
        amplitudes[(size_t)(nsrc + 1 + j)] = src_im[j];
    }
    NODAL_HIP_TRY(h, hipMemcpyAsync(h->sw_vals.p, amplitudes.data(), amplitudes.size() * 8, hipMemcpyHostToDevice, st));
    int32_t *rows_dev = h->sw_rows.as<int32_t>(), *slot_dev = h->sw_slot.as<int32_t>();
    return sweep_check_rows(h, what, row, nsrc, src_rows, rows_dev, slot_dev, rows_dev + ((nsrc + 15) & ~15));  // (waits)
}

// the right-hand side does not depend on omega: members (re, im) of the source stamp, element (row, y) at [2 row + y]
int ac_sources_stamp(nodal_ctx *h, int32_t nsrc, double *bvec) {
    hipStream_t st = h->stream;
    int32_t *slot_dev = h->sw_slot.as<int32_t>();
    if (h->ncomp > 0) {
        k_ac_sources_off<<<groups_of(h->ncomp, ATB), ATB, 0, st>>>(h->ncomp, h->type.as<uint8_t>(), nsrc, slot_dev);
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    NODAL_HIP_TRY(h, hipMemsetAsync(bvec, 0, (size_t)2 * h->n * 8, st));
    return stamp_rhs_multi(h, slot_dev, h->sw_vals.as<double>(), nsrc + 1, 2, bvec, 2, 1);
}

int ac_run(nodal_ctx *h, bool dense, int32_t nfreq, const double *omega, int64_t nreact, const uint8_t *kind,
           const double *value, const int32_t *lead_a, const int32_t *lead_b, int32_t nsrc, const int64_t *src_rows,
           const double *src_re, const double *src_im, int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b,
           double *wave_out, int32_t ncur, const int32_t *cur_index, double *cur_out, int32_t keep_every, double *x_out,
           double *peak_out, int32_t *peak_freq_out, double *resid_out, int32_t *info_out, double *ms_analysis,
           double *ms_factor) {
    const int64_t n = h->n, n2 = 2 * n;
    const int32_t K = h->K;
    hipStream_t st = h->stream;
    const double nan = __builtin_nan("");
    *ms_analysis = *ms_factor = 0.0;

    // ---- the arguments ----
    NODAL_TRY(ac_check_arguments(h, "ac sweep: ", nfreq, omega, nreact, kind, value, lead_a, lead_b));
    NODAL_TRY(ac_check_pairs(h, "ac sweep: ", "probe node", nprobe, probe_a, probe_b));
    for (int32_t t = 0; t < ncur; ++t)
        if (cur_index[t] < 0 || cur_index[t] >= nreact)
            return nodal_fail(h, NODAL_E_INVALID, "ac sweep: current probe outside the reactive elements");
    NODAL_TRY(ac_sources_check(h, "ac sweep: ", "source row", nsrc, src_rows, src_re, src_im));
    if (nfreq == 0) return NODAL_OK;

    const int32_t nkeep = (keep_every > 0 && x_out) ? nfreq / keep_every : 0;
    AcLedger ledger(h, nfreq, 1, resid_out, info_out);
    const size_t wave_words = (size_t)nfreq * nprobe * 2, cur_words = (size_t)nfreq * ncur * 2;
    if (n == 0) {  // (no unknowns: every lead is ground, nothing is driven)
        if (wave_out)
            for (size_t t = 0; t < wave_words; ++t) wave_out[t] = 0.0;
        return NODAL_OK;
    }
    const bool want_peak = (peak_out || peak_freq_out) && K > 0;

    // ---- once per call: the child's pattern, the elements and probes up, the right-hand side, the buffers ----
    nodal_ctx *c = nullptr;
    NODAL_TRY(ac_child(h, false, nreact, kind, lead_a, lead_b, ms_analysis, &c));
    AcSpec spec;  // the elements with their leads; lists: the probed elements, probe a, probe b
    NODAL_TRY(ac_upload_spec(h, nreact, kind, value, lead_a, lead_b,
                             {{cur_index, (size_t)ncur}, {probe_a, (size_t)nprobe}, {probe_b, (size_t)nprobe}}, nullptr, 0, &spec));
    // ac_vec: right-hand side | solution | defect | correction (2n each) | the judge's norms
    NODAL_HIP_TRY(h, h->ac_vec.reserve((size_t)4 * n2 * 8 + 5 * SLU_MULTI * 8 + 256));
    double *bvec = h->ac_vec.as<double>(), *xk = bvec + n2, *rvec = xk + n2, *dvec = rvec + n2, *norms = dvec + n2;
    // ac_out: phasors [nfreq][nprobe][2] | currents [nfreq][ncur][2] | residuals [nfreq] | peaks |x|^2 [K] | their frequencies [K]
    const size_t peak_words = want_peak ? (size_t)K : 0;
    NODAL_HIP_TRY(h, h->ac_out.reserve((wave_words + cur_words + (size_t)nfreq + 2 * peak_words + 2) * 8 + 64));
    double *wave_dev = h->ac_out.as<double>(), *cur_dev = wave_dev + wave_words, *resid_dev = cur_dev + cur_words,
           *peak_dev = resid_dev + nfreq;
    ledger.resid_dev = resid_dev;
    int32_t *peak_freq_dev = reinterpret_cast<int32_t *>(peak_dev + peak_words);
    if (want_peak) NODAL_HIP_TRY(h, hipMemsetAsync(peak_dev, 0xFF, peak_words * 12, st));  // (NaN and -1 until a frequency is taken in)
    double *ring = nullptr;
    if (nkeep > 0) {
        NODAL_HIP_TRY(h, h->ac_ring.reserve((size_t)std::min<int32_t>(RING, nkeep) * n2 * 8 + 64));
        ring = h->ac_ring.as<double>();
    }
    NODAL_TRY(ac_sources_stamp(h, nsrc, bvec));
    NODAL_WAIT_STREAM(h, st);  // (the elements and probes are the caller's)

    // ---- the frequencies ----
    uint64_t lu_epoch = 0;  // (never the child's numeric_epoch: every frequency is factored anew)
    bool peak_first = true;
    int32_t ring_fill = 0, ring_base = 0;  // kept solutions in the ring, and the index of the first of them
    auto flush_ring = [&]() -> int {
        if (ring_fill == 0) return NODAL_OK;
        NODAL_HIP_TRY(h, hipMemcpyAsync(x_out + (int64_t)ring_base * n2, ring, (size_t)ring_fill * n2 * 8, hipMemcpyDeviceToHost, st));
        NODAL_WAIT_STREAM(h, st);  // (the ring is written again by the frequencies that follow)
        ring_base += ring_fill;
        ring_fill = 0;
        return NODAL_OK;
    };
    for (int32_t f = 0; f < nfreq; ++f) {
        const double w = omega[f];
        NODAL_TRY(ac_child_values(h, false, w, spec.kind, spec.value));
        // the solve, on the child as both handle and solve context: every size read is 2n
        TransientSolver ts;
        ts.s = c;
        ts.lu_epoch = &lu_epoch;
        ts.rvec = rvec;
        ts.dvec = dvec;
        ts.norms = norms;
        ts.force_dense = dense;
        bool dead = false, judged = false;
        double ms_f = 0.0;
        int32_t inf = 0, it = 0;
        NODAL_TRY(nodal_lift_error(h, c, transient_solver_begin(c, ts, dense, 1, &dead, &ms_f)));
        if (ts.route == TR_ROUTE_LU) ac_add_factor_time(c, ms_f, ms_analysis, ms_factor);
        if (!dead) {
            double ms_none = 0.0;
            NODAL_TRY(nodal_lift_error(h, c, transient_solver_step(c, ts, bvec, xk, &inf, &it, &ledger.resid[f], &judged, &ms_none)));
            if (inf > 0 && dense) return nodal_fail(h, NODAL_E_SINGULAR, "singular matrix: a zero pivot or a floating sub-network");
        }
        const bool kept = nkeep > 0 && (f + 1) % keep_every == 0;
        if (dead || inf > 0) {
            ledger.mark_dead(f);
            if (kept) {
                NODAL_TRY(nodal_lift_error(h, c, dense_fill_nan(c, ring + (size_t)ring_fill * n2, n2)));
                if (++ring_fill == std::min<int32_t>(RING, nkeep)) NODAL_TRY(flush_ring());
            }
            continue;
        }
        ledger.on_host[(size_t)f] = judged;
        if (!judged) NODAL_HIP_TRY(h, hipMemcpyAsync(resid_dev + f, norms + 4 * SLU_MULTI, 8, hipMemcpyDeviceToDevice, st));
        // what the caller asked for of x(omega)
        if (nprobe > 0)
            k_ac_probe<<<groups_of(nprobe, ATB), ATB, 0, st>>>(nprobe, spec.list[1], spec.list[2], xk,
                                                              reinterpret_cast<double2 *>(wave_dev) + (size_t)f * nprobe);
        if (ncur > 0)
            k_ac_current<<<groups_of(ncur, ATB), ATB, 0, st>>>(ncur, w, spec.list[0], spec.kind, spec.value, spec.lead_a, spec.lead_b, xk,
                                                              reinterpret_cast<double2 *>(cur_dev) + (size_t)f * ncur);
        if (want_peak) {
            k_ac_peak<<<groups_of(K, ATB), ATB, 0, st>>>(K, f, peak_first ? 1 : 0, xk, peak_dev, peak_freq_dev);
            peak_first = false;
        }
        NODAL_HIP_TRY(h, hipGetLastError());
        if (kept) {
            NODAL_HIP_TRY(h, hipMemcpyAsync(ring + (size_t)ring_fill * n2, xk, (size_t)n2 * 8, hipMemcpyDeviceToDevice, st));
            if (++ring_fill == std::min<int32_t>(RING, nkeep)) NODAL_TRY(flush_ring());
        }
    }
    NODAL_TRY(flush_ring());

    // ---- after the last frequency: everything else comes down once ----
    if (want_peak && !peak_first) NODAL_TRY(ac_peak_root(h, K, peak_dev));
    if (wave_out && wave_words > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(wave_out, wave_dev, wave_words * 8, hipMemcpyDeviceToHost, st));
    if (cur_out && cur_words > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(cur_out, cur_dev, cur_words * 8, hipMemcpyDeviceToHost, st));
    if (want_peak) {
        if (peak_out) NODAL_HIP_TRY(h, hipMemcpyAsync(peak_out, peak_dev, (size_t)K * 8, hipMemcpyDeviceToHost, st));
        if (peak_freq_out) NODAL_HIP_TRY(h, hipMemcpyAsync(peak_freq_out, peak_freq_dev, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    }
    return ledger.finish([&](int32_t f) {
        if (wave_out) std::fill_n(wave_out + (size_t)f * nprobe * 2, 2 * (size_t)nprobe, nan);
        if (cur_out) std::fill_n(cur_out + (size_t)f * ncur * 2, 2 * (size_t)ncur, nan);
    });
}
