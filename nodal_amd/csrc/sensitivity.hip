// Adjoint sensitivities: the derivative of chosen outputs with respect to the value of EVERY component.
//
// Replaces a finite-difference loop of Circuit(netlist with one value nudged) + .solve() (reference
// nodal/nodal.py:306-336), two solves per component; the reference itself has nothing of the kind.
//
// The assembled system is G(p) x = A(p), p = the value column the last numeric assembly used.  An output is y = c^T x
// (plus, for the current of a resistor, its explicit dependence on that resistor's value).  With G^T lambda = c:
//     dy/dp_i = lambda^T (dA/dp_i - dG/dp_i x) + dy/dp_i|explicit
// Per table row i of value v, X(j) / L(j) = x[j] / lambda[j] with +0.0 for the ground lead, m = K + k_i,
// Rd = value[drv_i] (1 without a driver), from the stamps of stamp.hip:
//     R          (L(a) - L(b)) (X(a) - X(b)) / v^2, plus for every CCVS / CCCS row j driven by it
//                L(m_j) v_j (X(c_j) - X(d_j)) / v^2                     (k_sensitivity_cross)
//     A          L(a) - L(b)
//     E          L(m)
//     VCVS       L(m) (X(c) - X(d))                                      (VCCS rows carry this type)
//     CCVS, CCCS -L(m) (X(c) - X(d)) / Rd
// i.e. always D * w with D = L(a) - L(b) or L(m), and w a factor of the row alone: k_sensitivity_block forms w once per
// row and then walks the sixteen columns of the block.  No floating-point atomics: the cross terms of a resistor are
// added by one thread in table order, so a repeated call returns the same bits.
//
// The transposed solves are multi_rhs_solve (sparse.hip) with the AdjointClient below.  A passive network solves on the
// handle itself; any other gets a child context that holds G^T as CSR: its pattern is transposed on the host by a stable
// counting sort
// over the columns (rows come out with sorted columns, and the same input gives the same pattern), once per
// struct_epoch of the parent, and its values are gathered from the parent's `data` through the kept permutation on
// every call.
#include "table_rows.h"

#include <algorithm>

namespace {

constexpr int STB = 256;
constexpr int SCOLS = 16;  // outputs per launch of the table kernels (SLU_MULTI)

// ---- the outputs: check, value, right-hand side ----------------------------------------------------------------
// One thread per output q: value[q] = c^T x; *bad |= 1 for the current of a row that has none of its own to
// differentiate (a current source: the current IS the value; an internal row without a branch).
__global__ __launch_bounds__(STB) void k_sens_values(int32_t count, int32_t K, const int32_t *__restrict__ kind,
                                                     const int32_t *__restrict__ p, const int32_t *__restrict__ q2,
                                                     const uint8_t *__restrict__ type, const double *__restrict__ value,
                                                     const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                     const int32_t *__restrict__ k, const double *__restrict__ x,
                                                     double *__restrict__ out, int32_t *__restrict__ bad) {
    const int32_t q = blockIdx.x * STB + threadIdx.x;
    if (q >= count) return;
    double y = 0.0;
    if (kind[q] == 0) {
        y = lead(x, p[q]) - lead(x, q2[q]);
    } else {
        const int32_t i = p[q];
        const int t = type[i];
        if (t == NODAL_T_R) {
            const double v = lead(x, a[i]) - lead(x, b[i]);
            y = v / value[i];  // (as nodal_branches reports it)
        } else if (t != NODAL_T_A && k[i] >= 0) {
            y = x[(int64_t)K + k[i]];
        } else {
            atomicOr(bad, 1);
        }
    }
    out[q] = y;
}

// One thread per column y < cols of a zeroed block, element (row, y) at out[row * rs + y * cs]: the <= 2 entries of c.
__global__ __launch_bounds__(64) void k_sens_rhs(int cols, int32_t K, const int32_t *__restrict__ kind,
                                                 const int32_t *__restrict__ p, const int32_t *__restrict__ q2,
                                                 const uint8_t *__restrict__ type, const double *__restrict__ value,
                                                 const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                 const int32_t *__restrict__ k, double *__restrict__ out, int64_t rs,
                                                 int64_t cs) {
    const int y = threadIdx.x;
    if (y >= cols) return;
    double *col = out + (int64_t)y * cs;
    if (kind[y] == 0) {
        if (p[y] >= 0) col[(int64_t)p[y] * rs] += 1.0;
        if (q2[y] >= 0) col[(int64_t)q2[y] * rs] -= 1.0;
        return;
    }
    const int32_t i = p[y];
    if (type[i] == NODAL_T_R) {
        const double g = 1.0 / value[i];
        if (a[i] >= 0) col[(int64_t)a[i] * rs] += g;
        if (b[i] >= 0) col[(int64_t)b[i] * rs] -= g;
    } else if (k[i] >= 0) {
        col[((int64_t)K + k[i]) * rs] += 1.0;
    }
}

// ---- the table kernel ------------------------------------------------------------------------------------------
// the rows whose own current is the output of column y (-1: none): they get the explicit term -y / v
struct ExplicitRows { int32_t row[SCOLS]; };

// One thread per table row for the whole block: the row's record and its X(.) are loaded once, then the columns.
// IL: lam is interleaved by row, element (j, y) at lam[j * 16 + y] -- the sixteen L(j) of a lead are one 128-byte
// line, fetched as eight 16-byte loads; otherwise element (j, y) at lam[j * rs + y * cs].  sens[y * ncomp + i]:
// consecutive threads write consecutive doubles.
template <bool IL>
__global__ __launch_bounds__(STB) void k_sensitivity_block(int64_t ncomp, int32_t K, int cols,
                                                           const uint8_t *__restrict__ type,
                                                           const double *__restrict__ value,
                                                           const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                           const int32_t *__restrict__ c, const int32_t *__restrict__ d,
                                                           const int32_t *__restrict__ drv, const int32_t *__restrict__ k,
                                                           const double *__restrict__ x, const double *__restrict__ lam,
                                                           int64_t rs, int64_t cs, ExplicitRows ex,
                                                           double *__restrict__ sens) {
    const int64_t i = (int64_t)blockIdx.x * STB + threadIdx.x;
    if (i >= ncomp) return;
    // D = L(j1) - L(j2); w: the row's own factor, 0 for a row without a term; expl: a resistor's explicit term
    const RowTerm r = row_term(i, K, type, value, a, b, c, d, drv, k);
    const int32_t j1 = r.j1, j2 = r.j2;
    const bool mine = type[i] == NODAL_T_R;
    double w = r.none ? 0.0 : 1.0, expl = 0.0;
    if (r.reads_x) {
        const double u = lead(x, r.p1) - lead(x, r.p2);
        w = u / r.den;
        if (mine) {
            const double v = value[i];
            expl = -(u / v) / v;
        }
    }
    if constexpr (IL) {
        double D[SCOLS];
        const double2 *l1 = reinterpret_cast<const double2 *>(lam + (int64_t)(j1 < 0 ? 0 : j1) * SCOLS);
        const double2 *l2 = reinterpret_cast<const double2 *>(lam + (int64_t)(j2 < 0 ? 0 : j2) * SCOLS);
#pragma unroll
        for (int y = 0; y < SCOLS; y += 2) {
            double2 p1 = make_double2(0.0, 0.0), p2 = make_double2(0.0, 0.0);
            if (j1 >= 0) p1 = l1[y >> 1];
            if (j2 >= 0) p2 = l2[y >> 1];
            D[y] = p1.x - p2.x;
            D[y + 1] = p1.y - p2.y;
        }
#pragma unroll
        for (int y = 0; y < SCOLS; ++y) {
            if (y >= cols) break;
            double s = D[y] * w;
            if (mine && ex.row[y] == i) s += expl;
            sens[(int64_t)y * ncomp + i] = s;
        }
    } else {
        // (the dense panel's columns, a column solved alone: no line to share, the columns one after the other)
#pragma unroll 2
        for (int y = 0; y < cols; ++y) {
            const double p1 = j1 >= 0 ? lam[(int64_t)j1 * rs + (int64_t)y * cs] : 0.0;
            const double p2 = j2 >= 0 ? lam[(int64_t)j2 * rs + (int64_t)y * cs] : 0.0;
            double s = (p1 - p2) * w;
            if (mine && ex.row[y] == i) s += expl;
            sens[(int64_t)y * ncomp + i] = s;
        }
    }
}

// The cross terms of the resistors that drive CCVS / CCCS rows.  One thread per (distinct driver g, column y): the rows
// of its group rows[gptr[g] .. gptr[g + 1]) are added in table order onto what k_sensitivity_block left at the driver.
__global__ __launch_bounds__(STB) void k_sensitivity_cross(int64_t ndrivers, int64_t ncomp, int32_t K, int cols,
                                                           const int32_t *__restrict__ drivers,
                                                           const int32_t *__restrict__ gptr,
                                                           const int32_t *__restrict__ rows,
                                                           const uint8_t *__restrict__ type,
                                                           const double *__restrict__ value,
                                                           const int32_t *__restrict__ c, const int32_t *__restrict__ d,
                                                           const int32_t *__restrict__ k, const double *__restrict__ x,
                                                           const double *__restrict__ lam, int64_t rs, int64_t cs,
                                                           double *__restrict__ sens) {
    const int64_t t = (int64_t)blockIdx.x * STB + threadIdx.x;
    const int64_t g = t / SCOLS;
    const int y = (int)(t % SCOLS);
    if (g >= ndrivers || y >= cols) return;
    const int32_t i = drivers[g];
    if (type[i] != NODAL_T_R) return;  // (the front end admits no other driver; another one has no term)
    const double v = value[i];
    double acc = sens[(int64_t)y * ncomp + i];
    for (int32_t q = gptr[g]; q < gptr[g + 1]; ++q) {
        const double term = cross_term(rows[q], K, v, value, c, d, k, lam, rs, (int64_t)y * cs, x, 1, 0);
        acc += term;
    }
    sens[(int64_t)y * ncomp + i] = acc;
}

// child values: data_t[q] = data[perm[q]]
__global__ __launch_bounds__(STB) void k_gather_values(int64_t nnz, const int32_t *__restrict__ perm,
                                                       const double *__restrict__ data, double *__restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * STB + threadIdx.x;
    if (q < nnz) out[q] = data[perm[q]];
}

}  // namespace

// The CCVS / CCCS rows grouped by their driver, in table order inside a group, groups by driver row: kept on the
// device per table_epoch as [drivers (nd) | gptr (nd + 1) | rows (nc)].
int sens_cross_list(nodal_ctx *h) {
    if (h->sn_cross_epoch == h->table_epoch) return NODAL_OK;
    h->sn_ndrivers = h->sn_ncross = 0;
    const int64_t ncomp = h->ncomp;
    if (h->B > 0 && ncomp > 0) {
        // the host's view of the table when the handle keeps one, else the two columns come down
        std::vector<uint8_t> type_own;
        std::vector<int32_t> drv_own;
        const uint8_t *type = nullptr;
        const int32_t *drv = nullptr;
        const std::vector<int64_t> *branch_rows = nullptr;
        if (h->host.type.size() == (size_t)ncomp && h->host.drv.size() == (size_t)ncomp) {
            type = h->host.type.data();
            drv = h->host.drv.data();
            branch_rows = &h->host.branch_rows;
        } else {
            type_own.resize((size_t)ncomp);
            drv_own.resize((size_t)ncomp);
            NODAL_HIP_TRY(h, hipMemcpyAsync(type_own.data(), h->type.p, (size_t)ncomp, hipMemcpyDeviceToHost, h->stream));
            NODAL_HIP_TRY(h, hipMemcpyAsync(drv_own.data(), h->drv.p, (size_t)ncomp * 4, hipMemcpyDeviceToHost, h->stream));
            NODAL_WAIT_STREAM(h, h->stream);
            type = type_own.data();
            drv = drv_own.data();
        }
        std::vector<std::pair<int32_t, int32_t>> found;  // (driver, row)
        auto look = [&](int64_t i) {
            if ((type[i] == NODAL_T_CCVS || type[i] == NODAL_T_CCCS) && drv[i] >= 0 && drv[i] < ncomp)
                found.emplace_back(drv[i], (int32_t)i);
        };
        if (branch_rows)
            for (const int64_t i : *branch_rows) look(i);
        else
            for (int64_t i = 0; i < ncomp; ++i) look(i);
        std::stable_sort(found.begin(), found.end(),
                         [](const std::pair<int32_t, int32_t> &l, const std::pair<int32_t, int32_t> &r) {
                             return l.first != r.first ? l.first < r.first : l.second < r.second;
                         });
        std::vector<int32_t> drivers, gptr, rows;
        for (const auto &f : found) {
            if (drivers.empty() || drivers.back() != f.first) {
                drivers.push_back(f.first);
                gptr.push_back((int32_t)rows.size());
            }
            rows.push_back(f.second);
        }
        gptr.push_back((int32_t)rows.size());
        const size_t nd = drivers.size(), nc = rows.size();
        if (nc > 0) {
            std::vector<int32_t> packed;
            packed.reserve(2 * nd + 1 + nc);
            packed.insert(packed.end(), drivers.begin(), drivers.end());
            packed.insert(packed.end(), gptr.begin(), gptr.end());
            packed.insert(packed.end(), rows.begin(), rows.end());
            NODAL_HIP_TRY(h, h->sn_cross.reserve(packed.size() * 4 + 64));
            NODAL_HIP_TRY(h, hipMemcpyAsync(h->sn_cross.p, packed.data(), packed.size() * 4, hipMemcpyHostToDevice, h->stream));
            NODAL_WAIT_STREAM(h, h->stream);  // (the copy reads a vector that ends here)
            h->sn_ndrivers = (int64_t)nd;
            h->sn_ncross = (int64_t)nc;
        }
    }
    h->sn_cross_epoch = h->table_epoch;
    return NODAL_OK;
}

// A csr_only child context of h in *slot -- a matrix that no netlist stamped: G^T here, the AC analysis' doubled system in
// ac.hip -- made on first use, on h's streams, its solver options brought up to h's on every call.
nodal_ctx *csr_child(nodal_ctx *h, nodal_ctx **slot) {
    if (!*slot) {
        nodal_ctx *c = new nodal_ctx();
        c->device = h->device;
        c->stream = h->stream;  // shared: one ordered timeline
        c->stream2 = h->stream2;
        c->stream3 = h->stream3;
        for (int i = 0; i < 4; ++i) c->ev[i] = h->ev[i];
        for (int i = 0; i < 2; ++i) c->ev_la[i] = h->ev_la[i];
        for (int i = 0; i < 6; ++i) c->ev_bi[i] = h->ev_bi[i];
        c->owns_streams = false;
        c->stream_owner = h->stream_owner ? h->stream_owner : h;
        c->keep_host_table = false;
        c->csr_only = true;
        c->use_presolve = false;
        *slot = c;
    }
    nodal_ctx *c = *slot;
    // (not passive, never optimistic: the dense LU of the child pivots)
    c->passive_network = false;
    c->optimistic_nopivot = false;
    c->dense_blockinv = h->dense_blockinv;
    c->gj_scalar = h->gj_scalar;
    c->gepp_panel = h->gepp_panel;
    c->force_pivoting = h->force_pivoting;
    c->use_graphs = h->use_graphs;
    c->amg_min_n = h->amg_min_n;
    c->have_x = false;
    return c;
}

// The child context with G^T: made once, its pattern rebuilt when the parent's moves, its values gathered every call.
int sens_transposed_child(nodal_ctx *h) {
    const int64_t n = h->n, nnz = h->nnz;
    hipStream_t st = h->stream;
    if (!h->adjoint) h->adjoint_epoch = 0;
    nodal_ctx *c = csr_child(h, &h->adjoint);
    c->K = h->K;
    c->B = h->B;
    if (h->adjoint_epoch != h->struct_epoch || c->n != n || c->nnz != nnz) {
        c->have_numeric = false;
        std::vector<int32_t> indptr((size_t)n + 1), indices((size_t)nnz);
        NODAL_HIP_TRY(h, hipMemcpyAsync(indptr.data(), h->indptr.p, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, st));
        if (nnz > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(indices.data(), h->indices.p, (size_t)nnz * 4, hipMemcpyDeviceToHost, st));
        NODAL_WAIT_STREAM(h, st);
        // stable counting sort of the entries by column: entry q = (i, j) of G becomes entry (j, i) of G^T, and inside
        // a row of G^T the columns i come out ascending because the rows of G are walked in order
        std::vector<int32_t> tptr((size_t)n + 1, 0), tind((size_t)nnz), trow((size_t)nnz), perm((size_t)nnz), diag((size_t)n, -1);
        for (int64_t q = 0; q < nnz; ++q) {
            if (indices[q] < 0 || indices[q] >= n) return nodal_fail(h, NODAL_E_INVALID, "sensitivities: a column index out of range");
            ++tptr[(size_t)indices[q] + 1];
        }
        for (int64_t j = 0; j < n; ++j) tptr[j + 1] += tptr[j];
        {
            std::vector<int32_t> next(tptr.begin(), tptr.end() - 1);
            for (int64_t i = 0; i < n; ++i)
                for (int32_t q = indptr[i]; q < indptr[i + 1]; ++q) {
                    const int32_t j = indices[q], at = next[j]++;
                    tind[at] = (int32_t)i;
                    trow[at] = j;
                    perm[at] = q;
                    if (i == j) diag[j] = at;
                }
        }
        NODAL_HIP_TRY(h, c->indptr.reserve((size_t)(n + 1) * 4 + 16));
        NODAL_HIP_TRY(h, c->indices.reserve((size_t)nnz * 4 + 16));
        NODAL_HIP_TRY(h, c->rowidx.reserve((size_t)nnz * 4 + 16));
        NODAL_HIP_TRY(h, c->diag_pos.reserve((size_t)n * 4 + 16));
        NODAL_HIP_TRY(h, h->sn_perm.reserve((size_t)nnz * 4 + 16));
        NODAL_HIP_TRY(h, c->data.reserve((size_t)nnz * 8 + 16));
        NODAL_HIP_TRY(h, c->rhs.reserve((size_t)n * 8 + 16));
        NODAL_HIP_TRY(h, c->x.reserve((size_t)n * 8 + 16));
        NODAL_HIP_TRY(h, hipMemcpyAsync(c->indptr.p, tptr.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice, st));
        if (n > 0) NODAL_HIP_TRY(h, hipMemcpyAsync(c->diag_pos.p, diag.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        if (nnz > 0) {
            NODAL_HIP_TRY(h, hipMemcpyAsync(c->indices.p, tind.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, st));
            NODAL_HIP_TRY(h, hipMemcpyAsync(c->rowidx.p, trow.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, st));
            NODAL_HIP_TRY(h, hipMemcpyAsync(h->sn_perm.p, perm.data(), (size_t)nnz * 4, hipMemcpyHostToDevice, st));
        }
        NODAL_HIP_TRY(h, hipMemsetAsync(c->rhs.p, 0, (size_t)n * 8, st));
        NODAL_WAIT_STREAM(h, st);  // (the copies read vectors that end here)
        c->n = n;
        c->nnz = nnz;
        ++c->struct_epoch;  // whatever the child had cached about its own matrix is void
        h->adjoint_epoch = h->struct_epoch;
    }
    if (nnz > 0) {
        k_gather_values<<<groups_of(nnz, STB), STB, 0, st>>>(nnz, h->sn_perm.as<int32_t>(), h->data.as<double>(),
                                                             c->data.as<double>());
        NODAL_HIP_TRY(h, hipGetLastError());
    }
    c->have_numeric = true;
    return NODAL_OK;
}

int adjoint_context(nodal_ctx *h, nodal_ctx **s) {
    *s = h;
    if (h->B == 0 && h->passive_network) return NODAL_OK;
    NODAL_TRY(sens_transposed_child(h));
    *s = h->adjoint;
    return NODAL_OK;
}

void sens_free_child(nodal_ctx *h) {
    if (!h->adjoint) return;
    nodal_free_buffers(h->adjoint);
    delete h->adjoint;
    h->adjoint = nullptr;
    h->adjoint_epoch = 0;
}

int sens_rhs_block(nodal_ctx *h, const SensCall *call, int32_t m0, int cols, double *out, int64_t rs, int64_t cs) {
    k_sens_rhs<<<1, 64, 0, h->stream>>>(cols, h->K, call->kind + m0, call->p + m0, call->q2 + m0, h->type.as<uint8_t>(),
                                       assembled_values(h), h->a.as<int32_t>(), h->b.as<int32_t>(), h->k.as<int32_t>(),
                                       out, rs, cs);
    NODAL_HIP_TRY(h, hipGetLastError());
    return NODAL_OK;
}

int sens_block(nodal_ctx *h, const SensCall *call, int32_t m0, int cols, const double *lam, int64_t rs, int64_t cs) {
    const int64_t ncomp = h->ncomp;
    hipStream_t st = h->stream;
    if (ncomp > 0) {
        NODAL_HIP_TRY(h, h->sn_out.reserve((size_t)SCOLS * ncomp * 8 + 64));
        double *sens = h->sn_out.as<double>();
        ExplicitRows ex;
        for (int y = 0; y < SCOLS; ++y) ex.row[y] = -1;
        for (int y = 0; y < cols; ++y)
            if (call->kind_host[m0 + y] == 1) ex.row[y] = call->p_host[m0 + y];
        const double *value = assembled_values(h);
        const bool il = rs == SCOLS && cs == 1;
        auto launch = il ? k_sensitivity_block<true> : k_sensitivity_block<false>;
        launch<<<groups_of(ncomp, STB), STB, 0, st>>>(ncomp, h->K, cols, h->type.as<uint8_t>(), value,
                                                      h->a.as<int32_t>(), h->b.as<int32_t>(), h->c.as<int32_t>(),
                                                      h->d.as<int32_t>(), h->drv.as<int32_t>(), h->k.as<int32_t>(),
                                                      call->x, lam, rs, cs, ex, sens);
        if (h->sn_ncross > 0) {
            const int32_t *drivers = h->sn_cross.as<int32_t>(), *gptr = drivers + h->sn_ndrivers,
                          *rows = gptr + h->sn_ndrivers + 1;
            k_sensitivity_cross<<<groups_of(h->sn_ndrivers * SCOLS, STB), STB, 0, st>>>(
                h->sn_ndrivers, ncomp, h->K, cols, drivers, gptr, rows, h->type.as<uint8_t>(), value, h->c.as<int32_t>(),
                h->d.as<int32_t>(), h->k.as<int32_t>(), call->x, lam, rs, cs, sens);
        }
        NODAL_HIP_TRY(h, hipGetLastError());
        NODAL_HIP_TRY(h, hipMemcpyAsync(call->sens_out + (int64_t)m0 * ncomp, sens, (size_t)cols * ncomp * 8,
                                        hipMemcpyDeviceToHost, st));
    }
    NODAL_WAIT_STREAM(h, st);
    return NODAL_OK;
}

namespace {
// the driver's client: the columns are the outputs' c, a finished block goes through the table kernels.  It reads the
// interleaved block as it stands (k_sensitivity_block<true>) and asks for rows only when the caller wants the adjoints.
struct AdjointClient final : MultiRhsClient {
    nodal_ctx *h;
    const SensCall *call;
    AdjointClient(nodal_ctx *h_, const SensCall *call_) : h(h_), call(call_) {
        wants_rows = call->adjoint_out != nullptr;
        max_cols = SCOLS;
    }
    int build(int32_t m0, int cols, double *out, int64_t rs, int64_t cs) override {
        return sens_rhs_block(h, call, m0, cols, out, rs, cs);
    }
    int hand_over(int32_t m0, int cols, const double *lam, int64_t rs, int64_t cs, const double *rows) override {
        if (rows)
            NODAL_HIP_TRY(h, hipMemcpyAsync(call->adjoint_out + (int64_t)m0 * h->n, rows, (size_t)cols * h->n * 8,
                                            hipMemcpyDeviceToHost, h->stream));
        return sens_block(h, call, m0, cols, lam, rs, cs);  // (waits)
    }
    void all_singular(int32_t count) override {
        const double nan = __builtin_nan("");
        for (int64_t t = 0; t < (int64_t)count * h->ncomp; ++t) call->sens_out[t] = nan;
        if (call->adjoint_out)
            for (int64_t t = 0; t < (int64_t)count * h->n; ++t) call->adjoint_out[t] = nan;
    }
};
}  // namespace

int sens_run(nodal_ctx *h, bool dense, int32_t count, const int32_t *kind, const int32_t *p, const int32_t *q2,
             double *sens_out, double *value_out, double *adjoint_out, double *resid_out, int32_t *info_out) {
    const int64_t n = h->n, ncomp = h->ncomp;
    hipStream_t st = h->stream;
    for (int32_t q = 0; q < count; ++q) {
        if (kind[q] == 0) {
            if (p[q] < -1 || p[q] >= h->K || q2[q] < -1 || q2[q] >= h->K)
                return nodal_fail(h, NODAL_E_INVALID, "sensitivities: node index out of range");
        } else if (kind[q] == 1) {
            if (p[q] < 0 || p[q] >= ncomp) return nodal_fail(h, NODAL_E_INVALID, "sensitivities: table row out of range");
        } else {
            return nodal_fail(h, NODAL_E_INVALID, "sensitivities: unknown output kind");
        }
    }
    // the specification (kind | p | q2 as int32 [count] each), the values [count] and the verdict word
    const size_t words = ((size_t)3 * count + 3) & ~(size_t)1;
    NODAL_HIP_TRY(h, h->sn_spec.reserve(words * 4 + (size_t)count * 8 + 64));
    int32_t *kind_dev = h->sn_spec.as<int32_t>(), *p_dev = kind_dev + count, *q2_dev = p_dev + count;
    int32_t *bad_dev = q2_dev + count;
    double *value_dev = reinterpret_cast<double *>(kind_dev + words);
    NODAL_HIP_TRY(h, hipMemcpyAsync(kind_dev, kind, (size_t)count * 4, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(p_dev, p, (size_t)count * 4, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemcpyAsync(q2_dev, q2, (size_t)count * 4, hipMemcpyHostToDevice, st));
    NODAL_HIP_TRY(h, hipMemsetAsync(bad_dev, 0, 4, st));
    // the handle is left as it was found.  The single solve's solution is set aside: the kernels read it, and the
    // multigrid route writes h->x
    HandleKeeper keep;
    NODAL_TRY(keep.save(h, true));
    k_sens_values<<<groups_of(count, STB), STB, 0, st>>>(count, h->K, kind_dev, p_dev, q2_dev, h->type.as<uint8_t>(),
                                                         assembled_values(h), h->a.as<int32_t>(), h->b.as<int32_t>(),
                                                         h->k.as<int32_t>(), h->sn_x.as<double>(), value_dev, bad_dev);
    NODAL_HIP_TRY(h, hipGetLastError());
    if (value_out) NODAL_HIP_TRY(h, hipMemcpyAsync(value_out, value_dev, (size_t)count * 8, hipMemcpyDeviceToHost, st));
    int32_t bad = 0;
    NODAL_TRY(nodal_read_words(h, &bad, bad_dev, 4));  // (waits: the host copies above are done too)
    if (bad) return nodal_fail(h, NODAL_E_INVALID, "sensitivities: the current of a current source is its value, not an output");
    NODAL_TRY(sens_cross_list(h));

    SensCall call;
    call.kind = kind_dev;
    call.p = p_dev;
    call.q2 = q2_dev;
    call.kind_host = kind;
    call.p_host = p;
    call.x = h->sn_x.as<double>();
    call.sens_out = sens_out;
    call.adjoint_out = adjoint_out;
    if (n == 0) {  // (every lead is ground: nothing depends on anything)
        for (int64_t t = 0; t < (int64_t)count * ncomp; ++t) sens_out[t] = 0.0;
        for (int32_t q = 0; q < count; ++q) {
            info_out[q] = 0;
            if (resid_out) resid_out[q] = 0.0;
        }
        return NODAL_OK;
    }
    nodal_ctx *s = nullptr;
    NODAL_TRY(adjoint_context(h, &s));
    AdjointClient client(h, &call);
    int status = keep.restore(h, multi_rhs_solve(h, s, dense, count, resid_out, info_out, client), "sensitivities");
    const int w = nodal_wait_stream(h, st, NODAL_SITE);
    if (status == NODAL_OK) status = w;
    return status;
}
