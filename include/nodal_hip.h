/*
 * nodal_hip.h -- C ABI of libnodal_hip.so: MI355X (gfx950) assembly of the
 * modified-nodal-analysis system G x = A and its dense / sparse solve.
 *
 * The reference (EnricoMiccoli/nodal v1.3.0) has no FFI layer; its seam is the
 * Python pair Circuit.build_model / Circuit.solve.  Each entry point below
 * names the reference code it replaces (file:line into the reference tree).
 * The host-side mirror of the reference API that calls these through ctypes is
 * nodal_amd/circuit.py; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns a nodal_status (0 = OK); no exception crosses;
 *   - the caller owns all host buffers; the opaque handle owns device memory;
 *   - one handle per (device, stream); thread-compatible, not thread-safe;
 *   - node indices are int32, -1 means "lead is the ground node";
 *   - unknown vector layout: x[0:K] node potentials in nodenum order,
 *     x[K:K+B] branch currents in anomnum order (reference nodal/nodal.py:405-408).
 */
#ifndef NODAL_HIP_H
#define NODAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nodal_ctx *nodal_handle;

typedef enum {
    NODAL_OK = 0,
    NODAL_E_INVALID = 1,          /* bad argument / call order                      */
    NODAL_E_HIP = 2,              /* a HIP runtime call failed (see nodal_last_error) */
    NODAL_E_ZERO_RESISTANCE = 3,  /* -> ValueError   (reference nodal/models.py:14-17) */
    NODAL_E_STAMP_COLLISION = 4,  /* -> AssertionError (reference nodal/models.py:43,47,
                                      66,70,168,172,176,193,197: `assert G[i, j] == 0`) */
    NODAL_E_SINGULAR = 5,         /* zero pivot / floating sub-network / non-finite x */
    NODAL_E_NOMEM = 6,
    NODAL_E_UNSUPPORTED = 7
} nodal_status;

/* component type codes of the `type` column (nodal_amd/constants.py TYPE_CODE).
 * VCCS rows carry NODAL_T_VCVS: the reference dispatches them to write_VCVS
 * (reference nodal/nodal.py:377-378). */
enum { NODAL_T_R = 0, NODAL_T_A = 1, NODAL_T_E = 2, NODAL_T_VCVS = 3,
       NODAL_T_CCVS = 4, NODAL_T_CCCS = 5,
       /* internal (never produced by the netlist front end): transconductance stamp
        * without a branch unknown -- a current value*(e_c - e_d) flows from lead a to
        * lead b.  Used by the presolve that eliminates branch equations (presolve.hip). */
       NODAL_T_GM = 6 };

/* sparse solver selection for nodal_solve_sparse */
enum { NODAL_SPARSE_AUTO = 0,
       NODAL_SPARSE_PCG = 1,      /* SPD: multigrid-preconditioned flexible CG (Jacobi-CG when small) */
       NODAL_SPARSE_DENSIFY = 2,  /* scatter to a dense panel, LU with pivoting                      */
       NODAL_SPARSE_LU = 3,       /* general: block-preconditioned flexible GMRES (historic name)   */
       NODAL_SPARSE_DIRECT = 4 }; /* multifrontal LU (static matching, nested dissection, pivoting inside the
                                     fronts) + fp64 refinement: what AUTO falls back on when an iteration
                                     gives up -- spsolve's "any non-singular G" (reference nodal/nodal.py:325) */

/* ---- lifetime ---------------------------------------------------------- */
int nodal_create(int device_id, nodal_handle *out);
int nodal_destroy(nodal_handle h);
const char *nodal_last_error(nodal_handle h);
/* library / build identification, e.g. "nodal_hip 0.1 gfx950" */
const char *nodal_version(void);

/* ---- component table (replaces the per-component Python objects read by
 *      Circuit.build_model, reference nodal/nodal.py:338-368) --------------
 * Copies the structure-of-arrays table to HBM.  K = nums["kcl"], B = nums["be"].
 * The range check of the rows (nodes < K, drivers < ncomp, branch types <=> k >= 0)
 * runs on the device behind the copies; NODAL_E_INVALID as before for a bad row.
 * c, d, drv, k may be NULL -- all four together -- when B == 0 (resistors and current
 * sources read none of them): the columns then hold -1 on the device.  In a table WITH those columns they are
 * read for the rows whose type uses them (E .. CCCS and the internal GM) and taken as -1 on resistor and current-source
 * rows, whatever the caller's arrays hold there: only the dependent rows' entries travel (round 5).
 * Columns that live in pinned memory (nodal_host_alloc) are copied by DMA at link
 * rate; pageable memory goes through the runtime's staging copies. */
int nodal_upload_components(nodal_handle h, int64_t ncomp,
                            const uint8_t *type, const double *value,
                            const int32_t *a, const int32_t *b,
                            const int32_t *c, const int32_t *d,
                            const int32_t *drv, const int32_t *k,
                            int32_t K, int32_t B);
/* Page-locked host memory for the table's columns (what the lowering of a large netlist
 * writes into: reference nodal/nodal.py:338-368 builds Python objects there).  Needs a
 * HIP device; NODAL_E_HIP otherwise (callers fall back to ordinary memory). */
int nodal_host_alloc(size_t bytes, void **out);
int nodal_host_free(void *p);

/* Replace the value column only (same topology): `batch` members, row-major
 * [batch][ncomp].  Used for value sweeps (BASELINE.json config 4). */
int nodal_upload_values(nodal_handle h, int32_t batch, const double *values);

/* ---- assembly (replaces Circuit.build_model + models.write_*, reference
 *      nodal/nodal.py:338-398, nodal/models.py:13-214) ---------------------
 * symbolic: sparsity pattern (CSR, sorted columns) + ordered contribution
 *           lists; depends on topology only, reusable across a value sweep.
 * numeric : folds every matrix / rhs entry's contributions in component order
 *           (bit-identical to the reference's sequential += / = stamping) for
 *           batch member `member` (0 when no batch was uploaded).
 * On NODAL_E_ZERO_RESISTANCE / NODAL_E_STAMP_COLLISION, *bad_component (may be
 * NULL) receives the table row of the first offending component. */
int nodal_assemble_symbolic(nodal_handle h);
int nodal_assemble_numeric(nodal_handle h, int32_t member, int64_t *bad_component);

/* sizes after symbolic assembly */
int nodal_get_sizes(nodal_handle h, int64_t *n, int64_t *nnz, int64_t *ncontrib);

/* ---- export for parity / debugging (what the reference exposes as
 *      Circuit.G, Circuit.A; reference nodal/nodal.py:311,396-398) --------- */
int nodal_export_csr(nodal_handle h, int32_t *indptr, int32_t *indices,
                     double *data, double *rhs);
/* row-major n x n, as numpy's Circuit.G */
int nodal_export_dense(nodal_handle h, double *G, double *rhs);

/* ---- solve (replaces Circuit.solve, reference nodal/nodal.py:313-336) ----
 * dense : direct solve of the dense system, replacing LAPACK dgesv behind
 *         np.linalg.solve (reference nodal/nodal.py:327): partial pivoting with dgesv's
 *         pivot order for small systems, tournament pivoting for large general ones,
 *         pivot-free block elimination for (presolved) conductance networks -- see
 *         DESIGN.md section 3.2.  *info > 0: singular matrix (an exactly zero pivot, or
 *         a floating sub-network of a passive system) -> status NODAL_E_SINGULAR (host
 *         maps it to LinAlgError / UnconnectedCircuitError as reference
 *         nodal/nodal.py:328-335).
 * sparse: replaces scipy.sparse.linalg.spsolve (reference nodal/nodal.py:325).
 *         On a singular system x is filled with NaN, *info > 0 and the status is
 *         NODAL_OK: the reference's sparse path warns and returns NaNs, it does
 *         not raise.
 * x may be NULL to leave the solution on the device (nodal_download_x). */
int nodal_solve_dense(nodal_handle h, double *x, int32_t *info);
int nodal_solve_sparse(nodal_handle h, int32_t method, double *x, int32_t *info,
                       int32_t *iters, double *resid);
int nodal_download_x(nodal_handle h, double *x);

/* ---- equivalent-resistance sweep (replaces one equivalent_resistance() call per
 *      pair, reference nodal/equiv.py:31-61: deepcopy + rebuild + re-solve) ---------
 * For every pair (ia[q], ib[q]) of node indices (-1 = ground) a 1 A probe enters ia and
 * leaves ib; resistance[q] = e(ia) - e(ib).  G is factorised (dense) or its multigrid
 * hierarchy built (sparse) once for all pairs.  The circuit's own rhs is ignored, as
 * it is zero for the resistive networks the reference accepts here.  *info > 0:
 * singular network (dense: status NODAL_E_SINGULAR; sparse: NaNs, status OK). */
int nodal_solve_pairs(nodal_handle h, int32_t dense, int32_t npairs, const int32_t *ia,
                      const int32_t *ib, double *resistance, int32_t *info);

/* ---- source sweep (replaces a loop of Circuit(netlist with other source values) + .solve(), reference
 *      nodal/nodal.py:306-336: a .dc sweep of a supply, the load vectors of an IR-drop study) ---------------
 * Members m in [0, count): the system of the last nodal_assemble_numeric with the value of table row
 * rows[j] (type A or E) replaced by values[m * nsrc + j].  G is shared; only the rhs differs.
 * x_out [count][n] row-major, resid_out [count], info_out [count]; x_out / resid_out may be NULL.
 * resid_out[m] = ||G x_m - A_m||_inf / (||G||_inf ||x_m||_inf + ||A_m||_inf), computed on the device.
 * info_out[m] > 0: singular network (row of NaNs, status OK) -- except with dense != 0, where a singular G
 * returns NODAL_E_SINGULAR, as nodal_solve_dense does.  NODAL_E_INVALID: a row out of range, a row that is
 * not of type A or E, a repeated row, or no nodal_assemble_numeric before.  Neither the table nor the
 * assembled rhs changes; the solution of the last single solve is not kept (nodal_download_x needs a new one). */
int nodal_solve_sources(nodal_handle h, int32_t dense, int32_t count, int32_t nsrc, const int64_t *rows,
                        const double *values, double *x_out, double *resid_out, int32_t *info_out);

/* ---- branch currents and power (replaces a Python loop over Solution.result after Circuit.solve, reference
 *      nodal/nodal.py:313-336: the reference answers with potentials and branch unknowns only) ---------------
 * For the solution on the device, per table row i (the order of nodal_upload_components), e(-1) = +0.0:
 *   voltage[i] = e(a_i) - e(b_i);
 *   current[i] = voltage[i] / value_i for a resistor (one division; it flows from lead a to lead b), value_i for a
 *                current source, x[K + k_i] for the rows that own a branch unknown (E, VCVS, CCVS, CCCS).  For
 *                every type but R it flows from b to a inside the component, into node a (the reference's stamps:
 *                A[a] += J, G[a, K + k] = -1);
 *   power[i]   = what the row absorbs: voltage * current for a resistor, -(voltage * current) otherwise.
 * value_i is the value the last nodal_assemble_numeric used (its member of an uploaded value table).
 * totals2 = {sum of power over the resistors, sum over every other row}: Tellegen's theorem makes them cancel.
 * The sums have a fixed shape and use no atomics: a repeated call gives the same bits.  Each array may be NULL.
 * Where x holds NaN (a singular sparse system) so does everything that reads it.  NODAL_E_INVALID: no solution
 * on the handle (no solve yet, or a sweep since), or no component table. */
int nodal_branches(nodal_handle h, double *voltage, double *current, double *power, double *totals2);

/* ---- worst-case envelope of a source sweep (replaces the same loop over every member's Solution.result, reference
 *      nodal/nodal.py:313-336, per member of the loop nodal_solve_sources replaces) ---------------------------
 * The arguments and results of nodal_solve_sources, plus, over the members m with info_out[m] == 0:
 *   current_absmax [ncomp] = max_m |current_m[i]| (current as in nodal_branches; a swept current source counts
 *                            with its member's value), current_member [ncomp] a member that attains it;
 *   potential_min / potential_max [K] over x_m[j], j < K, with potential_min_member / potential_max_member [K];
 *   power_out [count][2]   = {dissipated, absorbed by the sources} of member m; NaN for a member that is left out.
 * Among exact ties the lowest member index is reported.  With every member left out (or count == 0): NaN and -1.
 * Each output may be NULL; with x_out == NULL no count x n array exists on the host at all -- the envelope is
 * accumulated on the device as each block of up to sixteen members is finished. */
int nodal_solve_sources_branches(nodal_handle h, int32_t dense, int32_t count, int32_t nsrc, const int64_t *rows,
                                 const double *values, double *x_out, double *resid_out, int32_t *info_out,
                                 double *current_absmax, int32_t *current_member, double *potential_min,
                                 int32_t *potential_min_member, double *potential_max, int32_t *potential_max_member,
                                 double *power_out);

/* ---- adjoint sensitivities (replaces a finite-difference loop of Circuit(netlist with one value nudged) + .solve(),
 *      reference nodal/nodal.py:306-336, two solves per component; the reference has no derivative of its own) ----
 * For the solution on the device and `count` outputs y_q = c_q^T x, the derivative of every output with respect to the
 * value of EVERY table row (the values the last nodal_assemble_numeric used): one solve with G^T per output, sixteen
 * outputs to a block, and one pass over the component table per block (csrc/sensitivity.hip states the per-row formulas).
 * kind[q] 0: y = e(p[q]) - e(q2[q]) (node indices, -1 ground); 1: y = current of table row p[q] (as nodal_branches;
 *            q2[q] is ignored).  The current of a current source is its value: NODAL_E_INVALID.
 * sens_out [count][ncomp] row-major; value_out [count] = y itself (may be NULL); adjoint_out [count][n] = the lambda of
 * G^T lambda = c (may be NULL); resid_out [count] = ||G^T lambda - c||_inf / (||G||_1 ||lambda||_inf + ||c||_inf),
 * computed on the device (may be NULL); info_out [count] as nodal_solve_sources: > 0 a singular network (rows of
 * NaNs, status OK) -- except with dense != 0, where a singular G returns NODAL_E_SINGULAR.
 * Needs the solution of a single solve on the handle (NODAL_E_INVALID otherwise, as nodal_branches) and leaves the handle
 * as it found it: the solution, the table, G, A.  No floating-point atomics: a repeated call gives the same bits. */
int nodal_sensitivities(nodal_handle h, int32_t dense, int32_t count, const int32_t *kind, const int32_t *p,
                        const int32_t *q2, double *sens_out, double *value_out, double *adjoint_out,
                        double *resid_out, int32_t *info_out);

/* ---- loss gradients (replaces one nodal_sensitivities output per unknown a loss touches: one adjoint solve and one
 *      [ncomp] row each; the reference has no derivative of its own) ----
 * For a scalar loss L = sum_m L_m(x_m) over `count` members that share G -- the members of a source sweep, or the single
 * solve -- and the caller's cotangent[m] = dL/dx_m (dense, [n]): lambda_m solves G^T lambda_m = cotangent[m], and
 *   grad_out[i]            = sum_m s_i(lambda_m, x_m) for EVERY table row i, s_i the per-row formula of
 *                            nodal_sensitivities without an explicit term (csrc/sensitivity.hip states them; R with the
 *                            cross terms of resistors that drive CCVS / CCCS rows, A, E, VCVS, CCVS, CCCS).  A loss that
 *                            reads the values themselves adds that part on its own.
 *   grad_sources_out[m][j] = s_{rows[j]}(lambda_m, .): member m's derivative with respect to its OWN value of swept row
 *                            rows[j] (the formula of an A or E row reads neither x nor the value).
 * grad_out at a swept row holds the same uniform formula, i.e. the sum over the members of grad_sources_out[.][j]: the
 * derivative with respect to a value all members would share.  G and the value column are those of the last
 * nodal_assemble_numeric.  x [count][n]: the members' solutions (what nodal_solve_sources returned); NULL: the solution of
 * the single solve on the handle (count must be 1 and nsrc 0).  rows [nsrc]: the swept table rows (type A or E, each named
 * once); may be NULL with nsrc 0.  grad_sources_out, adjoint_out [count][n] (the lambdas) and resid_out [count] may be
 * NULL; resid_out and info_out [count] mean what they mean in nodal_sensitivities.  A singular G with dense != 0 returns
 * NODAL_E_SINGULAR; otherwise NaN goes into everything a singular member feeds, and -- the sum is not defined with a
 * member missing -- into the whole of grad_out.  count == 0 writes zeros to grad_out.
 * NODAL_E_INVALID: no nodal_assemble_numeric before the call; x == NULL without a solution on the handle, with
 * count != 1 or with nsrc != 0; a swept row out of range, not an A / E row, or repeated.
 * One adjoint solve per member, sixteen members to a block, one pass over the component table per block; the sum over
 * the members is formed on the device in member order and nothing of size [count][ncomp] exists anywhere.  Leaves the
 * handle as it found it: the solution if any, the table, G, A.  No floating-point atomics: a repeated call gives the
 * same bits. */
int nodal_gradient(nodal_handle h, int32_t dense, int32_t count, const double *x, const double *cotangent, int32_t nsrc,
                   const int64_t *rows, double *grad_out, double *grad_sources_out, double *adjoint_out,
                   double *resid_out, int32_t *info_out);

/* ---- transient analysis (replaces a host loop of rebuild and solve per time step: with the reference a new netlist
 *      with companion rows, a new Circuit and a .solve() for every t_k, reference nodal/nodal.py:306-336) ----
 * The handle holds the circuit WITH one extra R row per capacitor, cap_rows [ncap] (table rows of type R): the companion
 * resistor of a capacitor C stepped with h, value h / C for backward Euler (method 0) and h / (2 C) for the trapezoidal
 * rule (method 1); its leads and its conductance g = 1 / value are read from the table on the device.  G is that of the
 * last nodal_assemble_numeric and does not change; step k = 1 .. steps solves G x_k = A_k + the history currents, J
 * injected into lead a and drawn from lead b of every capacitor, with v = x(a) - x(b) of x_{k-1} (ground: +0.0):
 *   method 0:  J_k = g v_{k-1}
 *   method 1:  J_k = 2 g v_{k-1} - J_{k-1}, J_0 = g v_0 (zero capacitor currents at t_0: x0 must be a DC operating point)
 * A_k is the right-hand side with the sources src_rows [nsrc] (type A or E, each named once) at src_values[k - 1][.]
 * ([steps][nsrc]; the other sources keep their table values).  x0 [n]: the state at t_0; only its potentials are read.
 *   wave_out [steps + 1][nprobe]  x_k(probe_a[p]) - x_k(probe_b[p]) (node indices, -1 ground), row 0 from x0; a probe
 *                                 with probe_a == probe_b reads exactly +0.0
 *   x_out [steps / keep_every][n] x_k of every keep_every-th step (keep_every 0: none)
 *   pot_min, pot_max [K]          lowest / highest potential of each node over the solved steps, pot_min_step,
 *                                 pot_max_step [K] a step that attains it (among exact ties the lowest); NaN and -1
 *                                 when no step was solved
 *   resid_out [steps]             the scaled residual of step k as nodal_solve_sources defines it
 *   info_out [steps]              > 0: singular (the step and every later one: NaN wherever they land, status OK) --
 *                                 except with dense != 0, where a singular G returns NODAL_E_SINGULAR
 *   iters_out [steps]             iterations of the step's solve (multigrid), 1 (sparse LU + refinement), 0 (dense panel)
 * Each output may be NULL.  Routes: n <= 64 the dense panel, factored anew every step; B == 0, all R > 0 and n > 4096 the
 * multigrid iteration on the hierarchy of step 1 (a step it gives up on, and every later one: the sparse direct solve);
 * everything else one sparse LU, per step two substitutions, one refinement step and the judgement (a step above the
 * bar is redone by the sparse direct solve).  Hierarchy and factors are kept on the handle until the next
 * nodal_assemble_numeric: a later call repeats neither.  nodal_last_timings afterwards: [0] host ms of the matrix work
 * this call did once (the factorisation; on the multigrid route step 1 with its setup), exactly 0.0 when it was kept;
 * [1] 0.0; [2] the whole call.
 * NODAL_E_INVALID: steps < 0, a method other than 0 / 1, a cap_rows entry out of range or not of type R, the source-row
 * errors of nodal_solve_sources, a probe node outside [-1, K), x0 == NULL, no nodal_assemble_numeric before the call.
 * One host wait per kept block of solutions and what the solvers look at; waveforms, envelope and residuals come down
 * once.  The handle's solution is dropped.  No floating-point atomics: a repeated call gives the same bits. */
int nodal_transient(nodal_handle h, int32_t dense, int32_t steps, int32_t method, int64_t ncap, const int64_t *cap_rows,
                    int32_t nsrc, const int64_t *src_rows, const double *src_values, const double *x0, int32_t nprobe,
                    const int32_t *probe_a, const int32_t *probe_b, double *wave_out, int32_t keep_every, double *x_out,
                    double *pot_min, int32_t *pot_min_step, double *pot_max, int32_t *pot_max_step, double *resid_out,
                    int32_t *info_out, int32_t *iters_out);

/* ---- transient analysis with inductors: RLC networks (nodal_transient is this call with nind == 0: the same launches at
 *      the same sizes, the same bits) ----
 * nodal_transient's arguments and rules, plus: the handle's table holds one more R row per inductor, ind_rows [nind]
 * (type R, checked on the device as cap_rows are): the companion resistor of an inductor L stepped with h, value L / h
 * for backward Euler and 2 L / h for the trapezoidal rule, g = 1 / value.  The inductor's current i counts positive from
 * lead a to lead b through the element; i0 [nind] is the state at t_0 (NULL: zero).  With v = x(a) - x(b):
 *   method 0:  i_k = i_{k-1} + g v_k,              J_k = -i_{k-1}
 *   method 1:  i_k = i_{k-1} + g (v_k + v_{k-1}),  J_k = -(i_{k-1} + g v_{k-1})
 * J_k injected into lead a and drawn from lead b like a capacitor's; in both methods i_k = -J_k + g v_k, formed by one
 * lane per inductor after the solve of step k.  A node's history currents are summed over its capacitors and then its
 * inductors, each in ascending order.
 *   cur_out [steps + 1][ncur]     i_k of the inductors cur_index [ncur] (indices into ind_rows), row 0 = i0
 *   i_final_out [nind]            every inductor's current after the last step
 * Each may be NULL.  A step without a state (info_out > 0) has NaN in its cur_out row, and any such step leaves NaN in
 * i_final_out.  With NODAL_OPT_TRANSIENT_TAPE set and nind > 0 NO tape is kept (the adjoint with inductors is not
 * implemented): a nodal_transient_gradient afterwards finds no recorded transient.
 * NODAL_E_INVALID, besides nodal_transient's: an ind_rows entry out of range or not of type R, a cur_index entry outside
 * [0, nind), inductors on a network without nodes.  The currents come down once, with the waveforms. */
int nodal_transient_rlc(nodal_handle h, int32_t dense, int32_t steps, int32_t method, int64_t ncap, const int64_t *cap_rows,
                        int32_t nsrc, const int64_t *src_rows, const double *src_values, const double *x0, int32_t nprobe,
                        const int32_t *probe_a, const int32_t *probe_b, double *wave_out, int32_t keep_every, double *x_out,
                        double *pot_min, int32_t *pot_min_step, double *pot_max, int32_t *pot_max_step, double *resid_out,
                        int32_t *info_out, int32_t *iters_out, int64_t nind, const int64_t *ind_rows, const double *i0,
                        int32_t ncur, const int32_t *cur_index, double *cur_out, double *i_final_out);

/* ---- nonlinear DC analysis: networks with diodes, by Newton's method (replaces a host loop that downloads x, evaluates
 *      the junctions in numpy, uploads a value column, re-assembles and solves per iteration; with the reference a new
 *      netlist, a new Circuit and a .solve() per iteration, reference nodal/nodal.py:306-336) ----
 * The handle holds the circuit WITH one extra R row per diode, diode_rows [ndiode] (table rows of type R, checked on the
 * device as cap_rows are; their table values are overwritten).  Diode d, anode = lead a and cathode = lead b of its row,
 * carries i(v) = i_sat[d] (exp(v / n_vt[d]) - 1) + gmin v from a to b at v = x(a) - x(b) (ground: +0.0); n_vt in volts
 * (emission coefficient times thermal voltage).  One word vh per diode is the limited junction voltage; vh_0 = v of x0
 * (x0 [n], NULL: zeros; only its potentials are read).  Iteration k = 0 .. linearises at vh_k,
 *   e = exp(vh / n_vt),  g = i_sat e / n_vt + gmin,  i = i_sat (e - 1) + gmin vh,  J = g vh - i
 * writes 1 / g into the diode's row of the value column on the device, assembles G anew (symbolic phase kept) and solves
 * G x_{k+1} = A + the J, injected into lead a and drawn from lead b (the capacitors' convention in nodal_transient); A has
 * the sources src_rows [nsrc] at src_values [nsrc] (nodal_solve_sources' row rules, one setting).  Then per diode, with
 * the raw v = x_{k+1}(a) - x_{k+1}(b) and v_crit = n_vt ln(n_vt / (sqrt(2) i_sat)), SPICE's junction limiting
 *   limited:  v > v_crit and |v - vh| > 2 n_vt
 *     vh > 0:   a = 1 + (v - vh) / n_vt,  vh' = a > 0 ? vh + n_vt ln a : v_crit
 *     vh <= 0:  vh' = n_vt ln(v / n_vt)
 *   otherwise vh' = v
 * and the diode's convergence test, with ihat = i + g (v - vh):
 *   |v - vh| <= reltol max(|v|, |vh|) + vntol  and  |i(v) - ihat| <= reltol max(|i(v)|, |ihat|) + abstol
 * The loop ends when no diode fails its test (*converged = 1), after max_iter iterations, on a singular iteration, or on
 * an iterate that is not finite or a g that overflows (*converged = 0; the loop never hangs).  ndiode == 0 is one linear
 * solve, converged after one iteration.
 *   x_out [n]                     the last iterate
 *   v_out, i_out, g_out [ndiode]  v, i(v), g(v) = i_sat exp(v / n_vt) / n_vt + gmin at the last iterate
 *   iterates_out [max_iter][n]    x_1 .. (rows past *iterations are left as they were)
 *   vh_out [max_iter + 1][ndiode] vh_0, vh_1 .. ; NaN past the last one formed
 *   record_out [max_iter][4]      per iteration: diodes that failed the test, diodes that were limited, max |v - vh|,
 *                                 the scaled residual of the solve as nodal_solve_sources defines it; zeros past
 *                                 *iterations
 *   info_out [max_iter]           > 0: the iteration was singular: NaN in its record, in x_out, v_out, i_out, g_out
 *                                 (status OK) -- except with dense != 0, where a singular G returns NODAL_E_SINGULAR
 *   iters_out [max_iter]          iterations of the solve (multigrid), 1 (sparse LU + refinement), 0 (dense panel)
 *   route_out [max_iter]          0 dense panel, 1 sparse LU, 2 multigrid, 3 the sparse direct solve took the step
 *                                 over (nodal_transient's fall-backs); -1 past *iterations
 * Each of them may be NULL; iterations and converged may not.  Routes as nodal_transient's, chosen anew every iteration,
 * and the matrix work is redone every iteration because the matrix moved: n <= 64 the dense panel; B == 0, all R > 0 and
 * n > 4096 the multigrid iteration, the hierarchy's values refreshed on its kept symbolic setup; everything else the
 * sparse LU, factored anew on its kept analysis.  nodal_last_timings afterwards: [0] host ms of the matrix work
 * (assembly, factorisation, hierarchy setup) summed over the iterations; [1] the part of [0] that was symbolic (an LU
 * analysis, a full hierarchy setup), exactly 0.0 when all of it was kept; [2] the whole call.
 * NODAL_E_INVALID: max_iter < 1, gmin or a tolerance negative or not finite, an i_sat or n_vt that is not > 0 and finite,
 * a diode_rows entry out of range or not of type R, diodes on a network without nodes, the source-row errors of
 * nodal_solve_sources, no nodal_assemble_numeric before the call.
 * Host waits per iteration: the assembly's status words, what the solver looks at, and ONE read of the record (with the
 * scaled residual where the solver left it on the device).  The counts are integer atomics and the maximum an integer
 * maximum over the bits of |v - vh|: no floating-point atomics, a repeated call gives the same bits.  Afterwards the
 * handle's value column holds 1 / g of the last linearisation in the diode rows (1.0 after an overflow), G is assembled
 * from it, factors or hierarchy belong to it; the solution is dropped, a recorded transient is void.  The host copy of
 * the values that the presolve of networks with branch rows keeps is NOT updated in the diode rows: no route of this call
 * or of nodal_transient reads them there; nodal_upload_values / nodal_upload_components before any other solve. */
int nodal_newton_dc(nodal_handle h, int32_t dense, int64_t ndiode, const int64_t *diode_rows, const double *i_sat,
                    const double *n_vt, double gmin, int32_t nsrc, const int64_t *src_rows, const double *src_values,
                    const double *x0, int32_t max_iter, double reltol, double vntol, double abstol, double *x_out,
                    double *v_out, double *i_out, double *g_out, double *iterates_out, double *vh_out, double *record_out,
                    int32_t *info_out, int32_t *iters_out, int32_t *route_out, int32_t *iterations, int32_t *converged);

/* ---- nonlinear DC analysis with bipolar transistors: Ebers-Moll in its transport form, by the same Newton loop ----
 * nodal_newton_dc's arguments and rules, plus ntr transports.  A bipolar transistor is two junction diodes, plain members
 * of diode_rows / i_sat / n_vt (the caller gives them i_sat = i_s / beta_f and i_s / beta_r), plus one transport current
 *   i_T = i_s[t] (exp(v_f / n_f) - exp(v_r / n_r))
 * from lead a to lead b through the element, v_f, v_r the voltages and n_f, n_r the n_vt of the diodes junction[t][0] = jf
 * and junction[t][1] = jr.  NPN or PNP is the caller's choice of leads alone.  The handle's table holds, beside the diodes'
 * R rows, two rows of type NODAL_T_GM per transport, gm_rows[t][0] (forward) and gm_rows[t][1] (reverse): both with the
 * transport's leads a, b, and c, d = lead a, lead b (anode, cathode) of the row of diode jf, respectively jr; their table
 * values are overwritten.  gmin stays on the junctions; a transport has none, is not limited and has no state word.
 * Iteration k linearises every diode as nodal_newton_dc does and every transport at the SAME limited voltages
 * vhf = vh[jf], vhr = vh[jr]:
 *   ef = exp(vhf / n_f),  er = exp(vhr / n_r),  gmf = (i_s ef) / n_f,  gmr = (i_s er) / n_r,  iT = i_s ef - i_s er
 *   JT = gmf vhf - gmr vhr - iT
 * every product and quotient rounded on its own, the sums from left to right.  gmf goes into the forward row's value and
 * -gmr into the reverse row's, G is assembled, and JT is injected into lead a and drawn from lead b: a node's right-hand
 * side gets the J of its diodes in ascending order and then the JT of its transports in ascending order.  After the solve,
 * per transport with the raw vf, vr of x_{k+1}:
 *   iT(v) = i_s exp(vf / n_f) - i_s exp(vr / n_r),  ihat = iT + gmf (vf - vhf) - gmr (vr - vhr)
 *   passes when |iT(v) - ihat| <= reltol max(|iT(v)|, |ihat|) + abstol      (false with a NaN anywhere)
 * The loop ends when no diode and no transport fails its test (*converged = 1), and otherwise as nodal_newton_dc's does; a
 * gmf or gmr that is not finite is an overflow like a g that overflows (*converged = 0, NaN in the outputs).
 *   it_out, gmf_out, gmr_out [ntr]  iT, gmf, gmr at the raw junction voltages of the last iterate.  The terminal currents
 *                                   are the caller's sums: for an NPN (a = C, b = E, jf = B->E, jr = B->C), positive INTO
 *                                   the terminal, I_C = iT - i[jr], I_B = i[jf] + i[jr], I_E = -(iT + i[jf])
 *   record_out [max_iter][5]        nodal_newton_dc's four words and the transports that failed the test
 * The other outputs are nodal_newton_dc's; vh_out has a column per diode, the junctions among them.  Routes are
 * nodal_newton_dc's: n <= 64 the dense panel, everything else the sparse LU factored anew on its kept analysis -- a
 * network with transports never takes the multigrid route, because GM rows make it non-passive.  ntr == 0 is
 * nodal_newton_dc: the same launches and the same bits (the record's fifth word 0.0).
 * NODAL_E_INVALID, besides nodal_newton_dc's: ntr < 0, a NULL array with ntr > 0, a gm_rows entry out of range or not of
 * type NODAL_T_GM, two rows of a transport that do not share their a, b, a row whose c, d are not the leads a, b of its
 * junction's diode row, a junction index outside [0, ndiode), an i_s that is not > 0 and finite.
 * Host waits: once per call the transports' check (one word); per iteration nodal_newton_dc's and one more word behind
 * the assembly's status words, when the stream has drained already (whether a gmf or gmr overflowed).  The transports'
 * count is an integer atomicAdd -- integer atomics only: a repeated call gives the same bits.  Afterwards the handle is as
 * nodal_newton_dc leaves it, the GM rows of the value column holding gmf, -gmr of the last linearisation (0.0 after an
 * overflow, beside 1.0 in the diode rows). */
int nodal_newton_dc_bjt(nodal_handle h, int32_t dense, int64_t ndiode, const int64_t *diode_rows, const double *i_sat,
                        const double *n_vt, double gmin, int32_t nsrc, const int64_t *src_rows, const double *src_values,
                        const double *x0, int32_t max_iter, double reltol, double vntol, double abstol, int64_t ntr,
                        const int64_t *gm_rows, const int32_t *junction, const double *i_s, double *x_out, double *v_out,
                        double *i_out, double *g_out, double *it_out, double *gmf_out, double *gmr_out, double *iterates_out,
                        double *vh_out, double *record_out, int32_t *info_out, int32_t *iters_out, int32_t *route_out,
                        int32_t *iterations, int32_t *converged);

/* ---- gradients through the operating point: the adjoint of the Newton solve (replaces finite differences, two whole
 *      Newton runs per parameter, and the host loop of download x, scipy transpose solve and numpy formulas; with the
 *      reference every such run is itself a rebuild and a .solve() per iteration, reference nodal/nodal.py:306-336) ----
 * The handle holds the circuit with one companion R row per diode exactly as nodal_newton_dc requires; diode_rows, i_sat,
 * n_vt, gmin and src_rows / src_values [nsrc] are those the operating point x [n] was found at (x is the caller's:
 * nodal_newton_dc drops the handle's solution), cotangent [n] = dL/dx.  At the operating point
 *   F(x, p) = G(p) x + S i(S^T x) - A(p) = 0,   i(v) = i_sat (exp(v / n_vt) - 1) + gmin v,
 * S the incidence of the diodes (+1 anode, -1 cathode), so J^T lambda = cotangent with J = G + S diag(g(v)) S^T taken at
 * v = S^T x ITSELF (not at the last limited voltages of the run, which are one step behind), and dL/dp = -lambda^T dF/dp.
 * On the handle's stream: v = x(a) - x(b) per diode; the linearisation at v (1 / g(v) into the diode rows of the value
 * column, J_hist = g v - i(v)); G assembled anew, symbolic phase kept; the right-hand side of a Newton iteration (the
 * sources at src_values plus the signed list add of J_hist) and the block judge of x against it -- because the
 * linearisation is at x this is the nonlinear KCL defect G x + S i(v) - A, scaled as nodal_solve_sources defines; the
 * transposed solve on the handle itself (B == 0 and all R > 0) or on the child that holds G^T, by nodal_newton_dc's routes
 * and fall-backs (n <= 64 the dense panel; B == 0, all R > 0 and n > 4096 multigrid with the hierarchy's values refreshed
 * on its kept symbolic setup; otherwise the sparse LU factored anew on its kept analysis; a step above the bar goes to
 * the sparse direct solve); then the formulas:
 *   grad_out [ncomp]          s_i(lambda, x) of every table row as nodal_gradient's (cross terms of CCVS / CCCS drivers
 *                             included); exactly +0.0 in the diode rows, whose table value is the device's own
 *   grad_isat_out [ndiode]    -D (e - 1),           D = lambda(a) - lambda(b), e = exp(v / n_vt) as the forward pass
 *   grad_nvt_out [ndiode]     D i_sat e v / n_vt^2
 *   grad_gmin_out [1]         the sum over the diodes of -D v, reduced in a fixed order (wavefront, workgroup, then one
 *                             pass over the workgroups' sums)
 *   grad_sources_out [nsrc]   lambda(a) - lambda(b) of an A row, lambda(K + k) of an E row
 *   adjoint_out [n]           lambda
 *   resid_out [1]             the scaled residual of the transposed solve
 *   op_resid_out [1]          the scaled residual of x as an operating point (above): a caller who hands in an x that is
 *                             no operating point, or whose values moved since, sees it here
 *   info_out [1]              0 solved, > 0 J is singular
 * Each may be NULL except grad_out (with ncomp > 0) and info_out.  A diode with both leads on one node gets three zeros.
 * A singular J returns NODAL_E_SINGULAR with dense != 0; otherwise NaN in everything lambda feeds, info_out > 0, status
 * OK, op_resid_out still valid.  A g that overflows (1 / g == 0): every output NaN, op_resid_out too, info_out 0, and the
 * handle is left as nodal_newton_dc leaves it after an overflow.  n == 0 writes zeros.  ndiode == 0 is nodal_gradient's
 * single solve on the caller's x, on the matrix the handle holds.
 * nodal_last_timings afterwards as nodal_newton_dc's: [0] host ms of the matrix work, [1] the part of it that was symbolic
 * -- exactly 0.0 on a second call on the same structure -- [2] the whole call.
 * NODAL_E_INVALID: nodal_newton_dc's diode and source-row cases, gmin negative or not finite, x or cotangent NULL with
 * n > 0, grad_out NULL with ncomp > 0, no nodal_assemble_numeric before the call.
 * Host waits: the diode check, the assembly's status words, what the solver looks at, one read of three words at the
 * end.  No floating-point atomics: a repeated call gives the same bits.  Afterwards the handle is as nodal_newton_dc
 * leaves it: the value column holds 1 / g(v) in the diode rows (1.0 after an overflow), G, factors and hierarchy belong
 * to it, the solution is dropped, a recorded transient is void; nodal_newton_dc's note on the host copy of the values
 * holds here too. */
int nodal_newton_gradient(nodal_handle h, int32_t dense, int64_t ndiode, const int64_t *diode_rows, const double *i_sat,
                          const double *n_vt, double gmin, int32_t nsrc, const int64_t *src_rows, const double *src_values,
                          const double *x, const double *cotangent, double *grad_out, double *grad_isat_out,
                          double *grad_nvt_out, double *grad_gmin_out, double *grad_sources_out, double *adjoint_out,
                          double *resid_out, double *op_resid_out, int32_t *info_out);

/* ---- nonlinear transient analysis: diodes in a network stepped in time, Newton's method inside every step (replaces a
 *      host loop around nodal_newton_dc that downloads x, rebuilds the history currents, uploads a value column,
 *      assembles and solves once per Newton iteration per step) ----
 * nodal_transient_rlc's arguments and rules, plus nodal_newton_dc's diodes: the handle's table holds one companion R row
 * per capacitor, then per inductor, then per diode, diode_rows [ndiode] (type R, checked on the device; their table
 * values are overwritten).  Diode d carries i(v) = i_sat[d] (exp(v / n_vt[d]) - 1) + gmin v from lead a (anode) to lead b
 * (cathode) of its row.  Step k = 1 .. steps, given x_{k-1}, the capacitors' history words, the inductors' currents and
 * the method:
 *   1. base_k = A_k + the capacitors' and inductors' history currents, exactly what nodal_transient_rlc builds, formed
 *      ONCE per step and held fixed over the step's Newton iterations
 *   2. vh^0 = x_{k-1}(a) - x_{k-1}(b) per diode (ground: +0.0)
 *   3. Newton iteration j = 0, 1, ..: linearise at vh^j with nodal_newton_dc's formulas and roundings
 *        e = exp(vh / n_vt),  g = i_sat e / n_vt + gmin,  i = i_sat (e - 1) + gmin vh,  J = g vh - i
 *      write 1 / g into the diode's row of the value column, assemble G (symbolic phase kept), solve
 *        G x = base_k + S J       (J injected into lead a, drawn from lead b; a node's J in ascending order of its diodes)
 *      by the route nodal_newton_dc would choose (n <= 64 the dense panel; B == 0, all R > 0 and n > 4096 multigrid;
 *      otherwise the sparse LU), then per diode nodal_newton_dc's junction limiting vh^{j+1} = pnjlim(v, vh^j) and its
 *      convergence test, unchanged.  The step has converged when no diode fails; x_k is that iterate
 *   4. after convergence what a linear step runs after its solve: the inductor lane (i_k and J_{k+1} from x_k, once per
 *      step), probes, envelope, the kept solutions
 * A diode has no memory: method 0 / 1 change the capacitors' and inductors' companions only, and method 1 needs a DC
 * start as before.
 *   info_out [steps]              0 solved; 1 singular (nodal_transient's rule, dense != 0: NODAL_E_SINGULAR); 2 the
 *                                 step's Newton loop did not converge in max_iter iterations, met an iterate that is not
 *                                 finite, or a g that overflowed (then the diode rows of the value column hold 1.0 and G
 *                                 is assembled from it).  Info 1 or 2: that step and every later one have no state, NaN
 *                                 wherever they were to land, status OK.  The loop never hangs
 *   resid_out [steps]             the LARGEST scaled residual of the step's linear solves, one per Newton iteration
 *   iters_out [steps]             of the step's last linear solve
 *   newton_out [steps]            Newton iterations of the step (0: a step without a state that ran none)
 *   updates_out [steps]           iterations of the step whose matrix work ran (below)
 *   dv_out, di_out [steps + 1][ndprobe]  v and i(v) of the diodes dprobe_index [ndprobe] (indices into diode_rows) at x_k,
 *                                 row 0 from x0
 *   vh_final_out [ndiode]         the limited junction voltages after the last step's last iteration (steps == 0: v of
 *                                 x0); NaN when a step had no state
 * Each may be NULL.  Reuse: an iteration skips the assembly and all matrix work behind it when every diode's 1 / g has
 * exactly the bits of the value G was last assembled from (reverse-biased junctions: i_sat e / n_vt below half an ulp of
 * gmin); the factors or the hierarchy then stay, as in a linear step.  The lane that limits and tests a diode also
 * evaluates the next linearisation's 1 / g and counts the diodes whose bits moved into the record the loop reads anyway:
 * no host wait of its own.  The first iteration of a call always assembles, and so does the one after a converged
 * iteration in which the limiter changed a diode (vh^0 of the next step is then not that lane's vh').  NODAL_TNL_REUSE=0
 * (read per call) assembles in every iteration: the same bits.
 * ndiode == 0: nodal_transient_rlc's launches and bits, newton_out 1 per solved step, updates_out 0.  n == 0, steps == 0:
 * as nodal_transient_rlc.  No tape is kept (NODAL_OPT_TRANSIENT_TAPE: the adjoint with diodes is not implemented).
 * nodal_last_timings afterwards as nodal_newton_dc's: [0] host ms of the matrix work summed over all iterations, [1]
 * the symbolic part of it, exactly 0.0 when all of it was kept, [2] the whole call.
 * NODAL_E_INVALID: nodal_transient_rlc's and nodal_newton_dc's cases, and a dprobe_index entry outside [0, ndiode).
 * Host waits per Newton iteration: nodal_newton_dc's -- the assembly's status words (where it ran), what the solver looks
 * at, ONE read of the record.  Integer atomics only: a repeated call gives the same bits.  Afterwards the handle is as
 * nodal_newton_dc leaves it. */
int nodal_transient_nl(nodal_handle h, int32_t dense, int32_t steps, int32_t method, int64_t ncap, const int64_t *cap_rows,
                       int32_t nsrc, const int64_t *src_rows, const double *src_values, const double *x0, int32_t nprobe,
                       const int32_t *probe_a, const int32_t *probe_b, double *wave_out, int32_t keep_every, double *x_out,
                       double *pot_min, int32_t *pot_min_step, double *pot_max, int32_t *pot_max_step, double *resid_out,
                       int32_t *info_out, int32_t *iters_out, int64_t nind, const int64_t *ind_rows, const double *i0,
                       int32_t ncur, const int32_t *cur_index, double *cur_out, double *i_final_out, int64_t ndiode,
                       const int64_t *diode_rows, const double *i_sat, const double *n_vt, double gmin, int32_t max_iter,
                       double reltol, double vntol, double abstol, int32_t ndprobe, const int32_t *dprobe_index,
                       int32_t *newton_out, int32_t *updates_out, double *dv_out, double *di_out, double *vh_final_out);

/* ---- nonlinear transient analysis with bipolar transistors: Ebers-Moll in its transport form inside every time step
 *      (replaces the host loop nodal_transient_nl was written to replace: per Newton iteration per step a download of x,
 *      the lanes in numpy, an upload of a value column, an assembly and a solve) ----
 * nodal_transient_nl's arguments and rules, plus nodal_newton_dc_bjt's ntr transports: gm_rows [ntr][2], junction [ntr][2]
 * and i_s [ntr] mean what they mean there.  The handle's table holds one companion R row per capacitor, then per
 * inductor, then per diode -- the transistors' junctions among them, plain members of diode_rows / i_sat / n_vt -- and
 * behind them two rows of type NODAL_T_GM per transport, gm_rows[t][0] (forward) and gm_rows[t][1] (reverse): both with
 * the transport's leads a, b, and c, d = lead a, lead b of the row of diode junction[t][0] = jf, respectively
 * junction[t][1] = jr; their table values are overwritten.  NPN or PNP is the caller's choice of leads alone.
 * A step is nodal_transient_nl's: base_k formed ONCE per step and held fixed, vh^0 = v of x_{k-1} once per step for every
 * diode, and Newton iteration j linearises every diode as there and every transport at the SAME limited voltages
 * vhf = vh^j[jf], vhr = vh^j[jr] with nodal_newton_dc_bjt's formulas and roundings
 *   ef = exp(vhf / n_f),  er = exp(vhr / n_r),  gmf = (i_s ef) / n_f,  gmr = (i_s er) / n_r,  iT = i_s ef - i_s er
 *   JT = gmf vhf - gmr vhr - iT
 * gmf into the forward row's value, -gmr into the reverse row's, then the assembly and the solve of
 *   G x = base_k + S J + P JT
 * (JT injected into lead a, drawn from lead b): a node's right-hand side gets base_k, then the J of its diodes in
 * ascending order, then the JT of its transports in ascending order.  After the solve the diodes' limiting and test and
 * per transport nodal_newton_dc_bjt's test at the raw vf, vr of the new x.  The step has converged when no diode and no
 * transport fails; the inductor lane runs once per step after that.  A transport has no memory, no gmin and no limiting.
 * NO reuse with transports: a call with ntr > 0 assembles in EVERY Newton iteration, updates_out[k] == newton_out[k].
 * gmf carries no gmin floor, so its bits move whenever a junction voltage moves; a rule that compares bits would almost
 * never fire.  NODAL_TNL_REUSE changes nothing in such a call.
 *   info_out [steps]           nodal_transient_nl's; 2 also for a gmf or gmr that is not finite (an overflow: the diode
 *                              rows of the value column then hold 1.0 and the GM rows 0.0, G is assembled from them,
 *                              that step and every later one are NaN)
 *   tv_out [steps + 1][ntprobe][2]  the raw v_f, v_r of the transports tprobe_index [ntprobe] (indices into the
 *                              transports) at x_k, row 0 from x0
 *   ti_out [steps + 1][ntprobe][3]  i_f, i_r -- the junctions' i(v) at those voltages, gmin included -- and
 *                              iT = i_s exp(v_f / n_f) - i_s exp(v_r / n_r).  The terminal currents are the caller's sums
 *                              as nodal_newton_dc_bjt gives them: I_C = iT - i_r, I_B = i_f + i_r, I_E = -(iT + i_f) for
 *                              an NPN.  NaN in the rows of steps without a state
 *   vh_final_out [ndiode]      all ndiode limited voltages, the junctions among them
 * Each may be NULL.  The other outputs are nodal_transient_nl's.  Routes: n <= 64 the dense panel, otherwise the sparse
 * LU factored anew in every iteration on its kept analysis; never the multigrid route, because GM rows make the network
 * non-passive.  ntr == 0 is nodal_transient_nl: the same launches and the same bits (nodal_transient_nl IS this call
 * with ntr == 0).
 * NODAL_E_INVALID: nodal_transient_nl's cases; ntr < 0, ntprobe < 0, a NULL array with ntr > 0 or ntprobe > 0, ntprobe > 0
 * with ntr == 0; a gm_rows entry out of range or not of type NODAL_T_GM, two rows of a transport that do not share their
 * a, b, a row whose c, d are not the leads a, b of its junction's diode row, a junction index outside [0, ndiode), an
 * i_s that is not > 0 and finite; a tprobe_index entry outside [0, ntr).  The handle stays usable.
 * Host waits: once per call the diodes' check and the transports' check (one word each); per Newton iteration
 * nodal_transient_nl's and one more word behind the assembly's status words, when the stream has drained already (whether
 * a gmf or gmr overflowed).  The probe lanes wait for nothing.  Integer atomics only: a repeated call gives the same bits.
 * Afterwards the handle is as nodal_newton_dc_bjt leaves it: the value column holds 1 / g of the last linearisation in the
 * diode rows and gmf, -gmr in the GM rows (1.0 and 0.0 after an overflow), G, factors and analysis belong to it, the
 * solution is dropped, a recorded transient is void. */
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
                           const int32_t *tprobe_index, double *tv_out, double *ti_out);

/* ---- gradients through time (replaces finite differences over whole transient runs: two nodal_transient calls per
 *      component; with the reference each of them a host loop of rebuild and solve, reference nodal/nodal.py:306-336) ----
 * The adjoint of the backward-Euler run the handle has RECORDED: with NODAL_OPT_TRANSIENT_TAPE set, a nodal_transient call
 * with method 0 whose every step ended with info 0 leaves x_0 .. x_steps, its capacitor rows and its swept rows on the
 * handle.  The tape is void after nodal_assemble_numeric, after an upload and after any later nodal_transient call (which
 * replaces it if it records).  For a scalar loss of the probe waveforms, wave_cot[k][p] = dL / d wave[k][p]
 * ([steps + 1][nprobe]; the probes (probe_a[p], probe_b[p]) need not be those of the recorded call; a probe with
 * probe_a == probe_b contributes nothing) gives c_k = sum_p wave_cot[k][p] (e(a_p) - e(b_p)), and with M = G, S the
 * capacitors' incidence, r_i their companion rows' values, g = 1 / r and lambda_{steps+1} = 0:
 *   M^T lambda_k = c_k + S (g o S^T lambda_{k+1}),  k = steps .. 1     (the forward step run backwards, transposed)
 *   grad_out[i]               = sum_k s_i(lambda_k, x_k) for every table row i that is not a companion row, s_i the
 *                               per-row formula of nodal_gradient (cross terms included); at a swept row the sum over the
 *                               steps, nodal_gradient's convention
 *   grad_out[cap_rows[i]]     = sum_k (lambda_k(a) - lambda_k(b)) ((x_k(a) - x_k(b)) - (x_{k-1}(a) - x_{k-1}(b))) / r_i^2:
 *                               the derivative with respect to the companion value r_i = h / C_i, so that
 *                               dL/dC_i = -(h / C_i^2) grad_out[cap_rows[i]]
 *   grad_sources_out[k-1][j]  = s_{src_rows[j]}(lambda_k): the derivative with respect to src_values[k-1][j]
 *   grad_x0_out               = c_0 + S (g o S^T lambda_1) = dL/dx0 ([n]; zero in the branch rows)
 *   adjoint_out [steps][n]    lambda_1 .. lambda_steps
 *   resid_out [steps]         the scaled residual of M^T lambda_k = its right-hand side, as nodal_solve_sources defines it
 *   info_out [steps]          > 0: singular (the step and every EARLIER one: NaN in everything they feed and in the whole
 *                             of grad_out and grad_x0_out, status OK) -- except with dense != 0: NODAL_E_SINGULAR
 * grad_sources_out, grad_x0_out, adjoint_out and resid_out may be NULL.  steps == 0: zeros in grad_out, grad_x0_out = c_0;
 * n == 0: zeros.  Routes as nodal_transient's; B == 0 and all R > 0 (M symmetric) re-uses the hierarchy or factors the
 * forward run left, every other network solves with the transposed matrix, factored once and kept like the forward
 * run's.  The sum over the steps is formed on the device in one fixed order -- descending k, sixteen steps to a block
 * (csrc/transient_gradient.hip) -- and comes down once.  nodal_last_timings afterwards: [0] host ms of the matrix work
 * this call did once, exactly 0.0 when it was kept or not needed; [1] 0.0; [2] the whole call.
 * NODAL_E_INVALID: no valid tape on the handle; a probe node outside [-1, K).
 * Leaves the handle as it found it: the solution if any, the table, G, A, the tape, the kept hierarchy and factors -- a
 * second call with other cotangents repeats no matrix work.  No floating-point atomics: a repeated call gives the same
 * bits. */
int nodal_transient_gradient(nodal_handle h, int32_t dense, int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b,
                             const double *wave_cot /* [steps + 1][nprobe] */,
                             double *grad_out /* [ncomp] of this handle, companion rows included */,
                             double *grad_sources_out /* [steps][nsrc] of the recorded call, may be NULL */,
                             double *grad_x0_out /* [n], may be NULL */,
                             double *adjoint_out /* [steps][n], may be NULL */,
                             double *resid_out /* [steps], may be NULL */, int32_t *info_out /* [steps] */);

/* ---- AC analysis: frequency sweeps of RLC networks (replaces a transient run per frequency, long enough to settle, with
 *      an amplitude fit afterwards; on the host: G exported, G + j B formed and solved anew per frequency) ----
 * The steady state at each angular frequency omega [nfreq] (rad/s).  G (n x n, n = K + B) is that of the last
 * nodal_assemble_numeric.  The reactive elements are arguments, not table rows: kind [nreact] (0 a capacitor, 1 an
 * inductor), value (farads or henries), lead_a, lead_b (node indices, -1 ground).  A capacitor has the susceptance
 * b = omega C, an inductor b = -1 / (omega L); B(omega) stamps every element like a conductance of value b (+b at (a, a)
 * and (b, b), -b at (a, b) and (b, a), ground leads dropped), and the phasors solve
 *   (G + j B) (x_r + j x_i) = s_r + j s_i
 * as the real system of 2n unknowns interleaved by unknown (real part of unknown i at 2i, imaginary part at 2i + 1; entry
 * (i, j) the block [[g, -b], [b, g]]), on a child context kept on the handle.  The excitation is small-signal: every
 * independent source (A, E) is OFF except src_rows [nsrc] (each named once), which carry the complex amplitudes
 * src_re + j src_im [nsrc], constant over the sweep; s_r (s_i) is the right-hand side of the table with every A / E
 * value replaced by the real (imaginary) part of its amplitude.  Dependent sources stay in G.
 *   wave_out [nfreq][nprobe][2]    x(probe_a[p]) - x(probe_b[p]) as (re, im); probe_a == probe_b reads exactly +0.0
 *   cur_out [nfreq][ncur][2]       j b_q (x(a) - x(b)), the current from lead a to lead b through element
 *                                  q = cur_index[t] (an index into the reactive list)
 *   x_out [nfreq / keep_every][n][2]  the solution of every keep_every-th frequency (keep_every 0: none)
 *   peak_out [K]                   per node the largest |x| over the solved frequencies, peak_freq_out [K] the frequency
 *                                  index that attains it (among exact ties the lowest); NaN and -1 when none was solved
 *   resid_out [nfreq]              the scaled residual of the real system, as nodal_solve_sources defines it
 *   info_out [nfreq]               > 0: singular at that frequency (NaN in its rows only, later frequencies are solved,
 *                                  status OK) -- except with dense != 0, where it returns NODAL_E_SINGULAR
 * Each output may be NULL.  Routes: 2n <= 64 the dense panel; dense != 0 the dense LU at any size; everything else the
 * sparse LU, factored anew per frequency on the kept analysis, two substitutions, one refinement step and the judgement
 * (a frequency above the bar is redone by the sparse direct solve).  The child's pattern (the union of G's and the
 * elements' node pairs) and the symbolic analysis are kept per structure and set of (kind, lead_a, lead_b): a later
 * call with other values, frequencies, sources or probes repeats neither.  An entry's susceptances are added in list
 * order (capacitors ascending, then inductors ascending) by one lane, no atomics: a repeated call gives the same bits.
 * nodal_last_timings afterwards: [0] host ms of the pattern and the symbolic analysis this call did, exactly 0.0 when
 * both were kept; [1] the ms of the numeric factorisations, summed; [2] the whole call.
 * NODAL_E_INVALID: no nodal_assemble_numeric before the call, nfreq < 0, an omega that is not finite and > 0, a kind other
 * than 0 / 1, a value that is not finite and > 0, a lead outside [-1, K), both leads of an element on one node, the
 * source-row errors of nodal_solve_sources, a probe node outside [-1, K), a cur_index outside [0, nreact).  nfreq == 0
 * does nothing; n == 0 gives zeros.
 * Phasors, currents, peaks and residuals come down once, after the last frequency.  Leaves the handle as it found it:
 * the solution if any, the table, G, A, what the last solve reported, the transient tape, the kept hierarchy and
 * factors. */
int nodal_ac_sweep(nodal_handle h, int32_t dense, int32_t nfreq, const double *omega /* [nfreq], rad/s, > 0 */,
                   int64_t nreact, const uint8_t *kind /* 0 capacitor, 1 inductor */, const double *value /* F or H */,
                   const int32_t *lead_a, const int32_t *lead_b /* node indices, -1 ground */,
                   int32_t nsrc, const int64_t *src_rows, const double *src_re, const double *src_im,
                   int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b, double *wave_out /* [nfreq][nprobe][2] */,
                   int32_t ncur, const int32_t *cur_index /* into the reactive list */, double *cur_out /* [nfreq][ncur][2] */,
                   int32_t keep_every, double *x_out /* [nfreq / keep_every][n][2] */,
                   double *peak_out /* [K] */, int32_t *peak_freq_out /* [K] */,
                   double *resid_out /* [nfreq] */, int32_t *info_out /* [nfreq] */);

/* ---- noise analysis: thermal-noise spectra of RLC networks (replaces one nodal_ac_sweep per resistor with a unit current
 *      through it, read at the output: as many solves per frequency as the network has resistors; the reference has no
 *      equivalent) ----
 * A(omega) = G + j B(omega) exactly as nodal_ac_sweep defines it, with the same reactive-element arguments.  Output p is
 * the node pair (out_a[p], out_b[p]), -1 the ground node, and y_p solves
 *   A(omega)^T y_p = e(out_a[p]) - e(out_b[p])        (the plain transpose, not the conjugate transpose).
 * Every table row k of type R with assembled value R_k > 0 and leads (a, b) contributes
 *   c_k(f, p) = 4 k_B T / R_k |y_p(a) - y_p(b)|^2     V^2 / Hz, k_B = 1.380649e-23 J / K, T = temperature (kelvin, one for
 *                                                     the whole network), a ground lead reads +0.0;
 * a row with both leads on one node, every other row type and a resistor with R_k <= 0 are noiseless: exactly +0.0.
 *   density_out [nfreq][nout]      S_out(f, p) = sum_k c_k(f, p)
 *   gain_out [nfreq][nout][2]      H(f, p) = y_p^T s as (re, im), nothing conjugated: s is the right-hand side of the table
 *                                  with source input_row (an A or E row) at amplitude 1 and every other independent source
 *                                  off, the source stamp of nodal_ac_sweep.  The input-referred density is S_out / |H|^2.
 *   contrib_out [nout][ncomp]      C_k(p) = sum_f weight[f] c_k(f, p), accumulated on the device in frequency order (the
 *                                  caller's weights: the trapezoid rule over its frequencies in Hz); the
 *                                  [nfreq][nout][ncomp] array never exists.  NaN throughout when any frequency is singular.
 *   resid_out [nfreq][nout]        the scaled residual of every output's real system, as nodal_solve_sources defines it
 *   info_out [nfreq]               > 0: singular at that frequency (NaN in its rows only, later frequencies are solved,
 *                                  status OK) -- except with dense != 0, where it returns NODAL_E_SINGULAR
 * Each output array may be NULL.  No forward solution is needed or made.  The transposed system lives on a child context:
 * when G is symmetric (no branch rows, every R > 0) A^T = A and it is the child of nodal_ac_sweep itself, pattern and
 * symbolic analysis shared with it in both directions; otherwise a second child built from the G^T that
 * nodal_sensitivities keeps, kept under the same key (structure, kinds, leads).  Per frequency ONE numeric factorisation
 * whatever nout is.  Routes: 2n <= 64 the dense panel and dense != 0 the dense LU at any size, the outputs as columns of
 * one multi-right-hand-side solve; everything else the sparse LU, factored anew per frequency on the kept analysis, per
 * output two substitutions, one refinement step and the judgement (an output above the bar is redone by the sparse direct
 * solve).  Then one pass over the component table per block of sixteen outputs: a lane per row, the sums over the rows by
 * a fixed-order reduction (wave shuffles, LDS, a fold over the workgroups' partials).  No floating-point atomics: a
 * repeated call gives the same bits.
 * nodal_last_timings afterwards: [0] host ms of the pattern and the symbolic analysis this call did, exactly 0.0 when
 * both were kept; [1] the ms of the numeric factorisations, summed; [2] the whole call.
 * NODAL_E_INVALID: every argument error of nodal_ac_sweep (frequencies, elements), a temperature that is not finite and
 * > 0, an output node outside [-1, K), an input_row that is neither -1 nor an A / E row, gain_out without an input_row,
 * contrib_out without weight.  nfreq == 0 and nout == 0 do nothing; n == 0 gives zeros.
 * Densities, gains and residuals come down once, after the last frequency, the contributions once.  Leaves the handle as
 * it found it: the solution if any, the table, G, A, what the last solve reported, the transient tape, the kept
 * hierarchy and factors, the kept work of nodal_ac_sweep. */
int nodal_ac_noise(nodal_handle h, int32_t dense, int32_t nfreq, const double *omega /* [nfreq], rad/s, > 0 */,
                   int64_t nreact, const uint8_t *kind /* 0 capacitor, 1 inductor */, const double *value /* F or H */,
                   const int32_t *lead_a, const int32_t *lead_b /* node indices, -1 ground */,
                   double temperature /* K, finite, > 0 */,
                   int32_t nout, const int32_t *out_a, const int32_t *out_b /* node indices, -1 ground */,
                   int64_t input_row /* -1: none */, const double *weight /* [nfreq] or NULL */,
                   double *density_out /* [nfreq][nout] */, double *gain_out /* [nfreq][nout][2] */,
                   double *contrib_out /* [nout][ncomp] */, double *resid_out /* [nfreq][nout] */,
                   int32_t *info_out /* [nfreq] */);

/* ---- AC port analysis: the multiport impedance matrix Z(j omega) of an RLC network over a list of frequencies (replaces
 *      one nodal_ac_sweep per port with an A source across it -- a numeric factorisation per port and frequency, and the
 *      source has to be in the netlist already -- and nodal_port_matrix, which sees G alone, at DC; the reference has no
 *      equivalent) ----
 * A(omega) = G + j B(omega) exactly as nodal_ac_sweep defines it, with the same reactive-element arguments.  Port q is the
 * ordered node pair (ia[q], ib[q]), -1 the ground node (potential +0.0); s_q = e(ia[q]) - e(ib[q]), real, zeros in the
 * branch rows.  There is no other excitation: every independent source is off, the dependent ones stay in G.  x_q solves
 *   A(omega) x_q = s_q                                  (A itself, not its transpose)
 * and
 *   z_out [nfreq][nports][nports][2]   z[f][p][q] = x_q[ia[p]] - x_q[ib[p]] as (re, im): volts at port p per ampere
 *                                      entering ia[q] and leaving ib[q], the sign convention of nodal_port_matrix.  A port
 *                                      with ia == ib has a row and a column of exactly +0.0 in both parts; two identical
 *                                      ports are legal
 *   node_peak_out [K]                  per node i the largest |x_q(i)| over all ports and all solved frequencies -- the
 *                                      worst transfer impedance magnitude from any port to that node --,
 *   node_peak_port_out [K],            the port and the frequency index that attain it (among exact ties the lowest
 *   node_peak_freq_out [K]             frequency, then the lowest port); NaN / -1 / -1 when no frequency was solved.  |x|^2
 *                                      is compared and the root taken once at the end.  Made when any of the three is given
 *   resid_out [nfreq][nports]          the scaled residual of every column's real system, as nodal_solve_sources defines it
 *   info_out [nfreq]                   > 0: singular at that frequency (NaN in its rows only, later frequencies are solved,
 *                                      status OK) -- except with dense != 0, where it returns NODAL_E_SINGULAR
 *   work_out [3]                       counts made on the host: [0] numeric factorisations (the dense routes: one per chunk
 *                                      of 512 ports and frequency), [1] applications of the sparse factors to a block of up
 *                                      to sixteen columns, [2] columns redone alone
 * Each output array may be NULL.  The matrix is the one nodal_ac_sweep keeps on the handle: pattern and symbolic analysis
 * are shared with it in both directions, and with nodal_ac_noise wherever that shares with nodal_ac_sweep.  Routes:
 * 2n <= 64 the dense panel and dense != 0 the dense LU at any size, the ports as columns of one multi-right-hand-side
 * solve, up to 512 at a time, every group of sixteen judged; everything else the sparse LU, factored ONCE per frequency
 * whatever nports is, then per block of up to sixteen ports one substitution with sixteen interleaved right-hand sides,
 * the block's residual, a second substitution, the correction and the block judgement.  A column above the bar (the
 * NODAL_MULTI_BAR knob) -- every column when the factorisation replaced pivots -- is redone alone by the sparse direct
 * solve, and the factors are made anew afterwards.  The finished blocks are read at the port nodes on the device
 * (csrc/ac_ports.hip): nfreq x nports^2 complex numbers come down, once, after the last frequency, with the peaks and the
 * dense routes' residuals (the sparse route reads a block's residuals when it judges it).  No floating-point atomics: a
 * repeated call gives the same bits.
 * nodal_last_timings afterwards: as after nodal_ac_sweep -- [0] host ms of the pattern and the symbolic analysis this call
 * did, exactly 0.0 when both were kept; [1] the ms of the numeric factorisations, summed; [2] the whole call.
 * NODAL_E_INVALID: every argument error of nodal_ac_sweep (no nodal_assemble_numeric before the call, nfreq < 0,
 * frequencies, elements), nports < 0, a port node outside [-1, K).  nfreq == 0 and nports == 0 do nothing; n == 0 gives
 * zeros.
 * Leaves the handle as it found it: the solution if any, the table, G, A, what the last solve reported, the transient
 * tape, the kept hierarchy and factors, the kept work of nodal_ac_sweep and nodal_ac_noise. */
int nodal_ac_ports(nodal_handle h, int32_t dense, int32_t nfreq, const double *omega /* [nfreq], rad/s, > 0 */,
                   int64_t nreact, const uint8_t *kind /* 0 capacitor, 1 inductor */, const double *value /* F or H */,
                   const int32_t *lead_a, const int32_t *lead_b /* node indices, -1 ground */,
                   int32_t nports, const int32_t *ia, const int32_t *ib /* node indices, -1 ground */,
                   double *z_out /* [nfreq][nports][nports][2] */,
                   double *node_peak_out /* [K] or NULL */, int32_t *node_peak_port_out /* [K] or NULL */,
                   int32_t *node_peak_freq_out /* [K] or NULL */,
                   double *resid_out /* [nfreq][nports] or NULL */, int32_t *info_out /* [nfreq] or NULL */,
                   int64_t *work_out /* [3] or NULL */);

/* ---- gradients through frequency: the adjoint of the AC analysis (replaces central differences of nodal_ac_sweep, two
 *      sweeps per component, capacitor, inductor and amplitude; the reference has no equivalent) ----
 * A(omega) = G + j B(omega) exactly as nodal_ac_sweep defines it, with the same frequency, reactive-element, source and
 * probe arguments.  The forward system is A x_f = s, s from the driven rows src_rows with amplitudes alpha_j, every other
 * independent source off; probe p reads W[f][p] = x_f(a_p) - x_f(b_p).  For a real scalar loss L of the probe phasors the
 * caller passes the cotangent
 *   wave_cot [nfreq][nprobe][2]        g[f][p] = dL/dRe W[f][p] + j dL/dIm W[f][p] as (re, im), so dL = Re(sum conj(g) dW)
 * and nothing else is conjugated anywhere.  The adjoint system is
 *   c_f = sum_p conj(g[f][p]) (e(a_p) - e(b_p))         (added in probe order; probes may share nodes; a_p == b_p adds nothing)
 *   A(omega_f)^T y_f = c_f                              (the plain transpose, as nodal_ac_noise has it)
 * and dL = sum_f Re(y_f^T (ds - dA x_f)).  With X, L the complex x_f, y_f (+0.0 at a ground lead), D the difference of L
 * and U that of X over the leads the static adjoint (nodal_sensitivities) names for the row, m = K + k the branch unknown:
 *   table row R, value v               Re(D U) / v^2, plus for every CCVS / CCCS row j it drives
 *                                      Re(L(m_j) v_j (X(c_j) - X(d_j))) / v^2, in table order
 *   VCVS (VCCS) row                    Re(L(m) U)
 *   CCVS, CCCS row                     -Re(L(m) U) / Rd
 *   A, E row, a row without a term     exactly +0.0 (the small-signal excitation never reads the table value)
 *   capacitor C on (a, b)              omega Im(D U)
 *   inductor L on (a, b)               Im(D U) / (omega L^2)
 *   amplitude of driven row j          conj(D_j), D_j = L(a) - L(b) for an A row and L(m) for an E row, in g's convention
 * Outputs, each may be NULL:
 *   wave_out [nfreq][nprobe][2]        the forward phasors, as nodal_ac_sweep gives them
 *   grad_out [ncomp]                   dL/d(table value), summed over the frequencies on the device in ascending index
 *   grad_react_out [nreact]            dL/dC, dL/dL with respect to the values as passed, summed likewise
 *   grad_sources_out [nfreq][nsrc][2]  the term of each frequency (the amplitudes are constant over the sweep: the caller sums)
 *   adjoint_out [nfreq / keep_every][n][2]   y of every keep_every-th frequency (keep_every == 0: none)
 *   resid_out [nfreq][2]               the scaled residual of the forward and of the adjoint system
 *   info_out [nfreq]                   > 0: singular at that frequency -- NaN in its rows and in the whole of grad_out and
 *                                      grad_react_out, status OK -- except with dense != 0, where it returns NODAL_E_SINGULAR
 *   work_out [3]                       as nodal_ac_ports counts it: numeric factorisations, block applications, columns
 *                                      redone alone
 * Routes: a symmetric G (no branch rows, every R > 0) has A^T = A, and s and c_f are two columns of ONE factorisation per
 * frequency on the matrix nodal_ac_sweep keeps; every other network solves one column there and one on the transposed
 * matrix nodal_ac_noise keeps, two factorisations per frequency.  Pattern and symbolic analysis are shared with
 * nodal_ac_sweep, nodal_ac_noise and nodal_ac_ports in both directions.  2n <= 64 the dense panel, dense != 0 the dense LU,
 * everything else the sparse LU with nodal_ac_ports' refinement, judgement and redo of a column above the bar.  The table
 * pass runs on the device (csrc/ac_gradient.hip), one lane per row, no floating-point atomics: a repeated call gives the
 * same bits.  Phasors, source terms and residuals come down once after the last frequency, the gradients once.
 * nodal_last_timings afterwards: as after nodal_ac_sweep.
 * NODAL_E_INVALID: every argument error of nodal_ac_sweep, a probe node outside [-1, K), wave_cot == NULL with nfreq > 0
 * and nprobe > 0, a cotangent that is not finite.  nfreq == 0, nprobe == 0 and n == 0 give zeros in the gradients.
 * Leaves the handle as it found it, the kept work of nodal_ac_sweep, nodal_ac_noise and nodal_ac_ports included. */
int nodal_ac_gradient(nodal_handle h, int32_t dense, int32_t nfreq, const double *omega /* [nfreq], rad/s, > 0 */,
                      int64_t nreact, const uint8_t *kind /* 0 capacitor, 1 inductor */, const double *value /* F or H */,
                      const int32_t *lead_a, const int32_t *lead_b /* node indices, -1 ground */,
                      int32_t nsrc, const int64_t *src_rows, const double *src_re, const double *src_im,
                      int32_t nprobe, const int32_t *probe_a, const int32_t *probe_b /* node indices, -1 ground */,
                      const double *wave_cot /* [nfreq][nprobe][2] */, double *wave_out /* [nfreq][nprobe][2] or NULL */,
                      double *grad_out /* [ncomp] or NULL */, double *grad_react_out /* [nreact] or NULL */,
                      double *grad_sources_out /* [nfreq][nsrc][2] or NULL */, int32_t keep_every,
                      double *adjoint_out /* [nfreq / keep_every][n][2] or NULL */,
                      double *resid_out /* [nfreq][2] or NULL */, int32_t *info_out /* [nfreq] or NULL */,
                      int64_t *work_out /* [3] or NULL */);

/* ---- multiport Thevenin / Norton equivalents (replaces a loop of equivalent_resistance over node pairs, reference
 *      nodal/equiv.py:31-61: one rebuild and solve per pair, resistive networks only, the number R(a, b) alone; the
 *      reference has no equivalent of an active network and no coupling between ports) ----
 * Port q is the ordered node pair (ia[q], ib[q]), either may be the ground node (-1, potential +0.0).  With G the matrix
 * of the last nodal_assemble_numeric and s_q = e(ia[q]) - e(ib[q]) (zeros in the branch rows), x_q solves G x_q = s_q --
 * G itself, not its transpose; the independent sources are off, the dependent ones stay -- and
 *   z_out[p][q] = x_q[ia[p]] - x_q[ib[p]]   volts at port p per ampere entering ia[q] and leaving ib[q] (the sign of
 *                                           nodal_solve_pairs), [nports][nports] row-major;
 *   voc_out[p]  = x[ia[p]] - x[ib[p]]       for the solution x of the single solve on the handle (may be NULL),
 * so that v = voc + z i for any currents i driven into the ports from outside.  A port with ia == ib has an all-zero row
 * and column, exactly.  The solves are those of nodal_solve_sources (one factorisation or one multigrid hierarchy, sixteen
 * ports to a block) and the finished blocks are read at the port nodes on the device (csrc/ports.hip): nports^2 numbers
 * come down, not nports x n.
 * resid_out [nports] = the scaled residual of column q as nodal_solve_sources defines it (may be NULL); info_out [nports]:
 * > 0 a singular network (column q is NaN in every row, status OK) -- except with dense != 0, where a singular G
 * returns NODAL_E_SINGULAR.  NODAL_E_INVALID: a node index outside [-1, K), no nodal_assemble_numeric before the call,
 * voc_out without a solution on the handle (as nodal_branches).  nports == 0 does nothing; n == 0 gives zeros.
 * Leaves the handle as it found it: the solution (if any), the table, G, A and what the last solve reported.  No
 * floating-point atomics: a repeated call gives the same bits. */
int nodal_port_matrix(nodal_handle h, int32_t dense, int32_t nports, const int32_t *ia, const int32_t *ib,
                      double *z_out /* [nports][nports] row-major */, double *voc_out /* [nports], may be NULL */,
                      double *resid_out /* [nports], may be NULL */, int32_t *info_out /* [nports] */);

/* scaled residual ||G x - A||_inf / (||G||_inf ||x||_inf + ||A||_inf) of the
 * solution currently on the device, computed on the device from the CSR form */
int nodal_residual(nodal_handle h, double *scaled_residual);

/* ---- whole-path entry for resident inputs --------------------------------
 * symbolic + numeric (member) + solve, nothing copied to the host.
 * dense != 0 selects the dense path.  Used by bench.py's timed region. */
int nodal_run(nodal_handle h, int32_t dense, int32_t member, int32_t reuse_symbolic,
              int32_t *info);

/* ---- batch variant (BASELINE.json config 4) -----------
 * Replaces a Python loop of `Circuit(netlist, sparse=True)` + `.solve()` (reference
 * nodal/nodal.py:306-336) over the members [first, first + count) of the value table
 * uploaded by nodal_upload_values: the members are assembled and solved on the device as
 * ONE block-diagonal system built from the single topology in HBM (sparse path).
 * x_out (may be NULL: results stay on the device, see nodal_batch_x_device) receives
 * count x n doubles, row m = unknown vector of member first + m.  info_out (may be NULL)
 * receives one int per member: 0 solved; > 0 singular network (row of NaNs, as the
 * reference's spsolve); < 0 minus the nodal_status the member's assembly failed with
 * (NODAL_E_ZERO_RESISTANCE, NODAL_E_STAMP_COLLISION; row of NaNs).  When the block system
 * cannot be solved as a whole the members are solved one by one, so only the offending
 * members are marked.  reuse_symbolic != 0 keeps the block pattern of the previous call
 * with the same topology and count. */
int nodal_run_batch(nodal_handle h, int32_t first, int32_t count, int32_t reuse_symbolic,
                    double *x_out, int32_t *info_out);
/* copy the count x n results of the last nodal_run_batch into DEVICE memory of the handle's
 * GPU (e.g. the send buffer of a collective); capacity_bytes is the size of that buffer */
int nodal_batch_x_device(nodal_handle h, void *device_dst, int64_t capacity_bytes);
/* the same for the n unknowns of the last single-circuit solve (nodal_solve_dense / nodal_solve_sparse /
 * nodal_run): x of an independent circuit into the send buffer of the all_gather that shares the ranks'
 * solutions (nodal_amd/batch.py ShardedCircuits; the D2D counterpart of nodal_download_x, which replaces the
 * host array the reference's Circuit.solve returns, reference nodal/nodal.py:336).  Returns when the copy is done. */
int nodal_x_device(nodal_handle h, void *device_dst, int64_t capacity_bytes);

/* ---- timing of the last call, measured with HIP events on the handle's
 *      stream: milliseconds spent in [symbolic, numeric, factor/solve] ----- */
int nodal_last_timings(nodal_handle h, double *ms3);
/* HIP-event duration (ms) and launch count of the dominant kernel class of the
 * last solve (SpMV for the iterative path, trailing GEMM update for dense LU) */
int nodal_last_kernel_stats(nodal_handle h, double *ms_total, int64_t *launches,
                            double *alg_bytes_or_flops);

/* iterations of the last sparse solve (0 for direct paths), multigrid levels used
 * and the solver's own relative residual estimate */
int nodal_last_solve_info(nodal_handle h, int32_t *iterations, int32_t *amg_levels,
                          double *relative_residual);

int nodal_synchronize(nodal_handle h);

/* ---- options -------------------------------------------------------------
 * NODAL_OPT_FORCE_PIVOTING (0/1): dense LU always searches pivots, even on
 *   passive networks (column diagonally dominant G) where it provably never swaps.
 * NODAL_OPT_GEPP_PANEL (0/1, default 1): partial pivoting factors a 32-column panel in one launch
 *   (registers) instead of two launches per column; both forms give the same bits (cross-check).
 * NODAL_OPT_EXTRA_STREAMS (0/1, default 0; environment NODAL_EXTRA_STREAMS): a handle that is used ALONE -- one
 *   handle in the process, one call at a time -- may spread independent pieces of a solve over streams of its own
 *   (the multigrid setup builds R beside A P, the direct factorisation runs the wide fronts of a level side by
 *   side).  Same kernels, same results.  Off by default: the runtime maps a process's streams onto a handful of
 *   hardware queues, and a second stream per handle makes the main streams of several handles share them.
 * NODAL_OPT_BORROW_TABLE (0/1, default 0): the caller promises that the columns it passes to
 *   nodal_upload_components stay valid and unchanged until the next upload or nodal_destroy.  The library then reads
 *   them in place where its host code needs the table (the presolve of systems with branch equations looks at the
 *   branch rows and at the rows touching an eliminated node) instead of keeping a copy of its own: the upload of a
 *   table with branches is DMA only.  nodal_amd/_ffi.py sets it (its Handle keeps the arrays alive).
 * NODAL_OPT_TRANSIENT_TAPE (0/1, default 0): a backward-Euler nodal_transient call keeps its states on the handle for
 *   nodal_transient_gradient, [steps + 1][n] doubles of device memory (a tape that does not fit is NODAL_E_NOMEM).  With
 *   0 nodal_transient allocates nothing more and does exactly what it did. */
enum {
    NODAL_OPT_FORCE_PIVOTING = 1, NODAL_OPT_GEPP_PANEL = 2, NODAL_OPT_EXTRA_STREAMS = 3, NODAL_OPT_BORROW_TABLE = 4,
    NODAL_OPT_TRANSIENT_TAPE = 5
};
int nodal_set_option(nodal_handle h, int32_t option, int32_t value);

/* ---- testing hooks (not part of the reference-facing surface) -------------
 * C[M x N] -= A[M x K] * B[K x N] on the device with the LU's trailing-update
 * kernel; host buffers, column-major, leading dimensions M, K, M. */
int nodal_debug_gemm(nodal_handle h, int32_t M, int32_t N, int32_t K, const double *A,
                     const double *B, double *C);
/* The dense path's pieces on host arrays of the caller's choosing (column-major): copied into the handle's scratch WITH
 * their padding rows, handed to the production function, copied back.  No arithmetic and no environment knob of their own.
 *
 * nodal_debug_gemm_ex: every entry point of gemm_f64.hip with the caller's leading dimensions.
 *   kind 0: gemm_f64 -- C (op)= A B, A: lda x K, B: ldb x N, C: ldc x N; mode 0 C -= A B, 1 C = A B, 2 C = -A B.
 *   kind 1: gemm_sub_tn_upper_f64 -- C -= At^T B for the upper block triangle of C, the diagonal blocks of `band` rows
 *           (a multiple of 128) whole; A is the K x M panel At (lda >= K, M columns); mode must be 0.
 *   kind 2: gemm_pair_f64 -- the first problem and (M2 .. ldc2) a second one in one launch, both in `mode`.
 *   C (and C2) come back whole, padding rows included.  band is read by kind 1 only, the second problem by kind 2 only. */
int nodal_debug_gemm_ex(nodal_handle h, int32_t kind, int32_t mode, int32_t band, int32_t M, int32_t N, int32_t K,
                        const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int32_t M2,
                        int32_t N2, int32_t K2, const double *A2, int64_t lda2, const double *B2, int64_t ldb2, double *C2,
                        int64_t ldc2);
/* nodal_debug_block_inverse: the block elimination's inverse of a diagonal block (block_elim.hip: one Gauss-Jordan
 *   workgroup up to w = 128, the 2 x 2 Schur formula above, 1 <= w <= 512) on A (lda x w).  Q (ldq x w) goes up as the
 *   caller filled it and comes back with the inverse in its leading w rows; *dinfo_out is 0 or `base` + the 1-based column
 *   of the first zero (or NaN) pivot.  variant: 0 rank-16 steps with DPP lane exchanges (the default form), 1 rank-16
 *   steps with bpermute exchanges (NODAL_GJ_DPP=0), 2 rank-4 steps (NODAL_GJ_SCALAR=2), 3 scalar steps (NODAL_GJ_SCALAR=1).
 *   The handle's own choice is put back afterwards. */
int nodal_debug_block_inverse(nodal_handle h, int32_t w, const double *A, int64_t lda, int32_t base, int32_t variant,
                              double *Q, int64_t ldq, int32_t *dinfo_out);
/* nodal_debug_dense_solve: dense_factor_solve_multi on A (n x n, leading dimension n) and B (n x nrhs) without any
 *   stamping, in the library's padded panel (padding rows filled with NaN).  route: the flags the dispatcher reads, set for
 *   this call and put back afterwards -- bit 0 passive (symmetric positive definite: no pivoting; above 256 unknowns the
 *   symmetric block elimination), bit 1 optimistic (no pivoting, the full block elimination), bit 2 force pivoting.
 *   X (n x nrhs), *info_out as dgesv.  ipiv_out[n]: the caller passes the identity 0 .. n-1; it comes back as the
 *   0-based LAPACK interchange list (row c was swapped with row ipiv[c]) of the pivoting routes and untouched otherwise.
 *   Overwrites the handle's dense panel and pivots (scratch of every dense solve); the table, the assembled system and
 *   the solution stay. */
int nodal_debug_dense_solve(nodal_handle h, int32_t n, int32_t nrhs, int32_t route, const double *A, const double *B,
                            double *X, int32_t *info_out, int32_t *ipiv_out);
/* the rhs columns nodal_solve_sources builds for the same arguments, [count][n] row-major */
int nodal_debug_sources_rhs(nodal_handle h, int32_t count, int32_t nsrc, const int64_t *rows,
                            const double *values, double *rhs_out);
/* The library's two residual judges -- the code behind nodal_residual and behind every resid_out / info_out of the
 * sweeps and the sensitivities -- on host vectors of the caller's choosing, which need not solve anything.
 * cols == 0: the single-vector judge on x[n], b[n] (b == NULL: the assembled right-hand side; layout must be 0).
 *   scaled_out[1]; norms_out[5] = {max|Gx-b|, max row sum |G|, max|x|, max|b|, poison flag} as the kernel leaves them.
 * cols 1 .. 16: the block judge on `cols` columns, element (i, y) of x and of b at [i * rs + y * cs]:
 *   layout 0: [cols][n] rows (rs 1, cs n); 1: interleaved [n][16] (rs 16, cs 1); 2: one shared column (rs 1, cs 0;
 *   cols must be 1).  scaled_out[cols]; norms_out[16 * 4]: per column y {max|b-Gx|, max|x|, max|b|} at [4y .. 4y+2],
 *   and the max row sum |G| at [3].
 * transposed != 0: against the G^T that the last nodal_sensitivities left on a handle whose network is not passive
 *   (its values are those of that call); b must be given.  NODAL_E_INVALID when the handle holds none.
 * Needs nodal_assemble_numeric (NODAL_E_INVALID otherwise, as for any other combination of cols and layout).  Leaves
 * the handle as it found it: solution, right-hand side, table, hierarchies and factorisations; scratch of its own. */
int nodal_debug_residual(nodal_handle h, int32_t transposed, int32_t cols, int32_t layout, const double *x,
                         const double *b, double *scaled_out, double *norms_out);
/* The sparse direct route's factors and substitutions with nothing behind them: slu_factor (which keeps a still-valid
 * analysis as usual), then exactly ONE application of the factors to the caller's r -- no Krylov step, no refinement,
 * no redo of a column by another path.  What every public entry point returns has been through one of those.
 * transposed == 0: the handle's G.  != 0: the G^T that the last nodal_sensitivities left on a handle whose network is
 *   not passive (the rule and the error of nodal_debug_residual).
 * cols == 1: slu_apply on r[n], z[n].  cols == 16: slu_apply_multi on sixteen columns interleaved by row, element (i, y)
 *   of r and of z at [i * 16 + y].  Anything else is NODAL_E_INVALID.
 * perturbed_out: the pivots the factorisation replaced (static-pivot rule); info_out: slu_factor's verdict (> 0:
 *   structurally singular; z is not written then).
 * Needs nodal_assemble_numeric (NODAL_E_INVALID otherwise).  Host vectors, scratch of its own; leaves solution,
 * right-hand side, table and hierarchies as it found them.  The direct route's cached analysis and factors of the
 * matrix in question ARE created or refreshed (as any direct solve would leave them). */
int nodal_debug_direct_apply(nodal_handle h, int32_t transposed, int32_t cols, const double *r, double *z,
                             int64_t *perturbed_out, int32_t *info_out);
/* The smoothed-aggregation hierarchy (csrc/sagg.hip) as the last setup or values-only refresh left it, raw: what the
 * tests compare level by level with an fp64 host reference of the setup's algebra (tests/hierarchy_reference.py).
 * The hierarchy is the handle's own or, when that holds none, the one of its presolved (branch-free) system.
 * Both calls are stream waits and device-to-host copies only: nothing is launched, nothing on the device is written,
 * the handle is left as found.  NODAL_E_INVALID when the handle holds no ready hierarchy.
 * nodal_debug_hierarchy_info: *nlev levels (<= 12); ints[l * 16 + k] per level l:
 *   0 n, 1 ld, 2 nc (rows of the next level; 0 on the last), 3 width (slots allocated for A), 4 maxlen (longest row),
 *   5 wfix (> 0: rows zero-padded to this many slots), 6 nnz, 7 rld, 8 rcap (row cap of R), 9 wslots, 10 fold_want (the
 *   setup wrote W), 11 fold (the cycle uses W), 12 d16 (adcol exists), 13 in_tail (the level runs inside the tail
 *   kernel), and -- the same on every level -- 14 refreshed (the last setup was a values-only refresh), 15
 *   dense_coarsest (coarse_inv exists).  reals[l * 2] = the prolongator's smoothing weight of level l, reals[l * 2 + 1]
 *   = the smoother's weight (the one in W).
 * nodal_debug_hierarchy_array: one device buffer of one level as raw bytes in the layout the kernels use: A, P and W
 *   column-major ELL (slot s of row i at [s * ld + i]), R in blocks of eight (entry t of coarse row I at
 *   [((t >> 3) * rld + I) * 8 + (t & 7)]), adcol int16 column - row.  *bytes_out = the extent the setup addresses:
 *   width*ld items for acol / aval / avalf / adcol, 4*ld for pcol / pval / pvalf, rcap*rld for rcol / rval / rvalf,
 *   wslots*ld for wcol / wval, n for alen / dinv / agg / wlen, nc for rlen; slots the setup does not write (past a row's
 *   padding, rows n .. ld) hold whatever the buffer held.  A buffer the level does not have (no next level, no W, no
 *   adcol) gives 0.  The one level that visits in three launches (directly above the dense tail) also has P2 = W -
 *   w D^-1 (A W): p2col / p2val (f32) 64*ld items laid out like W, p2len n, and d2 = P2^T dense, nc x ld row-major f32
 *   (zeros outside P2's pattern); 0 on every other level.  A level whose visit forms rc = W^T b also has W^T by coarse
 *   row: wtstart nc + 1 row starts (u32), and wtcol (fine row, ascending within a row) / wtval (f32, the bits of W's
 *   entry) / wtsrc (that entry's position slot * ld + row in wval), each 16*n items of which the first wtstart[nc] are
 *   written; 0 on every other level.  level == -1: coarse_inv, n_last x n_last row-major (`which` is ignored).  dst == NULL: the size
 *   only; otherwise capacity_bytes must cover it. */
enum {
    NODAL_HA_ACOL = 0, NODAL_HA_AVAL = 1, NODAL_HA_AVALF = 2, NODAL_HA_ALEN = 3, NODAL_HA_DINV = 4, NODAL_HA_ADCOL = 5,
    NODAL_HA_AGG = 6, NODAL_HA_PCOL = 7, NODAL_HA_PVAL = 8, NODAL_HA_PVALF = 9, NODAL_HA_RCOL = 10, NODAL_HA_RVAL = 11,
    NODAL_HA_RVALF = 12, NODAL_HA_RLEN = 13, NODAL_HA_WCOL = 14, NODAL_HA_WVAL = 15, NODAL_HA_WLEN = 16,
    NODAL_HA_P2COL = 17, NODAL_HA_P2VAL = 18, NODAL_HA_P2LEN = 19, NODAL_HA_D2 = 20,
    NODAL_HA_WTSTART = 21, NODAL_HA_WTCOL = 22, NODAL_HA_WTVAL = 23, NODAL_HA_WTSRC = 24
};
int nodal_debug_hierarchy_info(nodal_handle h, int32_t *nlev, int64_t *ints /* [12][16] */, double *reals /* [12][2] */);
int nodal_debug_hierarchy_array(nodal_handle h, int32_t level, int32_t which, void *dst, int64_t capacity_bytes,
                                int64_t *bytes_out);
/* ONE application of the multigrid cycle (csrc/sagg.hip cycle(), csrc/sagg_multi.h m_cycle()) to the caller's vector,
 * with no Krylov step behind it: what tests/cycle_reference.py states in numpy and tests/test_gpu_cycle.py compares.
 * The hierarchy is the one nodal_debug_hierarchy_info finds, as the last solve left it (sweep counts and K-cycle
 * switches included: no knob is read here); vectors have level 0's n entries (ints[0] of that call).
 * mode 0: the general route's call -- the start iterate w D^-1 r, then the cycle from f64 r to f64 z.
 * mode 1: the flexible CG's call -- the same cycle with f32 z (returned widened), whose last sweep also leaves the
 *   partial sums of z.r and z.u; dots_out[2] = those arrays summed in the order the iteration sums them.  A level 0
 *   with one sweep per side keeps its unfolded launches in this mode.
 * mode 2: the block iteration's call on sixteen columns interleaved by row, element (i, y) of r, u and z at
 *   [i * 16 + y]; dots_out[2][16] = the block's totals of z.r and z.u per column.  The block cycle runs at most two
 *   sweeps per side (a count of three from NODAL_SA_NU gives two) and folds nothing.
 * u: required in modes 1 and 2 (it stands where the iteration keeps A p), ignored in mode 0.
 * frozen == NULL: an adaptive K-cycle that leaves no sample.  Otherwise the caller's (s1, s2, t) -- three doubles,
 *   [16][3] in mode 2 -- are written where the frozen launches read them and the cycle runs frozen: r2 = rc - t A_c c1,
 *   correction P (s1 c1 + s2 c2); that cycle is linear in r.  Ignored where level 0 does not hand over through the
 *   K-cycle (params_out[10] says whether it was used).
 * params_out[16]: what the call ran with -- 0..2 sweeps at level 0 / 1 / deeper, 3 the tail's sweeps, 4 kcycle,
 *   5 klevels, 6 tail (first level inside the tail, -1 none), 7 tail_dense, 8 nlev, 9 level 0 took the folded
 *   prolongation in this mode, 10 frozen coefficients used, 11 the block's columns (16), 12 / 13 / 14 bit l: level l
 *   folds its first post-smoothing sweep / restricts from its right-hand side / visits in three launches, 15 the
 *   hierarchy was set up by the general route.
 * NODAL_E_INVALID: no ready hierarchy, an unknown mode, a missing u, or a hierarchy without a level outside the tail
 *   (where the block driver declines as well).  Host vectors; scratch of its own or the cycle's; launches no kernel a
 *   solve does not launch.  Leaves solution, right-hand side, table, hierarchy arrays, factorisations and the K-cycle's
 *   calibration state as it found them: a solve after it returns the bits of the same solve without it. */
int nodal_debug_cycle_apply(nodal_handle h, int32_t mode, const double *r, const double *u, const double *frozen,
                            double *z, double *dots_out /* [2] or [2][16] */, int32_t *params_out /* [16] */);
/* The plain-aggregation hierarchy (csrc/amg.hip: pairwise matching, aggregate-block smoother, K-cycle, LDS-resident
 * tail) -- the one that takes what the smoothed hierarchy declines -- as the last setup left it, raw, and ONE application
 * of its cycle: what tests/amg_reference.py states in numpy / scipy and tests/test_gpu_amg.py compares.  The hierarchy is
 * the handle's own or, where the handle holds none, the one on the context of its reduced system (presolve or low-degree
 * elimination, round after round).  NODAL_E_INVALID when the last sparse solve did not precondition with it (a dense or
 * direct solve, one the smoothed hierarchy took, a matrix assembled anew since): level 0 aliases the context's CSR
 * arrays, so a hierarchy is exported only while it is the live one.
 * nodal_debug_amg_info: *nlev levels (<= 16); ints[l * 8 + k] per level l: 0 n, 1 nnz, 2 nc (rows of the next level; 0
 *   on the last), 3 block (the level smooths with the aggregates' block inverses), 4 in_tail (the level runs inside the
 *   tail kernel).  words[16]: 0 tail (first level inside the tail kernel, -1 none), 1 kmax, 2 coarse_direct (coarse_inv
 *   exists), 3 block_smoother, 4 sweeps0, and the constants 5 BLOCK_MAX, 6 COARSEST_MAX, 7 K_MIN_ROWS,
 *   8 SPLIT_PROLONG_MIN, 9 DOT_BLOCKS, 10 the tail's LDS budget in bytes, 11 STREAM_CAP, 12 LONG_PART, 13 the most
 *   levels a tail holds.  reals[2]: theta (matching threshold), OMEGA (smoother weight).  tail[128], all zero without a
 *   tail: 0 nlev, 1 o_inv, 2 o_C1, 3 o_V1, 4 image_bytes, 5 total_bytes, and per tail level k at [8 + 14 k]: n, nnz, nc,
 *   o_data, o_dinv, o_indptr, o_memptr, o_indices, o_agg, o_mem, o_B, o_X, o_E, o_R (byte offsets into the tail's LDS;
 *   the image is its first image_bytes).
 * nodal_debug_amg_array: one device buffer of one level as raw bytes: the CSR matrix indptr (i32, n + 1) / indices (i32)
 *   / data (f64), dinv (f64, n), agg (i32, n: node -> aggregate), memptr (i32, nc + 1) / mem (i32, n: aggregate ->
 *   members), boff (u32, nc + 1: where each aggregate's block starts in binv, in doubles) and binv (the inverses of the
 *   aggregates' diagonal blocks, m x m in member order, TRANSPOSED; an aggregate above BLOCK_MAX members holds its m
 *   diagonal reciprocals).  A buffer the level does not have (agg / memptr / mem on the last level, boff / binv without
 *   the block smoother) gives 0.  level == NODAL_AMG_LEVEL_COARSE_INV: coarse_inv, n_last x n_last row-major;
 *   NODAL_AMG_LEVEL_TAIL_IMAGE: the packed image the tail kernel copies into LDS (`which` is ignored for both).
 *   dst == NULL: the size only; otherwise capacity_bytes must cover it.  Both calls are stream waits and device-to-host
 *   copies only: nothing is launched, nothing on the device is written.
 * nodal_debug_amg_apply: exactly one cycle(level) from r to z -- host vectors of that level's n entries -- for a level
 *   outside the tail; level 0 is the preconditioner's own call (one level only: z = dinv r).  params_out[16]: 0 nlev,
 *   1 tail, 2 kmax, 3 coarse_direct, 4 block_smoother, 5 sweeps0, 6 level, 7 the level smooths by blocks, 8 its coarse
 *   solve (0: none, the last level -- dense inverse or Jacobi; 1: the tail kernel; 2: direct / plain V hand-over; 3:
 *   two-step K-cycle), 9 the partial sums per dot product behind the correction's coefficients (0: s1 = 1, s2 = 0),
 *   10 prolongation in a launch of its own, 11 two Jacobi sweeps per side.  NODAL_E_INVALID also for an unknown level or
 *   one inside the tail.  Scratch of its own or the cycle's, no kernel a solve does not launch; solution, right-hand
 *   side, hierarchy arrays and factorisations stay as found: a solve after it returns the bits of the same solve
 *   without it. */
enum {
    NODAL_AA_INDPTR = 0, NODAL_AA_INDICES = 1, NODAL_AA_DATA = 2, NODAL_AA_DINV = 3, NODAL_AA_AGG = 4,
    NODAL_AA_MEMPTR = 5, NODAL_AA_MEM = 6, NODAL_AA_BOFF = 7, NODAL_AA_BINV = 8
};
enum { NODAL_AMG_LEVEL_COARSE_INV = -1, NODAL_AMG_LEVEL_TAIL_IMAGE = -2 };
int nodal_debug_amg_info(nodal_handle h, int32_t *nlev, int64_t *ints /* [16][8] */, int64_t *words /* [16] */,
                         double *reals /* [2] */, int64_t *tail /* [128] */);
int nodal_debug_amg_array(nodal_handle h, int32_t level, int32_t which, void *dst, int64_t capacity_bytes,
                          int64_t *bytes_out);
int nodal_debug_amg_apply(nodal_handle h, int32_t level, const double *r, double *z, int32_t *params_out /* [16] */);
/* The general route's restarted flexible GMRES and its block preconditioner (csrc/sparse_general.hip) with nothing
 * behind them: what tests/fgmres_reference.py states in numpy and tests/test_gpu_fgmres.py compares.
 * nodal_debug_fgmres_cycle: the production setup, then exactly ONE restart cycle of the production function -- no outer
 *   loop, no verdict, no presolve, no rescue by another solver.  No knob is read: the cycle runs with the arguments.
 *   system 0: the handle's assembled G, branch rows included.  1: the presolved, branch-free system the last sparse solve
 *     left on the reduced context (the rule of nodal_debug_hierarchy_info); NODAL_E_INVALID when there is none.
 *   precond 0: the block preconditioner (node block + multigrid + Schur diagonal), set up by the production setup.
 *     1: the sparse direct factors -- slu_factor, then slu_apply per column, as the refinement behind every sparse direct
 *     solve does; only with system 0.
 *   window 2 .. 41: column j is orthogonalised against v_s0 .. v_j, s0 = max(0, j + 1 - window).  max_cols 1 .. 40.
 *   rel_tol >= 0: the cycle stops once the estimate is <= rel_tol |b|; 0 never stops on the estimate.
 *   n: the system's unknowns as the caller sized its vectors (NODAL_E_INVALID when the system has another count).
 *   b: a host vector of n entries, or NULL for that system's own right-hand side.
 *   Returns x [n]; V [(count + 1)][n] and Z [count][n] without the device's row padding (capacity: (max_cols + 1) n
 *   and max_cols n; after a stop on the estimate row `count` of V holds what the buffer held: the kernel that scales
 *   v_count returns once the flag is up);
 *   gst [NODAL_FG_WORDS], the small least-squares problem as the device holds it (enum below: H row-major [41][40] with
 *   R = Q^T H-bar on and above the diagonal, the rotations, g, and the scalars); y [41], zero from `count` on;
 *   norms_out[2] = |b - A x| at the cycle's end and |b|, as the device summed them; params_out[16]: 0 n, 1 K (rows of
 *   the node block; n under precond 1), 2 ld (the device's row stride of V and Z), 3 count (columns run), 4 the window
 *   used, 5 use_sa (the smoothed hierarchy took the node block; else plain aggregation), 6 ell_spmv (the Krylov SpMV
 *   ran on the hierarchy's ELL copy), 7 the hierarchy's levels, 8 gd (workgroups of the dot-product kernels), 9 the
 *   cycle's breakdown flag (x is not updated then).  A zero b returns x = 0 and count 0 with nothing launched after
 *   the norm of b; V and Z are not written.
 *   NODAL_E_INVALID: arguments out of range, no such system, a matrix the setup finds singular.  Host vectors; the
 *   iterate and b live in scratch of the hook's own.  Solution, right-hand side and table stay as found; the
 *   preconditioner (node block, Schur diagonal, hierarchy or sparse LU factors), the Krylov storage and the K-cycle's
 *   calibration are left as the first cycle of a solve of that system leaves them: a solve after it returns the bits of
 *   the same solve without it.
 * nodal_debug_general_array: a stream wait and a device-to-host copy of one buffer, as the last precond-0 setup of
 *   nodal_debug_fgmres_cycle left it: the node block as CSR -- gn_indptr (i32, K + 1), gn_indices / gn_rowidx (i32, nnz
 *   of the block), gn_data (f64), gn_diag (i32, K: position of each row's diagonal) -- schur (f64, n - K: 1 / S~ per
 *   branch row), and the system that cycle ran on: indptr (i32, n + 1) / indices (i32) / data (f64) and its own
 *   right-hand side (f64, n); the reduced system has no other export.  dst == NULL: the size only; otherwise
 *   capacity_bytes must cover it.  NODAL_E_INVALID when no such setup stands (none yet, or the system was assembled
 *   anew since).  Nothing is launched, nothing on the device is written. */
enum {
    NODAL_FG_RESTART = 40, NODAL_FG_MAXV = NODAL_FG_RESTART + 1,
    NODAL_FG_H = 0,                                               /* [41][40] row-major: column j at [i * 40 + j] */
    NODAL_FG_CS = NODAL_FG_H + NODAL_FG_MAXV * NODAL_FG_RESTART,  /* [40] cosines of the rotations */
    NODAL_FG_SN = NODAL_FG_CS + NODAL_FG_RESTART,                 /* [40] sines */
    NODAL_FG_G = NODAL_FG_SN + NODAL_FG_RESTART,                  /* [41] the rotated right-hand side */
    NODAL_FG_INV_H = NODAL_FG_G + NODAL_FG_MAXV,                  /* 1 / h_{j+1,j} of the last column */
    NODAL_FG_EST = NODAL_FG_INV_H + 1,                            /* the residual estimate |g_{count}| */
    NODAL_FG_DONE = NODAL_FG_INV_H + 2, NODAL_FG_COUNT = NODAL_FG_INV_H + 3, NODAL_FG_INFO = NODAL_FG_INV_H + 4,
    NODAL_FG_TOLB = NODAL_FG_INV_H + 5,
    NODAL_FG_LOG = NODAL_FG_INV_H + 6,                            /* [40] |w after the projections|^2 / |w|^2 */
    NODAL_FG_WORDS = NODAL_FG_LOG + NODAL_FG_RESTART
};
enum {
    NODAL_GA_GN_INDPTR = 0, NODAL_GA_GN_INDICES = 1, NODAL_GA_GN_ROWIDX = 2, NODAL_GA_GN_DATA = 3, NODAL_GA_GN_DIAG = 4,
    NODAL_GA_SCHUR = 5, NODAL_GA_INDPTR = 6, NODAL_GA_INDICES = 7, NODAL_GA_DATA = 8, NODAL_GA_RHS = 9
};
int nodal_debug_fgmres_cycle(nodal_handle h, int32_t system, int32_t precond, int32_t window, int32_t max_cols,
                             double rel_tol, int64_t n, const double *b, double *x_out, double *V_out, double *Z_out,
                             double *gst_out /* [NODAL_FG_WORDS] */, double *y_out /* [41] */, double *norms_out /* [2] */,
                             int64_t *params_out /* [16] */);
int nodal_debug_general_array(nodal_handle h, int32_t which, void *dst, int64_t capacity_bytes, int64_t *bytes_out);
/* The presolve's plan, rewrite and recovery (csrc/presolve.hip) and the scan under its renumbering (csrc/scan.hip) with
 * no solve and no acceptance test behind them: what tests/presolve_reference.py states as linear algebra on the
 * original G x = b and tests/test_gpu_presolve.py compares.  The hooks have no arithmetic and no knob of their own and
 * launch no kernel a solve does not launch.
 * nodal_debug_presolve_build: for the handle's assembled member, whatever its size (the n > 512 and sparse-switch
 *   thresholds belong to the callers), the plan -- the one made ahead during the assembly when it stands, as a solve
 *   takes it -- then the rewrite into the reduced context and that context's symbolic (unless kept) and numeric
 *   assembly, exactly as a sparse solve's presolve does them.  info[16]: 0 the plan is ok (0: declined, nothing below
 *   but 4 .. 6, 11 .. 13 is set), 1 the rewrite succeeded (0: a row it cannot express, nothing assembled), 2 Kr,
 *   3 max_level, 4 pivots, 5 branches kept, 6 components of the reduced table, 7 its unknowns, 8 entries of its matrix,
 *   9 its passive_network, 10 same_topology: the reduced context's symbolic assembly was reused, 11 the plan was the
 *   one made ahead, 12 K, 13 B.  A declined plan or a failed rewrite is a result, not an error.  NODAL_E_INVALID: no
 *   assembled system with branch equations and a host copy of its table; a stamping error of the reduced table comes
 *   back as the reduced assembly's status.  The handle's solution, right-hand side and matrix stay as found; the
 *   reduced context is left as the presolve of a solve leaves it before its solver runs.
 * nodal_debug_presolve_array: one array of what the last nodal_debug_presolve_build left (enum below), host structs
 *   flattened or one device-to-host copy behind a stream wait.  The plan: pivots (i32, sorted), the expressions in plan
 *   order -- p, q, c, d (i32), cst, g (f64) -- the kept branches in branch order -- kk, type, a, b, c, d (i32), value
 *   (f64) -- row_of, level_of (i32, B).  The device's newidx (i32, K).  The reduced component table: type (u8), value
 *   (f64), a, b, c, d, k (i32).  The reduced context's CSR (indptr i32 n' + 1, indices i32, data f64) and right-hand
 *   side (f64 n').  dst == NULL: the size only.  NODAL_E_INVALID when no such build stands (none yet, the system
 *   assembled or the table uploaded anew since, or the array belongs to a stage the build did not reach).
 * nodal_debug_presolve_recover: presolve_recover of that build on the caller's y (host, ny = Kr + kept entries; it
 *   need not solve anything): the handle's x is filled with NaN, then the recovery kernels run as in a solve; x_out
 *   [n].  Whatever solution the handle held is put back and its flag stays: a solve after the hooks returns the bits of
 *   the same solve without them.
 * nodal_debug_scan_u32: scan_exclusive_u32 of in [n] (host) in scratch of the hook's own sized by scan_tmp_bytes; in_place
 *   != 0 scans the device copy onto itself; total_out != NULL asks for the device total.  out [n]. */
enum {
    NODAL_PS_PIVOTS = 0, NODAL_PS_EXPR_P = 1, NODAL_PS_EXPR_Q = 2, NODAL_PS_EXPR_C = 3, NODAL_PS_EXPR_D = 4,
    NODAL_PS_EXPR_CST = 5, NODAL_PS_EXPR_G = 6, NODAL_PS_KEPT_KK = 7, NODAL_PS_KEPT_TYPE = 8, NODAL_PS_KEPT_A = 9,
    NODAL_PS_KEPT_B = 10, NODAL_PS_KEPT_C = 11, NODAL_PS_KEPT_D = 12, NODAL_PS_KEPT_VALUE = 13, NODAL_PS_ROW_OF = 14,
    NODAL_PS_LEVEL_OF = 15, NODAL_PS_NEWIDX = 16, NODAL_PS_R_TYPE = 17, NODAL_PS_R_VALUE = 18, NODAL_PS_R_A = 19,
    NODAL_PS_R_B = 20, NODAL_PS_R_C = 21, NODAL_PS_R_D = 22, NODAL_PS_R_K = 23, NODAL_PS_R_INDPTR = 24,
    NODAL_PS_R_INDICES = 25, NODAL_PS_R_DATA = 26, NODAL_PS_R_RHS = 27
};
int nodal_debug_presolve_build(nodal_handle h, int64_t *info /* [16] */);
int nodal_debug_presolve_array(nodal_handle h, int32_t which, void *dst, int64_t capacity_bytes, int64_t *bytes_out);
int nodal_debug_presolve_recover(nodal_handle h, int64_t ny, const double *y, double *x_out);
int nodal_debug_scan_u32(nodal_handle h, int64_t n, const uint32_t *in, uint32_t *out, int32_t in_place,
                         uint32_t *total_out);
/* The rounds of the exact low-degree elimination (csrc/lowdeg.hip) as the last solve left them, round by round: what
 * tests/lowdeg_reference.py restates in exact rational arithmetic on each round's own parent matrix and
 * tests/test_gpu_lowdeg.py compares.  The hooks have no arithmetic of their own and change nothing a later solve reads:
 * a solve after them returns the bits of the same solve without them.
 * nodal_debug_lowdeg_info: walks h -> its reduced context -> ... while a context's cached decision (ld_state 2: child
 *   built, 3: child built and a floating leftover found) stands for its present matrix.  *rounds (at most
 *   NODAL_LD_MAX_ROUNDS); ints [48][8] per round: 0 the parent's n, 1 its nnz, 2 the child's n, 3 its nnz, 4 the
 *   parent's ld_state, 5 the child's ld_rounds, 6 its ld_slow_rounds, 7 its ncontrib.  A round of state 3 is the last.
 * nodal_debug_lowdeg_array: a stream wait and a device-to-host copy of one array of round `round` (enum below): the
 *   parent's newidx (i32, n), right-hand side (f64, n: the vector that round read -- the last pair's during a pair
 *   sweep), grounded flags (u8, n) and solution (f64, n; 0 bytes when none was recovered); the child's indptr (i32,
 *   n' + 1), indices (i32), diag_pos (i32, n'), data (f64), right-hand side (f64, n'), grounded flags (u8, n'),
 *   solution (f64, n'; 0 bytes when it was never solved), cptr (i32, nnz' + 1) and contrib (u32, ncontrib).  The LAST
 *   child's data, right-hand side and flags belong to its own solver by now: for these the hook runs that round's
 *   production kernels (schur_values, reduce_rhs) again on the kept lists into scratch of its own and copies that.
 *   dst == NULL: the size only, nothing launched.  NODAL_E_INVALID: no such round or array, a destination too small.
 * nodal_debug_floating_small: the one-workgroup connected-components verdict (small_floating_check, through
 *   csr_floating_check_small) on the caller's graph: host CSR (indptr i32 n + 1, indices i32, self-loops allowed),
 *   grounded (u8, n); *floating = 1 if some component holds no grounded node.  Every index is checked on the host
 *   first.  NODAL_E_INVALID for a malformed graph and above 4096 nodes (nothing is uploaded or launched then). */
enum {
    NODAL_LD_MAX_ROUNDS = 48,
    NODAL_LD_P_NEWIDX = 0, NODAL_LD_P_RHS = 1, NODAL_LD_P_GROUNDED = 2, NODAL_LD_P_X = 3, NODAL_LD_C_INDPTR = 4,
    NODAL_LD_C_INDICES = 5, NODAL_LD_C_DIAG_POS = 6, NODAL_LD_C_DATA = 7, NODAL_LD_C_RHS = 8, NODAL_LD_C_GROUNDED = 9,
    NODAL_LD_C_X = 10, NODAL_LD_C_CPTR = 11, NODAL_LD_C_CONTRIB = 12
};
int nodal_debug_lowdeg_info(nodal_handle h, int32_t *rounds, int64_t *ints /* [48][8] */);
int nodal_debug_lowdeg_array(nodal_handle h, int32_t round, int32_t which, void *dst, int64_t capacity_bytes,
                             int64_t *bytes_out);
int nodal_debug_floating_small(nodal_handle h, int64_t n, const int32_t *indptr, const int32_t *indices,
                               const uint8_t *grounded, int32_t *floating);

#ifdef __cplusplus
}
#endif
#endif /* NODAL_HIP_H */
