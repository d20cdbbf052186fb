"""ctypes binding of libnodal_hip.so (include/nodal_hip.h).

There is no CPU fallback: if the library is missing, or no MI355X is visible
when a handle is created, this raises.  The library itself is loadable on a
machine without a GPU (symbol checks only).
"""

import atexit
import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnodal_hip.so")

OK, E_INVALID, E_HIP, E_ZERO_RESISTANCE, E_STAMP_COLLISION, E_SINGULAR, E_NOMEM, \
    E_UNSUPPORTED = range(8)
SPARSE_AUTO, SPARSE_PCG, SPARSE_DENSIFY, SPARSE_LU, SPARSE_DIRECT = range(5)
OPT_FORCE_PIVOTING = 1
OPT_GEPP_PANEL = 2
OPT_EXTRA_STREAMS = 3
OPT_BORROW_TABLE = 4
OPT_TRANSIENT_TAPE = 5

_p = C.POINTER
_i32p, _i64p, _f64p, _u8p = _p(C.c_int32), _p(C.c_int64), _p(C.c_double), _p(C.c_uint8)
_u32p = _p(C.c_uint32)

# name -> (restype, argtypes); every symbol include/nodal_hip.h declares
SIGNATURES = {
    "nodal_version": (C.c_char_p, []),
    "nodal_create": (C.c_int, [C.c_int, _p(C.c_void_p)]),
    "nodal_destroy": (C.c_int, [C.c_void_p]),
    "nodal_last_error": (C.c_char_p, [C.c_void_p]),
    "nodal_upload_components": (C.c_int, [C.c_void_p, C.c_int64, _u8p, _f64p, _i32p, _i32p,
                                          _i32p, _i32p, _i32p, _i32p, C.c_int32, C.c_int32]),
    "nodal_host_alloc": (C.c_int, [C.c_size_t, _p(C.c_void_p)]),
    "nodal_host_free": (C.c_int, [C.c_void_p]),
    "nodal_upload_values": (C.c_int, [C.c_void_p, C.c_int32, _f64p]),
    "nodal_assemble_symbolic": (C.c_int, [C.c_void_p]),
    "nodal_assemble_numeric": (C.c_int, [C.c_void_p, C.c_int32, _i64p]),
    "nodal_get_sizes": (C.c_int, [C.c_void_p, _i64p, _i64p, _i64p]),
    "nodal_export_csr": (C.c_int, [C.c_void_p, _i32p, _i32p, _f64p, _f64p]),
    "nodal_export_dense": (C.c_int, [C.c_void_p, _f64p, _f64p]),
    "nodal_solve_dense": (C.c_int, [C.c_void_p, _f64p, _i32p]),
    "nodal_solve_sparse": (C.c_int, [C.c_void_p, C.c_int32, _f64p, _i32p, _i32p, _f64p]),
    "nodal_download_x": (C.c_int, [C.c_void_p, _f64p]),
    "nodal_solve_pairs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _i32p, _i32p, _f64p, _i32p]),
    "nodal_solve_sources": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _i64p, _f64p, _f64p, _f64p,
                                      _i32p]),
    "nodal_branches": (C.c_int, [C.c_void_p, _f64p, _f64p, _f64p, _f64p]),
    "nodal_solve_sources_branches": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _i64p, _f64p, _f64p, _f64p,
                                               _i32p, _f64p, _i32p, _f64p, _i32p, _f64p, _i32p, _f64p]),
    "nodal_sensitivities": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _i32p, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p,
                                      _i32p]),
    "nodal_gradient": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p, _f64p, C.c_int32, _i64p, _f64p, _f64p, _f64p,
                                 _f64p, _i32p]),
    "nodal_transient": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _i64p, C.c_int32, _i64p, _f64p,
                                  _f64p, C.c_int32, _i32p, _i32p, _f64p, C.c_int32, _f64p, _f64p, _i32p, _f64p, _i32p,
                                  _f64p, _i32p, _i32p]),
    "nodal_transient_rlc": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _i64p, C.c_int32, _i64p, _f64p,
                                      _f64p, C.c_int32, _i32p, _i32p, _f64p, C.c_int32, _f64p, _f64p, _i32p, _f64p, _i32p,
                                      _f64p, _i32p, _i32p, C.c_int64, _i64p, _f64p, C.c_int32, _i32p, _f64p, _f64p]),
    "nodal_newton_dc": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, _i64p, _f64p, _f64p, C.c_double, C.c_int32, _i64p, _f64p,
                                  _f64p, C.c_int32, C.c_double, C.c_double, C.c_double, _f64p, _f64p, _f64p, _f64p, _f64p,
                                  _f64p, _f64p, _i32p, _i32p, _i32p, _i32p, _i32p]),
    "nodal_newton_dc_bjt": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, _i64p, _f64p, _f64p, C.c_double, C.c_int32, _i64p,
                                      _f64p, _f64p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int64, _i64p, _i32p,
                                      _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p,
                                      _i32p, _i32p, _i32p, _i32p]),
    "nodal_newton_gradient": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, _i64p, _f64p, _f64p, C.c_double, C.c_int32, _i64p,
                                        _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p]),
    "nodal_transient_nl": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _i64p, C.c_int32, _i64p, _f64p,
                                     _f64p, C.c_int32, _i32p, _i32p, _f64p, C.c_int32, _f64p, _f64p, _i32p, _f64p, _i32p,
                                     _f64p, _i32p, _i32p, C.c_int64, _i64p, _f64p, C.c_int32, _i32p, _f64p, _f64p,
                                     C.c_int64, _i64p, _f64p, _f64p, C.c_double, C.c_int32, C.c_double, C.c_double,
                                     C.c_double, C.c_int32, _i32p, _i32p, _i32p, _f64p, _f64p, _f64p]),
    "nodal_transient_nl_bjt": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _i64p, C.c_int32, _i64p,
                                         _f64p, _f64p, C.c_int32, _i32p, _i32p, _f64p, C.c_int32, _f64p, _f64p, _i32p, _f64p,
                                         _i32p, _f64p, _i32p, _i32p, C.c_int64, _i64p, _f64p, C.c_int32, _i32p, _f64p, _f64p,
                                         C.c_int64, _i64p, _f64p, _f64p, C.c_double, C.c_int32, C.c_double, C.c_double,
                                         C.c_double, C.c_int32, _i32p, _i32p, _i32p, _f64p, _f64p, _f64p, C.c_int64, _i64p,
                                         _i32p, _f64p, C.c_int32, _i32p, _f64p, _f64p]),
    "nodal_transient_gradient": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p,
                                           _f64p, _i32p]),
    "nodal_ac_sweep": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p, C.c_int64, _u8p, _f64p, _i32p, _i32p, C.c_int32,
                                 _i64p, _f64p, _f64p, C.c_int32, _i32p, _i32p, _f64p, C.c_int32, _i32p, _f64p, C.c_int32,
                                 _f64p, _f64p, _i32p, _f64p, _i32p]),
    "nodal_ac_noise": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p, C.c_int64, _u8p, _f64p, _i32p, _i32p, C.c_double,
                                 C.c_int32, _i32p, _i32p, C.c_int64, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p]),
    "nodal_ac_ports": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p, C.c_int64, _u8p, _f64p, _i32p, _i32p, C.c_int32,
                                 _i32p, _i32p, _f64p, _f64p, _i32p, _i32p, _f64p, _i32p, _i64p]),
    "nodal_ac_gradient": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p, C.c_int64, _u8p, _f64p, _i32p, _i32p, C.c_int32,
                                    _i64p, _f64p, _f64p, C.c_int32, _i32p, _i32p, _f64p, _f64p, _f64p, _f64p, _f64p,
                                    C.c_int32, _f64p, _f64p, _i32p, _i64p]),
    "nodal_port_matrix": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _i32p, _i32p, _f64p, _f64p, _f64p, _i32p]),
    "nodal_residual": (C.c_int, [C.c_void_p, _f64p]),
    "nodal_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _i32p]),
    "nodal_run_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _f64p, _i32p]),
    "nodal_batch_x_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "nodal_x_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "nodal_last_timings": (C.c_int, [C.c_void_p, _f64p]),
    "nodal_last_kernel_stats": (C.c_int, [C.c_void_p, _f64p, _i64p, _f64p]),
    "nodal_last_solve_info": (C.c_int, [C.c_void_p, _i32p, _i32p, _f64p]),
    "nodal_synchronize": (C.c_int, [C.c_void_p]),
    "nodal_set_option": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "nodal_debug_gemm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _f64p, _f64p, _f64p]),
    "nodal_debug_gemm_ex": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_int32, _f64p, C.c_int64, _f64p, C.c_int64, _f64p, C.c_int64,
                                      C.c_int32, C.c_int32, C.c_int32, _f64p, C.c_int64, _f64p, C.c_int64, _f64p, C.c_int64]),
    "nodal_debug_block_inverse": (C.c_int, [C.c_void_p, C.c_int32, _f64p, C.c_int64, C.c_int32, C.c_int32, _f64p, C.c_int64,
                                            _i32p]),
    "nodal_debug_dense_solve": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _f64p, _f64p, _f64p, _i32p, _i32p]),
    "nodal_debug_sources_rhs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _i64p, _f64p, _f64p]),
    "nodal_debug_residual": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _f64p, _f64p, _f64p, _f64p]),
    "nodal_debug_direct_apply": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _f64p, _f64p, _i64p, _i32p]),
    "nodal_debug_hierarchy_info": (C.c_int, [C.c_void_p, _i32p, _i64p, _f64p]),
    "nodal_debug_hierarchy_array": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _i64p]),
    "nodal_debug_cycle_apply": (C.c_int, [C.c_void_p, C.c_int32, _f64p, _f64p, _f64p, _f64p, _f64p, _i32p]),
    "nodal_debug_amg_info": (C.c_int, [C.c_void_p, _i32p, _i64p, _i64p, _f64p, _i64p]),
    "nodal_debug_amg_array": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _i64p]),
    "nodal_debug_amg_apply": (C.c_int, [C.c_void_p, C.c_int32, _f64p, _f64p, _i32p]),
    "nodal_debug_fgmres_cycle": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int64,
                                           _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _i64p]),
    "nodal_debug_general_array": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, _i64p]),
    "nodal_debug_presolve_build": (C.c_int, [C.c_void_p, _i64p]),
    "nodal_debug_presolve_array": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, _i64p]),
    "nodal_debug_presolve_recover": (C.c_int, [C.c_void_p, C.c_int64, _f64p, _f64p]),
    "nodal_debug_scan_u32": (C.c_int, [C.c_void_p, C.c_int64, _u32p, _u32p, C.c_int32, _u32p]),
    "nodal_debug_lowdeg_info": (C.c_int, [C.c_void_p, _i32p, _i64p]),
    "nodal_debug_lowdeg_array": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, _i64p]),
    "nodal_debug_floating_small": (C.c_int, [C.c_void_p, C.c_int64, _i32p, _i32p, _u8p, _i32p]),
}

# nodal_debug_lowdeg_info: the eight words of a round; nodal_debug_lowdeg_array: `which` in the header's order
# (NODAL_LD_*) with the item type of each array -- p_*: the round's parent, the rest its child (the reduced network)
LOWDEG_MAX_ROUNDS = 48
LOWDEG_INFO = ("n", "nnz", "child_n", "child_nnz", "ld_state", "ld_rounds", "ld_slow_rounds", "ncontrib")
LOWDEG_ARRAYS = (("p_newidx", np.int32), ("p_rhs", np.float64), ("p_grounded", np.uint8), ("p_x", np.float64),
                 ("indptr", np.int32), ("indices", np.int32), ("diag_pos", np.int32), ("data", np.float64),
                 ("rhs", np.float64), ("grounded", np.uint8), ("x", np.float64), ("cptr", np.int32),
                 ("contrib", np.uint32))

# nodal_debug_presolve_build: the words of info; nodal_debug_presolve_array: `which` in the header's order (NODAL_PS_*)
# with the item type of each array -- the plan (pivots, expressions, kept branches, row_of, level_of), the device's
# newidx, the reduced component table, the reduced context's CSR and right-hand side
PRESOLVE_INFO = ("ok", "built", "Kr", "max_level", "npivots", "nkept", "ncomp", "n", "nnz", "passive", "same_topology",
                 "ahead", "K", "B")
PRESOLVE_PLAN_ARRAYS = 16  # the first so many arrays belong to the plan: they exist for a declined plan too
PRESOLVE_ARRAYS = (("pivots", np.int32), ("expr_p", np.int32), ("expr_q", np.int32), ("expr_c", np.int32),
                   ("expr_d", np.int32), ("expr_cst", np.float64), ("expr_g", np.float64), ("kept_kk", np.int32),
                   ("kept_type", np.int32), ("kept_a", np.int32), ("kept_b", np.int32), ("kept_c", np.int32),
                   ("kept_d", np.int32), ("kept_value", np.float64), ("row_of", np.int32), ("level_of", np.int32),
                   ("newidx", np.int32), ("r_type", np.uint8), ("r_value", np.float64), ("r_a", np.int32),
                   ("r_b", np.int32), ("r_c", np.int32), ("r_d", np.int32), ("r_k", np.int32), ("r_indptr", np.int32),
                   ("r_indices", np.int32), ("r_data", np.float64), ("r_rhs", np.float64))

# nodal_debug_fgmres_cycle: the small least-squares problem's block of doubles in the header's layout (NODAL_FG_*), and
# the names of the words of params_out
FG_RESTART = 40
FG_MAXV = FG_RESTART + 1
FG_H = 0                              # [41][40] row-major
FG_CS = FG_H + FG_MAXV * FG_RESTART   # [40]
FG_SN = FG_CS + FG_RESTART            # [40]
FG_G = FG_SN + FG_RESTART             # [41]
FG_INV_H = FG_G + FG_MAXV
FG_EST, FG_DONE, FG_COUNT, FG_INFO, FG_TOLB, FG_LOG = (FG_INV_H + k for k in range(1, 7))
FG_WORDS = FG_LOG + FG_RESTART
FGMRES_PARAMS = ("n", "K", "ld", "count", "window", "use_sa", "ell_spmv", "levels", "gd", "breakdown")
# nodal_debug_general_array: `which` in the header's order (NODAL_GA_*) with the item type of each buffer
GENERAL_ARRAYS = (("gn_indptr", np.int32), ("gn_indices", np.int32), ("gn_rowidx", np.int32), ("gn_data", np.float64),
                  ("gn_diag", np.int32), ("schur", np.float64), ("indptr", np.int32), ("indices", np.int32),
                  ("data", np.float64), ("rhs", np.float64))

# nodal_debug_amg_array: `which` in the header's order (NODAL_AA_*) with the item type of each buffer, the two special
# level numbers, and the names of the words nodal_debug_amg_info / nodal_debug_amg_apply return
AMG_ARRAYS = (("indptr", np.int32), ("indices", np.int32), ("data", np.float64), ("dinv", np.float64),
              ("agg", np.int32), ("memptr", np.int32), ("mem", np.int32), ("boff", np.uint32), ("binv", np.float64))
AMG_LEVEL_COARSE_INV = -1
AMG_LEVEL_TAIL_IMAGE = -2
AMG_LEVEL_INFO = ("n", "nnz", "nc", "block", "in_tail")
AMG_WORDS = ("tail", "kmax", "coarse_direct", "block_smoother", "sweeps0", "BLOCK_MAX", "COARSEST_MAX", "K_MIN_ROWS",
             "SPLIT_PROLONG_MIN", "DOT_BLOCKS", "TAIL_LDS_BUDGET", "STREAM_CAP", "LONG_PART", "TAIL_MAX_LEVELS")
AMG_TAIL_WORDS = ("nlev", "o_inv", "o_C1", "o_V1", "image_bytes", "total_bytes")
AMG_TAIL_LEVEL = ("n", "nnz", "nc", "o_data", "o_dinv", "o_indptr", "o_memptr", "o_indices", "o_agg", "o_mem",
                  "o_B", "o_X", "o_E", "o_R")
AMG_APPLY_PARAMS = ("nlev", "tail", "kmax", "coarse_direct", "block_smoother", "sweeps0", "level", "block", "handover",
                    "nparts", "split_prolong", "two_sweeps")

# nodal_debug_hierarchy_array: `which` in the header's order (NODAL_HA_*) with the item type of each buffer, and the
# names of the sixteen info words of a level (nodal_debug_hierarchy_info)
HIERARCHY_ARRAYS = (("acol", np.int32), ("aval", np.float64), ("avalf", np.float32), ("alen", np.int32),
                    ("dinv", np.float64), ("adcol", np.int16), ("agg", np.int32), ("pcol", np.int32),
                    ("pval", np.float64), ("pvalf", np.float32), ("rcol", np.int32), ("rval", np.float64),
                    ("rvalf", np.float32), ("rlen", np.int32), ("wcol", np.int32), ("wval", np.float32),
                    ("wlen", np.int32), ("p2col", np.int32), ("p2val", np.float32), ("p2len", np.int32),
                    ("d2", np.float32), ("wtstart", np.uint32), ("wtcol", np.int32), ("wtval", np.float32),
                    ("wtsrc", np.int32))
HIERARCHY_INFO = ("n", "ld", "nc", "width", "maxlen", "wfix", "nnz", "rld", "rcap", "wslots", "fold_want", "fold", "d16",
                  "in_tail", "refreshed", "dense_coarsest")

# nodal_debug_cycle_apply: the sixteen words of params_out
CYCLE_PARAMS = ("nu0", "nu1", "nu2", "tail_nu", "kcycle", "klevels", "tail", "tail_dense", "nlev", "fold0", "frozen",
                "columns", "fold_mask", "restrict_mask", "visit_mask", "general")

# csrc/galerkin_groups.h: what a coarse row may have to share a wavefront with three others in the Galerkin sums
# (tests/test_galerkin_groups_host.py holds these against the header)
GALERKIN_SUB_ROWS = 4
GALERKIN_SUB_ENTRIES = 32
GALERKIN_SUB_PRODUCTS = 128
GALERKIN_SUB_COLUMNS = 16
GALERKIN_DYN_PRODUCTS = 1024  # (knobs.h: the default of NODAL_SA_GLIST, the product list of a 64-slot level)

_lib = None
_live = weakref.WeakSet()  # handles still open; closed before the HIP runtime unloads


@atexit.register
def _close_all():
    _closing[0] = True
    for h in list(_live):
        h.close()


class NodalHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"libnodal_hip status {status}: {message}")
        self.status = status


def load():
    """Load libnodal_hip.so and set the prototypes.  Raises OSError with build
    instructions when the library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(
                f"{LIB_PATH} not found: build it with `make` (or "
                "`python -c 'import __graft_entry__ as g; g.build()'`) -- "
                "nodal_amd has no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def _ptr(arr, ctype):
    return arr.ctypes.data_as(_p(ctype))


# ---- pinned host arrays for large component tables ---------------------------------
# A table column allocated here is page-locked: nodal_upload_components then copies it by
# DMA at link rate instead of through the runtime's staging buffers.  Blocks are recycled
# (hipHostMalloc of tens of MB costs milliseconds); without a HIP device the arrays are
# ordinary numpy memory.
PINNED_MIN_BYTES = 1 << 20
_PINNED_POOL = {}          # bytes -> [address, ...] of free blocks
_PINNED_POOL_BYTES = [0]
_PINNED_POOL_MAX = 1 << 30
_pinned_ok = [None]
_closing = [False]


def _pinned_release(addr, nbytes):
    if _lib is None or _closing[0]:
        return  # (interpreter shutdown: the runtime frees what is left)
    if _PINNED_POOL_BYTES[0] + nbytes <= _PINNED_POOL_MAX:
        _PINNED_POOL.setdefault(nbytes, []).append(addr)
        _PINNED_POOL_BYTES[0] += nbytes
    else:
        _lib.nodal_host_free(C.c_void_p(addr))


def host_empty(count, dtype):
    """1-D numpy array of `count` items, in pinned host memory when it is large and a HIP
    device is there, ordinary memory otherwise."""
    dtype = np.dtype(dtype)
    nbytes = int(count) * dtype.itemsize
    if nbytes < PINNED_MIN_BYTES or _pinned_ok[0] is False:
        return np.empty(count, dtype=dtype)
    try:
        lib = load()
    except OSError:
        _pinned_ok[0] = False
        return np.empty(count, dtype=dtype)
    size = (nbytes + 4095) & ~4095
    free = _PINNED_POOL.get(size)
    if free:
        addr = free.pop()
        _PINNED_POOL_BYTES[0] -= size
    else:
        out = C.c_void_p()
        if lib.nodal_host_alloc(size, C.byref(out)) != OK or not out.value:
            _pinned_ok[0] = False
            return np.empty(count, dtype=dtype)
        _pinned_ok[0] = True
        addr = out.value
    buf = (C.c_char * size).from_address(addr)
    # every array (and view) made from `buf` keeps it alive; the block goes back to the pool with it
    weakref.finalize(buf, _pinned_release, addr, size)
    return np.frombuffer(buf, dtype=dtype, count=count)


class Handle:
    """Owns one nodal_handle (device memory + stream) on `device`."""

    def __init__(self, device=0):
        self.lib = load()
        self._h = C.c_void_p()
        status = self.lib.nodal_create(device, C.byref(self._h))
        if status != OK:
            raise NodalHipError(
                status, f"nodal_create(device={device}) failed: no usable MI355X "
                "(HIP device) is visible; nodal_amd has no CPU fallback")
        self.n = self.nnz = self.ncontrib = 0
        self._ncomp = self._K = 0
        # upload() keeps the table's columns alive (self._keep) until the next upload: the library may read them in place
        self.lib.nodal_set_option(self._h, OPT_BORROW_TABLE, 1)
        _live.add(self)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.nodal_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def closed(self):
        return not getattr(self, "_h", None)

    def _check(self, status, allow=()):
        if status != OK and status not in allow:
            raise NodalHipError(status, self.lib.nodal_last_error(self._h).decode())
        return status

    # -- table ------------------------------------------------------------
    def upload(self, table):
        # B == 0: resistors and current sources only -- the four columns they never read stay home (unless the table
        # was given GM rows, which read their control leads without a branch unknown)
        plain = table.B == 0 and not getattr(table, "controlled", False)
        names = ("type", "value", "a", "b") if plain else ("type", "value", "a", "b", "c", "d", "drv", "k")
        cols = [np.ascontiguousarray(getattr(table, n)) for n in names]
        self._keep = cols
        t, v, a, b = cols[:4]
        rest = [_ptr(x, C.c_int32) for x in cols[4:]] or [None] * 4
        self.n_members = table.K + table.B
        self._ncomp, self._K = int(table.ncomp), int(table.K)
        self._check(self.lib.nodal_upload_components(
            self._h, table.ncomp, _ptr(t, C.c_uint8), _ptr(v, C.c_double),
            _ptr(a, C.c_int32), _ptr(b, C.c_int32), *rest, table.K, table.B))

    def upload_values(self, values):
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.ndim == 2
        self._check(self.lib.nodal_upload_values(self._h, values.shape[0], _ptr(values, C.c_double)))

    # -- assembly ---------------------------------------------------------
    def assemble_symbolic(self):
        self._check(self.lib.nodal_assemble_symbolic(self._h))
        self._refresh_sizes()

    def _refresh_sizes(self):
        n, nnz, nc = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.nodal_get_sizes(self._h, C.byref(n), C.byref(nnz), C.byref(nc)))
        self.n, self.nnz, self.ncontrib = n.value, nnz.value, nc.value

    def assemble_numeric(self, member=0):
        """Returns (status, bad_component): status is OK, E_ZERO_RESISTANCE or
        E_STAMP_COLLISION."""
        bad = C.c_int64(-1)
        status = self._check(self.lib.nodal_assemble_numeric(self._h, member, C.byref(bad)),
                             allow=(E_ZERO_RESISTANCE, E_STAMP_COLLISION))
        return status, bad.value

    def export_csr(self, values=True):
        indptr = np.empty(self.n + 1, dtype=np.int32)
        indices = np.empty(self.nnz, dtype=np.int32)
        data = np.empty(self.nnz, dtype=np.float64) if values else None
        rhs = np.empty(self.n, dtype=np.float64) if values else None
        self._check(self.lib.nodal_export_csr(
            self._h, _ptr(indptr, C.c_int32), _ptr(indices, C.c_int32),
            _ptr(data, C.c_double) if values else None,
            _ptr(rhs, C.c_double) if values else None))
        return indptr, indices, data, rhs

    def export_dense(self):
        G = np.empty((self.n, self.n), dtype=np.float64)
        rhs = np.empty(self.n, dtype=np.float64)
        self._check(self.lib.nodal_export_dense(self._h, _ptr(G, C.c_double), _ptr(rhs, C.c_double)))
        return G, rhs

    # -- solve ------------------------------------------------------------
    def solve_dense(self, download=True):
        """Returns (x or None, info).  info > 0: exact zero pivot (singular)."""
        x = host_empty(self.n, np.float64) if download else None  # (pinned when large: the copy down is plain DMA)
        info = C.c_int32(0)
        self._check(self.lib.nodal_solve_dense(
            self._h, _ptr(x, C.c_double) if download else None, C.byref(info)),
            allow=(E_SINGULAR,))
        return x, info.value

    def solve_sparse(self, method=SPARSE_AUTO, download=True):
        """Returns (x or None, info, iterations, relative residual)."""
        x = host_empty(self.n, np.float64) if download else None  # (pinned when large: the copy down is plain DMA)
        info, iters, resid = C.c_int32(0), C.c_int32(0), C.c_double(0)
        self._check(self.lib.nodal_solve_sparse(
            self._h, method, _ptr(x, C.c_double) if download else None,
            C.byref(info), C.byref(iters), C.byref(resid)))
        return x, info.value, iters.value, resid.value

    def solve_pairs(self, ia, ib, dense):
        """Equivalent resistance for every node-index pair; returns (R array, info)."""
        ia = np.ascontiguousarray(ia, dtype=np.int32)
        ib = np.ascontiguousarray(ib, dtype=np.int32)
        out = np.empty(len(ia), dtype=np.float64)
        info = C.c_int32(0)
        self._check(self.lib.nodal_solve_pairs(self._h, int(dense), len(ia), _ptr(ia, C.c_int32),
                                               _ptr(ib, C.c_int32), _ptr(out, C.c_double),
                                               C.byref(info)), allow=(E_SINGULAR,))
        return out, info.value

    def solve_sources(self, rows, values, dense):
        """Source sweep: values [M, nsrc] replace the values of table rows `rows` (type A or E) member by
        member.  Returns (x [M, n], info [M], scaled residual [M]); with dense, a singular G raises
        NodalHipError(E_SINGULAR)."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.ndim == 2 and values.shape[1] == len(rows)
        count = values.shape[0]
        x = np.empty((count, self.n), dtype=np.float64)
        info = np.zeros(count, dtype=np.int32)
        resid = np.zeros(count, dtype=np.float64)
        self._check(self.lib.nodal_solve_sources(self._h, int(dense), count, len(rows), _ptr(rows, C.c_int64),
                                                 _ptr(values, C.c_double), _ptr(x, C.c_double),
                                                 _ptr(resid, C.c_double), _ptr(info, C.c_int32)))
        return x, info, resid

    def solve_sources_branches(self, rows, values, dense, keep_solutions=True):
        """solve_sources plus the sweep's worst-case envelope, accumulated on the device.  Returns
        (x [M, n] or None, info, scaled residual, envelope dict: current_absmax / current_member [ncomp],
        potential_min / potential_min_member / potential_max / potential_max_member [K], power [M, 2]).  With
        keep_solutions False no [M, n] array is allocated anywhere on the host."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.ndim == 2 and values.shape[1] == len(rows)
        count = values.shape[0]
        ncomp, K = self._ncomp, self._K
        x = np.empty((count, self.n), dtype=np.float64) if keep_solutions else None
        info = np.zeros(count, dtype=np.int32)
        resid = np.zeros(count, dtype=np.float64)
        env = {"current_absmax": np.empty(ncomp), "current_member": np.empty(ncomp, dtype=np.int32),
               "potential_min": np.empty(K), "potential_min_member": np.empty(K, dtype=np.int32),
               "potential_max": np.empty(K), "potential_max_member": np.empty(K, dtype=np.int32),
               "power": np.empty((count, 2))}
        self._check(self.lib.nodal_solve_sources_branches(
            self._h, int(dense), count, len(rows), _ptr(rows, C.c_int64), _ptr(values, C.c_double),
            _ptr(x, C.c_double) if keep_solutions else None, _ptr(resid, C.c_double), _ptr(info, C.c_int32),
            *(_ptr(env[key], C.c_int32 if key.endswith("member") else C.c_double) for key in env)))
        return x, info, resid, env

    def branches(self, voltage=True, current=True, power=True):
        """Branch quantities of the solution on the device, in table row order: (voltage, current, power,
        dissipated, absorbed_by_sources); an array that is not asked for is None.  NodalHipError(E_INVALID) when
        the handle holds no solution."""
        out = [host_empty(self._ncomp, np.float64) if want else None for want in (voltage, current, power)]
        totals = np.zeros(2)
        self._check(self.lib.nodal_branches(self._h, *(_ptr(a, C.c_double) if a is not None else None for a in out),
                                            _ptr(totals, C.c_double)))
        return out[0], out[1], out[2], float(totals[0]), float(totals[1])

    def sensitivities(self, kind, p, q2, dense, adjoints=False, out=None):
        """Adjoint sensitivities of the outputs (kind, p, q2) (sensitivity.resolve_outputs) for the solution on the
        device.  Returns (values [M, ncomp], output values [M], adjoints [M, n] or None, scaled residual [M], info
        [M]); NodalHipError(E_INVALID) when the handle holds no solution, with dense a singular G raises
        NodalHipError(E_SINGULAR).  `out`: a C-contiguous float64 [M, ncomp] array to receive the values (a caller
        that repeats the call keeps one page-locked array instead of locking a new one every time)."""
        kind, p, q2 = (np.ascontiguousarray(v, dtype=np.int32) for v in (kind, p, q2))
        count = len(kind)
        assert len(p) == count and len(q2) == count
        if out is not None:
            assert out.shape == (count, self._ncomp) and out.dtype == np.float64 and out.flags.c_contiguous
            sens = out
        else:
            # (page-locked when large: the blocks come down by plain DMA)
            sens = host_empty(count * self._ncomp, np.float64).reshape(count, self._ncomp)
        lam = host_empty(count * self.n, np.float64).reshape(count, self.n) if adjoints else None
        y = np.zeros(count, dtype=np.float64)
        resid = np.zeros(count, dtype=np.float64)
        info = np.zeros(count, dtype=np.int32)
        self._check(self.lib.nodal_sensitivities(
            self._h, int(dense), count, _ptr(kind, C.c_int32), _ptr(p, C.c_int32), _ptr(q2, C.c_int32),
            _ptr(sens, C.c_double), _ptr(y, C.c_double), _ptr(lam, C.c_double) if adjoints else None,
            _ptr(resid, C.c_double), _ptr(info, C.c_int32)))
        return sens, y, lam, resid, info

    def gradient(self, cotangents, dense, rows=None, solutions=None, adjoints=False):
        """The gradient of a scalar loss with respect to every component value (nodal_gradient): cotangents [M, n] =
        dL/dx_m, solutions [M, n] the members' solutions (None: the single solve's solution on the device, M == 1 and
        no swept rows), rows the swept table rows of the sweep the members come from.  Returns (values [ncomp], source
        values [M, len(rows)], adjoints [M, n] or None, scaled residual [M], info [M]); NodalHipError(E_INVALID) as
        the header lists, with dense a singular G raises NodalHipError(E_SINGULAR)."""
        cot = np.ascontiguousarray(cotangents, dtype=np.float64)
        assert cot.ndim == 2 and cot.shape[1] == self.n
        count = cot.shape[0]
        rows = np.ascontiguousarray(rows if rows is not None else [], dtype=np.int64)
        x = None
        if solutions is not None:
            x = np.ascontiguousarray(solutions, dtype=np.float64)
            assert x.shape == cot.shape
        grad = np.zeros(self._ncomp, dtype=np.float64)
        gsrc = np.zeros((count, len(rows)), dtype=np.float64)
        lam = host_empty(count * self.n, np.float64).reshape(count, self.n) if adjoints else None
        resid = np.zeros(count, dtype=np.float64)
        info = np.zeros(count, dtype=np.int32)
        self._check(self.lib.nodal_gradient(
            self._h, int(dense), count, _ptr(x, C.c_double) if x is not None else None, _ptr(cot, C.c_double),
            len(rows), _ptr(rows, C.c_int64) if len(rows) else None, _ptr(grad, C.c_double), _ptr(gsrc, C.c_double),
            _ptr(lam, C.c_double) if adjoints else None, _ptr(resid, C.c_double), _ptr(info, C.c_int32)))
        return grad, gsrc, lam, resid, info

    def port_matrix(self, ia, ib, dense, voc=True):
        """The open-circuit impedance matrix seen from the ports (ia[q], ib[q]) (node indices, -1 ground;
        ports.resolve_ports) and, with voc, their open-circuit voltages for the solution on the device.  Returns
        (Z [P, P], V_oc [P] or None, info [P], scaled residual [P]); NodalHipError(E_INVALID) for an index out of
        range or, with voc, when the handle holds no solution; with dense a singular G raises
        NodalHipError(E_SINGULAR)."""
        ia, ib = (np.ascontiguousarray(v, dtype=np.int32) for v in (ia, ib))
        count = len(ia)
        assert ia.ndim == 1 and ib.shape == ia.shape
        z = np.zeros((count, count), dtype=np.float64)
        v_oc = np.zeros(count, dtype=np.float64) if voc else None
        resid = np.zeros(count, dtype=np.float64)
        info = np.zeros(count, dtype=np.int32)
        self._check(self.lib.nodal_port_matrix(
            self._h, int(dense), count, _ptr(ia, C.c_int32), _ptr(ib, C.c_int32), _ptr(z, C.c_double),
            _ptr(v_oc, C.c_double) if voc else None, _ptr(resid, C.c_double), _ptr(info, C.c_int32)))
        return z, v_oc, info, resid

    def transient(self, cap_rows, rows, values, x0, ia, ib, dense, method=0, keep_every=0, envelope=False):
        """Time stepping on a handle that holds the circuit with its companion resistors (nodal_transient): cap_rows
        their table rows, values [steps, len(rows)] the swept sources step by step, x0 [n] the state at t_0, (ia, ib)
        the probes' node indices.  Returns (waveforms [steps + 1, P], solutions [steps // keep_every, n] or None,
        envelope dict or None, scaled residual [steps], info [steps], iterations [steps]); NodalHipError(E_INVALID) as
        the header lists, with dense a singular G raises NodalHipError(E_SINGULAR)."""
        return self._transient(cap_rows, rows, values, x0, ia, ib, dense, method, keep_every, envelope)[:6]

    def transient_rlc(self, cap_rows, ind_rows, rows, values, x0, i0, ia, ib, cur_index, dense, method=0, keep_every=0,
                      envelope=False):
        """transient() with inductors (nodal_transient_rlc): ind_rows their companion rows, i0 [L] their currents at t_0,
        cur_index [Q] the inductors whose currents are wanted.  Returns transient()'s six and (currents [steps + 1, Q],
        final currents [L])."""
        return self._transient(cap_rows, rows, values, x0, ia, ib, dense, method, keep_every, envelope,
                               inductors=(ind_rows, i0, cur_index))

    def transient_nl(self, cap_rows, ind_rows, diode_rows, i_sat, n_vt, gmin, rows, values, x0, i0, ia, ib, cur_index,
                     diode_index, dense, max_iter, reltol, vntol, abstol, method=0, keep_every=0, envelope=False):
        """transient_rlc() with diodes (nodal_transient_nl): diode_rows their companion rows, i_sat, n_vt [D], diode_index
        [Q] the diodes whose v and i(v) are wanted step by step.  Returns transient_rlc()'s eight and a dict: newton
        [steps], updates [steps], v, i [steps + 1, Q], vh [D]."""
        return self._transient(cap_rows, rows, values, x0, ia, ib, dense, method, keep_every, envelope,
                               inductors=(ind_rows, i0, cur_index),
                               diodes=(diode_rows, i_sat, n_vt, gmin, max_iter, reltol, vntol, abstol, diode_index))

    def transient_nl_bjt(self, cap_rows, ind_rows, diode_rows, i_sat, n_vt, gmin, gm_rows, junction, i_s, rows, values, x0,
                         i0, ia, ib, cur_index, diode_index, transistor_index, dense, max_iter, reltol, vntol, abstol, method=0,
                         keep_every=0, envelope=False):
        """transient_nl() with bipolar transistors (nodal_transient_nl_bjt): the handle's table holds two GM rows per
        transport behind the diodes' rows -- gm_rows int64 [T, 2] (forward, reverse), junction int32 [T, 2] (indices into
        the diodes: jf, jr), i_s [T]; transistor_index [Q] the transports whose junction voltages and currents are wanted
        step by step.  Returns transient_nl()'s nine, the dict with tv [steps + 1, Q, 2] (v_f, v_r) and ti
        [steps + 1, Q, 3] (i_f, i_r, iT) as well; vh [D] covers the junctions.  T == 0 is transient_nl(), bit for bit."""
        return self._transient(cap_rows, rows, values, x0, ia, ib, dense, method, keep_every, envelope,
                               inductors=(ind_rows, i0, cur_index),
                               diodes=(diode_rows, i_sat, n_vt, gmin, max_iter, reltol, vntol, abstol, diode_index),
                               transports=(gm_rows, junction, i_s, transistor_index))

    def _transient(self, cap_rows, rows, values, x0, ia, ib, dense, method, keep_every, envelope, inductors=None,
                   diodes=None, transports=None):
        cap_rows = np.ascontiguousarray(cap_rows, dtype=np.int64)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.ndim == 2 and values.shape[1] == len(rows)
        steps = values.shape[0]
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        assert x0.shape == (self.n,)
        ia, ib = (np.ascontiguousarray(v, dtype=np.int32) for v in (ia, ib))
        assert ia.ndim == 1 and ib.shape == ia.shape
        wave = np.zeros((steps + 1, len(ia)), dtype=np.float64)
        kept = steps // keep_every if keep_every > 0 else 0
        x = host_empty(kept * self.n, np.float64).reshape(kept, self.n) if keep_every > 0 else None
        K = self._K
        env = None
        if envelope:
            env = {"potential_min": np.empty(K), "potential_min_step": np.empty(K, dtype=np.int32),
                   "potential_max": np.empty(K), "potential_max_step": np.empty(K, dtype=np.int32)}
        resid = np.zeros(steps, dtype=np.float64)
        info = np.zeros(steps, dtype=np.int32)
        iters = np.zeros(steps, dtype=np.int32)
        env_ptrs = [_ptr(env[key], C.c_int32 if key.endswith("step") else C.c_double) for key in env] if env else [None] * 4
        args = [self._h, int(dense), steps, int(method), len(cap_rows), _ptr(cap_rows, C.c_int64) if len(cap_rows) else None,
                len(rows), _ptr(rows, C.c_int64) if len(rows) else None, _ptr(values, C.c_double) if values.size else None,
                _ptr(x0, C.c_double), len(ia), _ptr(ia, C.c_int32) if len(ia) else None, _ptr(ib, C.c_int32) if len(ib) else None,
                _ptr(wave, C.c_double), int(keep_every), _ptr(x, C.c_double) if x is not None and kept else None, *env_ptrs,
                _ptr(resid, C.c_double), _ptr(info, C.c_int32), _ptr(iters, C.c_int32)]
        if inductors is None:
            self._check(self.lib.nodal_transient(*args))
            return wave, x, env, resid, info, iters, None, None
        ind_rows = np.ascontiguousarray(inductors[0], dtype=np.int64)
        i0 = np.ascontiguousarray(inductors[1], dtype=np.float64)
        cur_index = np.ascontiguousarray(inductors[2], dtype=np.int32)
        assert ind_rows.ndim == 1 and i0.shape == ind_rows.shape and cur_index.ndim == 1
        cur = np.zeros((steps + 1, len(cur_index)), dtype=np.float64)
        final = np.zeros(len(ind_rows), dtype=np.float64)
        args += [len(ind_rows), _ptr(ind_rows, C.c_int64) if len(ind_rows) else None,
                 _ptr(i0, C.c_double) if len(i0) else None, len(cur_index), _ptr(cur_index, C.c_int32) if len(cur_index) else None,
                 _ptr(cur, C.c_double) if cur.size else None, _ptr(final, C.c_double) if len(final) else None]
        if diodes is None:
            self._check(self.lib.nodal_transient_rlc(*args))
            return wave, x, env, resid, info, iters, cur, final
        diode_rows = np.ascontiguousarray(diodes[0], dtype=np.int64)
        i_sat, n_vt = (np.ascontiguousarray(v, dtype=np.float64) for v in diodes[1:3])
        gmin, max_iter, reltol, vntol, abstol = diodes[3:8]
        index = np.ascontiguousarray(diodes[8], dtype=np.int32)
        D = len(diode_rows)
        assert diode_rows.ndim == 1 and i_sat.shape == (D,) and n_vt.shape == (D,) and index.ndim == 1
        out = {"newton": np.zeros(steps, dtype=np.int32), "updates": np.zeros(steps, dtype=np.int32),
               "v": np.zeros((steps + 1, len(index)), dtype=np.float64), "i": np.zeros((steps + 1, len(index)), dtype=np.float64),
               "vh": np.zeros(D, dtype=np.float64)}
        args += [D, _ptr(diode_rows, C.c_int64) if D else None, _ptr(i_sat, C.c_double) if D else None,
                 _ptr(n_vt, C.c_double) if D else None, float(gmin), int(max_iter), float(reltol), float(vntol), float(abstol),
                 len(index), _ptr(index, C.c_int32) if len(index) else None, _ptr(out["newton"], C.c_int32),
                 _ptr(out["updates"], C.c_int32), _ptr(out["v"], C.c_double) if out["v"].size else None,
                 _ptr(out["i"], C.c_double) if out["i"].size else None, _ptr(out["vh"], C.c_double) if D else None]
        if transports is None:
            self._check(self.lib.nodal_transient_nl(*args))
            return wave, x, env, resid, info, iters, cur, final, out
        gm_rows = np.ascontiguousarray(transports[0], dtype=np.int64).reshape(-1, 2)
        junction = np.ascontiguousarray(transports[1], dtype=np.int32).reshape(-1, 2)
        i_s = np.ascontiguousarray(transports[2], dtype=np.float64)
        tindex = np.ascontiguousarray(transports[3], dtype=np.int32)
        T = len(gm_rows)
        assert junction.shape == (T, 2) and i_s.shape == (T,) and tindex.ndim == 1
        out["tv"] = np.zeros((steps + 1, len(tindex), 2), dtype=np.float64)
        out["ti"] = np.zeros((steps + 1, len(tindex), 3), dtype=np.float64)
        self._check(self.lib.nodal_transient_nl_bjt(
            *args, T, _ptr(gm_rows, C.c_int64) if T else None, _ptr(junction, C.c_int32) if T else None,
            _ptr(i_s, C.c_double) if T else None, len(tindex), _ptr(tindex, C.c_int32) if len(tindex) else None,
            _ptr(out["tv"], C.c_double) if out["tv"].size else None, _ptr(out["ti"], C.c_double) if out["ti"].size else None))
        return wave, x, env, resid, info, iters, cur, final, out

    def newton_dc(self, diode_rows, i_sat, n_vt, gmin, rows, values, x0, dense, max_iter, reltol, vntol, abstol,
                  keep_iterates=False):
        """Newton's method on a handle that holds the circuit with one companion resistor per diode (nodal_newton_dc):
        diode_rows their table rows, i_sat, n_vt [D], values [len(rows)] the one setting of the swept sources, x0 [n] or
        None.  Returns a dict: x [n], v, i, g [D], iterations, converged, record [iterations, 4], info, iters, route
        [iterations], and with keep_iterates iterates [iterations, n] and vh [iterations + 1, D] (None otherwise);
        NodalHipError(E_INVALID) as the header lists, with dense a singular G raises NodalHipError(E_SINGULAR)."""
        diode_rows = np.ascontiguousarray(diode_rows, dtype=np.int64)
        i_sat, n_vt = (np.ascontiguousarray(v, dtype=np.float64) for v in (i_sat, n_vt))
        D = len(diode_rows)
        assert diode_rows.ndim == 1 and i_sat.shape == (D,) and n_vt.shape == (D,)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.shape == (len(rows),)
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            assert x0.shape == (self.n,)
        max_iter = int(max_iter)
        x = np.zeros(self.n, dtype=np.float64)
        v, i, g = (np.zeros(D, dtype=np.float64) for _ in range(3))
        iterates = np.zeros((max_iter, self.n), dtype=np.float64) if keep_iterates else None
        vh = np.zeros((max_iter + 1, D), dtype=np.float64) if keep_iterates else None
        record = np.zeros((max_iter, 4), dtype=np.float64)
        info, iters, route = (np.zeros(max_iter, dtype=np.int32) for _ in range(3))
        iterations, converged = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.nodal_newton_dc(
            self._h, int(dense), D, _ptr(diode_rows, C.c_int64) if D else None, _ptr(i_sat, C.c_double) if D else None,
            _ptr(n_vt, C.c_double) if D else None, float(gmin), len(rows), _ptr(rows, C.c_int64) if len(rows) else None,
            _ptr(values, C.c_double) if len(rows) else None, _ptr(x0, C.c_double) if x0 is not None else None, max_iter,
            float(reltol), float(vntol), float(abstol), _ptr(x, C.c_double) if self.n else None,
            _ptr(v, C.c_double) if D else None, _ptr(i, C.c_double) if D else None, _ptr(g, C.c_double) if D else None,
            _ptr(iterates, C.c_double) if keep_iterates and self.n else None, _ptr(vh, C.c_double) if keep_iterates and D else None,
            _ptr(record, C.c_double), _ptr(info, C.c_int32), _ptr(iters, C.c_int32), _ptr(route, C.c_int32),
            C.byref(iterations), C.byref(converged)))
        r = iterations.value
        return {"x": x, "v": v, "i": i, "g": g, "iterations": r, "converged": bool(converged.value), "record": record[:r],
                "info": info[:r], "iters": iters[:r], "route": route[:r],
                "iterates": iterates[:r] if keep_iterates else None, "vh": vh[:r + 1] if keep_iterates else None}

    def newton_dc_bjt(self, diode_rows, i_sat, n_vt, gmin, gm_rows, junction, i_s, rows, values, x0, dense, max_iter, reltol,
                      vntol, abstol, keep_iterates=False):
        """newton_dc() with bipolar transistors (nodal_newton_dc_bjt): the handle's table holds two GM rows per
        transport beside the diodes' rows -- gm_rows int64 [T, 2] (forward, reverse), junction int32 [T, 2] (indices into
        the diodes: jf, jr), i_s [T].  Returns newton_dc()'s dict with record [iterations, 5] (the fifth word: transports
        that failed the test) and it, gmf, gmr [T] of the last iterate.  T == 0 is newton_dc(), bit for bit."""
        diode_rows = np.ascontiguousarray(diode_rows, dtype=np.int64)
        i_sat, n_vt = (np.ascontiguousarray(v, dtype=np.float64) for v in (i_sat, n_vt))
        D = len(diode_rows)
        assert diode_rows.ndim == 1 and i_sat.shape == (D,) and n_vt.shape == (D,)
        gm_rows = np.ascontiguousarray(gm_rows, dtype=np.int64).reshape(-1, 2)
        junction = np.ascontiguousarray(junction, dtype=np.int32).reshape(-1, 2)
        i_s = np.ascontiguousarray(i_s, dtype=np.float64)
        T = len(gm_rows)
        assert junction.shape == (T, 2) and i_s.shape == (T,)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.shape == (len(rows),)
        if x0 is not None:
            x0 = np.ascontiguousarray(x0, dtype=np.float64)
            assert x0.shape == (self.n,)
        max_iter = int(max_iter)
        x = np.zeros(self.n, dtype=np.float64)
        v, i, g = (np.zeros(D, dtype=np.float64) for _ in range(3))
        it, gmf, gmr = (np.zeros(T, dtype=np.float64) for _ in range(3))
        iterates = np.zeros((max_iter, self.n), dtype=np.float64) if keep_iterates else None
        vh = np.zeros((max_iter + 1, D), dtype=np.float64) if keep_iterates else None
        record = np.zeros((max_iter, 5), dtype=np.float64)
        info, iters, route = (np.zeros(max_iter, dtype=np.int32) for _ in range(3))
        iterations, converged = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.nodal_newton_dc_bjt(
            self._h, int(dense), D, _ptr(diode_rows, C.c_int64) if D else None, _ptr(i_sat, C.c_double) if D else None,
            _ptr(n_vt, C.c_double) if D else None, float(gmin), len(rows), _ptr(rows, C.c_int64) if len(rows) else None,
            _ptr(values, C.c_double) if len(rows) else None, _ptr(x0, C.c_double) if x0 is not None else None, max_iter,
            float(reltol), float(vntol), float(abstol), T, _ptr(gm_rows, C.c_int64) if T else None,
            _ptr(junction, C.c_int32) if T else None, _ptr(i_s, C.c_double) if T else None,
            _ptr(x, C.c_double) if self.n else None, _ptr(v, C.c_double) if D else None, _ptr(i, C.c_double) if D else None,
            _ptr(g, C.c_double) if D else None, _ptr(it, C.c_double) if T else None, _ptr(gmf, C.c_double) if T else None,
            _ptr(gmr, C.c_double) if T else None, _ptr(iterates, C.c_double) if keep_iterates and self.n else None,
            _ptr(vh, C.c_double) if keep_iterates and D else None, _ptr(record, C.c_double), _ptr(info, C.c_int32),
            _ptr(iters, C.c_int32), _ptr(route, C.c_int32), C.byref(iterations), C.byref(converged)))
        r = iterations.value
        return {"x": x, "v": v, "i": i, "g": g, "it": it, "gmf": gmf, "gmr": gmr, "iterations": r,
                "converged": bool(converged.value), "record": record[:r], "info": info[:r], "iters": iters[:r],
                "route": route[:r], "iterates": iterates[:r] if keep_iterates else None,
                "vh": vh[:r + 1] if keep_iterates else None}

    def newton_gradient(self, diode_rows, i_sat, n_vt, gmin, rows, values, x, cotangent, dense, adjoints=False):
        """The adjoint of the Newton solve at the operating point x (nodal_newton_gradient), on a handle that holds the
        circuit with one companion resistor per diode: diode_rows, i_sat, n_vt [D], gmin and the one setting values
        [len(rows)] of the swept sources as newton_dc() took them, x [n] its answer, cotangent [n] = dL/dx.  Returns a
        dict: grad [ncomp] of this handle's table (+0.0 in the companion rows), i_sat, n_vt [D], gmin (float), sources
        [len(rows)], adjoint [n] or None, resid and op_resid (floats: the scaled residuals of the transposed solve and of
        x as an operating point), info; NodalHipError(E_INVALID) as the header lists, with dense a singular J raises
        NodalHipError(E_SINGULAR)."""
        diode_rows = np.ascontiguousarray(diode_rows, dtype=np.int64)
        i_sat, n_vt = (np.ascontiguousarray(v, dtype=np.float64) for v in (i_sat, n_vt))
        D = len(diode_rows)
        assert diode_rows.ndim == 1 and i_sat.shape == (D,) and n_vt.shape == (D,)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.shape == (len(rows),)
        x, cot = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, cotangent))
        assert x.shape == (self.n,) and cot.shape == (self.n,)
        grad = np.zeros(self._ncomp, dtype=np.float64)
        gis, gnv = np.zeros(D, dtype=np.float64), np.zeros(D, dtype=np.float64)
        gsrc = np.zeros(len(rows), dtype=np.float64)
        lam = np.zeros(self.n, dtype=np.float64) if adjoints else None
        ggmin, resid, op_resid, info = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
        self._check(self.lib.nodal_newton_gradient(
            self._h, int(dense), D, _ptr(diode_rows, C.c_int64) if D else None, _ptr(i_sat, C.c_double) if D else None,
            _ptr(n_vt, C.c_double) if D else None, float(gmin), len(rows), _ptr(rows, C.c_int64) if len(rows) else None,
            _ptr(values, C.c_double) if len(rows) else None, _ptr(x, C.c_double) if self.n else None,
            _ptr(cot, C.c_double) if self.n else None, _ptr(grad, C.c_double), _ptr(gis, C.c_double) if D else None,
            _ptr(gnv, C.c_double) if D else None, C.byref(ggmin), _ptr(gsrc, C.c_double) if len(rows) else None,
            _ptr(lam, C.c_double) if adjoints and self.n else None, C.byref(resid), C.byref(op_resid),
            C.byref(info)))
        return {"grad": grad, "i_sat": gis, "n_vt": gnv, "gmin": ggmin.value, "sources": gsrc, "adjoint": lam,
                "resid": resid.value, "op_resid": op_resid.value, "info": int(info.value)}

    def transient_gradient(self, steps, nsrc, ia, ib, cotangents, dense, adjoints=False):
        """The adjoint of the transient run this handle recorded (nodal_transient_gradient; OPT_TRANSIENT_TAPE): steps
        and nsrc those of that run, (ia, ib) the probes' node indices, cotangents [steps + 1, P] = dL / d waveforms.
        Returns (grad [ncomp] of this handle's table, companion rows included, source derivatives [steps, nsrc], dL/dx0
        [n], adjoints [steps, n] or None, scaled residual [steps], info [steps]); NodalHipError(E_INVALID) without a
        valid tape, with dense a singular G raises NodalHipError(E_SINGULAR)."""
        ia, ib = (np.ascontiguousarray(v, dtype=np.int32) for v in (ia, ib))
        assert ia.ndim == 1 and ib.shape == ia.shape
        cot = np.ascontiguousarray(cotangents, dtype=np.float64)
        assert cot.shape == (steps + 1, len(ia))
        grad = np.zeros(self._ncomp, dtype=np.float64)
        gsrc = np.zeros((steps, nsrc), dtype=np.float64)
        gx0 = np.zeros(self.n, dtype=np.float64)
        lam = host_empty(steps * self.n, np.float64).reshape(steps, self.n) if adjoints else None
        resid = np.zeros(steps, dtype=np.float64)
        info = np.zeros(steps, dtype=np.int32)
        self._check(self.lib.nodal_transient_gradient(
            self._h, int(dense), len(ia), _ptr(ia, C.c_int32) if len(ia) else None, _ptr(ib, C.c_int32) if len(ib) else None,
            _ptr(cot, C.c_double) if cot.size else None, _ptr(grad, C.c_double), _ptr(gsrc, C.c_double),
            _ptr(gx0, C.c_double), _ptr(lam, C.c_double) if adjoints and steps else None, _ptr(resid, C.c_double),
            _ptr(info, C.c_int32)))
        return grad, gsrc, gx0, lam, resid, info

    def ac_sweep(self, omega, kind, value, lead_a, lead_b, rows, amplitudes, ia, ib, cur_index, dense, keep_every=0,
                 peaks=False):
        """Frequency sweep on the circuit's own handle (nodal_ac_sweep): omega [F] in rad/s, the reactive elements as
        kind [E] (0 capacitor, 1 inductor), value [E], lead_a / lead_b [E] node indices, rows [R] the driven A / E rows
        with their complex amplitudes [R] (every other source is off), (ia, ib) the probes' node indices, cur_index [Q]
        the elements whose currents are wanted.  Returns (phasors complex128 [F, P], currents complex128 [F, Q],
        solutions complex128 [F // keep_every, n] or None, (peak magnitude [K], peak frequency index [K]) or None,
        scaled residual [F], info [F]); NodalHipError(E_INVALID) as the header lists, with dense a singular frequency
        raises NodalHipError(E_SINGULAR)."""
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        kind = np.ascontiguousarray(kind, dtype=np.uint8)
        value = np.ascontiguousarray(value, dtype=np.float64)
        lead_a, lead_b = (np.ascontiguousarray(v, dtype=np.int32) for v in (lead_a, lead_b))
        assert omega.ndim == 1 and kind.ndim == 1 and value.shape == kind.shape == lead_a.shape == lead_b.shape
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        amplitudes = np.asarray(amplitudes, dtype=np.complex128)
        assert rows.ndim == 1 and amplitudes.shape == rows.shape
        src_re, src_im = np.ascontiguousarray(amplitudes.real), np.ascontiguousarray(amplitudes.imag)
        ia, ib = (np.ascontiguousarray(v, dtype=np.int32) for v in (ia, ib))
        assert ia.ndim == 1 and ib.shape == ia.shape
        cur_index = np.ascontiguousarray(cur_index, dtype=np.int32)
        assert cur_index.ndim == 1
        nfreq, K = len(omega), self._K
        wave = np.zeros((nfreq, len(ia)), dtype=np.complex128)
        cur = np.zeros((nfreq, len(cur_index)), dtype=np.complex128)
        kept = nfreq // keep_every if keep_every > 0 else 0
        x = np.zeros((kept, self.n), dtype=np.complex128) if keep_every > 0 else None
        peak = (np.empty(K), np.empty(K, dtype=np.int32)) if peaks else None
        resid = np.zeros(nfreq, dtype=np.float64)
        info = np.zeros(nfreq, dtype=np.int32)

        def opt(arr, ctype):  # (an empty array goes as NULL)
            return _ptr(arr, ctype) if arr is not None and arr.size else None

        self._check(self.lib.nodal_ac_sweep(
            self._h, int(dense), nfreq, opt(omega, C.c_double), len(kind), opt(kind, C.c_uint8), opt(value, C.c_double),
            opt(lead_a, C.c_int32), opt(lead_b, C.c_int32), len(rows), opt(rows, C.c_int64), opt(src_re, C.c_double),
            opt(src_im, C.c_double), len(ia), opt(ia, C.c_int32), opt(ib, C.c_int32), opt(wave, C.c_double), len(cur_index),
            opt(cur_index, C.c_int32), opt(cur, C.c_double), int(keep_every), opt(x, C.c_double),
            opt(peak[0], C.c_double) if peaks else None, opt(peak[1], C.c_int32) if peaks else None,
            _ptr(resid, C.c_double), _ptr(info, C.c_int32)))
        return wave, cur, x, peak, resid, info

    def ac_noise(self, omega, kind, value, lead_a, lead_b, temperature, oa, ob, dense, input_row=-1, weight=None):
        """Thermal-noise spectra on the circuit's own handle (nodal_ac_noise): omega [F] in rad/s and the reactive
        elements as ac_sweep takes them, the temperature in kelvin, (oa, ob) the outputs' node indices [P], input_row
        the A / E row the gain is taken from (-1: none), weight [F] the quadrature weights of the integrated
        contributions (None: none are made).  Returns (density [F, P], gain complex128 [F, P] or None, contributions
        [P, ncomp] or None, scaled residual [F, P], info [F]); NodalHipError(E_INVALID) as the header lists, with dense
        a singular frequency raises NodalHipError(E_SINGULAR)."""
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        kind = np.ascontiguousarray(kind, dtype=np.uint8)
        value = np.ascontiguousarray(value, dtype=np.float64)
        lead_a, lead_b = (np.ascontiguousarray(v, dtype=np.int32) for v in (lead_a, lead_b))
        assert omega.ndim == 1 and kind.ndim == 1 and value.shape == kind.shape == lead_a.shape == lead_b.shape
        oa, ob = (np.ascontiguousarray(v, dtype=np.int32) for v in (oa, ob))
        assert oa.ndim == 1 and ob.shape == oa.shape
        nfreq, nout = len(omega), len(oa)
        if weight is not None:
            weight = np.ascontiguousarray(weight, dtype=np.float64)
            assert weight.shape == omega.shape
        density = np.zeros((nfreq, nout), dtype=np.float64)
        gain = np.zeros((nfreq, nout), dtype=np.complex128) if input_row >= 0 else None
        contrib = np.zeros((nout, self._ncomp), dtype=np.float64) if weight is not None else None
        resid = np.zeros((nfreq, nout), dtype=np.float64)
        info = np.zeros(nfreq, dtype=np.int32)

        def opt(arr, ctype):  # (an empty array goes as NULL)
            return _ptr(arr, ctype) if arr is not None and arr.size else None

        self._check(self.lib.nodal_ac_noise(
            self._h, int(dense), nfreq, opt(omega, C.c_double), len(kind), opt(kind, C.c_uint8), opt(value, C.c_double),
            opt(lead_a, C.c_int32), opt(lead_b, C.c_int32), float(temperature), nout, opt(oa, C.c_int32), opt(ob, C.c_int32),
            int(input_row), _ptr(weight, C.c_double) if weight is not None else None, opt(density, C.c_double),
            _ptr(gain, C.c_double) if gain is not None else None,
            _ptr(contrib, C.c_double) if contrib is not None else None, _ptr(resid, C.c_double), _ptr(info, C.c_int32)))
        return density, gain, contrib, resid, info

    def ac_ports(self, omega, kind, value, lead_a, lead_b, ia, ib, dense, peaks=False):
        """The multiport impedance matrix over a frequency sweep on the circuit's own handle (nodal_ac_ports): omega [F]
        in rad/s and the reactive elements as ac_sweep takes them, (ia, ib) the ports' node indices [P].  Returns (z
        complex128 [F, P, P], (peak magnitude [K], peak port int32 [K], peak frequency index int32 [K]) or None, scaled
        residual [F, P], info [F], work int64 [3]: numeric factorisations, block applications of the sparse factors,
        columns redone alone); NodalHipError(E_INVALID) as the header lists, with dense a singular frequency raises
        NodalHipError(E_SINGULAR)."""
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        kind = np.ascontiguousarray(kind, dtype=np.uint8)
        value = np.ascontiguousarray(value, dtype=np.float64)
        lead_a, lead_b = (np.ascontiguousarray(v, dtype=np.int32) for v in (lead_a, lead_b))
        assert omega.ndim == 1 and kind.ndim == 1 and value.shape == kind.shape == lead_a.shape == lead_b.shape
        ia, ib = (np.ascontiguousarray(v, dtype=np.int32) for v in (ia, ib))
        assert ia.ndim == 1 and ib.shape == ia.shape
        nfreq, nports, K = len(omega), len(ia), self._K
        z = np.zeros((nfreq, nports, nports), dtype=np.complex128)
        peak = None
        if peaks:  # (what the library leaves when no frequency is solved, for the calls that do nothing as well)
            peak = (np.full(K, np.nan), np.full(K, -1, dtype=np.int32), np.full(K, -1, dtype=np.int32))
        resid = np.zeros((nfreq, nports), dtype=np.float64)
        info = np.zeros(nfreq, dtype=np.int32)
        work = np.zeros(3, dtype=np.int64)

        def opt(arr, ctype):  # (an empty array goes as NULL)
            return _ptr(arr, ctype) if arr is not None and arr.size else None

        self._check(self.lib.nodal_ac_ports(
            self._h, int(dense), nfreq, opt(omega, C.c_double), len(kind), opt(kind, C.c_uint8), opt(value, C.c_double),
            opt(lead_a, C.c_int32), opt(lead_b, C.c_int32), nports, opt(ia, C.c_int32), opt(ib, C.c_int32),
            opt(z, C.c_double), opt(peak[0], C.c_double) if peaks else None, opt(peak[1], C.c_int32) if peaks else None,
            opt(peak[2], C.c_int32) if peaks else None, opt(resid, C.c_double), opt(info, C.c_int32),
            _ptr(work, C.c_int64)))
        return z, peak, resid, info, work

    def ac_gradient(self, omega, kind, value, lead_a, lead_b, rows, amplitudes, ia, ib, cotangents, dense, adjoints=False):
        """The adjoint of the frequency sweep on the circuit's own handle (nodal_ac_gradient): omega [F] in rad/s, the
        reactive elements, the driven rows with their complex amplitudes and the probes as ac_sweep takes them,
        cotangents complex128 [F, P] = dL/dRe W + j dL/dIm W of the probe phasors W.  Returns (phasors complex128
        [F, P], grad [ncomp], grad_reactive [E], source terms complex128 [F, R], adjoints complex128 [F, n] or None,
        scaled residual [F, 2] of the forward and the adjoint system, info [F], work int64 [3] as ac_ports counts it);
        NodalHipError(E_INVALID) as the header lists, with dense a singular frequency raises
        NodalHipError(E_SINGULAR)."""
        omega = np.ascontiguousarray(omega, dtype=np.float64)
        kind = np.ascontiguousarray(kind, dtype=np.uint8)
        value = np.ascontiguousarray(value, dtype=np.float64)
        lead_a, lead_b = (np.ascontiguousarray(v, dtype=np.int32) for v in (lead_a, lead_b))
        assert omega.ndim == 1 and kind.ndim == 1 and value.shape == kind.shape == lead_a.shape == lead_b.shape
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        amplitudes = np.asarray(amplitudes, dtype=np.complex128)
        assert rows.ndim == 1 and amplitudes.shape == rows.shape
        src_re, src_im = np.ascontiguousarray(amplitudes.real), np.ascontiguousarray(amplitudes.imag)
        ia, ib = (np.ascontiguousarray(v, dtype=np.int32) for v in (ia, ib))
        assert ia.ndim == 1 and ib.shape == ia.shape
        nfreq, nprobe = len(omega), len(ia)
        cot = np.ascontiguousarray(cotangents, dtype=np.complex128)
        assert cot.shape == (nfreq, nprobe)
        wave = np.zeros((nfreq, nprobe), dtype=np.complex128)
        grad = np.zeros(self._ncomp, dtype=np.float64)
        greact = np.zeros(len(kind), dtype=np.float64)
        gsrc = np.zeros((nfreq, len(rows)), dtype=np.complex128)
        lam = np.zeros((nfreq, self.n), dtype=np.complex128) if adjoints else None
        resid = np.zeros((nfreq, 2), dtype=np.float64)
        info = np.zeros(nfreq, dtype=np.int32)
        work = np.zeros(3, dtype=np.int64)

        def opt(arr, ctype):  # (an empty array goes as NULL)
            return _ptr(arr, ctype) if arr is not None and arr.size else None

        self._check(self.lib.nodal_ac_gradient(
            self._h, int(dense), nfreq, opt(omega, C.c_double), len(kind), opt(kind, C.c_uint8), opt(value, C.c_double),
            opt(lead_a, C.c_int32), opt(lead_b, C.c_int32), len(rows), opt(rows, C.c_int64), opt(src_re, C.c_double),
            opt(src_im, C.c_double), nprobe, opt(ia, C.c_int32), opt(ib, C.c_int32), opt(cot, C.c_double),
            opt(wave, C.c_double), opt(grad, C.c_double), opt(greact, C.c_double), opt(gsrc, C.c_double),
            1 if adjoints else 0, opt(lam, C.c_double), opt(resid, C.c_double), opt(info, C.c_int32), _ptr(work, C.c_int64)))
        return wave, grad, greact, gsrc, lam, resid, info, work

    def debug_sources_rhs(self, rows, values):
        """The right-hand sides solve_sources builds, [M, n] (testing hook)."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.ndim == 2 and values.shape[1] == len(rows)
        out = np.empty((values.shape[0], self.n), dtype=np.float64)
        self._check(self.lib.nodal_debug_sources_rhs(self._h, values.shape[0], len(rows), _ptr(rows, C.c_int64),
                                                     _ptr(values, C.c_double), _ptr(out, C.c_double)))
        return out

    def debug_residual(self, x, b=None, cols=0, layout=0, transposed=False):
        """The library's residual judges on vectors of the caller's choosing (testing hook).  cols 0: the
        single-vector judge on x [n], b [n] (None: the assembled right-hand side); returns (scaled residual,
        norms [5] = max|Gx-b|, max row sum |G|, max|x|, max|b|, poison flag).  cols 1..16: the block judge on x, b of
        shape [cols, n] (layout 0), [n, 16] (layout 1) or [n] (layout 2, cols 1); returns (scaled [cols], norms
        [16, 4]: per column max|b-Gx|, max|x|, max|b|; [0, 3] = max row sum |G|).  transposed: against the G^T the
        last sensitivities() call left on the handle."""
        shape = (self.n,) if cols == 0 or layout == 2 else (cols, self.n) if layout == 0 else (self.n, 16)
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == shape, (x.shape, shape)
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.float64)
            assert b.shape == shape, (b.shape, shape)
        scaled = np.zeros(max(cols, 1), dtype=np.float64)
        norms = np.zeros(5 if cols == 0 else 64, dtype=np.float64)
        self._check(self.lib.nodal_debug_residual(self._h, int(bool(transposed)), cols, layout, _ptr(x, C.c_double),
                                                  _ptr(b, C.c_double) if b is not None else None,
                                                  _ptr(scaled, C.c_double), _ptr(norms, C.c_double)))
        return (float(scaled[0]), norms) if cols == 0 else (scaled, norms.reshape(16, 4))

    def debug_direct_apply(self, r, cols=1, transposed=False):
        """z = (the sparse direct route's factors)^-1 r and nothing else: one factorisation, one substitution, no
        refinement (testing hook).  cols 1: r [n]; cols 16: r [n, 16], sixteen columns interleaved by row.
        transposed: the G^T the last sensitivities() call left on the handle.  Returns (z, replaced pivots, info)."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        assert r.shape == ((self.n,) if cols == 1 else (self.n, cols)), (r.shape, cols)
        z = np.full(r.shape, np.nan, dtype=np.float64)
        perturbed, info = C.c_int64(-1), C.c_int32(-1)
        self._check(self.lib.nodal_debug_direct_apply(self._h, int(bool(transposed)), cols, _ptr(r, C.c_double),
                                                      _ptr(z, C.c_double), C.byref(perturbed), C.byref(info)))
        return z, perturbed.value, info.value

    def debug_hierarchy(self):
        """The multigrid hierarchy of the last sparse solve as the setup left it (testing hook): a list with one dict
        per level -- the info words (HIERARCHY_INFO, ints), "omega_p" and "omega", and every device buffer of
        HIERARCHY_ARRAYS as a flat numpy array in the kernels' own layout, padding included (empty where the level
        has none); the last level's dict also holds "coarse_inv" (flat, n x n row-major; empty without a dense
        coarsest level).  Nothing is decoded here."""
        nlev = C.c_int32(0)
        ints = np.zeros((12, 16), dtype=np.int64)
        reals = np.zeros((12, 2), dtype=np.float64)
        self._check(self.lib.nodal_debug_hierarchy_info(self._h, C.byref(nlev), _ptr(ints, C.c_int64),
                                                        _ptr(reals, C.c_double)))

        def fetch(level, which, dtype):
            size = C.c_int64(0)
            self._check(self.lib.nodal_debug_hierarchy_array(self._h, level, which, None, 0, C.byref(size)))
            out = np.empty(size.value // np.dtype(dtype).itemsize, dtype=dtype)
            if size.value:
                self._check(self.lib.nodal_debug_hierarchy_array(self._h, level, which, C.c_void_p(out.ctypes.data),
                                                                 out.nbytes, C.byref(size)))
                assert size.value == out.nbytes
            return out

        levels = []
        for l in range(nlev.value):
            lv = {name: int(ints[l, k]) for k, name in enumerate(HIERARCHY_INFO)}
            lv["omega_p"], lv["omega"] = float(reals[l, 0]), float(reals[l, 1])
            for which, (name, dtype) in enumerate(HIERARCHY_ARRAYS):
                lv[name] = fetch(l, which, dtype)
            levels.append(lv)
        levels[-1]["coarse_inv"] = fetch(-1, 0, np.float64)
        return levels

    def debug_cycle_apply(self, r, mode=0, u=None, frozen=None):
        """z = ONE application of the multigrid cycle to r, nothing behind it (testing hook; nodal_hip.h).  mode 0: the
        general route's call; 1: the flexible CG's (z stored in f32); 2: the block cycle, r [n0, 16].  u (modes 1, 2;
        zeros when not given) stands where the iteration keeps A p.  frozen: (s1, s2, t), [16, 3] in mode 2, for a
        frozen K-cycle; None: adaptive.  Returns (z, dots, params): dots None / [2] / [2, 16] = z.r and z.u as the
        device summed them, params a dict of CYCLE_PARAMS."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        assert r.ndim == (2 if mode == 2 else 1) and (mode != 2 or r.shape[1] == 16), (r.shape, mode)
        if u is None and mode != 0:
            u = np.zeros_like(r)
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            assert u.shape == r.shape, (u.shape, r.shape)
        if frozen is not None:
            frozen = np.ascontiguousarray(frozen, dtype=np.float64)
            assert frozen.shape == ((16, 3) if mode == 2 else (3,)), frozen.shape
        z = np.full(r.shape, np.nan, dtype=np.float64)
        dots = np.full((2, 16) if mode == 2 else 2, np.nan, dtype=np.float64)
        params = np.zeros(16, dtype=np.int32)
        self._check(self.lib.nodal_debug_cycle_apply(self._h, mode, _ptr(r, C.c_double),
                                                     _ptr(u, C.c_double) if u is not None else None,
                                                     _ptr(frozen, C.c_double) if frozen is not None else None,
                                                     _ptr(z, C.c_double), _ptr(dots, C.c_double), _ptr(params, C.c_int32)))
        return z, (None if mode == 0 else dots), {name: int(params[k]) for k, name in enumerate(CYCLE_PARAMS)}

    def debug_amg(self):
        """The plain-aggregation hierarchy (csrc/amg.hip) the last sparse solve preconditioned with, raw (testing
        hook): (levels, info).  levels: one dict per level with the words of AMG_LEVEL_INFO and every buffer of
        AMG_ARRAYS as a flat numpy array (empty where the level has none).  info: the words of AMG_WORDS, "theta",
        "OMEGA", "coarse_inv" (flat, row-major; empty without one), "tail_image" (uint8; empty without a tail) and
        "tdesc": None or the words of AMG_TAIL_WORDS plus "lv", a list of dicts of AMG_TAIL_LEVEL.  Nothing is
        decoded here.  NodalHipError (NODAL_E_INVALID) when that solve used another preconditioner or none."""
        nlev = C.c_int32(0)
        ints = np.zeros((16, 8), dtype=np.int64)
        words = np.zeros(16, dtype=np.int64)
        reals = np.zeros(2, dtype=np.float64)
        tail = np.zeros(128, dtype=np.int64)
        self._check(self.lib.nodal_debug_amg_info(self._h, C.byref(nlev), _ptr(ints, C.c_int64), _ptr(words, C.c_int64),
                                                  _ptr(reals, C.c_double), _ptr(tail, C.c_int64)))

        def fetch(level, which, dtype):
            size = C.c_int64(0)
            self._check(self.lib.nodal_debug_amg_array(self._h, level, which, None, 0, C.byref(size)))
            out = np.empty(size.value // np.dtype(dtype).itemsize, dtype=dtype)
            if size.value:
                self._check(self.lib.nodal_debug_amg_array(self._h, level, which, C.c_void_p(out.ctypes.data),
                                                           out.nbytes, C.byref(size)))
                assert size.value == out.nbytes
            return out

        levels = []
        for l in range(nlev.value):
            lv = {name: int(ints[l, k]) for k, name in enumerate(AMG_LEVEL_INFO)}
            for which, (name, dtype) in enumerate(AMG_ARRAYS):
                lv[name] = fetch(l, which, dtype)
            levels.append(lv)
        info = {name: int(words[k]) for k, name in enumerate(AMG_WORDS)}
        info["theta"], info["OMEGA"] = float(reals[0]), float(reals[1])
        info["coarse_inv"] = fetch(AMG_LEVEL_COARSE_INV, 0, np.float64)
        info["tail_image"] = fetch(AMG_LEVEL_TAIL_IMAGE, 0, np.uint8)
        info["tdesc"] = None
        if info["tail"] >= 0:
            td = {name: int(tail[k]) for k, name in enumerate(AMG_TAIL_WORDS)}
            td["lv"] = [{name: int(tail[8 + 14 * k + j]) for j, name in enumerate(AMG_TAIL_LEVEL)}
                        for k in range(td["nlev"])]
            info["tdesc"] = td
        return levels, info

    def debug_amg_apply(self, r, level=0):
        """z = ONE cycle of the plain-aggregation hierarchy at `level` (outside the tail) applied to r, nothing behind
        it (testing hook; nodal_hip.h).  Returns (z, params): params a dict of AMG_APPLY_PARAMS."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        assert r.ndim == 1, r.shape
        nlev, ints = C.c_int32(0), np.zeros((16, 8), dtype=np.int64)
        words, reals, tail = np.zeros(16, dtype=np.int64), np.zeros(2), np.zeros(128, dtype=np.int64)
        self._check(self.lib.nodal_debug_amg_info(self._h, C.byref(nlev), _ptr(ints, C.c_int64), _ptr(words, C.c_int64),
                                                  _ptr(reals, C.c_double), _ptr(tail, C.c_int64)))
        if 0 <= level < nlev.value:  # (the library reads the level's n entries; it answers for any other level itself)
            assert r.shape[0] == ints[level, 0], (r.shape, int(ints[level, 0]))
        z = np.full(r.shape, np.nan, dtype=np.float64)
        params = np.zeros(16, dtype=np.int32)
        self._check(self.lib.nodal_debug_amg_apply(self._h, level, _ptr(r, C.c_double), _ptr(z, C.c_double),
                                                   _ptr(params, C.c_int32)))
        return z, {name: int(params[k]) for k, name in enumerate(AMG_APPLY_PARAMS)}

    def debug_fgmres_cycle(self, system=0, precond=0, window=FG_MAXV, max_cols=FG_RESTART, rel_tol=0.0, b=None, n=None):
        """ONE restart cycle of the general route's flexible GMRES, nothing behind it (testing hook; nodal_hip.h).
        system 0: the handle's G; 1: the presolved system of the last sparse solve (pass its n, or leave it to a first
        sizing call).  precond 0: the block preconditioner; 1: the sparse direct factors.  Returns a dict: x [n],
        V [count + 1, n], Z [count, n], H [41, 40], cs [40], sn [40], g [41], y [41], gst (the whole block), rnorm,
        bnorm, inv_h, est, done, tolb and the words of FGMRES_PARAMS."""
        if n is None and system == 0:
            n = self.n
        elif n is None:  # (a presolved system that reached the iteration has a hierarchy: level 0 is the system)
            nlev, ints, reals = C.c_int32(0), np.zeros((12, 16), dtype=np.int64), np.zeros((12, 2))
            self._check(self.lib.nodal_debug_hierarchy_info(self._h, C.byref(nlev), _ptr(ints, C.c_int64),
                                                            _ptr(reals, C.c_double)))
            n = int(ints[0, 0])
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.float64)
            assert b.shape == (n,), (b.shape, n)
        x = np.full(n, np.nan)
        V = np.full((max_cols + 1, n), np.nan)
        Z = np.full((max_cols, n), np.nan)
        gst = np.full(FG_WORDS, np.nan)
        y = np.full(FG_MAXV, np.nan)
        norms = np.full(2, np.nan)
        params = np.zeros(16, dtype=np.int64)
        self._check(self.lib.nodal_debug_fgmres_cycle(self._h, system, precond, window, max_cols, float(rel_tol), n,
                                                      _ptr(b, C.c_double) if b is not None else None, _ptr(x, C.c_double),
                                                      _ptr(V, C.c_double), _ptr(Z, C.c_double), _ptr(gst, C.c_double),
                                                      _ptr(y, C.c_double), _ptr(norms, C.c_double), _ptr(params, C.c_int64)))
        out = {name: int(params[k]) for k, name in enumerate(FGMRES_PARAMS)}
        count = out["count"]
        assert out["n"] == n and 0 <= count <= max_cols, (out, n)
        out.update(x=x, V=V[:count + 1] if count else V[:0], Z=Z[:count], gst=gst, y=y,
                   H=gst[FG_H:FG_CS].reshape(FG_MAXV, FG_RESTART), cs=gst[FG_CS:FG_SN], sn=gst[FG_SN:FG_G],
                   g=gst[FG_G:FG_INV_H], inv_h=float(gst[FG_INV_H]), est=float(gst[FG_EST]), done=float(gst[FG_DONE]),
                   gcount=float(gst[FG_COUNT]), tolb=float(gst[FG_TOLB]), rnorm=float(norms[0]), bnorm=float(norms[1]))
        return out

    def debug_presolve_build(self):
        """Plan, rewrite and reduced assembly of the presolve for the assembled member, as a sparse solve does them and
        nothing behind them (testing hook; nodal_hip.h).  Returns a dict: the words of PRESOLVE_INFO (ok False: the
        plan declined; built False: the rewrite met a row it cannot express) and the arrays of PRESOLVE_ARRAYS the
        build reached -- the plan's always, newidx, the reduced table (r_*), CSR and right-hand side when built."""
        info = np.zeros(16, dtype=np.int64)
        self._check(self.lib.nodal_debug_presolve_build(self._h, _ptr(info, C.c_int64)))
        out = {name: int(info[k]) for k, name in enumerate(PRESOLVE_INFO)}
        for which, (name, dtype) in enumerate(PRESOLVE_ARRAYS):
            if which >= PRESOLVE_PLAN_ARRAYS and not out["built"]:
                break
            size = C.c_int64(0)
            self._check(self.lib.nodal_debug_presolve_array(self._h, which, None, 0, C.byref(size)))
            arr = np.empty(size.value // np.dtype(dtype).itemsize, dtype=dtype)
            if size.value:
                self._check(self.lib.nodal_debug_presolve_array(self._h, which, C.c_void_p(arr.ctypes.data), arr.nbytes,
                                                                C.byref(size)))
                assert size.value == arr.nbytes
            out[name] = arr
        return out

    def debug_presolve_recover(self, y):
        """presolve_recover of the last debug_presolve_build on y (Kr + kept entries, need not solve anything): x [n],
        NaN where no recovery kernel wrote (testing hook).  The handle's solution stays as found."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        x = np.zeros(self.n)
        self._check(self.lib.nodal_debug_presolve_recover(self._h, len(y), _ptr(y, C.c_double), _ptr(x, C.c_double)))
        return x

    def debug_scan_u32(self, values, in_place=False, total=True):
        """scan_exclusive_u32 of `values` (testing hook): (the exclusive prefix sums, the device total or None)."""
        values = np.ascontiguousarray(values, dtype=np.uint32)
        out = np.empty_like(values)
        tot = C.c_uint32(0)
        self._check(self.lib.nodal_debug_scan_u32(self._h, len(values), _ptr(values, C.c_uint32), _ptr(out, C.c_uint32),
                                                  int(bool(in_place)), C.byref(tot) if total else None))
        return out, (int(tot.value) if total else None)

    def debug_lowdeg(self):
        """The rounds of the low-degree elimination as the last solve left them (testing hook; nodal_hip.h): a list
        with one dict per round -- the words of LOWDEG_INFO and the arrays of LOWDEG_ARRAYS (p_x / x empty when that
        context holds no solution).  An empty list: the last solve did not take the route."""
        nr, ints = C.c_int32(0), np.zeros((LOWDEG_MAX_ROUNDS, 8), dtype=np.int64)
        self._check(self.lib.nodal_debug_lowdeg_info(self._h, C.byref(nr), _ptr(ints, C.c_int64)))
        rounds = []
        for r in range(nr.value):
            rd = {name: int(ints[r, k]) for k, name in enumerate(LOWDEG_INFO)}
            for which, (name, dtype) in enumerate(LOWDEG_ARRAYS):
                size = C.c_int64(0)
                self._check(self.lib.nodal_debug_lowdeg_array(self._h, r, which, None, 0, C.byref(size)))
                arr = np.empty(size.value // np.dtype(dtype).itemsize, dtype=dtype)
                if size.value:
                    self._check(self.lib.nodal_debug_lowdeg_array(self._h, r, which, C.c_void_p(arr.ctypes.data),
                                                                  arr.nbytes, C.byref(size)))
                    assert size.value == arr.nbytes
                rd[name] = arr
            rounds.append(rd)
        return rounds

    def debug_floating_small(self, indptr, indices, grounded):
        """small_floating_check on a host CSR graph (testing hook): 1 if a component holds no grounded node, else 0.
        NodalHipError(E_INVALID) above 4096 nodes or for a malformed graph."""
        indptr = np.ascontiguousarray(indptr, dtype=np.int32)
        indices = np.ascontiguousarray(indices, dtype=np.int32)
        grounded = np.ascontiguousarray(grounded, dtype=np.uint8)
        n = len(indptr) - 1
        assert n >= 0 and len(grounded) == n and len(indices) == indptr[-1]
        floating = C.c_int32(-1)
        self._check(self.lib.nodal_debug_floating_small(self._h, n, _ptr(indptr, C.c_int32), _ptr(indices, C.c_int32),
                                                        _ptr(grounded, C.c_uint8), C.byref(floating)))
        return int(floating.value)

    def debug_general_arrays(self):
        """What the last precond-0 setup of debug_fgmres_cycle left, raw (testing hook): a dict of GENERAL_ARRAYS --
        the node block as CSR with gn_rowidx and gn_diag, schur = 1 / S~ per branch row, and the CSR arrays and
        right-hand side of the system that cycle ran on."""
        return {name: self._general_array(which, dtype) for which, (name, dtype) in enumerate(GENERAL_ARRAYS)}

    def _general_array(self, which, dtype):
        size = C.c_int64(0)
        self._check(self.lib.nodal_debug_general_array(self._h, which, None, 0, C.byref(size)))
        out = np.empty(size.value // np.dtype(dtype).itemsize, dtype=dtype)
        if size.value:
            self._check(self.lib.nodal_debug_general_array(self._h, which, C.c_void_p(out.ctypes.data), out.nbytes,
                                                           C.byref(size)))
            assert size.value == out.nbytes
        return out

    def download_x(self):
        x = host_empty(self.n, np.float64)
        self._check(self.lib.nodal_download_x(self._h, _ptr(x, C.c_double)))
        return x

    def residual(self):
        r = C.c_double(0)
        self._check(self.lib.nodal_residual(self._h, C.byref(r)))
        return r.value

    def run(self, dense, member=0, reuse_symbolic=False):
        info = C.c_int32(0)
        self._check(self.lib.nodal_run(self._h, int(dense), member, int(reuse_symbolic),
                                       C.byref(info)), allow=(E_SINGULAR,))
        self._refresh_sizes()
        return info.value

    def run_batch(self, first, count, reuse_symbolic=False, download=True):
        """Members [first, first + count) of the uploaded value table as one block-diagonal
        system.  Returns ([count, n] array or None, info[count])."""
        x = np.empty((count, self.n_members), dtype=np.float64) if download else None
        info = np.zeros(count, dtype=np.int32)
        self._check(self.lib.nodal_run_batch(self._h, first, count, int(reuse_symbolic),
                                             _ptr(x, C.c_double) if download else None,
                                             _ptr(info, C.c_int32)))
        return x, info

    def batch_x_to_device(self, data_ptr, capacity_bytes):
        """Copy the last run_batch's results into device memory (a torch tensor's data_ptr())."""
        self._check(self.lib.nodal_batch_x_device(self._h, C.c_void_p(data_ptr), capacity_bytes))

    def x_to_device(self, data_ptr, capacity_bytes):
        """Copy the last single-circuit solution into device memory (a torch tensor's data_ptr())."""
        self._check(self.lib.nodal_x_device(self._h, C.c_void_p(data_ptr), capacity_bytes))

    def timings(self):
        ms = (C.c_double * 3)()
        self._check(self.lib.nodal_last_timings(self._h, ms))
        return list(ms)

    def kernel_stats(self):
        ms, launches, alg = C.c_double(0), C.c_int64(0), C.c_double(0)
        self._check(self.lib.nodal_last_kernel_stats(self._h, C.byref(ms), C.byref(launches),
                                                     C.byref(alg)))
        return ms.value, launches.value, alg.value

    def set_option(self, option, value):
        self._check(self.lib.nodal_set_option(self._h, option, int(value)))

    def debug_gemm(self, A, B, Cm):
        """C - A @ B through the LU's trailing-update kernel (testing hook)."""
        A, B, Cm = (np.asfortranarray(x, dtype=np.float64) for x in (A, B, Cm))
        out = Cm.copy(order="F")
        self._check(self.lib.nodal_debug_gemm(self._h, A.shape[0], B.shape[1], A.shape[1],
                                              _ptr(A, C.c_double), _ptr(B, C.c_double),
                                              _ptr(out, C.c_double)))
        return out

    # nodal_debug_gemm_ex: kind and mode in the header's order
    GEMM_KINDS = ("plain", "tn_upper", "pair")
    GEMM_MODES = ("sub", "set", "setneg")
    # nodal_debug_block_inverse: variant in the header's order
    INVERSE_VARIANTS = ("rank16_dpp", "rank16_bpermute", "rank4", "scalar")

    def debug_gemm_ex(self, kind, mode, sizes, A, B, Cm, band=128, second=None):
        """An entry point of gemm_f64.hip on arrays whose row counts ARE the leading dimensions (testing hook): sizes =
        (M, N, K), A [lda, K] (kind "tn_upper": the K x M panel, [lda, M]), B [ldb, N], Cm [ldc, N].  kind "pair":
        second = (sizes2, A2, B2, C2).  Returns the whole C image(s), padding rows included."""
        def prep(sizes, A_, B_, C_):
            A_, B_ = (np.asfortranarray(x, dtype=np.float64) for x in (A_, B_))
            out = np.array(C_, dtype=np.float64, order="F", copy=True)
            M, N, K = sizes
            assert B_.shape[1] == N and out.shape[1] == N and A_.shape[1] == (M if kind == "tn_upper" else K)
            return [M, N, K, _ptr(A_, C.c_double), A_.shape[0], _ptr(B_, C.c_double), B_.shape[0],
                    _ptr(out, C.c_double), out.shape[0]], (A_, B_, out)
        a0, keep0 = prep(sizes, A, B, Cm)
        if second is not None:
            a1, keep1 = prep(*second)
        else:
            a1, keep1 = [0, 0, 0, None, 0, None, 0, None, 0], (None, None, None)
        self._check(self.lib.nodal_debug_gemm_ex(self._h, self.GEMM_KINDS.index(kind), self.GEMM_MODES.index(mode), band,
                                                 *a0, *a1))
        return keep0[2] if second is None else (keep0[2], keep1[2])

    def debug_block_inverse(self, A, w, variant, base=0, Q=None):
        """invert_diag of block_elim.hip on the leading w x w block of the Fortran-ordered A [lda, w] (testing hook).  Q
        [ldq, w] goes up as given (default: NaN) and comes back with the inverse; returns (Q, dinfo)."""
        A = np.asfortranarray(A, dtype=np.float64)
        out = np.full((w, w), np.nan, order="F") if Q is None else np.array(Q, dtype=np.float64, order="F", copy=True)
        assert A.shape[1] == w and out.shape[1] == w
        dinfo = C.c_int32(0)
        self._check(self.lib.nodal_debug_block_inverse(self._h, w, _ptr(A, C.c_double), A.shape[0], base,
                                                       self.INVERSE_VARIANTS.index(variant), _ptr(out, C.c_double),
                                                       out.shape[0], C.byref(dinfo)))
        return out, dinfo.value

    def debug_dense_solve(self, A, B, passive=False, optimistic=False, force_pivoting=False):
        """dense_factor_solve_multi on A [n, n] and B [n, nrhs] with the dispatcher's route flags (testing hook).
        Returns (X [n, nrhs], info, rows): rows[i] = the original row that stands at position i after the interchanges
        the route applied (the identity for the routes that do not pivot)."""
        A = np.asfortranarray(A, dtype=np.float64)
        B = np.asfortranarray(B, dtype=np.float64)
        n, nrhs = B.shape
        assert A.shape == (n, n)
        X = np.full((n, nrhs), np.nan, order="F")
        ipiv = np.arange(n, dtype=np.int32)
        info = C.c_int32(0)
        route = int(bool(passive)) | int(bool(optimistic)) << 1 | int(bool(force_pivoting)) << 2
        self._check(self.lib.nodal_debug_dense_solve(self._h, n, nrhs, route, _ptr(A, C.c_double), _ptr(B, C.c_double),
                                                     _ptr(X, C.c_double), C.byref(info), _ptr(ipiv, C.c_int32)))
        rows = np.arange(n)
        for c, p in enumerate(ipiv):
            if p != c:
                rows[c], rows[p] = rows[p], rows[c]
        return X, info.value, rows

    def solve_info(self):
        """(iterations, multigrid levels, relative residual) of the last sparse solve."""
        it, lv, rr = C.c_int32(0), C.c_int32(0), C.c_double(0)
        self._check(self.lib.nodal_last_solve_info(self._h, C.byref(it), C.byref(lv), C.byref(rr)))
        return it.value, lv.value, rr.value

    def synchronize(self):
        self._check(self.lib.nodal_synchronize(self._h))
