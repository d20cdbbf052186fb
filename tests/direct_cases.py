"""The inputs of the unrefined checks of the sparse direct route, in one place: tests/test_gpu_direct_unrefined.py and
its child tests/direct_unrefined_child.py run them on the device, tests/test_direct_analysis.py guards on the host that
each table still sits in the kernel regime it was chosen for.

A front's width decides which kernels of csrc/sparse_direct.hip factor it and substitute through it:

    "wave1"      <= 64             factor_fronts_wave<1>
    "wave2"      65 .. 84          factor_fronts_wave<2>
    "wide"       85 .. 256         level_panel_regs<2>, level_swaps_trsm, level_rank_update, extend_add_child
    "apply_big"  > 256             the same, and level_fwd_gather / level_fwd_super / level_bwd_u12 / level_bwd_super
                                   (panels of more than 512 rows: level_panel_regs<4>)
"""
import numpy as np

from nodal_amd import generators as gen

COLS = 16  # right-hand sides of slu_apply_multi, interleaved by row


def _graded(N, decades, seed):
    rng = np.random.default_rng(seed)
    return 10.0 ** rng.uniform(-decades / 2, decades / 2, gen.grid_resistor_count(N))


# name (a word: it travels on the child's command line) -> (table builder, width class of the largest front)
CASES = {
    "grid3": (lambda: gen.grid_table(3), "wave1"),
    "tree3000": (lambda: gen.binary_tree_table(3000), "wave1"),
    "ladder4000": (lambda: gen.ladder_table(4000), "wave1"),
    "wires30_80": (lambda: gen.grid_with_wires_table(30, 80), "wave1"),
    "grid45_6dec": (lambda: gen.grid_table(45, _graded(45, 6, 1)), "wave2"),
    "cfg5_48": (lambda: gen.cfg5_table(48), "wave2"),
    "grid60": (lambda: gen.grid_table(60), "wide"),
    "cfg5_90": (lambda: gen.cfg5_table(90), "wide"),
    "grid140_6dec": (lambda: gen.grid_table(140, _graded(140, 6, 2)), "wide"),
    "grid200": (lambda: gen.grid_table(200), "apply_big"),
    "cfg5_420": (lambda: gen.cfg5_table(420), "apply_big"),
}

# the host emulation needs tens of seconds on this one: its width is asserted on the device run's own trace instead
HOST_GUARD_CASES = [name for name in CASES if name != "cfg5_420"]


def width_class(width):
    return "wave1" if width <= 64 else "wave2" if width <= 84 else "wide" if width <= 256 else "apply_big"


# ---- right-hand sides: the same bits in the parent and in the child (seeded by the size) ----
SINGLE = ("assembled", "unit", "gaussian")
ZERO_COLUMN, SCALED_COLUMN, SCALE = 6, 8, 1e12


def single_rhs(A):
    """[3, n]: the assembled right-hand side, the unit vector at row n // 3, one Gaussian vector"""
    nn = len(A)
    unit = np.zeros(nn)
    unit[nn // 3] = 1.0
    return np.stack([np.asarray(A, dtype=np.float64), unit, np.random.default_rng(1000 + nn).standard_normal(nn)])


def block_rhs(A):
    """[16, n], sixteen different columns: Gaussian ones, the assembled right-hand side (column 1), a unit vector
    (column 3), an all-zero column (ZERO_COLUMN) and one Gaussian column times 1e12 (SCALED_COLUMN)"""
    nn = len(A)
    B = np.random.default_rng(2000 + nn).standard_normal((COLS, nn))
    B[1] = A
    B[3] = 0.0
    B[3, nn // 3] = 1.0
    B[ZERO_COLUMN] = 0.0
    B[SCALED_COLUMN] *= SCALE
    return B


def interleaved(B):
    """[cols, n] -> the [n, 16] layout of slu_apply_multi"""
    return np.ascontiguousarray(B.T)


def apply_all(h, A, transposed=False):
    """Every right-hand side of a case through the hook on an open handle: (z1 [3, n], z16 [16, n], the verdicts
    [(perturbed, info)] of the four calls)."""
    z1, verdicts = [], []
    for r in single_rhs(A):
        z, pert, info = h.debug_direct_apply(r, cols=1, transposed=transposed)
        z1.append(z)
        verdicts.append((pert, info))
    z, pert, info = h.debug_direct_apply(interleaved(block_rhs(A)), cols=COLS, transposed=transposed)
    verdicts.append((pert, info))
    return np.stack(z1), np.ascontiguousarray(z.T), np.array(verdicts, dtype=np.int64)
