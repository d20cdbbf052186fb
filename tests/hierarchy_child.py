"""The shapes of tests/test_gpu_hierarchy.py and, run as a program, its child process: NODAL_SA_GCAP and NODAL_SA_GG are
read once per process, so the Galerkin kernel's row loop (every workgroup walks many coarse rows, as on the 1e6-node
grid) and its small groups (level-0 rows of R need several) get a process of their own.

As a program: sets up the random-valued grid(100) through the multigrid route, runs check_hierarchy on the exported
hierarchy itself and prints one line `hierarchy child ok <level sizes> <error / bound per quantity>`."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from nodal_amd import _ffi, generators as gen  # noqa: E402


def grid_values(N, seed=100):
    """One resistance per grid resistor, uniform in [1, 3] ohm (within one decade: the setup takes them; a uniform grid
    would make transpositions and slot mix-ups invisible)."""
    return np.random.default_rng(seed).uniform(1.0, 3.0, size=gen.grid_resistor_count(N))


def grid100():
    return gen.grid_table(100, grid_values(100))


def grid3d(side=16):
    """A 3-D seven-point grid, side^3 nodes, the last one ground: level-0 rows of seven."""
    k = np.arange(side ** 3).reshape(side, side, side)
    a = np.concatenate([k[:-1].ravel(), k[:, :-1].ravel(), k[:, :, :-1].ravel()])
    b = np.concatenate([k[1:].ravel(), k[:, 1:].ravel(), k[:, :, 1:].ravel()])
    values = np.random.default_rng(16).uniform(1.0, 3.0, size=len(a))
    return gen.passive_table(a, b, values, 0, side ** 3 - 1)


def cfg5(N=66):
    """Config 5 (voltage and dependent sources on a grid) with random resistances: the presolve leaves a non-symmetric
    node system of N^2 - 1 unknowns, which takes the multigrid only above the dense solve's 4096."""
    table = gen.cfg5_table(N)
    res = table.type == 0
    table.value[res] = np.random.default_rng(5).uniform(1.0, 3.0, size=int(res.sum()))
    return table


def solve_and_export(table, method=_ffi.SPARSE_PCG, extra_streams=False, members=None):
    """Set the table up on a fresh handle, solve through `method`, export the hierarchy.  members: a [M, ncomp] value
    table; every member is assembled and solved in turn on the same handle (a values-only refresh from the second on).
    Returns (handle, [levels per solve])."""
    h = _ffi.Handle(0)
    if extra_streams:
        h.set_option(_ffi.OPT_EXTRA_STREAMS, 1)
    h.upload(table)
    if members is not None:
        h.upload_values(members)
    h.assemble_symbolic()
    exports = []
    for member in range(1 if members is None else len(members)):
        assert h.assemble_numeric(member)[0] == _ffi.OK
        _, info, _, _ = h.solve_sparse(method=method)
        assert info == 0, info
        resid = h.residual()
        assert resid <= 1e-12, resid
        levels = h.debug_hierarchy()
        assert h.solve_info()[1] == len(levels), (h.solve_info(), len(levels))
        exports.append(levels)
    return h, exports


def main():
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from hierarchy_reference import check_hierarchy, coverage
    h, (levels,) = solve_and_export(grid100())
    h.close()
    stats = check_hierarchy(levels)
    print("hierarchy child ok", coverage(levels)[1], " ".join(f"{k}={v:.3g}" for k, v in sorted(stats.items())))


if __name__ == "__main__":
    main()
