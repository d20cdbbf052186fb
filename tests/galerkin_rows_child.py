"""The shapes of tests/test_gpu_galerkin_rows.py and, run as a program, its child process: NODAL_SA_GROWS, NODAL_SA_GDYN,
NODAL_SA_GCAP and NODAL_SA_GG are read once per process.

As a program: `galerkin_rows_child.py OUT.npz SHAPE...` sets every named shape up through the multigrid route, runs
check_hierarchy on the export and writes the coarse matrices of every level to OUT.npz (`<shape>/<level>/<array>`);
`galerkin_rows_child.py declined` solves the networks whose hierarchy the setup declines and prints the outcomes.  One
JSON line on stdout either way."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from nodal_amd import _ffi, generators as gen  # noqa: E402

MATRIX = ("acol", "alen", "aval", "avalf", "dinv")


def chord_grid(N, share, seed):
    """grid(N) with resistances uniform in [1, 3] ohm, plus chords: a random permutation of the nodes, consecutive pairs
    of its first `share` joined by a resistor -- at most one chord per node, level-0 rows of at most six entries."""
    rng = np.random.default_rng(seed)
    k = np.arange(N * N).reshape(N, N)
    a = np.concatenate([k[:, :-1].ravel(), k[:-1].ravel()])
    b = np.concatenate([k[:, 1:].ravel(), k[1:].ravel()])
    perm = rng.permutation(N * N)[:int(share * N * N) // 2 * 2]
    a, b = np.concatenate([a, perm[0::2]]), np.concatenate([b, perm[1::2]])
    return gen.passive_table(a, b, rng.uniform(1.0, 3.0, size=len(a)), 0, N * N - 1)


def chord10():
    return chord_grid(60, 0.10, 610)


def chord20():
    """The level where most rows fall back to the whole wavefront.  (With 30 % chords the device's aggregation gives
    level-1 rows above the cap of 64 columns, seeds 630-632 alike, and 25 % likewise: that shape is among DECLINED.)"""
    return chord_grid(60, 0.20, 620)


def chord30():
    return chord_grid(60, 0.30, 630)


def chord_all():
    """grid(40) with a chord at every node: coarse rows above the row cap, the multigrid setup declines."""
    return chord_grid(40, 1.0, 640)


def grid100():
    from tests.hierarchy_child import grid100 as table
    return table()


def grid3d():
    from tests.hierarchy_child import grid3d as table
    return table()


SHAPES = {"chord10": chord10, "chord20": chord20, "grid100": grid100, "grid3d": grid3d}
DECLINED = {"chord_all": chord_all, "chord30": chord30}


def solve_declined(name):
    """(info, iterations, levels, residual, whether a smoothed-aggregation hierarchy is there to export)"""
    h = _ffi.Handle(0)
    h.upload(DECLINED[name]())
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    _, info, _, _ = h.solve_sparse(method=_ffi.SPARSE_PCG)
    resid = h.residual()
    iters, levels, _ = h.solve_info()
    try:
        h.debug_hierarchy()
        exported = True
    except _ffi.NodalHipError:
        exported = False
    h.close()
    return info, iters, levels, resid, exported


def matrices(levels):
    return {f"{l}/{name}": lv[name] for l, lv in enumerate(levels) for name in MATRIX}


def main():
    from tests.hierarchy_child import solve_and_export
    from tests.hierarchy_reference import check_hierarchy, coverage
    if sys.argv[1] == "declined":
        print(json.dumps({name: solve_declined(name) for name in DECLINED}))
        return
    arrays, report = {}, {}
    for shape in sys.argv[2:]:
        h, (levels,) = solve_and_export(SHAPES[shape]())
        h.close()
        report[shape] = {"stats": check_hierarchy(levels), "sizes": coverage(levels)[1]}
        arrays.update({f"{shape}/{k}": v for k, v in matrices(levels).items()})
    np.savez(sys.argv[1], **arrays)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
