"""The device side of tests/test_gpu_cycle.py and, run as a program, its child process (the knobs NODAL_SA_FOLD_POST,
NODAL_SA_RESTRICT_B, NODAL_SA_FOLD_VISIT, NODAL_SA_TAIL_DENSE, NODAL_SA_KCYCLE and NODAL_POISON are read once per
process; NODAL_SA_NU per call, so it is set per shape here).

run(shape): sets the network up on a fresh handle, solves it once so that the hierarchy exists, exports the hierarchy
and applies nodal_debug_cycle_apply to the test vectors in every (mode, frozen) case of the shape.  Returns a flat dict
of arrays: the export ("L<l>.<name>"), the vectors and per case "z.<mode>.<frozen>", "dots...", "params...".

As a program: `cycle_child.py <out dir> <shape> ...` leaves <out dir>/<shape>.npz per shape and `cycle child ok`."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import fold_visit_child as fv  # noqa: E402
import hierarchy_child as hc  # noqa: E402
from nodal_amd import _ffi  # noqa: E402

# (s1, s2, t): near what the adaptive cycles of these grids find, with full mantissas like the means of samples the
# solver freezes.  A short decimal is a poor stand-in: with t = 0.95 = 19/20 - 2^-55 the product t v1 of every f32 v1
# whose mantissa 5 divides is a short number up to that 2^-55, a thousandth of the entries of r2 = rc - t v1 are exact
# f32 ties but for it, and the device's fused multiply-add sees the 2^-55 where numpy's multiply-then-subtract has
# rounded it away: about a hundred entries of z one f32 unit apart (0.04 - 0.07 of E, measured on grid100).
FROZEN = np.array([1.0537219483, 0.8491370221, 0.9512398877])
ALL = ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1))

# shape: (table, NODAL_SA_NU or None, method, ((mode, frozen), ...))
SHAPES = {
    "grid100": (hc.grid100, None, _ffi.SPARSE_PCG, ALL),
    "grid100_222": (hc.grid100, "222", _ffi.SPARSE_PCG, ((0, 0), (1, 0), (2, 0))),
    "grid100_312": (hc.grid100, "312", _ffi.SPARSE_PCG, ((0, 0), (2, 0))),
    "grid3d_16": (hc.grid3d, None, _ffi.SPARSE_PCG, ((0, 0), (1, 0), (2, 0))),
    "grid400": (fv.grid400, None, _ffi.SPARSE_PCG, ((0, 0), (2, 0))),
    "cfg5_66": (hc.cfg5, None, _ffi.SPARSE_LU, ((0, 0), (0, 1))),
    "cfg5_100": (fv.cfg5_100, None, _ffi.SPARSE_LU, ((0, 0), (0, 1))),
}


def vectors(n):
    """[n, 4], fixed seeds: random, smooth (the product of two half sine waves over the index grid), unit, zero."""
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    rows = (n + side - 1) // side
    smooth = np.sin(np.pi * (i % side + 0.5) / side) * np.sin(np.pi * (i // side + 0.5) / rows)
    unit = np.zeros(n)
    unit[n // 2 + side // 3] = 1.0
    return np.stack([np.random.default_rng(11).standard_normal(n), smooth, unit, np.zeros(n)], axis=1)


def block_vectors(n):
    """[n, 16]: sixteen different columns of different sizes, the zero and the unit vector among them."""
    rng = np.random.default_rng(12)
    v4 = vectors(n)
    cols = [v4[:, 0], v4[:, 1], v4[:, 2], v4[:, 3]]
    for k in range(12):
        cols.append(rng.standard_normal(n) * (1.0 + k) + (k % 3) * v4[:, 1])
    return np.ascontiguousarray(np.stack(cols, axis=1))


def block_frozen():
    return np.ascontiguousarray(FROZEN[None, :] * (1.0 + 0.02 * np.arange(16))[:, None])


def with_nu(nu):
    if nu is None:
        os.environ.pop("NODAL_SA_NU", None)
    else:
        os.environ["NODAL_SA_NU"] = nu


def run(shape):
    table, nu, method, cases = SHAPES[shape]
    before = os.environ.get("NODAL_SA_NU")
    with_nu(nu)
    try:
        h, (levels,) = hc.solve_and_export(table(), method)
        out = {"nlev": np.int64(len(levels)), "iterations": np.int64(h.solve_info()[0])}
        for l, lv in enumerate(levels):
            for k, v in lv.items():
                out[f"L{l}.{k}"] = v if isinstance(v, np.ndarray) else np.float64(v)
        if method == _ffi.SPARSE_PCG:  # (the system the flexible CG solved: its matrix is level 0's)
            out["rhs"] = h.export_csr()[3]
        n = levels[0]["n"]
        v4, v16 = vectors(n), block_vectors(n)
        u4 = np.random.default_rng(13).standard_normal((n, 4))
        u16 = np.ascontiguousarray(np.random.default_rng(14).standard_normal((n, 16)))
        out.update(v4=v4, v16=v16, u4=u4, u16=u16)
        for mode, frozen in cases:
            key = f"{mode}.{frozen}"
            if mode == 2:
                z, dots, params = h.debug_cycle_apply(v16, mode=2, u=u16, frozen=block_frozen() if frozen else None)
            else:
                zs, ds = [], []
                for y in range(4):
                    zy, dy, params = h.debug_cycle_apply(np.ascontiguousarray(v4[:, y]), mode=mode,
                                                         u=np.ascontiguousarray(u4[:, y]) if mode else None,
                                                         frozen=FROZEN if frozen else None)
                    zs.append(zy)
                    ds.append(dy if dy is not None else np.zeros(2))
                z, dots = np.stack(zs, axis=1), np.stack(ds, axis=1)
            out["z." + key], out["dots." + key] = z, dots
            out["params." + key] = np.array([params[k] for k in _ffi.CYCLE_PARAMS], dtype=np.int64)
        h.close()
        return out
    finally:
        with_nu(before)


def levels_of(data):
    """The export back as Handle.debug_hierarchy() gives it."""
    words = set(_ffi.HIERARCHY_INFO)
    levels = []
    for l in range(int(data["nlev"])):
        lv = {}
        for k in data:
            if k.startswith(f"L{l}."):
                name = k.split(".", 1)[1]
                v = data[k]
                lv[name] = int(v) if name in words else (float(v) if v.ndim == 0 else v)
        levels.append(lv)
    return levels


def params_of(data, mode, frozen):
    return {k: int(v) for k, v in zip(_ffi.CYCLE_PARAMS, data[f"params.{mode}.{frozen}"])}


def main():
    out = sys.argv[1]
    for name in sys.argv[2:]:
        assert re.fullmatch(r"\w+", name)
        np.savez(os.path.join(out, name + ".npz"), **run(name))
    print("cycle child ok")


if __name__ == "__main__":
    main()
