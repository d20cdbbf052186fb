"""The shapes of tests/test_gpu_amg.py and, run as a program, its child process.

NODAL_SAGG is read once per process and NODAL_SAGG=0 is the only way to put a network the smoothed hierarchy would take
through csrc/amg.hip, so the shapes marked `child` run in a process of their own; the NODAL_AMG_* knobs are read at
every setup and are simply set around each shape (`setenv` / `delenv`: os.environ here, monkeypatch in the test).

run(name) sets the shape up on a fresh handle, solves it, exports the hierarchy (Handle.debug_amg()) and applies ONE
cycle (Handle.debug_amg_apply) at level 0 and at every other level outside the tail to four vectors: random, a unit
vector at a member of the level's largest aggregate (the hub's, where there is one), a vector constant on that aggregate,
and zero.  As a program: `amg_child.py <out dir> <shape> ...` pickles each shape's result to <out dir>/<shape>.pkl and
prints `amg child ok`."""
import os
import pickle
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from nodal_amd import _ffi, generators as gen  # noqa: E402

KNOBS = ("NODAL_AMG_BLOCK", "NODAL_AMG_SWEEPS0", "NODAL_AMG_NOTAIL", "NODAL_AMG_KMAX", "NODAL_AMG_PASSES0",
         "NODAL_AMG_PASSES1", "NODAL_AMG_THETA", "NODAL_AMG_KEEP_DENSE")


def graded(side, decades, seed):
    """Resistances 10^U(-decades / 2, decades / 2): the setup picks the contrast mode by itself."""
    rng = np.random.default_rng(seed)
    return gen.grid_table(side, 10.0 ** rng.uniform(-decades / 2, decades / 2, gen.grid_resistor_count(side)))


def mild(side, seed):
    """Resistances in [0.5, 2]: point mode."""
    return gen.grid_table(side, np.random.default_rng(seed).uniform(0.5, 2.0, gen.grid_resistor_count(side)))


def anisotropic(side=60, seed=61):
    ga, gb, _ = gen._grid_arrays(side)
    vals = np.random.default_rng(seed).uniform(0.5, 2.0, len(ga))
    return gen.grid_table(side, np.where(gb == ga + 1, vals, 1000.0 * vals))  # vertical links 1000 x the horizontal ones


def with_hub(side, grid_values, spokes, spoke_values, seed):
    """The grid plus a hub (node side^2) tied to `spokes` of its nodes, ground a node of its own behind node 0."""
    rng = np.random.default_rng(seed)
    ga, gb, _ = gen._grid_arrays(side)
    nn = side * side
    ends = rng.choice(nn, spokes, replace=False).astype(np.int64)
    a = np.concatenate([ga, np.full(spokes, nn, dtype=np.int64), [0]])
    b = np.concatenate([gb, ends, [nn + 1]])
    vals = np.concatenate([grid_values(rng, len(ga)), spoke_values(rng, spokes), [1.0]])
    return gen.passive_table(a, b, vals, nn - 1, nn + 1)


def hub_contrast():
    """~100 strong spokes (0.005-0.02 ohm) on the four-decade grid: the hub's aggregate exceeds BLOCK_MAX."""
    return with_hub(60, lambda rng, k: 10.0 ** rng.uniform(-2, 2, k), 100, lambda rng, k: rng.uniform(0.005, 0.02, k), 62)


def hub_spokes():
    """3300 ordinary spokes: a row block above STREAM_CAP, a row that straddles a chunk (most spoke nodes pair up among
    themselves first: the hub's aggregate has hundreds of members only)."""
    return with_hub(60, lambda rng, k: rng.uniform(0.5, 2.0, k), 3300, lambda rng, k: rng.uniform(0.5, 2.0, k), 63)


def hub_strong():
    """3300 STRONG spokes on the mild grid: every spoke node's strongest link is the hub's, so in contrast mode they all
    wait for the hub's pair and join it -- an aggregate of thousands of members (restrict_sum's chunked walk)."""
    return with_hub(60, lambda rng, k: rng.uniform(0.5, 2.0, k), 3300, lambda rng, k: rng.uniform(0.005, 0.02, k), 67)


def cfg5(N=70):
    """Config 5 with random resistances: the presolve leaves a non-symmetric node system on the reduced context."""
    table = gen.cfg5_table(N)
    res = table.type == 0
    table.value[res] = np.random.default_rng(5).uniform(1.0, 3.0, size=int(res.sum()))
    return table


def expander(n=2000, seed=12):
    """The network of test_expander_like_network_keeps_the_jacobi_preconditioner at n = 2000."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, 3 * n)
    b = rng.integers(0, n, 3 * n)
    keep = a != b
    ring = np.arange(n)
    a = np.concatenate([a[keep], ring, [0]])
    b = np.concatenate([b[keep], (ring + 1) % n, [n]])
    return gen.passive_table(a, b, rng.uniform(0.5, 2.0, len(a)), n // 2, n)


PCG, AUTO = _ffi.SPARSE_PCG, _ffi.SPARSE_AUTO
# name: (table, method, knobs, child)
SHAPES = {
    "contrast60": (lambda: graded(60, 4, 60), PCG, {}, False),
    "aniso60": (anisotropic, PCG, {}, False),
    "hub_contrast": (hub_contrast, PCG, {}, False),
    "hub_point": (hub_spokes, PCG, {"NODAL_AMG_BLOCK": "0"}, False),
    "hub_block": (hub_spokes, PCG, {"NODAL_AMG_BLOCK": "1"}, False),
    "hub_strong": (hub_strong, PCG, {}, False),
    "point60": (lambda: mild(60, 64), PCG, {}, True),
    "point60_one_sweep": (lambda: mild(60, 64), PCG, {"NODAL_AMG_SWEEPS0": "1"}, True),
    "point60_notail": (lambda: mild(60, 64), PCG, {"NODAL_AMG_NOTAIL": "1"}, True),
    "point60_kmax2": (lambda: mild(60, 64), PCG, {"NODAL_AMG_NOTAIL": "1", "NODAL_AMG_KMAX": "2", "NODAL_AMG_PASSES0": "2",
                                                 "NODAL_AMG_PASSES1": "2"}, True),
    "cfg5_point": (cfg5, AUTO, {"NODAL_AMG_BLOCK": "0"}, True),
    "cfg5_block": (cfg5, AUTO, {"NODAL_AMG_BLOCK": "1"}, True),
    "point450": (lambda: mild(450, 65), PCG, {}, True),
    "contrast450": (lambda: graded(450, 4, 66), PCG, {}, False),
    "expander": (expander, PCG, {}, False),
}


def solve(table, method):
    h = _ffi.Handle(0)
    h.upload(table)
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    _, info, iters, _ = h.solve_sparse(method=method, download=False)
    assert info == 0, info
    resid = h.residual()
    assert resid <= 1e-12, resid
    return h, iters


def probe_vectors(lv, last, seed):
    """[4, n]: random, unit at the first member of the largest aggregate, constant on that aggregate, zero."""
    n = lv["n"]
    v = np.zeros((4, n))
    v[0] = np.random.default_rng(seed).standard_normal(n)
    if last:
        v[1, n // 2] = 1.0
        v[2, : max(1, n // 3)] = 1.0
    else:
        I = int(np.argmax(np.diff(lv["memptr"])))
        members = lv["mem"][lv["memptr"][I]:lv["memptr"][I + 1]]
        v[1, members[0]] = 1.0
        v[2, members] = 1.0
    return v


def export_and_apply(h):
    levels, info = h.debug_amg()
    outside = [l for l in range(len(levels)) if not levels[l]["in_tail"]]
    applies = {}
    for l in outside:
        r = probe_vectors(levels[l], l == len(levels) - 1, 1000 + l)
        z, params = [], None
        for k in range(4):
            zk, params = h.debug_amg_apply(r[k], level=l)
            z.append(zk)
        applies[l] = {"r": r, "z": np.stack(z), "params": params}
    return levels, info, applies


def run(name, setenv=None, delenv=None):
    table, method, knobs, _ = SHAPES[name]
    setenv = setenv or os.environ.__setitem__
    delenv = delenv or (lambda k: os.environ.pop(k, None))
    for k in KNOBS:
        delenv(k)
    for k, v in knobs.items():
        setenv(k, v)
    h, iters = solve(table(), method)
    levels, info, applies = export_and_apply(h)
    csr = h.export_csr()[:3] if method == PCG else None  # (the general route's level 0 is the reduced context's node block)
    h.close()
    for k in KNOBS:
        delenv(k)
    return {"levels": levels, "info": info, "applies": applies, "csr": csr, "iterations": iters}


def forced_block(out):
    """The two solves of test_multigrid_block_smoother_forced_on_uniform_and_general_networks (tests/test_gpu_kernels.py)
    in a process in which the smoothed hierarchy is off, so that NODAL_AMG_BLOCK=1 is read at all: per table the solution
    and what the test asserts on, in <out>/forced_block.npz; a marker line on stderr before each table's trace."""
    os.environ["NODAL_AMG_BLOCK"] = "1"
    data = {}
    for name, table in (("grid80", gen.grid_table(80)), ("cfg5_90", gen.cfg5_table(90))):
        print(f"[child] {name}", file=sys.stderr, flush=True)
        h = _ffi.Handle(0)
        h.upload(table)
        h.assemble_symbolic()
        assert h.assemble_numeric()[0] == _ffi.OK
        x, info, iters, _ = h.solve_sparse()
        data[name + ".x"], data[name + ".info"], data[name + ".iters"] = np.array(x), info, iters
        data[name + ".residual"] = h.residual()
        h.close()
    np.savez(os.path.join(out, "forced_block.npz"), **data)
    print("amg child ok")


def main():
    out = sys.argv[1]
    if sys.argv[2:] == ["--forced-block"]:
        return forced_block(out)
    for name in sys.argv[2:]:
        assert re.fullmatch(r"\w+", name)
        with open(os.path.join(out, name + ".pkl"), "wb") as f:
            pickle.dump(run(name), f)
    print("amg child ok")


if __name__ == "__main__":
    main()
