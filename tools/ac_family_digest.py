"""The bits of the four small-signal analyses (nodal_ac_sweep, nodal_ac_noise, nodal_ac_ports, nodal_ac_gradient) as
SHA-256 digests per output array, for comparing two builds of the library on one machine: a restructuring of
csrc/ac*.hip and noise.hip must leave every digest as it was.

Cases, each through all four analyses on one handle, every call made twice (the second is the one whose
`timings[0] == 0.0` says that pattern and symbolic analysis were kept):

    tiny_panel        4 nodes and an E source, 2n = 10: the dense panel on the sparse path, the transposed child
    forced_dense      grid(7) with an E source, dense at 2n = 98, 17 probes / outputs / ports: two groups of a chunk
    lu_transposed     grid(9) with an E source, the sparse LU at 2n = 162, 17 outputs / ports on the transposed child
    lu_symmetric      the passive grid(9) with two A sources: noise and the gradient share h->ac with the sweep
    singular_panel    a frequency that is singular alone in the middle of a sweep (tests/test_gpu_ac_family.py), 2n = 8
    singular_lu       the same at 2n = 84, the sparse LU
    no_frequencies    lu_symmetric's network with nfreq = 0
    no_unknowns       a table whose every lead is ground, n = 0

keep_every, peaks, currents, contributions and the input gain are asked for in every call.  `work` and
`timings[0] == 0.0` are recorded as values.

    python tools/ac_family_digest.py --out A.json [--root TREE]     the library and package of TREE (default: this tree)
    python tools/ac_family_digest.py --compare A.json B.json        exit status 1 unless every digest and value is equal
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

OMEGA = 2.0 * np.pi * np.logspace(-2, 1, 5)
SINGULAR_OMEGA = np.array([0.5, 1.0, 2.0])


def grid(N, sources):
    from nodal_amd import generators as gen
    return list(gen.grid_rows(N)) + [list(s) for s in sources]


def island(sections, source):
    """tests/test_gpu_ac_family.py's network: singular at omega = 1 alone"""
    rows = []
    for k in range(sections):
        rows.append([f"rp{k}", "R", "2", f"n{k}", "g"])
        if k + 1 < sections:
            rows.append([f"rs{k}", "R", "1", f"n{k}", f"n{k + 1}"])
    rows += [["ri", "R", "1", "u1", "u2"], ["s1", source, "1", "n0", "g"]]
    return rows, [("cd", 0.5, "n1", "g"), ("ci", 1.0, "u1", "g")], [("li", 1.0, "u1", "g")]


def seeded_elements(labels, rng):
    caps = [(f"c{i}", float(rng.uniform(0.5, 2.0)), node, "g") for i, node in enumerate(labels)]
    inds = [(f"l{i}", float(rng.uniform(0.5, 3.0)), labels[i], labels[i + 1]) for i in range(0, len(labels) - 1, 5)]
    return caps, inds


def run_case(rows, caps, inds, sources, npairs, omega, sparse, rng):
    """every analysis twice on one handle; {analysis: ([arrays of the second call], values)}"""
    import nodal_amd as n
    from nodal_amd.ac import resolve_amplitudes, resolve_reactive
    nl = n.Netlist.from_rows(rows)
    c = n.Circuit(nl, sparse=sparse)
    h = c._handle
    labels = sorted(nl.nodenum, key=nl.nodenum.get)
    K = len(labels)
    if caps is None:
        caps, inds = seeded_elements(labels, rng) if K else ([], [])
    _, kind, value, ea, eb = resolve_reactive(nl, caps, inds)
    srows, amps = resolve_amplitudes(nl, sources)
    if K:
        pa = rng.integers(0, K, npairs).astype(np.int32)
        pb = rng.integers(-1, K, npairs).astype(np.int32)
    else:
        pa = pb = np.full(npairs, -1, dtype=np.int32)
    cur = np.arange(min(3, len(kind)), dtype=np.int32)
    cot = rng.uniform(-1, 1, (len(omega), npairs)) + 1j * rng.uniform(-1, 1, (len(omega), npairs))
    weight = np.linspace(0.5, 1.5, len(omega))
    dense = not sparse
    calls = {
        "ac_sweep": lambda: h.ac_sweep(omega, kind, value, ea, eb, srows, amps, pa, pb, cur, dense=dense, keep_every=2, peaks=True),
        "ac_noise": lambda: h.ac_noise(omega, kind, value, ea, eb, 300.0, pa, pb, dense=dense, input_row=int(srows[0]), weight=weight),
        "ac_ports": lambda: h.ac_ports(omega, kind, value, ea, eb, pa, pb, dense=dense, peaks=True),
        "ac_gradient": lambda: h.ac_gradient(omega, kind, value, ea, eb, srows, amps, pa, pb, cot, dense=dense, adjoints=True),
    }
    result = {}
    for name, call in calls.items():
        kept = []
        for _ in range(2):
            out = call()
            kept.append(float(h.timings()[0]) == 0.0)
        arrays, values = [], {"timings0_is_zero": kept}
        for item in out:
            for a in (item if isinstance(item, tuple) else (item,)):
                if a is not None:
                    arrays.append(np.ascontiguousarray(a))
        if name in ("ac_ports", "ac_gradient"):
            values["work"] = [int(w) for w in arrays.pop()]
        values["info"] = [int(i) for i in arrays[-1]]
        result[name] = (arrays, values)
    h.close()
    return result


def measure():
    rng = np.random.default_rng(71)
    e_source = [("e1", "E", "1", "3", "g")]
    cases = {
        "tiny_panel": (*island(2, "E"), {"s1": 1 - 0.5j}, 3, OMEGA, True),
        "forced_dense": (grid(7, e_source), None, None, {"e1": 1 + 1j}, 17, OMEGA, False),
        "lu_transposed": (grid(9, e_source), None, None, {"e1": 0.5 - 2j}, 17, OMEGA, True),
        "lu_symmetric": (grid(9, [("a1", "A", "1", "2", "g"), ("a2", "A", "2", "40", "7")]), None, None, {"a1": 1j, "a2": 2.0}, 5, OMEGA, True),
        "singular_panel": (*island(2, "A"), {"s1": 1 - 0.5j}, 3, SINGULAR_OMEGA, True),
        "singular_lu": (*island(40, "A"), {"s1": 1 - 0.5j}, 3, SINGULAR_OMEGA, True),
        "no_frequencies": (grid(9, [("a1", "A", "1", "2", "g")]), None, None, {"a1": 1.0}, 2, OMEGA[:0], True),
        "no_unknowns": ([["r1", "R", "2", "g", "g"], ["a1", "A", "1", "g", "g"]], [], [], {"a1": 1.0}, 2, OMEGA, True),
    }
    digests, values = {}, {}
    for case, (rows, caps, inds, sources, npairs, omega, sparse) in cases.items():
        for analysis, (arrays, vals) in run_case(rows, caps, inds, sources, npairs, omega, sparse, rng).items():
            for k, a in enumerate(arrays):
                digests[f"{case}/{analysis}/{k}:{a.dtype}{list(a.shape)}"] = hashlib.sha256(a.tobytes()).hexdigest()
            values[f"{case}/{analysis}"] = vals
        print(case, "done", flush=True)
    return {"digests": digests, "values": values}


def compare(a_path, b_path):
    with open(a_path) as f:
        a = json.load(f)
    with open(b_path) as f:
        b = json.load(f)
    differ = [key for part in ("digests", "values") for key in sorted(set(a[part]) | set(b[part]))
              if a[part].get(key) != b[part].get(key)]
    print(f"{len(a['digests'])} digests, {len(a['values'])} value records:", "all equal" if not differ else f"{len(differ)} differ")
    for key in differ:
        print("  differs:", key)
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="ac_family_digest.json")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the tree whose nodal_amd package and library are measured")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path.insert(0, os.path.abspath(args.root))
    import nodal_amd
    print("measuring", os.path.dirname(os.path.abspath(nodal_amd.__file__)), flush=True)
    record = {"tool": "tools/ac_family_digest.py", **measure()}
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("wrote", args.out, len(record["digests"]), "digests")


if __name__ == "__main__":
    main()
