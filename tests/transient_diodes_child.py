"""Child process of tests/test_gpu_transient_diodes.py: the clamps-at-rest cases under whatever NODAL_TNL_REUSE the parent
set, every output of each run in <out dir>/<name>.npz (the parent runs the same `outputs` in its own process)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import nodal_amd as n  # noqa: E402
from tests import transient_nl_reference as tn  # noqa: E402

RUNS = {"dense_False": (4, False), "dense_True": (4, True), "lu_False": (12, False), "lu_True": (12, True)}


def outputs(name):
    """the run `name`: a dict of arrays, everything Circuit.transient returns but the timings"""
    size, sparse = RUNS[name]
    rows, caps, inds, diodes, dt, steps, sources = tn.reuse_case(size)
    circ = n.Circuit(n.Netlist.from_rows([list(r) for r in rows]), sparse=sparse, device=0)
    nodes = sorted(circ.netlist.nodenum, key=circ.netlist.nodenum.get)
    tr = circ.transient(caps, dt, steps, sources=sources, probes=nodes, diodes=diodes, diode_probes=[d[0] for d in diodes],
                        keep_every=1, envelope=True, max_iter=50, **tn.TIGHT)
    env = tr.envelope
    return {"waveforms": tr.waveforms, "solutions": tr.solutions, "info": tr.info, "scaled_residual": tr.scaled_residual,
            "iterations": tr.iterations, "newton_iterations": tr.newton_iterations, "matrix_updates": tr.matrix_updates,
            "diode_voltages": tr.diode_voltages, "diode_currents": tr.diode_currents, "final_junctions": tr.final_junctions,
            "potential_min": env.potential_min, "potential_min_step": env.potential_min_step,
            "potential_max": env.potential_max, "potential_max_step": env.potential_max_step}


def main():
    out = sys.argv[1]
    for name in sys.argv[2:]:
        np.savez(os.path.join(out, name + ".npz"), **outputs(name))
    print("transient diodes child ok")


if __name__ == "__main__":
    main()
