"""Child process of tests/test_gpu_direct_unrefined.py: the knobs of the sparse direct route that are read once per
process (NODAL_DIRECT_SUPER, NODAL_DIRECT_APPLY_STEPPED, NODAL_DIRECT_LDS_BS, NODAL_DIRECT_BIG_DIM) reach the library
through this process's environment, which the parent sets.

For every case named on the command line (tests/direct_cases.py) the factors are applied, unrefined, to the case's
right-hand sides through nodal_debug_direct_apply; <out dir>/<case>.npz receives z1 [3, n], z16 [16, n], the verdicts
[4, 2] = (replaced pivots, info) of the four calls and the largest front the analysis reported.  A line `CASE <case>`
goes to stderr in front of each, so that the parent can tell whose trace lines follow.  The parent judges."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from nodal_amd import _ffi  # noqa: E402
from oracle import nodal_oracle as oracle  # noqa: E402
from tests.direct_cases import CASES, apply_all  # noqa: E402


def main():
    out = sys.argv[1]
    for name in sys.argv[2:]:
        assert re.fullmatch(r"\w+", name)
        print("CASE", name, file=sys.stderr, flush=True)
        table = CASES[name][0]()
        _, A = oracle.assemble_fast(table)
        h = _ffi.Handle(0)
        h.upload(table)
        h.assemble_symbolic()
        assert h.assemble_numeric()[0] == _ffi.OK
        z1, z16, verdicts = apply_all(h, A)
        h.close()
        np.savez(os.path.join(out, name + ".npz"), z1=z1, z16=z16, verdicts=verdicts)
    print("direct unrefined child ok")


if __name__ == "__main__":
    main()
