"""Child process of tests/test_gpu_dense_blocks.py::test_elimination_switches_give_identical_bits.

The block elimination's switches are read once per process (NODAL_BI_MASKED, NODAL_BI_UNMASK_ROWS, NODAL_BI_EARLY_COPY,
NODAL_BI_SYM, NODAL_BI_FIRST_BLOCKS, NODAL_GJ_DPP).  This solves a fixed set of systems under whatever the parent set:
the exact families (tests/dense_reference.py) and the float SPD family at n = 700 and 1400 with the mixed block widths
512 -> 256 -> 128, both forms of the elimination, through nodal_debug_dense_solve, and the random-graph network at n = 1898
through solve_dense.  It asserts the exact results and the backward-error bar itself and prints one SHA-256 over the
bytes of every float solution: the parent compares the digests of the settings that change streams or lane exchanges
only."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from nodal_amd import _ffi  # noqa: E402
from tests import dense_reference as dr  # noqa: E402


def main():
    os.environ["NODAL_BI_SWITCH"], os.environ["NODAL_BI_SWITCH2"] = dr.WIDTH_PATTERNS["mixed"][1:]
    os.environ.pop("NODAL_BI_WIDTH", None)
    digest = hashlib.sha256()
    h = _ffi.Handle(0)
    for n in (700, 1400):
        for symmetric in (True, False):
            A = dr.exact_matrix(n, dr.SOLVE_SPACING, symmetric, seed=n)
            X0 = dr.integer_rhs(n, 7, n)
            X, info, _ = h.debug_dense_solve(A, A @ X0, passive=symmetric, optimistic=not symmetric)
            assert info == 0 and np.array_equal(X, X0), ("exact", n, symmetric, np.argwhere(X != X0)[:4])
            A = dr.spd_dominant(n, n)
            B = np.random.default_rng(n).standard_normal((n, 7))
            X, info, _ = h.debug_dense_solve(A, B, passive=symmetric, optimistic=not symmetric)
            eta = dr.backward_error(A, X, B).max()
            assert info == 0 and eta <= n * dr.EPS, ("float", n, symmetric, eta / (n * dr.EPS))
            digest.update(X.tobytes())
    h.close()
    os.environ.pop("NODAL_BI_SWITCH")
    os.environ.pop("NODAL_BI_SWITCH2")
    from tests.test_gpu_kernels import _random_graph_table
    h = _ffi.Handle(0)
    h.upload(_random_graph_table(1898, 6, 1898))
    h.assemble_symbolic()
    assert h.assemble_numeric()[0] == _ffi.OK
    x, info = h.solve_dense()
    assert info == 0 and h.residual() <= 1e-14
    digest.update(np.asarray(x).tobytes())
    h.close()
    print("dense variant digest", digest.hexdigest())


if __name__ == "__main__":
    main()
