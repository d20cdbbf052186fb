"""Child process of tests/test_gpu_fold_post.py (NODAL_SA_FOLD_POST is read once per process).

The shapes of tests/tail_dense_child.py plus the full-size grid(1000), solved the same way and reported the same way:
`RESULT <shape> <info> <iterations, comma separated>` on stdout, the solution in <out dir>/<shape>.npy, and a line
`SHAPE <shape>` on stderr in front of each shape's `[sagg]` trace lines."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from nodal_amd import generators as gen  # noqa: E402
from tail_dense_child import SHAPES as TAIL_SHAPES, single  # noqa: E402

SHAPES = dict(TAIL_SHAPES)
SHAPES["grid1000"] = lambda: single(gen.grid_table(1000))


def main():
    out = sys.argv[1]
    for name in sys.argv[2:]:
        assert re.fullmatch(r"\w+", name)
        print("SHAPE", name, file=sys.stderr, flush=True)
        info, its, x = SHAPES[name]()
        np.save(os.path.join(out, name + ".npy"), x)
        print("RESULT", name, info, ",".join(str(i) for i in its) if its is not None else "-", flush=True)
    print("fold post child ok")


if __name__ == "__main__":
    main()
