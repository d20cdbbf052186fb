"""Child process of tests/test_gpu_presolve.py::test_without_keep_a_stubborn_source_ends_the_plan.

NODAL_PRESOLVE_KEEP is read once per process.  Builds the presolve of the three stubborn kinds -- the small families of
tests/presolve_reference.py and _stubborn_sources(12, kind) of tests/test_gpu_parity.py -- through
nodal_debug_presolve_build and prints, per case, whether the plan was ok and whether the rewrite ran, as one JSON
object behind the words `presolve child`.  The parent runs it under NODAL_PRESOLVE_KEEP=0 and expects every plan
declined."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import nodal_amd as n  # noqa: E402
from nodal_amd import _ffi  # noqa: E402
from nodal_amd.lowering import lower  # noqa: E402
from tests import presolve_reference as ref  # noqa: E402
from tests.test_gpu_parity import _stubborn_sources  # noqa: E402


def main():
    families = ref.families()
    tables = {}
    for kind in ("cascade", "feedback", "stacked"):
        tables[kind] = lower(n.Netlist.from_rows(_stubborn_sources(12, kind)))
        tables["stubborn_" + kind] = families["stubborn_" + kind][0].table()
    got = {}
    for name, table in tables.items():
        h = _ffi.Handle(0)
        h.upload(table)
        h.assemble_symbolic()
        assert h.assemble_numeric()[0] == _ffi.OK
        out = h.debug_presolve_build()
        got[name] = {"ok": out["ok"], "built": out["built"]}
        h.close()
    print("presolve child", json.dumps(got))


if __name__ == "__main__":
    main()
