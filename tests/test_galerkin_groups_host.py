"""The rule that cuts a row of R into the Galerkin kernel's groups (nodal_amd/csrc/galerkin_groups.h) on the CPU:
tools/galerkin_groups_host_check.cpp, built with the address and undefined-behaviour sanitizers, runs it on random and
degenerate rows (every entry in exactly one group, no group above a cap, the same boundary whichever lane counts it), and
the capacities of the shared path that nodal_amd/_ffi.py mirrors for the GPU tests are the header's."""
import os
import re
import shutil
import subprocess

import pytest

from nodal_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_group_rule_on_the_host(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "galerkin_groups_host_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tools", "galerkin_groups_host_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]  # (also: nothing for the sanitizers to report)
    assert "galerkin groups ok" in r.stdout
    m = re.search(r"capacities rows=(\d+) entries=(\d+) products=(\d+) columns=(\d+)", r.stdout)
    assert tuple(int(x) for x in m.groups()) == (_ffi.GALERKIN_SUB_ROWS, _ffi.GALERKIN_SUB_ENTRIES,
                                                 _ffi.GALERKIN_SUB_PRODUCTS, _ffi.GALERKIN_SUB_COLUMNS)


def test_the_mirrored_capacities_are_the_headers():
    with open(os.path.join(ROOT, "nodal_amd", "csrc", "galerkin_groups.h")) as f:
        text = f.read()
    for name in ("GALERKIN_SUB_ROWS", "GALERKIN_SUB_ENTRIES", "GALERKIN_SUB_PRODUCTS", "GALERKIN_SUB_COLUMNS"):
        m = re.search(r"constexpr int " + name + r" = (\d+);", text)
        assert m and int(m.group(1)) == getattr(_ffi, name), name
    with open(os.path.join(ROOT, "nodal_amd", "csrc", "knobs.h")) as f:
        m = re.search(r'SA_GLIST\{"NODAL_SA_GLIST", (\d+)\}', f.read())
    assert m and int(m.group(1)) == _ffi.GALERKIN_DYN_PRODUCTS
