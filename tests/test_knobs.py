"""The environment knobs of the native library are declared once, in nodal_amd/csrc/knobs.h: no other file reads the
environment or spells a knob's name, DESIGN.md's table lists exactly the header's knobs, and every parse rule of the
header gives what the expression it replaced gave (tools/knobs_host_check.cpp, under the sanitizers)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nodal_amd", "csrc")
HEADER = os.path.join(CSRC, "knobs.h")

DECLARATION = re.compile(r'^inline constexpr (\w+) (\w+)\{"((?:NODAL|SLU)_[A-Z0-9_]+)"(?:, ([^}]+))?\};'
                         r'  // (process|call|create|load|mixed): (\S.*)$')
KINDS_WITH_DEFAULT = {"Int", "Int64", "Double"}


def _sources(*dirs):
    for d in dirs:
        for path in sorted(glob.glob(os.path.join(d, "**", "*"), recursive=True)):
            if os.path.isfile(path) and os.path.splitext(path)[1] in (".h", ".hip", ".cpp", ".hpp", ".c", ".cc"):
                yield path


def _header_knobs():
    """name -> (kind, default or None), from the one-line declarations of knobs.h."""
    knobs = {}
    with open(HEADER) as f:
        for line in f:
            if not line.startswith("inline constexpr"):
                continue
            m = DECLARATION.match(line.rstrip("\n"))
            assert m, "knobs.h: a declaration that is not in the one-line form: " + line
            kind, short, name, default, _when, _what = m.groups()
            assert name not in knobs, name + " is declared twice"
            assert short == (name[len("NODAL_"):] if name.startswith("NODAL_") else name), (short, name)
            assert (default is not None) == (kind in KINDS_WITH_DEFAULT), line
            knobs[name] = (kind, default)
    return knobs


def _design_table():
    """name -> (kind, default or None), from the five-column table of DESIGN.md's knob section."""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    section = text.split("\n### Tuning and diagnostic knobs", 1)[1].split("\n## ", 1)[0]
    rows = {}
    for line in section.split("\n"):
        cells = [c.strip() for c in line.strip().strip("|").split("|")] if line.startswith("|") else []
        m = re.fullmatch(r"`((?:NODAL|SLU)_[A-Z0-9_]+)`", cells[0]) if len(cells) == 5 else None
        if not m:
            continue
        assert m.group(1) not in rows, m.group(1) + " is listed twice"
        assert cells[3] in ("process", "call", "create", "load", "mixed"), line
        rows[m.group(1)] = (cells[1], None if cells[2] == "—" else cells[2])
    return rows


def test_only_the_header_reads_the_environment():
    assert os.path.isfile(HEADER)
    stray = [p for p in _sources(CSRC, os.path.join(ROOT, "include"))
             if p != HEADER and "getenv(" in open(p).read()]
    assert stray == []


def test_knob_names_are_spelled_once():
    literal = re.compile(r'"(?:NODAL|SLU)_[A-Z0-9_]+"')
    stray = [(os.path.relpath(p, ROOT), s) for p in _sources(CSRC) if p != HEADER
             for s in literal.findall(open(p).read())]
    assert stray == []
    assert len(_header_knobs()) >= 90  # (89 NODAL_* and SLU_DEBUG when the header was written; knobs are only added)


def test_design_table_matches_the_header():
    header, table = _header_knobs(), _design_table()
    assert sorted(table) == sorted(header)
    assert {k: table[k] for k in header} == header


def test_every_parse_rule_equals_the_expression_it_replaced(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "knobs_host_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tools", "knobs_host_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]  # (also: nothing for the sanitizers to report)
