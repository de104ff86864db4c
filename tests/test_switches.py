"""The process-wide environment switches as one table (csrc/cnf_switch.h) on the CPU (tests/support/switch_test.cpp): every
kind's parse rule at its edges, one read per process -- and the documents that list the switches name exactly the table's set:
the A/B-switch sentence of DESIGN section 4.7 and the switch table of tools/README.md.  Nothing else in csrc/ parses a CNF_
variable."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "continuousnf.jl_amd", "csrc")
NAME = re.compile(r"`(CNF_[A-Z0-9_]+)")          # a name as the documents write it: at the start of a code span


@pytest.fixture(scope="module")
def switch_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("switch") / "switch_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "support", "switch_test.cpp")], check=True)
    return subprocess.run([exe], capture_output=True, text=True, timeout=60)


@pytest.fixture(scope="module")
def table_names(switch_run):
    names = [l for l in switch_run.stdout.split() if l.startswith("CNF_")]
    assert len(names) == len(set(names)) >= 24
    return set(names)


def test_parse_rules_hold_at_their_edges_and_a_switch_is_read_once(switch_run):
    """The checks are the program's own (tests/support/switch_test.cpp): it prints each one that fails and ends with `ok`."""
    assert switch_run.returncode == 0 and switch_run.stdout.strip().endswith("ok"), switch_run.stdout[-2000:] + switch_run.stderr


def test_design_sentence_names_the_tables_set(table_names):
    txt = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = txt[txt.index("### 4.7 "):txt.index("\n## 5. ")]
    sentence = sec[sec.index("A/B switches (environment"):]
    sentence = sentence[:sentence.index("; compile time:")]
    named = set(NAME.findall(sentence))
    assert named == table_names, sorted(named ^ table_names)


def test_tools_readme_table_names_the_tables_set(table_names):
    txt = open(os.path.join(ROOT, "tools", "README.md")).read()
    tail = txt[txt.index("Environment switches read by `libcnfhip.so`"):]
    rows = tail[tail.index("\n| variable |"):].lstrip("\n").split("\n\n")[0].splitlines()[2:]
    assert len(rows) >= 20 and all(r.startswith("| `CNF_") for r in rows), rows
    named = set(n for r in rows for n in NAME.findall(r.split(" | ")[0]))
    assert named == table_names, sorted(named ^ table_names)


def test_no_other_file_of_csrc_parses_a_switch():
    files = [f for f in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) if os.path.basename(f) != "cnf_switch.h"]
    assert len(files) > 40
    assert [os.path.basename(f) for f in files if 'getenv("CNF_' in open(f).read()] == []
