"""What a gradient call leaves on the handle for the calls that follow (csrc/cnf_record.h) against the table of the loose fields
it replaced: every call-level event from every reachable state, every query after each -- on the CPU
(tests/support/record_test.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_transitions_and_queries(tmp_path):
    exe = str(tmp_path / "record_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "support", "record_test.cpp")],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok: "), r.stdout + r.stderr
