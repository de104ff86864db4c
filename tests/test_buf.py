"""The handle's owning buffer (csrc/cnf_buf.h) over a counting allocator that can fail, and the adjoint's table of Tsit5
coefficients against the oracle's digits -- on the CPU (tests/support/buf_test.cpp)."""
import os
import re
import subprocess

import numpy as np

from oracle.cnf_oracle import TSIT5_A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffer_invariants_and_adjoint_tableau(tmp_path):
    # the TS_ macros and tsit5_row as the library compiles them, without the HIP headers around them
    dev = open(os.path.join(ROOT, "continuousnf.jl_amd", "csrc", "cnf_dev.h")).read()
    m = re.search(r"#define TS_A21.*?inline void tsit5_row\(int s, float\* a\) \{.*?\n\}\n", dev, re.S)
    assert m, "cnf_dev.h: the TS_ macros and tsit5_row were not found"
    (tmp_path / "tsit5_rows.inc").write_text(m.group(0))
    exe = str(tmp_path / "buf_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-D__host__=", "-D__device__=", "-I", str(tmp_path), "-o", exe,
                    os.path.join(ROOT, "tests", "support", "buf_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] in ("a", "kc"):
            rows[(w[0], int(w[1]))] = np.array(w[2:], dtype=np.float32)
        elif w[0] == "b":
            rows["b"] = np.array(w[1:], dtype=np.float32)
    f32 = lambda xs: np.array(xs, dtype=np.float32)
    for s in range(6):                       # a[s][i] = a_{s+1, i+1}; kc[s][d] = a[s][s - 1 - d], zero beyond
        a = f32(list(TSIT5_A[s]) + [0.0] * (5 - s))
        assert np.array_equal(rows[("a", s)], a), (s, rows[("a", s)], a)
        kc = f32([TSIT5_A[s][s - 1 - d] if s - 1 - d >= 0 else 0.0 for d in range(5)])
        assert np.array_equal(rows[("kc", s)], kc), (s, rows[("kc", s)], kc)
    assert np.array_equal(rows["b"], f32(TSIT5_A[6]))
