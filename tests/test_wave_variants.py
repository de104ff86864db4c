"""Which k_solve_wave instantiation a query gets (csrc/cnf_wave_variants.h) against the table of the selection functions it
replaced: every form over input tiles 1..3, hidden tiles 1..7, the three modes and both second-layer flags -- on the CPU
(tests/support/wave_variants_test.cpp, tests/support/wave_variants.expected)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_variant_table(tmp_path):
    exe = str(tmp_path / "wave_variants_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "support", "wave_variants_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    with open(os.path.join(ROOT, "tests", "support", "wave_variants.expected")) as f:
        want = f.read().splitlines()
    got = r.stdout.splitlines()
    assert len(got) == len(want) == 7 * 3 * 7 * 3 * 2 * 2
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, f"{len(diff)} queries answered differently (got, expected): {diff[:8]}"
