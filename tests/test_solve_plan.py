"""The route of a solve as a value (csrc/cnf_solve_plan.h) on the CPU (tests/support/solve_plan_test.cpp): every combination
of what a call asks and what the kernels' predicates answer keeps the rules the drivers of solve_core rely on -- one first driver;
no one-launch solve under lock-step or no_persist; a tangent call's launch is the wave kernel's; no path on the fused step
kernel; an in-launch gradient gets the wave launch or is refused; what trace_fused and tsolve_ok imply; at most one of the
wave / bcast / k_trace3s launches -- and the routes of DESIGN section 4.7's kernel table come out by name."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_route_keeps_the_drivers_rules(tmp_path):
    exe = str(tmp_path / "solve_plan_test")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "continuousnf.jl_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "support", "solve_plan_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr
