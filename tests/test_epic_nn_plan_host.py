"""The compact search's planner (slowflow_amd/csrc/epic_nn_plan.h: forms, the images that fit, slices and their bytes) on the CPU:
tests/host/test_epic_nn_plan.cpp, which includes nothing but that header, under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_epic_nn_plan_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_epic_nn_plan")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(ROOT, "slowflow_amd", "csrc"), os.path.join(ROOT, "tests", "host", "test_epic_nn_plan.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "epic_nn_plan tests OK" in r.stdout, r.stdout + r.stderr[-2000:]
