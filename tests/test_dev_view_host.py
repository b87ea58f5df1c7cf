"""The device seam's argument arithmetic (slowflow_amd/csrc/dev_view.h: the sign and extent rule, strides_nest, byte ranges and their overlap) on the CPU:
tests/host/test_dev_view.cpp, which includes nothing but that header, under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_view_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_dev_view")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(ROOT, "slowflow_amd", "csrc"), os.path.join(ROOT, "tests", "host", "test_dev_view.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dev_view tests OK" in r.stdout, r.stdout + r.stderr[-2000:]
