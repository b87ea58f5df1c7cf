"""The heap of the GPU's graph search (slowflow_amd/csrc/epic_heap.h) on the CPU: tests/host/test_epic_heap.cpp drives its push / pop and the
std::priority_queue of host/epic.cpp with the same operation sequences and compares every pop, ties included; built with the address and
undefined-behaviour sanitizers and run as that program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_epic_heap_pops_in_the_priority_queues_order(tmp_path):
    exe = str(tmp_path / "test_epic_heap")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(ROOT, "slowflow_amd", "csrc"), os.path.join(ROOT, "tests", "host", "test_epic_heap.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "epic_heap tests OK" in r.stdout, r.stdout + r.stderr[-2000:]
