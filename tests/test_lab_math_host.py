"""The Lab arithmetic of slowflow_amd/csrc/lab_math.h on the CPU (tests/host/test_lab_math.cpp): the one function the host test and k_rgb8_to_lab share.
Its cube root and exponential are written from IEEE fp64 operations, so the g++ build speaks for the gfx950 build (csrc/Makefile: -ffp-contract=off
-fno-fast-math).  Every comparison is on bit patterns."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
CSRC = os.path.join(ROOT, "slowflow_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "test_lab_math.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_lab_256.json")
NAMES = ("sfa_rgb8_to_lab_device", "sfa_sequence_lab", "sfa_epic_job_create", "sfa_epic_job_upload", "sfa_epic_job_set_lab", "sfa_epic_job_upload_device",
         "sfa_epic_job_set_matches_device", "sfa_epic_job_run", "sfa_epic_job_download", "sfa_epic_job_upload_flow", "sfa_epic_job_download_device", "sfa_job_set_flow_epic")


def build_with_host_epic(exe):
    """the program linked against host/epic.cpp: its reference is rgb8_to_lab itself"""
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", "-DWITH_HOST_EPIC", "-I", CSRC, "-I", HOST, SRC, os.path.join(HOST, "libslowflow_host.a"),
                        "-L", os.path.join(ROOT, "slowflow_amd"), "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "slowflow_amd"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_lab_math_equals_rgb8_to_lab_on_every_8_bit_triple(tmp_path):
    """all 2^24 triples at norm 1, then ties to even, 16-bit samples at 1/255, values outside 0 .. 255, -0.0, +-Inf and NaN: zero differing values"""
    exe = build_with_host_epic(str(tmp_path / "test_lab_math"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lab_math tests OK" in r.stdout, r.stdout + r.stderr[-2000:]
    assert "all 2^24 8-bit triples at norm 1: 0 values differ" in r.stdout


def test_lab_math_header_under_sanitizers(tmp_path):
    """the header and libm alone (the reference: rgb8_to_lab's statements with nearbyintf, pow and exp) under the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "test_lab_math_san")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", CSRC, SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lab_math tests OK" in r.stdout, r.stdout + r.stderr[-2000:]


def test_lab_math_equals_the_reference_rgb_to_lab(tmp_path):
    """the reference's own rgb_to_lab (image.c:694-726) on 256 x 256 random 8-bit triples against the header, directly.  Where oracle/_ref was not built the
    reference answers with the SHA-256 of the planes it gave when it was (tests/golden/ref_lab_256.json)."""
    from test_epic import RefEpic, _ref_epic_loads
    w = h = 256
    rgb = np.random.default_rng(20250).integers(0, 256, (3, h, w)).astype(np.float32)
    exe = str(tmp_path / "test_lab_math_plain")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-I", CSRC, SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rgb.tofile(str(tmp_path / "rgb.bin"))
    # (the plain build's `conv` is its libm reference; the header is what the GPU kernel runs, so take the header through the test's own comparison first)
    r = subprocess.run([exe, "conv", str(tmp_path / "rgb.bin"), str(w * h), "1", str(tmp_path / "libm.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "header", str(tmp_path / "rgb.bin"), str(w * h), "1", str(tmp_path / "lab.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(str(tmp_path / "lab.bin"), np.float32).reshape(3, h, w)
    assert np.array_equal(got.view(np.uint32), np.fromfile(str(tmp_path / "libm.bin"), np.float32).reshape(3, h, w).view(np.uint32))
    recorded = json.load(open(GOLDEN))
    assert recorded["seed"] == 20250 and recorded["shape"] == [3, h, w]
    if _ref_epic_loads():
        want = RefEpic().lab(rgb, w, h)[:, :, :w]
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
        assert hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest() == recorded["sha256"]
    assert hashlib.sha256(got.tobytes()).hexdigest() == recorded["sha256"]
    assert len(np.unique(got[0])) > 200 and np.isfinite(got).all()


def test_entry_points_declared_exported_and_bound():
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    header = open(os.path.join(ROOT, "include", "slowflow_amd.h")).read()
    L = C.CDLL(sfa.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in sfa.EXPORTS, name
        assert hasattr(L, name), name
    assert "sfa_epic_job_destroy" in sfa.EXPORTS and hasattr(L, "sfa_epic_job_destroy")
    for name in ("upload", "set_lab", "upload_device", "set_matches_device", "run", "download", "upload_flow", "download_device"):
        assert callable(getattr(sfa.EpicJob, name)), name
    assert callable(sfa.Context.epic_job) and callable(sfa.Job.set_flow_epic) and callable(sfa.Sequence.lab_from)
    mk = open(os.path.join(ROOT, "slowflow_amd", "csrc", "Makefile")).read()
    assert "epic_init.hip" in mk and "lab_math.h" in mk
    import sys
    was = "torch" in sys.modules
    from slowflow_amd import device
    assert callable(device.rgb8_to_lab) and callable(device.epic)
    assert was or "torch" not in sys.modules                                   # torch stays lazily imported
    # the header's two functions call no math library: the host build and the device build are one function
    src = open(os.path.join(ROOT, "slowflow_amd", "csrc", "lab_math.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "#include <cmath>" not in code and "math.h" not in code and not re.search(r"\b(pow|exp|cbrt|log|nearbyintf|fma)\s*\(", code)
