"""dense_tracking's reduced reference image on the CPU: slowflow_amd/csrc/ref_image.h and host/ref_image.cpp (tests/host/test_ref_image.cpp, its own main,
built with the address and undefined-behaviour sanitizers) against tests/ref_image_ref.py, the numpy restatement written from INTEGRATION.md 4c''s
definition.  Every comparison of images is == on bytes.  The two restatements share no code; a float64 convolution bounds both from outside."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ref_image_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
SRC = [os.path.join(ROOT, "tests", "host", "test_ref_image.cpp"), os.path.join(HOST, "ref_image.cpp"), os.path.join(HOST, "image.cpp")]
NAMES = ("sfa_reference_grid", "sfa_reference_taps", "sfa_reference_lab_device", "sfa_reference_lab", "sfa_track_job_upload_fill_reference",
         "sfa_track_job_upload_fill_reference_device")

# (w, h, skip, norm, top): the GPU test's shapes, the size-rule cases that are served, one frame-sized image
CASES = [(9, 5, 1, 1.0, 256), (13, 9, 3, 1.0, 256), (140, 44, 1, 1.0, 256), (268, 76, 3, 1.0, 256), (5, 8, 1, 1.0, 256), (52, 30, 0, 1.0, 256),
         (37, 21, 1, 1.0 / 255, 65536), (1024, 436, 1, 1.0, 256), (1024, 436, 3, 1.0, 256)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ref_image") / "test_ref_image_san")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-I", HOST] + SRC +
                       ["-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def noise(w, h, top, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, top, (3, h, w)).astype(np.float32)
    if top > 256:                                                      # 16-bit samples: some that round to 255.5 -> 256 -> saturate, and ties of the 8-bit step
        x[0, 0, :4] = [65535, 65408, 65407.5, 127.5]
    return x


def host_rgb8(exe, tmp_path, rgb, skip, norm):
    _, h, w = rgb.shape
    np.ascontiguousarray(rgb, np.float32).tofile(str(tmp_path / "in.bin"))
    r = subprocess.run([exe, "run", str(tmp_path / "in.bin"), str(w), str(h), str(skip), repr(float(np.float32(norm))), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    gw, gh = (w, h) if skip == 0 else R.grid(w, h, skip)
    return np.fromfile(str(tmp_path / "out.bin"), np.uint8).reshape(3, gh, gw)


def test_taps_refusals_and_sizes_in_the_program(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ref_image tests OK" in r.stdout, r.stdout + r.stderr


def test_the_restatement_states_the_definition():
    assert R.taps(1)[0].tolist() == [1, 14, 62, 102, 62, 14, 1] and R.taps(3)[0].tolist() == [1, 8, 27, 56, 72, 56, 27, 8, 1]
    assert R.taps(1)[0].sum() == 256 and R.taps(3)[0].sum() == 256 and R.taps(7)[0].sum() == 257
    assert R.grid(7, 8, 1) is None and R.grid(5, 8, 1) == (2, 4) and R.grid(1024, 436, 1) == (512, 218) and R.grid(1024, 436, 3) == (256, 109)
    t = R.tie_image()
    d, up, even = (R.reference_rgb8(t, 1, tie=k) for k in ("defined", "up", "even"))
    assert d.shape == (3, 3, 5)
    assert (d[:, 1, 0] != up[:, 1, 0]).all()                            # the SSE2 part rounds its ties to even
    assert np.argwhere(d != even).tolist() == [[1, 1, 4], [2, 1, 4]]    # the scalar tail (3 * 10 & ~3 = 28: elements 28 and 29) rounds them up


@pytest.mark.parametrize("w,h,skip,norm,top", CASES)
def test_host_function_equals_the_restatement(exe, tmp_path, w, h, skip, norm, top):
    rgb = noise(w, h, top, seed=w * 1000 + h + skip)
    want = R.reference_rgb8(rgb, skip, norm)
    got = host_rgb8(exe, tmp_path, rgb, skip, norm)
    assert got.shape == want.shape and np.array_equal(got, want)
    if skip:
        # a restatement wrong as a whole (a transposed pass, another border) leaves this bound, which is derived from the taps and not measured
        bound = 255 * 2 * float(np.abs(R.taps(skip)[0] / 256.0 - R.taps(skip)[1].astype(np.float64)).sum()) + 1
        assert bound < 8
        assert np.abs(got.astype(np.float64) - R.float_reference(R.to_8bit(rgb, norm), skip)).max() <= bound


def test_host_function_on_the_tie_image(exe, tmp_path):
    t = R.tie_image()
    want = R.reference_rgb8(t, 1)
    assert not np.array_equal(want, R.reference_rgb8(t, 1, tie="up")) and not np.array_equal(want, R.reference_rgb8(t, 1, tie="even"))
    assert np.array_equal(host_rgb8(exe, tmp_path, t, 1, 1.0), want)


def test_refused_sizes_and_skips_in_the_program(exe, tmp_path):
    for w, h, skip in ((7, 8, 1), (8, 7, 1), (16, 16, 2), (16, 16, 7), (64, 64, 8)):
        np.zeros((3, h, w), np.float32).tofile(str(tmp_path / "in.bin"))
        r = subprocess.run([exe, "run", str(tmp_path / "in.bin"), str(w), str(h), str(skip), "1", str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "refused" in r.stderr, (w, h, skip)


def test_entry_points_declared_exported_and_bound():
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    header = open(os.path.join(ROOT, "include", "slowflow_amd.h")).read()
    L = C.CDLL(sfa.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in sfa.EXPORTS and hasattr(L, name), name
    assert header.count("dense_tracking.cpp:931-955") >= 4              # every entry point cites the lines it restates
    mk = open(os.path.join(ROOT, "slowflow_amd", "csrc", "Makefile")).read()
    assert "ref_image.hip" in mk and "ref_image.h" in mk
    # host only: the grid and the taps need no GPU
    assert sfa.reference_grid(1024, 436, 1) == (512, 218) and sfa.reference_grid(1024, 436, 3) == (256, 109) and sfa.reference_grid(5, 8, 1) == (2, 4)
    assert sfa.reference_grid(9, 5, 0) == (9, 5)
    assert sfa.reference_taps(1).tolist() == [1, 14, 62, 102, 62, 14, 1] and sfa.reference_taps(3).tolist() == [1, 8, 27, 56, 72, 56, 27, 8, 1]
    assert sfa.reference_taps(0).tolist() == []
    for w, h, skip, word in ((7, 8, 1, "resize"), (16, 16, 2, "skip = 2"), (16, 16, 7, "257"), (64, 64, 8, "skip = 8")):
        with pytest.raises(sfa.SlowflowError, match=word):
            sfa.reference_grid(w, h, skip)
    with pytest.raises(sfa.SlowflowError, match="skip = 5"):
        sfa.reference_taps(5)
    for name in ("reference_lab",):
        assert callable(getattr(sfa.Context, name))
    assert callable(sfa.TrackJob.upload_fill_reference) and callable(sfa.TrackJob.upload_fill_reference_device)
    import sys
    was = "torch" in sys.modules
    from slowflow_amd import device
    assert callable(device.reference_lab)
    assert was or "torch" not in sys.modules                           # torch stays lazily imported
