"""Raw Bayer ingest, the part that needs no GPU: the pixel-by-pixel restatement the GPU tests compare against (tests/mosaic_ref.py) is `==` to the
whole-array formulations of tests/test_host.py -- which the existing tests pin to the host binary --, the crop reference is what it says, and the
binding, the header and the kernels' tile constant agree."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mosaic_ref as mr
import slowflow_amd as sfa
from test_host import bayer_cv8u_numpy, bayer_numpy, raw_weights_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")


@pytest.mark.parametrize("rx,ry", mr.REDS)
def test_restatement_equals_the_pinned_formulations(rx, ry):
    w, h = 37, 22
    rng = np.random.default_rng(100 + rx + 2 * ry)
    m = rng.uniform(20, 4000, (h, w)).astype(np.float32)
    assert np.array_equal(mr.bayer_gr(m, rx, ry), bayer_numpy(m, rx, ry))
    m8 = rng.uniform(-20, 300, (h, w)).astype(np.float32)
    m8[3, 5:9] = [0.5, 1.5, 2.5, 254.5]                                          # halves round to even
    assert np.array_equal(mr.bayer_cv8u(m8, rx, ry), bayer_cv8u_numpy(m8, rx, ry))
    m16 = rng.integers(0, 65536, (h, w)).astype(np.uint16)                       # a 16-bit input saturates
    assert np.array_equal(mr.bayer_cv8u(m16, rx, ry), bayer_cv8u_numpy(m16.astype(np.float32), rx, ry))
    for weight in (0.5, 1.0, 2.0, 5.0):
        assert np.array_equal(mr.raw_weights(w, h, rx, ry, weight), raw_weights_numpy(w, h, rx, ry, weight))


def test_zero_green_gives_the_pinned_inf_and_nan():
    rng = np.random.default_rng(7)
    m = rng.uniform(20, 4000, (12, 14)).astype(np.float32)
    m[4:8, 5:9] = 0
    with np.errstate(all="ignore"):
        want = bayer_numpy(m, 1, 0)
    got = mr.bayer_gr(m, 1, 0)
    assert np.isnan(got).any() and np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("method", [0, 2])
def test_crop_reference_keeps_the_pattern_of_the_full_mosaic(method):
    """demosaic-then-slice at an odd origin equals, away from the crop's own border, the demosaicing of the sliced mosaic with the red site moved by the
    origin's parity -- and differs from it with the red site left where it was: the crop must not flip the pattern"""
    rng = np.random.default_rng(3)
    m = rng.integers(1, 256, (29, 41)).astype(np.uint8)
    x0, y0, w, h = 3, 5, 20, 12
    ref = mr.demosaic_crop(m, 1, 0, method, (x0, y0), (w, h))
    assert ref.shape == (3, h, w)
    part = m[y0:y0 + h, x0:x0 + w]
    moved = mr.demosaic(part, (1 - x0) % 2, (0 - y0) % 2, method)
    kept = mr.demosaic(part, 1, 0, method)
    inner = (slice(None), slice(2, -2), slice(2, -2))
    assert np.array_equal(ref[inner], moved[inner]) and not np.array_equal(ref[inner], kept[inner])
    assert np.array_equal(mr.demosaic_crop(m, 1, 0, method), mr.demosaic(m, 1, 0, method))


def test_binding_header_and_tile_constant_agree():
    src = open(os.path.join(ROOT, "slowflow_amd", "csrc", "mosaic.hip")).read()
    tx, ty = re.search(r"constexpr int MOS_TX = (\d+), MOS_TY = (\d+);", src).groups()
    assert sfa.MOSAIC_TILE == (int(tx), int(ty))
    new = ["sfa_demosaic_device", "sfa_sequence_upload_mosaic_device", "sfa_sequence_upload_mosaic", "sfa_job_set_raw_weights", "sfa_sequence_rescale"]
    assert all(n in sfa.EXPORTS for n in new)
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    L = sfa.lib()
    assert all(hasattr(L, n) for n in new)
    for cls, names in ((sfa.Sequence, ("upload_mosaic", "upload_mosaic_device", "rescale_from")), (sfa.Job, ("set_raw_weights",))):
        assert all(callable(getattr(cls, n, None)) for n in names)
    from slowflow_amd import device
    import ctypes as C
    assert callable(device.demosaic) and C.sizeof(device.MosaicDesc) == 48      # int, 3 x long long, 4 x int
    hdr = open(os.path.join(ROOT, "include", "slowflow_amd.h")).read()
    assert "typedef struct sfa_mosaic_desc { int dtype; long long frame, row, column; int W, H, x0, y0; } sfa_mosaic_desc;" in hdr


def test_import_does_not_import_torch():
    r = subprocess.run([sys.executable, "-c", "import sys; import slowflow_amd; from slowflow_amd import device; assert 'torch' not in sys.modules"],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_rescale_size_and_sigma_rules():
    assert mr.rescaled_size(64, 48, 0.5) == (32, 24) and mr.rescaled_size(64, 48, 0.25) == (16, 12) and mr.rescaled_size(64, 48, 0.3) == (19, 14)
    assert mr.rescaled_size(5, 7, 0.5) == (2, 4)                                 # lrint: halves to even
    assert mr.rescale_sigma(0.5) == 1.0 and abs(mr.rescale_sigma(0.25) - 2 ** 0.5) < 1e-7


def test_driver_refuses_gpu_ingest_where_the_host_needs_the_frames(tmp_path):
    """gpu_ingest 1 with raw 0, deep_matching 1 or a verbosity that writes the frames: exit status 1, the key named, before a frame is read or a GPU asked for"""
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    base = "file\t%s/f_%%03i.pgm\noutput\t%s/out\nJets\t1\nstart\t1\ngpu_ingest\t1\n" % (tmp_path, tmp_path)
    for extra, word in (("raw\t0\ndeep_matching\t0\n", "raw 0"), ("raw\t1\nraw_demosaicing\t0\ndeep_matching\t1\n", "deep_matching 1"),
                        ("raw\t1\nraw_demosaicing\t2\ndeep_matching\t0\nverbose\t0000100000\n", "verbos")):
        cfg = tmp_path / "a.cfg"
        cfg.write_text(base + extra)
        r = subprocess.run([os.path.join(HOST, "slow_flow"), str(cfg), "-overwrite"], capture_output=True, text=True)
        assert r.returncode == 1 and "gpu_ingest" in r.stderr and word in r.stderr, (r.returncode, r.stderr)
        assert not (tmp_path / "out").exists()
