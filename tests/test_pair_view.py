"""CPU-side checks of the pair jobs' device seam (slowflow_amd/device.py: pair_job_upload_device, pair_job_set_flow_device, pair_job_download_device,
refine_pairs' geometry and split) on hand-made objects that carry a __cuda_array_interface__ dict, and of the new C-ABI symbols in the header, both
library builds and lib().  Every refusal here is raised before the library is called: the fake job has no handle."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import slowflow_amd as sfa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sfa_pair_job_create", "sfa_pair_job_destroy", "sfa_pair_job_upload", "sfa_pair_job_run", "sfa_pair_job_download",
               "sfa_pair_job_upload_device", "sfa_pair_job_set_flow_device", "sfa_pair_job_download_device", "sfa_pair_job_download_system"]


class Fake:
    def __init__(self, shape, typestr="<f4", strides=None, ptr=0x7F0000001000, readonly=False):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, readonly), "version": 3, "strides": strides}


class FakeJob:
    """what the seam reads of a PairJob before it calls the library"""
    w, h, n, h_, ctx = 7, 5, 4, None, None


def test_pair_geometry_of_planar_interleaved_and_cropped_frames():
    from slowflow_amd import device
    w, h = 7, 5
    assert device.pair_geometry(device.device_view(Fake((4, 2, 3, h, w)))) == (4, h, w)
    assert device.pair_geometry(device.device_view(Fake((4, 2, h, w, 3), "|u1"))) == (4, h, w)
    crop = Fake((2, 2, 3, h, w), "<u2", strides=tuple(2 * s for s in (6 * 8 * 10, 3 * 8 * 10, 8 * 10, 10, 1)))
    v = device.device_view(crop)
    assert device.pair_geometry(v) == (2, h, w)
    _, lay = device.frames_layout(v, w, h, 2)
    assert (lay.dtype, lay.window, lay.frame, lay.channel, lay.row, lay.column) == (2, 480, 240, 80, 10, 1)
    _, lay = device.frames_layout(device.device_view(Fake((4, 2, h, w, 3), "|u1")), w, h, 2)
    assert (lay.dtype, lay.window, lay.frame, lay.channel, lay.row, lay.column) == (1, 210, 105, 1, 21, 3)
    # H = 3 fits both readings: planar unless the caller says otherwise
    amb = device.device_view(Fake((1, 2, 3, 3, 3)))
    assert device.pair_geometry(amb) == (1, 3, 3) and device.pair_geometry(amb, channels_last=True) == (1, 3, 3)
    assert device.pair_geometry(device.device_view(Fake((1, 2, 3, 9, 3)))) == (1, 9, 3)            # [B,2,3,H,W] with W = 3 stays planar


@pytest.mark.parametrize("fake,words", [
    (Fake((2, 3, 5, 7)), ("frames", "rank 4", "5 dimensions")),
    (Fake((2, 3, 3, 5, 7)), ("frames", "3 frames per pair")),
    (Fake((2, 1, 3, 5, 7)), ("frames", "1 frames per pair")),
    (Fake((2, 2, 4, 5, 7)), ("frames", "neither")),
    (Fake((2, 2, 5, 7, 3)), ("frames", "neither")),                                       # interleaved, but the caller said planar
])
def test_pair_geometry_refuses(fake, words):
    from slowflow_amd import device
    kw = {"channels_last": False} if fake.__cuda_array_interface__["shape"] == (2, 2, 5, 7, 3) else {}
    with pytest.raises(sfa.SlowflowError) as e:
        device.pair_geometry(device.device_view(fake, name="frames"), **kw)
    assert all(w in str(e.value) for w in words), str(e.value)


def test_the_seam_refuses_before_it_calls_the_library():
    from slowflow_amd import device
    job = FakeJob()

    def refused(call, *words):
        with pytest.raises(sfa.SlowflowError) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)

    refused(lambda: device.pair_job_upload_device(job, Fake((4, 2, 3, 5))), "frames", "rank 4")
    refused(lambda: device.pair_job_upload_device(job, Fake((4, 3, 3, 5, 7))), "frames", "neither", "[B,2,3,5,7]")
    refused(lambda: device.pair_job_upload_device(job, Fake((4, 2, 3, 5, 8))), "frames", "neither")
    refused(lambda: device.pair_job_upload_device(job, Fake((4, 2, 3, 5, 7), "<f2")), "frames", "<f2")
    refused(lambda: device.pair_job_upload_device(job, object()), "frames", "__cuda_array_interface__")
    refused(lambda: device.pair_job_set_flow_device(job, Fake((4, 2, 5))), "flow", "rank 3")
    refused(lambda: device.pair_job_set_flow_device(job, Fake((4, 2, 5, 8))), "flow", "[B,2,5,7]")
    refused(lambda: device.pair_job_set_flow_device(job, Fake((4, 2, 5, 7), "|u1")), "flow", "fp32")
    refused(lambda: device.pair_job_download_device(job, Fake((4, 2, 5, 7), readonly=True)), "out_flow", "read-only")
    refused(lambda: device.pair_job_download_device(job, Fake((4, 2, 5, 7), "<u2")), "out_flow", "outputs are fp32")
    refused(lambda: device.pair_job_download_device(job, Fake((4, 3, 5, 7))), "out_flow", "[B,2,5,7]")


def test_a_device_view_made_earlier_is_checked_like_the_object_it_came_from():
    """device_view hands a DeviceView through (refine passes .sub() views on): its element type and shape are still checked"""
    import numpy as np
    from slowflow_amd import device
    job = FakeJob()
    u8 = device.device_view(Fake((4, 2, 5, 7), "|u1"))
    for call in (lambda: device.pair_job_set_flow_device(job, u8), lambda: device.pair_job_set_flow_device(job, u8.sub(1, 2)),
                 lambda: device.job_set_flow_device(job, u8), lambda: device.device_view(u8.sub(0, 1), name="flow", kinds=("f4",))):
        with pytest.raises(sfa.SlowflowError) as e:
            call()
        assert all(w in str(e.value) for w in ("flow", "u1", "fp32")), str(e.value)
    f8 = device.device_view(Fake((4, 6), "<f8"), kinds=("f8",))
    assert f8.dtype is None and device.device_view(f8.sub(1, 2), kinds=("f8",), shape=(2, 6)).kind == "f8"
    with pytest.raises(sfa.SlowflowError, match="fp32"):
        device.device_view(f8, kinds=("f4",))
    with pytest.raises(sfa.SlowflowError, match=r"a: \[4,7\] expected"):                   # a numpy integer is a size, not "any"
        device.device_view(Fake((4, 6)), name="a", shape=(4, np.int64(7)))
    assert device.device_view(Fake((4, 6)), shape=(None, "w")).shape == (4, 6)


def test_pair_sizes_split_like_refine():
    from slowflow_amd import device
    assert device.pair_sizes(1) == [1] and device.pair_sizes(128) == [128]
    assert device.pair_sizes(129) == [65, 64] and device.pair_sizes(130) == [65, 65] and device.pair_sizes(257) == [86, 86, 85]
    for B in (1, 127, 128, 129, 255, 256, 257, 1000):
        s = device.pair_sizes(B)
        assert sum(s) == B and max(s) <= device.MAX_BATCH and max(s) - min(s) <= 1


def test_new_symbols_are_declared_exported_and_bound():
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slowflow_amd.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name + " is not declared"
        assert name in sfa.EXPORTS
    from slowflow_amd import device
    L = device._lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    assert L.sfa_pair_job_upload_device.argtypes is not None and L.sfa_pair_job_download_device.argtypes is not None
    for name in ("upload", "run", "download", "download_system", "upload_device", "set_flow_device", "download_device", "close"):
        assert callable(getattr(sfa.PairJob, name))
    assert callable(device.refine_pairs) and callable(device.release_jobs)
    # the entry points refuse a null job by name instead of touching it (no GPU needed)
    L.sfa_last_error.restype = C.c_char_p
    assert L.sfa_pair_job_run(None) == -1 and b"sfa_pair_job_run" in L.sfa_last_error(None)
    assert L.sfa_pair_job_upload_device(None, 0, 1, None, None) == -1 and b"sfa_pair_job_upload_device" in L.sfa_last_error(None)


def test_the_release_library_exports_the_new_symbols_and_no_switch():
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    rel = os.path.join(ROOT, "slowflow_amd", "csrc", "build_release", "libslowflow_amd.so")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "slowflow_amd", "csrc"), "-j4", "release"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = subprocess.run(["nm", "-D", "--defined-only", rel], capture_output=True, text=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [n for n in NEW_SYMBOLS if n not in names]
    assert "k_data_2f_fused" in out                                # the kernel's host stub: the release build runs the fused kernel
    assert b"SFA_PAIR_UNFUSED" not in open(rel, "rb").read()       # and holds no switch that would select the stored stack
    L = C.CDLL(rel)
    L.sfa_last_error.restype = C.c_char_p
    assert L.sfa_debug_set(b"SFA_PAIR_UNFUSED", b"1") != 0 and b"release build" in L.sfa_last_error(None)
