"""CPU-side checks of the device seam: slowflow_amd.device.device_view on hand-made objects that carry a __cuda_array_interface__ dict, the lazy
import (import slowflow_amd pulls in neither torch nor the device module), and the new C-ABI symbols in the header, both library builds and lib()."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

import slowflow_amd as sfa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["sfa_dev_layout_default", "sfa_job_upload_device", "sfa_job_set_flow_device", "sfa_job_download_device", "sfa_job_changes",
               "sfa_sequence_upload_device", "sfa_ctx_wait_stream", "sfa_ctx_signal_stream"]


class Fake:
    def __init__(self, shape, typestr="<f4", strides=None, ptr=0x7F0000001000, readonly=False):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, readonly), "version": 3, "strides": strides}


def test_contiguous_and_given_strides():
    from slowflow_amd import device
    v = device.device_view(Fake((2, 3, 3, 5, 7)), name="frames", ndim=5)
    assert (v.ptr, v.dtype, v.itemsize, v.shape) == (0x7F0000001000, 0, 4, (2, 3, 3, 5, 7)) and v.strides == (315, 105, 35, 7, 1)
    v = device.device_view(Fake((2, 5, 7, 3), "|u1", strides=(400, 40, 3, 1)), ndim=4)
    assert (v.dtype, v.itemsize, v.strides) == (1, 1, (400, 40, 3, 1))
    v = device.device_view(Fake((4, 6), "<u2", strides=(64, 2)))
    assert (v.dtype, v.itemsize, v.strides) == (2, 2, (32, 1))
    v = device.device_view(Fake((4, 2, 5, 7), strides=(0, 4000, 80, 4)))          # a window stride of 0: windows share their data
    assert v.strides == (0, 1000, 20, 1)
    s = v.sub(1, 2)
    assert s.shape == (2, 2, 5, 7) and s.ptr == v.ptr and device.device_view(s) is s
    v = device.device_view(Fake((4, 6), strides=(48, 4))).sub(3, 1)
    assert v.ptr == 0x7F0000001000 + 3 * 48


def test_layout_of_planar_interleaved_and_cropped_frames():
    from slowflow_amd import device
    w, h, F = 7, 5, 3
    n, lay = device.frames_layout(device.device_view(Fake((2, F, 3, h, w))), w, h, F)
    assert n == 2 and (lay.dtype, lay.window, lay.frame, lay.channel, lay.row, lay.column) == (0, 315, 105, 35, 7, 1)
    n, lay = device.frames_layout(device.device_view(Fake((2, F, h, w, 3), "|u1")), w, h, F)
    assert (lay.dtype, lay.window, lay.frame, lay.channel, lay.row, lay.column) == (1, 315, 105, 1, 21, 3)
    crop = Fake((2, F, 3, h, w), strides=tuple(4 * s for s in (9 * 8 * 10, 3 * 8 * 10, 8 * 10, 10, 1)))
    _, lay = device.frames_layout(device.device_view(crop), w, h, F)
    assert (lay.window, lay.frame, lay.channel, lay.row, lay.column) == (720, 240, 80, 10, 1)
    with pytest.raises(sfa.SlowflowError, match="neither"):
        device.frames_layout(device.device_view(Fake((2, F, 4, h, w))), w, h, F)
    # H = 3 fits both readings: planar unless the caller says otherwise
    amb = device.device_view(Fake((1, 1, 3, 3, 3)))
    assert device.frames_layout(amb, 3, 3, 1)[1].column == 1 and device.frames_layout(amb, 3, 3, 1, channels_last=True)[1].column == 3


@pytest.mark.parametrize("fake,kw,words", [
    (Fake((4, 6), strides=(26, 4)), {}, ("byte strides", "item size 4")),
    (Fake((4, 6), "<u2", strides=(12, 1)), {}, ("byte strides", "item size 2")),
    (Fake((4, 6), ">f4"), {}, ("byte order",)),
    (Fake((4, 6), "<f2"), {}, ("element type", "<f2")),
    (Fake((4, 6), "<f8"), {}, ("element type", "<f8")),
    (Fake((4, 6), "<i4"), {}, ("element type", "<i4")),
    (Fake((4, 6), readonly=True), {"writable": True}, ("read-only",)),
    (Fake((4, 6), "|u1"), {"writable": True}, ("outputs are fp32",)),
    (Fake((4, 6)), {"ndim": 4}, ("rank 2", "4 dimensions")),
    (Fake((4, 0)), {}, ("empty",)),
])
def test_device_view_refuses(fake, kw, words):
    from slowflow_amd import device
    with pytest.raises(sfa.SlowflowError) as e:
        device.device_view(fake, name="the_argument", **kw)
    assert "the_argument" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)


def test_a_read_only_input_is_accepted_and_a_host_array_is_not():
    import numpy as np
    from slowflow_amd import device
    assert device.device_view(Fake((4, 6), readonly=True)).shape == (4, 6)
    with pytest.raises(sfa.SlowflowError, match="__cuda_array_interface__"):
        device.device_view(np.zeros((4, 6), np.float32), name="frames")


def test_stream_handles():
    from slowflow_amd import device

    class S:
        cuda_stream = 0x1234
    assert device.stream_handle(None) == 0 and device.stream_handle(0) == 0 and device.stream_handle(77) == 77 and device.stream_handle(S()) == 0x1234


def test_import_does_not_pull_in_torch():
    code = ("import sys; import slowflow_amd; assert 'torch' not in sys.modules and 'slowflow_amd.device' not in sys.modules; "
            "import slowflow_amd.device; assert 'torch' not in sys.modules; print('lazy')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0 and "lazy" in r.stdout, r.stdout + r.stderr


def test_new_symbols_are_declared_exported_and_bound():
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slowflow_amd.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name + " is not declared"
        assert name in sfa.EXPORTS
    assert "sfa_dev_layout" in src and "SFA_DEV_U16" in src
    from slowflow_amd import device
    L = device._lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    assert L.sfa_job_upload_device.argtypes is not None and L.sfa_ctx_wait_stream.argtypes is not None
    assert C.sizeof(device.DevLayout) == 48 and device.DevLayout.window.offset == 8
    lay = device.default_layout(1024, 436, 3)
    assert (lay.dtype, lay.column, lay.row, lay.channel, lay.frame, lay.window) == (0, 1, 1024, 1024 * 436, 3 * 1024 * 436, 9 * 1024 * 436)
    for cls, name in ((sfa.Job, "upload_device"), (sfa.Job, "set_flow_device"), (sfa.Job, "download_device"), (sfa.Job, "changes"),
                      (sfa.Sequence, "upload_device"), (sfa.Context, "wait_stream"), (sfa.Context, "signal_stream")):
        assert callable(getattr(cls, name))
    assert callable(device.refine)


def test_the_release_library_exports_the_new_symbols():
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("hipcc not available")
    rel = os.path.join(ROOT, "slowflow_amd", "csrc", "build_release", "libslowflow_amd.so")
    if not os.path.exists(rel):                                   # tests/test_abi.py builds it for its own comparison; built here only where that has not run
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "slowflow_amd", "csrc"), "-j4", "release"], capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = subprocess.run(["nm", "-D", "--defined-only", rel], capture_output=True, text=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [n for n in NEW_SYMBOLS if n not in names]
    assert "k_pack_frames" in out and "k_pack_flow" in out and "k_unpack_planes" in out      # the kernels' host stubs: device_io.hip is in the build
