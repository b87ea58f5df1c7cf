"""slowflow_amd.device -- the device seam of the C-ABI (include/slowflow_amd.h: sfa_job_upload_device ...) for Python callers: frames, initial flow
and results that live in GPU memory go in and out of a job without a host copy.

The core takes any object with `__cuda_array_interface__` (torch-ROCm tensors, cupy arrays ...) and needs no torch; `import slowflow_amd` does not
import this module, and this module imports torch only inside demosaic(), rgb8_to_lab(), epic(), refine(), refine_pairs(), track() and flow_quantiles(), to allocate the outputs
and to find the caller's current stream (on_stream, the one stream bracket of the five).  device_view is the one place an argument's element type, rank
and shape are checked.  refine() is the multi-frame path on resident jobs; refine_pairs() the two-frame path on resident pair jobs, which
never waits for the GPU; track() dense_tracking's accumulation, energies and fusion on a resident track job, which does not wait either;
flow_quantiles() adaptiveFR's flow-magnitude quantile and maximum of groups of flows, left in GPU memory.

Stream contract: the library works on the context's own stream.  Context.wait_stream(s) before the first call makes that stream wait for what the
caller has submitted to s; Context.signal_stream(s) after the last makes s wait for the library.  refine() and refine_pairs() do both.  With the two in place a tensor
freed or reused on s is ordered after the library's last access, so torch's caching allocator needs no record_stream.
"""
import contextlib
import ctypes as C
import sys
from collections import OrderedDict

import numpy as np

import slowflow_amd as sfa

MAX_BATCH = 128                                   # windows of one job (csrc/sfa_internal.h: kMaxBatch)
DTYPES = {"f4": 0, "u1": 1, "u2": 2}              # sfa_dev_dtype by typestr kind + size
KIND_NAMES = {"f4": "fp32", "f8": "fp64", "i4": "int32", "i8": "int64", "u1": "uint8", "u2": "uint16", "u8": "uint64"}


class DevLayout(C.Structure):
    """sfa_dev_layout: element type and element strides of (window, frame, channel, row, column)"""
    _fields_ = [("dtype", C.c_int), ("window", C.c_longlong), ("frame", C.c_longlong), ("channel", C.c_longlong), ("row", C.c_longlong),
                ("column", C.c_longlong)]


class DeviceView:
    """pointer, element type (sfa_dev_dtype, or None where none names it), shape and ELEMENT strides of a device array; kind: the typestr's kind + size ("f4")"""

    def __init__(self, ptr, dtype, itemsize, shape, strides, owner=None, kind=None):
        self.ptr, self.dtype, self.itemsize, self.shape, self.strides, self.owner = ptr, dtype, itemsize, tuple(shape), tuple(strides), owner
        self.kind = kind if kind is not None else next((k for k, d in DTYPES.items() if d == dtype), None)

    def sub(self, start, n):
        """elements [start, start + n) of the first dimension"""
        assert 0 <= start and n >= 1 and start + n <= self.shape[0]
        return DeviceView(self.ptr + start * self.strides[0] * self.itemsize, self.dtype, self.itemsize, (n,) + self.shape[1:], self.strides, self.owner, self.kind)


def device_view(obj, writable=False, name="array", ndim=None, kinds=None, shape=None, contiguous=False):
    """obj.__cuda_array_interface__ -> DeviceView.  Refuses (SlowflowError naming `name`): a tensor on the CPU and objects without the interface (host
    arrays), element types other than fp32 / u8 / u16, non-native byte order, byte strides that are no multiple of the item size, a read-only object asked
    for as an output, a rank other than `ndim`, a shape other than `shape` (an entry that is None or a letter such as "B" takes any size; the rank
    follows from it), and with `contiguous` any strides but the dense ones.  kinds: the element types taken instead of those three, e.g. ("f8",) for the
    track job's fp64 flow (the view's dtype is then None where no sfa_dev_dtype names it).  Whether the pointer is device memory of the job's GPU is the
    library's check, made before anything is launched."""
    if shape is not None:
        ndim = len(shape)
    if isinstance(obj, DeviceView):
        v = obj
        if kinds is not None and v.kind not in kinds:           # (a view made earlier with other kinds, or by hand)
            raise sfa.SlowflowError(f"{name}: element type {v.kind!r}, expected {' or '.join(KIND_NAMES[k] for k in kinds)}")
    else:
        if getattr(obj, "is_cuda", True) is False:              # a torch tensor on the CPU raises from its __cuda_array_interface__
            raise sfa.SlowflowError(f"{name}: a tensor on {getattr(obj, 'device', 'the host')}, not in GPU memory (the device entry points take device memory)")
        cai = getattr(obj, "__cuda_array_interface__", None)
        if cai is None:
            raise sfa.SlowflowError(f"{name}: {type(obj).__name__} has no __cuda_array_interface__ (a host array? the device entry points take device memory)")
        typestr = cai["typestr"]
        order, kind = typestr[0], typestr[1:]
        native = "<" if sys.byteorder == "little" else ">"
        if order not in (native, "|", "="):
            raise sfa.SlowflowError(f"{name}: byte order of typestr {typestr!r} is not the machine's")
        if kinds is not None and kind not in kinds:
            raise sfa.SlowflowError(f"{name}: element type {typestr!r}, expected {' or '.join(KIND_NAMES[k] for k in kinds)}")
        if kinds is None and kind not in DTYPES:
            raise sfa.SlowflowError(f"{name}: element type {typestr!r} is not supported (fp32, uint8 and uint16 are; fp16, bf16, fp64 and signed integers are not)")
        item = int(kind[1:])
        dims = tuple(int(s) for s in cai["shape"])
        ptr, readonly = cai["data"]
        if writable and readonly:
            raise sfa.SlowflowError(f"{name}: the object is read-only and cannot be an output")
        if writable and kinds is None and kind != "f4":
            raise sfa.SlowflowError(f"{name}: outputs are fp32, not {typestr!r}")
        bst = cai.get("strides")
        if bst is None:
            st, acc = [], 1
            for s in reversed(dims):
                st.append(acc)
                acc *= s
            st = tuple(reversed(st))
        else:
            if any(int(b) % item for b in bst):
                raise sfa.SlowflowError(f"{name}: byte strides {tuple(bst)} are not multiples of the item size {item}")
            st = tuple(int(b) // item for b in bst)
        if any(s == 0 for s in dims):
            raise sfa.SlowflowError(f"{name}: empty array, shape {dims}")
        v = DeviceView(int(ptr or 0), DTYPES.get(kind), item, dims, st, obj, kind)
    if ndim is not None and len(v.shape) != ndim:
        raise sfa.SlowflowError(f"{name}: rank {len(v.shape)}, shape {v.shape}; {ndim} dimensions expected")
    if shape is not None and any(want is not None and not isinstance(want, str) and got != want for got, want in zip(v.shape, shape)):
        raise sfa.SlowflowError(f"{name}: [{','.join('*' if want is None else str(want) for want in shape)}] expected, got shape {v.shape}")
    if contiguous and v.strides != tuple(int(np.prod(v.shape[i + 1:])) for i in range(len(v.shape))):
        raise sfa.SlowflowError(f"{name}: a contiguous array expected, element strides {v.strides}")
    return v


def frames_size(v, channels_last=None):
    """(h, w) of frames [B,F,3,H,W] (planar) or [B,F,H,W,3] (interleaved).  channels_last None: told from the shape, planar where both fit."""
    last = (v.shape[2] != 3 and v.shape[4] == 3) if channels_last is None else channels_last
    return (v.shape[2], v.shape[3]) if last else (v.shape[3], v.shape[4])


def frames_layout(v, w, h, F, channels_last=None, name="frames"):
    """[B,F,3,H,W] (planar) or [B,F,H,W,3] (interleaved) -> (B, DevLayout).  channels_last None: told from the shape, planar where both fit."""
    planar, inter = v.shape[1:] == (F, 3, h, w), v.shape[1:] == (F, h, w, 3)
    if channels_last is None:
        channels_last = inter and not planar
    if not (inter if channels_last else planar):
        raise sfa.SlowflowError(f"{name}: shape {v.shape} is neither [B,{F},3,{h},{w}] nor [B,{F},{h},{w},3]")
    s = v.strides
    lay = DevLayout(v.dtype, s[0], s[1], s[4], s[2], s[3]) if channels_last else DevLayout(v.dtype, s[0], s[1], s[2], s[3], s[4])
    return v.shape[0], lay


class MosaicDesc(C.Structure):
    """sfa_mosaic_desc: element type, element strides of (frame, row, column), the full mosaic's size and the crop's origin"""
    _fields_ = [("dtype", C.c_int), ("frame", C.c_longlong), ("row", C.c_longlong), ("column", C.c_longlong), ("W", C.c_int), ("H", C.c_int), ("x0", C.c_int),
                ("y0", C.c_int)]


_LL4, _LL3 = C.c_longlong * 4, C.c_longlong * 3
_bound = False


def _lib():
    global _bound
    L = sfa.lib()
    if not _bound:
        L.sfa_job_upload_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(DevLayout), C.c_void_p]
        L.sfa_job_set_flow_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.sfa_job_download_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sfa_job_changes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.sfa_sequence_upload_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(DevLayout)]
        L.sfa_pair_job_upload_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(DevLayout)]
        L.sfa_pair_job_set_flow_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.sfa_pair_job_download_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.sfa_ctx_wait_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.sfa_ctx_signal_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.sfa_dev_layout_default.argtypes = [C.POINTER(DevLayout), C.c_int, C.c_int, C.c_int]
        L.sfa_dev_layout_default.restype = None
        L.sfa_demosaic_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(MosaicDesc), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.sfa_sequence_upload_mosaic_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(MosaicDesc), C.c_int, C.c_int, C.c_int]
        L.sfa_track_job_upload_flows_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sfa_track_job_upload_frames_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.sfa_track_job_download_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sfa_track_job_upload_occlusions_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.sfa_track_job_download_rate_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
        L.sfa_track_job_download_best_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.sfa_track_job_upload_fill_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sfa_flow_magnitude_quantiles_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                          C.c_float, C.c_float, C.c_void_p]
        L.sfa_rgb8_to_lab_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        L.sfa_reference_lab_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.sfa_track_job_upload_fill_reference_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        L.sfa_epic_job_upload_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.sfa_epic_job_set_matches_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.sfa_epic_job_download_device.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _bound = True
    return L


def default_layout(w, h, n_frames):
    """sfa_dev_layout_default: contiguous planar fp32 [n][n_frames][3][h][w]"""
    lay = DevLayout()
    _lib().sfa_dev_layout_default(C.byref(lay), int(w), int(h), int(n_frames))
    return lay


def stream_handle(stream):
    """None / 0: the device's null stream (torch's default stream); an int: a hipStream_t; else an object with .cuda_stream (torch.cuda.Stream)"""
    if stream is None:
        return 0
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)


def wait_stream(ctx, stream=None):
    ctx._ck(_lib().sfa_ctx_wait_stream(ctx.h, C.c_void_p(stream_handle(stream))), "sfa_ctx_wait_stream")


def signal_stream(ctx, stream=None):
    ctx._ck(_lib().sfa_ctx_signal_stream(ctx.h, C.c_void_p(stream_handle(stream))), "sfa_ctx_signal_stream")


def job_upload_device(job, frames, b0=0, chw=None, channels_last=None):
    F = job.n_frames
    v = device_view(frames, name="frames", ndim=5)
    n, lay = frames_layout(v, job.w, job.h, F, channels_last)
    cw = None
    keep = None
    if chw is not None:
        keep = [np.ascontiguousarray(c, np.float32) for c in chw]
        assert all(c.shape == (job.h, sfa.stride_of(job.w)) for c in keep), "channel weights are 3 host planes (h, stride_of(w))"
        cw = (C.c_void_p * 3)(*[c.ctypes.data for c in keep])
    job.ctx._ck(_lib().sfa_job_upload_device(job.h_, int(b0), n, C.c_void_p(v.ptr), C.byref(lay), cw), "sfa_job_upload_device")


def _set_flow_device(job, fn, size, flow, b0, n):
    """the start flow of a job or a pair job: `fn` the C function, `size` the attribute that holds the job's batch size"""
    if flow is None:
        n = getattr(job, size) - b0 if n is None else n
        job.ctx._ck(getattr(_lib(), fn)(job.h_, int(b0), int(n), None, None), fn)
        return
    v = device_view(flow, name="flow", kinds=("f4",), shape=("B", 2, job.h, job.w))
    job.ctx._ck(getattr(_lib(), fn)(job.h_, int(b0), v.shape[0], C.c_void_p(v.ptr), _LL4(*v.strides)), fn)


def _download_device(job, fn, out_flow, b0, takes_occ=False, out_occ=None):
    """the flow of a job or a pair job: `fn` the C function; takes_occ: it has the two arguments of an optional occlusion destination"""
    v = device_view(out_flow, writable=True, name="out_flow", shape=("B", 2, job.h, job.w))
    args = [job.h_, int(b0), v.shape[0], C.c_void_p(v.ptr), _LL4(*v.strides)]
    if out_occ is not None:
        o = device_view(out_occ, writable=True, name="out_occ", shape=(v.shape[0], job.h, job.w))
        args += [C.c_void_p(o.ptr), _LL3(*o.strides)]
    elif takes_occ:
        args += [None, None]
    job.ctx._ck(getattr(_lib(), fn)(*args), fn)


def job_set_flow_device(job, flow, b0=0, n=None):
    _set_flow_device(job, "sfa_job_set_flow_device", "batch", flow, b0, n)


def job_download_device(job, out_flow, out_occ=None, b0=0):
    _download_device(job, "sfa_job_download_device", out_flow, b0, True, out_occ)


def job_changes(job, b0=0, n=None):
    n = job.batch - b0 if n is None else n
    out = np.zeros((max(n, 0), 2), np.float32)
    job.ctx._ck(_lib().sfa_job_changes(job.h_, int(b0), int(n), C.c_void_p(out.ctypes.data)), "sfa_job_changes")
    return out


def sequence_upload_device(seq, frames, f0=0, channels_last=None):
    v = device_view(frames, name="frames", ndim=4)
    # a sequence's frames are the windows of a [N,1,...] array
    v5 = DeviceView(v.ptr, v.dtype, v.itemsize, (v.shape[0], 1) + v.shape[1:], (v.strides[0], 0) + v.strides[1:], v.owner)
    n, lay = frames_layout(v5, seq.w, seq.h, 1, channels_last)
    lay.frame, lay.window = lay.window, 0                       # sfa_sequence_upload_device steps by layout.frame
    seq.ctx._ck(_lib().sfa_sequence_upload_device(seq.h_, int(f0), n, C.c_void_p(v.ptr), C.byref(lay)), "sfa_sequence_upload_device")


def mosaic_desc(v, origin=(0, 0), size=None):
    """a DeviceView of mosaics [N,H,W] -> (N, MosaicDesc, (w, h)): the crop of `size` = (w, h) at `origin` = (x0, y0); size None: the rest of the mosaic"""
    N, H, W = v.shape
    x0, y0 = int(origin[0]), int(origin[1])
    w, h = (W - x0, H - y0) if size is None else (int(size[0]), int(size[1]))
    return N, MosaicDesc(v.dtype, v.strides[0], v.strides[1], v.strides[2], W, H, x0, y0), (w, h)


def sequence_upload_mosaic_device(seq, mosaic, red=(1, 0), method=0, f0=0, origin=(0, 0), size=None):
    v = device_view(mosaic, name="mosaic", ndim=3)
    n, desc, (w, h) = mosaic_desc(v, origin, size if size is not None else (seq.w, seq.h))
    if (w, h) != (seq.w, seq.h):
        raise sfa.SlowflowError(f"size: the crop is {w} x {h}, the sequence {seq.w} x {seq.h}")
    seq.ctx._ck(_lib().sfa_sequence_upload_mosaic_device(seq.h_, int(f0), n, C.c_void_p(v.ptr), C.byref(desc), int(method), int(red[0]), int(red[1])),
                "sfa_sequence_upload_mosaic_device")


@contextlib.contextmanager
def on_stream(torch, ctx, like, stream, alloc):
    """The stream bracket of the public functions.  `stream` None is the current stream of the device of `like`; alloc(device) makes the outputs under that
    stream, so that they belong to it; then the context's stream waits for it, the body enqueues, and it waits for the context -- also when the body
    raises.  Yields (stream, the outputs)."""
    if stream is None:
        stream = torch.cuda.current_stream(like.device)
    with torch.cuda.stream(stream):
        outputs = alloc(like.device)
    wait_stream(ctx, stream)
    try:
        yield stream, outputs
    finally:
        signal_stream(ctx, stream)


def demosaic(ctx, mosaic, red=(1, 0), method=0, origin=(0, 0), size=None, *, stream=None):
    """Demosaic N Bayer mosaics that live on the context's GPU: mosaic = a torch tensor [N,H,W] (fp32, uint8 or uint16; any strides with a positive column
    stride); red = (red_x, red_y), the cfg's raw_red_loc; method 0 (bayer2rgbGR) or 2 (the 8-bit OpenCV conversion); origin / size = the crop (x0, y0) /
    (w, h) inside the mosaic (default: all of it).  Returns a new fp32 tensor [N,3,h,w] with the bits of the host routines.  Ordered after what `stream`
    (default: torch.cuda.current_stream) holds at the call, and `stream` waits for it afterwards; the call only enqueues."""
    import torch
    v = device_view(mosaic, name="mosaic", ndim=3)
    n, desc, (w, h) = mosaic_desc(v, origin, size)
    if w < 1 or h < 1:
        raise sfa.SlowflowError(f"size: the crop {w} x {h} at origin {tuple(origin)} of the {v.shape[2]} x {v.shape[1]} mosaic is empty")
    with on_stream(torch, ctx, mosaic, stream, lambda dev: torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)) as (_, out):
        ov = device_view(out, writable=True, name="out")
        ctx._ck(_lib().sfa_demosaic_device(ctx.h, n, C.c_void_p(v.ptr), C.byref(desc), int(method), int(red[0]), int(red[1]), C.c_void_p(ov.ptr), _LL4(*ov.strides),
                                           w, h), "sfa_demosaic_device")
    return out


def rgb8_to_lab(ctx, rgb, norm=1.0, *, stream=None, out=None):
    """The L*a*b* image EpicFlow's saliency reads (host/epic.cpp: rgb8_to_lab; csrc/lab_math.h) of n frames that live on the context's GPU: rgb = a torch
    fp32 tensor [n,3,h,w] of any strides holding the samples as they were read; every sample times `norm` (1/255 for 16-bit frames) is rounded to 8 bits
    first.  Returns a new fp32 tensor [n,3,h,w] (L, a c, b c), or fills `out` (any strides that keep its elements apart, no overlap with rgb) and returns
    it; the bits of the host function.  Ordered after what `stream` (default: torch.cuda.current_stream) holds at the call, and `stream` waits for it
    afterwards; the call only enqueues."""
    import torch
    v = device_view(rgb, name="rgb", kinds=("f4",), shape=("n", 3, None, None))
    n, _, h, w = v.shape
    with on_stream(torch, ctx, rgb, stream, lambda dev: torch.empty((n, 3, h, w), dtype=torch.float32, device=dev) if out is None else out) as (_, res):
        ov = device_view(res, writable=True, name="out", shape=(n, 3, h, w))
        ctx._ck(_lib().sfa_rgb8_to_lab_device(ctx.h, n, w, h, C.c_void_p(v.ptr), _LL4(*v.strides), float(norm), C.c_void_p(ov.ptr), _LL4(*ov.strides)),
                "sfa_rgb8_to_lab_device")
    return res


def reference_lab(ctx, rgb, skip, norm=1.0, *, return_rgb8=False, stream=None, out=None, out_rgb8=None):
    """dense_tracking's reduced reference image (dense_tracking.cpp:931-955; csrc/ref_image.hip) of n frames that live on the context's GPU: rgb = a torch
    fp32 tensor [n,3,h,w] of any strides holding the samples as they were read; 8 bits, OpenCV's 8-bit Gaussian blur and its bilinear reduction to the grid
    of sfa.reference_grid(w, h, skip), then the Lab image, in one kernel.  Returns a new fp32 tensor [n,3,gh,gw] (or fills `out`); with return_rgb8 (or
    out_rgb8) also the reduced 8-bit RGB image, uint8 [n,3,gh,gw], the edge detector's input.  skip 0 is rgb8_to_lab.  Stream order as rgb8_to_lab."""
    import torch
    v = device_view(rgb, name="rgb", kinds=("f4",), shape=("n", 3, None, None))
    n, _, h, w = v.shape
    gw, gh = sfa.reference_grid(w, h, skip)
    want8 = return_rgb8 or out_rgb8 is not None

    def alloc(dev):
        res = torch.empty((n, 3, gh, gw), dtype=torch.float32, device=dev) if out is None else out
        r8 = (torch.empty((n, 3, gh, gw), dtype=torch.uint8, device=dev) if out_rgb8 is None else out_rgb8) if want8 else None
        return res, r8

    with on_stream(torch, ctx, rgb, stream, alloc) as (_, (res, r8)):
        ov = device_view(res, writable=True, name="out", shape=(n, 3, gh, gw))
        qv = device_view(r8, writable=True, name="out_rgb8", kinds=("u1",), shape=(n, 3, gh, gw)) if want8 else None
        ctx._ck(_lib().sfa_reference_lab_device(ctx.h, n, w, h, int(skip), C.c_void_p(v.ptr), _LL4(*v.strides), float(norm), C.c_void_p(ov.ptr), _LL4(*ov.strides),
                                                C.c_void_p(qv.ptr) if qv else None, _LL4(*qv.strides) if qv else None), "sfa_reference_lab_device")
    return (res, r8) if want8 else res


def epic_job_upload_device(job, lab=None, cost=None, i0=0, cost_has_euc=False):
    lv = device_view(lab, name="lab", kinds=("f4",), shape=("n", 3, job.h, job.w)) if lab is not None else None
    cv = device_view(cost, name="cost", kinds=("f4",), shape=("n", job.h, job.w)) if cost is not None else None
    if lv is not None and cv is not None and lv.shape[0] != cv.shape[0]:
        raise sfa.SlowflowError(f"cost: {cv.shape[0]} maps for {lv.shape[0]} Lab images")
    n = lv.shape[0] if lv is not None else cv.shape[0] if cv is not None else 0
    job.ctx._ck(_lib().sfa_epic_job_upload_device(job.h_, int(i0), n, C.c_void_p(lv.ptr) if lv else None, _LL4(*lv.strides) if lv else None,
                                                  C.c_void_p(cv.ptr) if cv else None, _LL3(*cv.strides) if cv else None, int(bool(cost_has_euc))),
                "sfa_epic_job_upload_device")


def epic_job_set_matches_device(job, i, matches):
    if matches is None or (hasattr(matches, "shape") and matches.shape[0] == 0):
        job.ctx._ck(_lib().sfa_epic_job_set_matches_device(job.h_, int(i), None, 0), "sfa_epic_job_set_matches_device")
        return
    v = device_view(matches, name="matches", kinds=("f4",), shape=("nm", 4), contiguous=True)
    job.ctx._ck(_lib().sfa_epic_job_set_matches_device(job.h_, int(i), C.c_void_p(v.ptr), v.shape[0]), "sfa_epic_job_set_matches_device")


def epic_job_download_device(job, out_flow, i0=0):
    v = device_view(out_flow, writable=True, name="out_flow", shape=("n", 2, job.h, job.w))
    job.ctx._ck(_lib().sfa_epic_job_download_device(job.h_, int(i0), v.shape[0], C.c_void_p(v.ptr), _LL4(*v.strides)), "sfa_epic_job_download_device")


def epic(ctx, params, lab, cost, matches, *, cost_has_euc=False, stream=None, workspace_bytes=0):
    """EpicFlow's interpolation (epic(), epic_flow_extended/epic.cpp:147-235) of n images whose inputs live on the context's GPU, on a resident epic job:
    lab = a torch fp32 tensor [n,3,h,w] (rgb8_to_lab's; None with params.saliency_th == 0), cost = [n,h,w] edge costs (cost_has_euc: params.euc is in
    them already; else the job adds it), matches = a list of n [nm_i,4] arrays of x1 y1 x2 y2: torch tensors on the GPU (contiguous fp32) or host arrays
    (those are tested for finite values).  Returns (flow, rc): a new fp32 tensor [n,2,h,w] on the GPU that refine(flow=) and refine_pairs(flow0=) take as
    it is, and epic()'s return value per image (1: no match left, a field of zeros).  The planes equal Context.epic_batch's bit for bit.  The call
    WAITS for the GPU where the chain reads the survivors of its filters; an image that does not fit workspace_bytes even alone raises."""
    import torch
    cv = device_view(cost, name="cost", kinds=("f4",), shape=("n", None, None))
    n, h, w = cv.shape
    if len(matches) != n:
        raise sfa.SlowflowError(f"matches: {len(matches)} lists for {n} cost maps")
    if lab is None and params.saliency_th != 0:                   # (the job is kept between calls, and with it the last call's saliency planes)
        raise sfa.SlowflowError("lab: None with saliency_th != 0: the saliency filter reads the Lab images")
    if stream is None:
        stream = torch.cuda.current_stream(cost.device)
    staged = []
    with torch.cuda.stream(stream):                               # host match lists go up on the caller's stream, which the context then waits for
        for i, m in enumerate(matches):
            if m is not None and not hasattr(m, "__cuda_array_interface__") and not getattr(m, "is_cuda", False):
                a = np.ascontiguousarray(m, dtype=np.float32).reshape(-1, 4)
                if not np.isfinite(a).all():
                    raise sfa.SlowflowError(f"matches[{i}]: a coordinate that is not finite")
                m = torch.from_numpy(a).to(cost.device) if len(a) else None
            staged.append(m)
    job = _cached_job(ctx, "_epic_jobs", (w, h, n, bytes(params)), lambda: sfa.EpicJob(ctx, params, w, h, n))
    with on_stream(torch, ctx, cost, stream, lambda dev: torch.empty((n, 2, h, w), dtype=torch.float32, device=dev)) as (_, flow):
        epic_job_upload_device(job, lab if params.saliency_th != 0 else None, cost, 0, cost_has_euc)
        for i, m in enumerate(staged):
            epic_job_set_matches_device(job, i, m)
        rc, _ = job.run(n, workspace_bytes)
        epic_job_download_device(job, flow, 0)
    return flow, rc


def pair_sizes(B):
    """a batch of B windows or pairs as jobs of at most MAX_BATCH each, of equal or nearly equal size: the split of refine() and refine_pairs()"""
    pieces = -(-B // MAX_BATCH)
    return [B // pieces + (1 if i < B % pieces else 0) for i in range(pieces)]


def _cached_job(ctx, cache_name, key, create):
    """the job kept on the context under `key` from call to call, or create() in its place (two per cache at most: a batch beyond MAX_BATCH splits into at
    most two sizes)"""
    cache = ctx.__dict__.setdefault(cache_name, OrderedDict())
    job = cache.get(key)
    if job is not None and job.h_:
        cache.move_to_end(key)
        return job
    while len(cache) >= 2:
        cache.popitem(last=False)[1].close()
    job = cache[key] = create()
    return job


def _job_for(ctx, params, w, h, nb):
    return _cached_job(ctx, "_refine_jobs", (bytes(params), w, h, nb), lambda: sfa.Job(ctx, params, w, h, nb))


def release_jobs(ctx):
    """closes the jobs refine() and refine_pairs() keep on the context (they hold their device memory between calls)"""
    for job in ctx.__dict__.pop("_refine_jobs", {}).values():
        job.close()
    for job in ctx.__dict__.pop("_epic_jobs", {}).values():
        job.close()
    for job in ctx.__dict__.pop("_refine_pair_jobs", {}).values():
        job.close()
    for job in ctx.__dict__.pop("_track_jobs", {}).values():
        job.close()


def refine(ctx, params, frames, flow=None, *, normalize=False, want_occ=False, stream=None, channels_last=None, raw_weights=None):
    """Refine the flow of B frame windows that live on the context's GPU: frames = a torch tensor [B,F,3,H,W] or [B,F,H,W,3] (fp32, uint8 or uint16;
    any strides with a positive column stride), F = 2 (S - 1) + 1; flow = None (zeros) or an fp32 tensor [B,2,H,W].  Returns (flow [B,2,H,W], occlusions
    [B,H,W] or None, change norms as a numpy array [B,2]), the tensors on the frames' device.  The work is ordered after what `stream` (default:
    torch.cuda.current_stream) holds at the call, and `stream` waits for it afterwards; the call itself returns when the refinement has run (sfa_job_run
    takes its break decisions on the host).  B > 128 is split into jobs of equal or nearly equal size.
    normalize=True: the frames go through a Sequence first -- normalize() over the B x F frames as passed, the bits of Sequence.normalize -- and the
    statistics replace params.norm_avg / norm_std (of a copy), as the driver does.  Without it the frames are taken as they are.
    The jobs stay on the context for the next call of the same shape and parameters (release_jobs(ctx) or ctx.close() frees them); with normalize=True
    the statistics are part of the parameters, so that mode creates its jobs per call and closes them before it returns.
    raw_weights = (red_x, red_y, weight): every window runs with rawWeighting's channel weights (the cfg's raw_red_loc and raw_weight), formed on the GPU."""
    import torch
    F = 2 * (params.S - 1) + 1
    fv = device_view(frames, name="frames", ndim=5)
    h, w = frames_size(fv, channels_last)
    B, _ = frames_layout(fv, w, h, F, channels_last)
    flv = device_view(flow, name="flow", kinds=("f4",), shape=(B, 2, h, w)) if flow is not None else None
    change = np.zeros((B, 2), np.float32)
    seq = None

    def outputs(dev):
        return torch.empty((B, 2, h, w), dtype=torch.float32, device=dev), (torch.empty((B, h, w), dtype=torch.float32, device=dev) if want_occ else None)
    try:
        with on_stream(torch, ctx, frames, stream, outputs) as (stream, (out, occ)):
            ov, cv = device_view(out, writable=True, name="out_flow"), (device_view(occ, writable=True, name="out_occ") if want_occ else None)
            if normalize:
                params = type(params).from_buffer_copy(params)
                seq = sfa.Sequence(ctx, w, h, B * F)
                for b in range(B):                               # window-major: sequence frame b F + f
                    _, lay = frames_layout(fv.sub(b, 1), w, h, F, channels_last)
                    lay.window = 0
                    ctx._ck(_lib().sfa_sequence_upload_device(seq.h_, b * F, F, C.c_void_p(fv.ptr + b * fv.strides[0] * fv.itemsize), C.byref(lay)),
                            "sfa_sequence_upload_device")
                avg, std = seq.normalize()
                for k in range(3):
                    params.norm_avg[k], params.norm_std[k] = avg[k], std[k]
            b0 = 0
            for n in pair_sizes(B):
                # the statistics of normalize=True are part of a job's parameters and differ from call to call: such a job is not kept
                job = _job_for(ctx, params, w, h, n) if seq is None else sfa.Job(ctx, params, w, h, n)
                if seq is not None:
                    for b in range(n):
                        job.upload_resident(b, seq, [(b0 + b) * F + f for f in range(F)])
                else:
                    job_upload_device(job, fv.sub(b0, n), channels_last=channels_last)
                job_set_flow_device(job, flv.sub(b0, n) if flv is not None else None, 0, n)
                if raw_weights is not None:                      # after the uploads: they set the windows' weights to ones
                    job.set_raw_weights((raw_weights[0], raw_weights[1]), raw_weights[2], 0, n)
                job.run()
                job_download_device(job, ov.sub(b0, n), cv.sub(b0, n) if want_occ else None)
                change[b0:b0 + n] = job_changes(job, 0, n)
                b0 += n
                if seq is not None:
                    signal_stream(ctx, stream)
                    job.close()
    finally:                                                     # after the bracket's signal
        if seq is not None:
            seq.close()
    return out, occ, change


# ---- resident pair jobs (sfa_pair_job): the two-frame refinement -------------------------------------------------------------------------------
def pair_job_upload_device(job, frames, b0=0, channels_last=None):
    v = device_view(frames, name="frames", ndim=5)
    n, lay = frames_layout(v, job.w, job.h, 2, channels_last)
    job.ctx._ck(_lib().sfa_pair_job_upload_device(job.h_, int(b0), n, C.c_void_p(v.ptr), C.byref(lay)), "sfa_pair_job_upload_device")


def pair_job_set_flow_device(job, flow, b0=0, n=None):
    _set_flow_device(job, "sfa_pair_job_set_flow_device", "n", flow, b0, n)


def pair_job_download_device(job, out_flow, b0=0):
    _download_device(job, "sfa_pair_job_download_device", out_flow, b0)


def pair_geometry(fv, channels_last=None):
    """frames [B,2,3,H,W] or [B,2,H,W,3] as a DeviceView -> (B, h, w); SlowflowError naming `frames` for anything else (three frames, a wrong rank ...)"""
    if len(fv.shape) != 5:
        raise sfa.SlowflowError(f"frames: rank {len(fv.shape)}, shape {fv.shape}; 5 dimensions expected")
    if fv.shape[1] != 2:
        raise sfa.SlowflowError(f"frames: shape {fv.shape} holds {fv.shape[1]} frames per pair; [B,2,3,H,W] or [B,2,H,W,3] expected")
    h, w = frames_size(fv, channels_last)
    return frames_layout(fv, w, h, 2, channels_last)[0], h, w


def _pair_job_for(ctx, params, w, h, n):
    return _cached_job(ctx, "_refine_pair_jobs", (w, h, n, bytes(params) if params is not None else None), lambda: sfa.PairJob(ctx, w, h, n, params))


def refine_pairs(ctx, frames, flow0=None, params=None, *, stream=None, channels_last=None):
    """The two-frame refinement (variational.c) of B frame pairs that live on the context's GPU: frames = a torch tensor [B,2,3,H,W] or [B,2,H,W,3] (fp32,
    uint8 or uint16; any strides with a positive column stride), frame 0 = im1, frame 1 = im2; flow0 = None (zeros) or an fp32 tensor [B,2,H,W]; params =
    None (variational_params_default) or a Params2f.  Returns a new fp32 tensor [B,2,H,W] on the frames' device.  The work is ordered after what `stream`
    (default: torch.cuda.current_stream) holds at the call, and `stream` waits for it afterwards; the call only enqueues and never waits for the GPU (a
    pair job of a new shape is created first, which does).  B > 128 is split into jobs of equal or nearly equal size.  The jobs stay on the context per
    (w, h, n, params) for the next call (release_jobs(ctx) or ctx.close() frees them)."""
    import torch
    fv = device_view(frames, name="frames")
    B, h, w = pair_geometry(fv, channels_last)
    flv = device_view(flow0, name="flow0", kinds=("f4",), shape=(B, 2, h, w)) if flow0 is not None else None
    sizes = pair_sizes(B)
    by_size = {n: _pair_job_for(ctx, params, w, h, n) for n in sorted(set(sizes), reverse=True)}       # creating a job waits for the context's stream: before the bracket
    with on_stream(torch, ctx, frames, stream, lambda dev: torch.empty((B, 2, h, w), dtype=torch.float32, device=dev)) as (_, out):
        ov = device_view(out, writable=True, name="out_flow")
        b0 = 0
        for n in sizes:
            job = by_size[n]
            pair_job_upload_device(job, fv.sub(b0, n), channels_last=channels_last)
            pair_job_set_flow_device(job, flv.sub(b0, n) if flv is not None else None, 0, n)
            job.run()
            pair_job_download_device(job, ov.sub(b0, n))
            b0 += n
    return out


# ---- resident track jobs (sfa_track_job): dense_tracking's accumulation, energies and fusion -----------------------------------------------------
_LL5 = C.c_longlong * 5


def track_job_upload_flows_device(job, r, fwd, bwd, s0=0):
    src, rJ = job.params.source[r], job.params.r_Jets[r]
    fv = device_view(fwd, name="fwd", kinds=("f4",), shape=("ns", rJ, 2, src.sh, src.sw))
    bv = device_view(bwd, name="bwd", kinds=("f4",), shape=(fv.shape[0], rJ, 2, src.sh, src.sw))
    if bv.strides != fv.strides:
        raise sfa.SlowflowError(f"bwd: element strides {bv.strides} differ from fwd's {fv.strides}: the two directions share one layout")
    job.ctx._ck(_lib().sfa_track_job_upload_flows_device(job.h_, int(s0), fv.shape[0], int(r), C.c_void_p(fv.ptr), C.c_void_p(bv.ptr), _LL5(*fv.strides)),
                "sfa_track_job_upload_flows_device")


def track_job_upload_frames_device(job, frames, s0=0):
    v = device_view(frames, name="frames", kinds=("f4",), shape=("ns", job.Jets + 1, 3, job.h, job.w))
    job.ctx._ck(_lib().sfa_track_job_upload_frames_device(job.h_, int(s0), v.shape[0], C.c_void_p(v.ptr), _LL5(*v.strides)), "sfa_track_job_upload_frames_device")


def track_job_download_device(job, flow, slot=None, occ=None, stats=None, s0=0):
    ns = int(flow.shape[0])
    fv = device_view(flow, writable=True, name="flow", kinds=("f8",), shape=(ns, 2, job.gh, job.gw))
    ptrs = [C.c_void_p(device_view(a, writable=True, name=name, kinds=(kind,), shape=shape, contiguous=True).ptr) if a is not None else None
            for a, name, kind, shape in ((slot, "slot", "i4", (ns, job.gh, job.gw)), (occ, "occ", "u1", (ns, job.gh, job.gw)), (stats, "stats", "f8", (ns, 3)))]
    job.ctx._ck(_lib().sfa_track_job_download_device(job.h_, int(s0), ns, C.c_void_p(fv.ptr), _LL4(*fv.strides), *ptrs), "sfa_track_job_download_device")


def track_job_upload_occlusions_device(job, r, occ, s0=0):
    if not 0 <= r < job.K:                          # (the shape below comes from the rate's source)
        raise sfa.SlowflowError(f"sfa_track_job_upload_occlusions_device: r = {r} names none of the job's {job.K} rates")
    src, rJ = job.params.source[r], job.params.r_Jets[r]
    v = device_view(occ, name="occ", kinds=("u1", "f4"), shape=("ns", rJ, src.sh, src.sw))
    job.ctx._ck(_lib().sfa_track_job_upload_occlusions_device(job.h_, int(s0), v.shape[0], int(r), C.c_void_p(v.ptr), DTYPES[v.kind], _LL4(*v.strides)),
                "sfa_track_job_upload_occlusions_device")


# the packed outputs of a rate, in the C call's order, and their element types (the occlusion word's 64 bits also into an int64 array)
RATE_OUTPUTS = (("tracked", ("i4",)), ("energy", ("f8",)), ("occ_bits", ("u8", "i8")), ("occluded", ("u1",)))


def track_job_download_rate_device(job, r, acc=None, tracked=None, energy=None, occ_bits=None, occluded=None, s0=0):
    given = [a for a in (acc, tracked, energy, occ_bits, occluded) if a is not None]
    if not given:
        raise sfa.SlowflowError("download_rate_device: no output given")
    ns = int(given[0].shape[0])
    av = device_view(acc, writable=True, name="acc", kinds=("f8",), shape=(ns, 2, job.gh, job.gw)) if acc is not None else None
    ptrs = [C.c_void_p(device_view(a, writable=True, name=name, kinds=kinds, shape=(ns, job.gh, job.gw), contiguous=True).ptr) if a is not None else None
            for a, (name, kinds) in zip((tracked, energy, occ_bits, occluded), RATE_OUTPUTS)]
    job.ctx._ck(_lib().sfa_track_job_download_rate_device(job.h_, int(s0), ns, int(r), C.c_void_p(av.ptr) if av else None, _LL4(*av.strides) if av else None, *ptrs),
                "sfa_track_job_download_rate_device")


def track_job_download_best_device(job, best, s0=0):
    v = device_view(best, writable=True, name="best", kinds=("u1",), shape=("ns", job.gh, job.gw), contiguous=True)
    job.ctx._ck(_lib().sfa_track_job_download_best_device(job.h_, int(s0), v.shape[0], C.c_void_p(v.ptr)), "sfa_track_job_download_best_device")


def track_job_upload_fill_device(job, lab, edges, s0=0):
    ev = device_view(edges, name="edges", kinds=("f4",), shape=("ns", job.gh, job.gw))
    lv = device_view(lab, name="lab", kinds=("f4",), shape=(ev.shape[0], 3, job.gh, job.gw)) if lab is not None else None
    job.ctx._ck(_lib().sfa_track_job_upload_fill_device(job.h_, int(s0), ev.shape[0], C.c_void_p(lv.ptr) if lv else None, _LL4(*lv.strides) if lv else None,
                                                        C.c_void_p(ev.ptr), _LL3(*ev.strides)), "sfa_track_job_upload_fill_device")


def track_job_upload_fill_reference_device(job, rgb, edges, norm=1.0, s0=0):
    ev = device_view(edges, name="edges", kinds=("f4",), shape=("ns", job.gh, job.gw))
    rv = device_view(rgb, name="rgb", kinds=("f4",), shape=(ev.shape[0], 3, job.h, job.w)) if rgb is not None else None
    job.ctx._ck(_lib().sfa_track_job_upload_fill_reference_device(job.h_, int(s0), ev.shape[0], C.c_void_p(rv.ptr) if rv else None, _LL4(*rv.strides) if rv else None,
                                                                  float(norm), C.c_void_p(ev.ptr), _LL3(*ev.strides)), "sfa_track_job_upload_fill_reference_device")


def track(ctx, params, flows, frames, *, occlusions=None, rates=False, stream=None, fill=None, lab=None, edges=None):
    """dense_tracking's accumulation, energies and fusion of ns start_jets whose inputs live on the context's GPU.  params: sfa.track_params(...) with
    do_fuse 1, n >= ns; flows = [(fwd_r, bwd_r), ...], one pair of fp32 tensors [ns, r_Jets[r], 2, sh, sw] per rate; frames = an fp32 tensor
    [ns, Jets + 1, 3, h, w] of normalised frames; any strides with a positive column stride.  occlusions: with params.use_occlusions one tensor
    [ns, r_Jets[r], sh, sw] per rate, uint8 (the raw occlusion images) or fp32 (the labels refine() returns as occ, turned into the driver's grey image);
    refused without it.  Returns (flow [ns,2,gh,gw] float64, slot [ns,gh,gw] int32, occ [ns,gh,gw] uint8, stats [ns,3] float64: energy, bound, iterations)
    as new tensors on that device; with rates=True a fifth value, dict(rate=[one dict per rate of new tensors acc float64 [ns,2,gh,gw] (the last
    accumulated step), tracked int32, energy float64 (+Inf: no hypothesis), occ_bits uint64, occluded uint8 [ns,gh,gw]], best=uint8 [ns,gh,gw]): what
    TrackJob.download_rate and download_best give.  The work is ordered after what `stream` (default: torch.cuda.current_stream) holds at the call, and `stream` waits for it afterwards; the call only enqueues (a job of new
    parameters is created first, which waits).  The job stays on the context for the next call (ctx.close() frees it).
    fill: a sfa.track_fill_params(...) makes it a job that fills in (at most 8 rates): lab = an fp32 tensor [ns, 3, gh, gw] of the Lab images at the
    grid's size (None where fill.epic.saliency_th == 0) and edges = an fp32 tensor [ns, gh, gw] of edge cost maps; slot then counts 2 K slots, slot
    2 r + 1 the fill-in of rate r, and the call waits where the fill-in reads its counts."""
    import torch
    if len(flows) != params.K:
        raise sfa.SlowflowError(f"flows: {len(flows)} (fwd, bwd) pairs for {params.K} rates")
    if params.use_occlusions and occlusions is None:
        raise sfa.SlowflowError("occlusions: None, but params.use_occlusions is set: one tensor of occlusion images per rate")
    if occlusions is not None and not params.use_occlusions:
        raise sfa.SlowflowError("occlusions: given, but params.use_occlusions is 0: the job would not read them")
    if occlusions is not None and len(occlusions) != params.K:
        raise sfa.SlowflowError(f"occlusions: {len(occlusions)} tensors for {params.K} rates")
    fv = device_view(frames, name="frames", kinds=("f4",), shape=("ns", params.Jets + 1, 3, params.h, params.w))   # every view is checked before a job is created or anything uploaded
    ns = fv.shape[0]
    if not 1 <= ns <= params.n:
        raise sfa.SlowflowError(f"frames: {ns} start_jets, the parameters' capacity n is {params.n}")
    for r, (fwd, bwd) in enumerate(flows):
        src = params.source[r]
        for a, nm in ((fwd, "flows[%d] fwd" % r), (bwd, "flows[%d] bwd" % r)):
            device_view(a, name=nm, kinds=("f4",), shape=(ns, params.r_Jets[r], 2, src.sh, src.sw))
        if occlusions is not None:
            device_view(occlusions[r], name="occlusions[%d]" % r, kinds=("u1", "f4"), shape=(ns, params.r_Jets[r], src.sh, src.sw))
    if fill is None and (lab is not None or edges is not None):
        raise sfa.SlowflowError("lab / edges: given without fill: the job would not read them")
    if fill is not None and edges is None:
        raise sfa.SlowflowError("edges: None, but fill is given: one edge cost map per start_jet")
    job = _cached_job(ctx, "_track_jobs", bytes(params) + (bytes(fill) if fill is not None else b""), lambda: sfa.TrackJob(ctx, params, fill))     # creating a job waits for the context's stream: before the bracket
    g = (ns, job.gh, job.gw)
    def outputs(dev):
        out = (torch.empty((ns, 2, job.gh, job.gw), dtype=torch.float64, device=dev), torch.empty(g, dtype=torch.int32, device=dev),
               torch.empty(g, dtype=torch.uint8, device=dev), torch.empty((ns, 3), dtype=torch.float64, device=dev))
        if not rates:
            return out
        rate = [dict(acc=torch.empty((ns, 2, job.gh, job.gw), dtype=torch.float64, device=dev), tracked=torch.empty(g, dtype=torch.int32, device=dev),
                     energy=torch.empty(g, dtype=torch.float64, device=dev), occ_bits=torch.empty(g, dtype=torch.uint64, device=dev),
                     occluded=torch.empty(g, dtype=torch.uint8, device=dev)) for _ in range(params.K)]
        return out + (dict(rate=rate, best=torch.empty(g, dtype=torch.uint8, device=dev)),)
    with on_stream(torch, ctx, frames, stream, outputs) as (_, out):
        for r, (fwd, bwd) in enumerate(flows):
            track_job_upload_flows_device(job, r, fwd, bwd)
            if occlusions is not None:
                track_job_upload_occlusions_device(job, r, occlusions[r])
        track_job_upload_frames_device(job, frames)
        if fill is not None:
            track_job_upload_fill_device(job, lab, edges)
        job.run(ns)
        track_job_download_device(job, *out[:4])
        if rates:
            for r, d in enumerate(out[4]["rate"]):
                track_job_download_rate_device(job, r, d["acc"], d["tracked"], d["energy"], d["occ_bits"], d["occluded"])
            track_job_download_best_device(job, out[4]["best"])
    return out


# ---- adaptiveFR's frame-rate decision (sfa_flow_magnitude_quantiles_device): quantile and maximum of the flow magnitude, per group ------------------
def flow_quantiles(ctx, flow, q=0.99, scale=1.0, counts=None, *, stream=None, out=None):
    """adaptiveFR's quantile and maximum of the flow magnitude (adaptiveFR.cpp:644-668) for G groups of flow fields that live on the context's GPU: flow =
    an fp32 tensor [G,n,2,h,w], or [n,2,h,w] as one group, with any strides whose row and column strides are positive (a permuted channels-last
    [G,n,h,w,2], padded rows and slices are read in place); every value is multiplied by `scale` first; counts = None (all n fields) or G numbers, group
    g then takes its first counts[g] fields.  Returns a float64 tensor [G,2] on the flow's device, row g = (quantile, maximum) of group g with the bits
    Context.flow_magnitude_quantile gives for the same values; out = such a tensor (contiguous) to write into instead of a new one.  The work is ordered
    after what `stream` (default: torch.cuda.current_stream) holds at the call, and `stream` waits for it afterwards; the call only enqueues and never waits
    for the GPU (a call that needs more scratch than the context holds replaces it first, which does)."""
    import torch
    v = device_view(flow, name="flow", kinds=("f4",))
    if len(v.shape) == 4:
        v = DeviceView(v.ptr, v.dtype, v.itemsize, (1,) + v.shape, (0,) + v.strides, v.owner)
    v = device_view(v, name="flow", shape=("G", "n", 2, "h", "w"))
    G, n, _, h, w = v.shape
    ca = None
    if counts is not None:
        counts = [int(c) for c in counts]
        if len(counts) != G:
            raise sfa.SlowflowError(f"counts: {len(counts)} entries for {G} groups")
        ca = (C.c_int * G)(*counts)
    s = v.strides
    def out_view(o):
        return device_view(o, writable=True, name="out", kinds=("f8",), shape=(G, 2), contiguous=True)
    given = out
    if given is not None:
        out_view(given)                                          # a refusal touches neither stream
    with on_stream(torch, ctx, flow, stream, lambda dev: torch.empty((G, 2), dtype=torch.float64, device=dev) if given is None else given) as (_, out):
        op = out_view(out).ptr
        ctx._ck(_lib().sfa_flow_magnitude_quantiles_device(ctx.h, G, n, ca, C.c_void_p(v.ptr), C.c_void_p(v.ptr + s[2] * v.itemsize), _LL4(s[0], s[1], s[3], s[4]),
                                                           w, h, float(scale), float(q), C.c_void_p(op)), "sfa_flow_magnitude_quantiles_device")
    return out
