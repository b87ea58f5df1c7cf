"""Resident pair jobs (include/slowflow_amd.h: sfa_pair_job_*; slowflow_amd.PairJob, slowflow_amd/device.py: refine_pairs): the two-frame refinement of
pairs that stay on the GPU, with the derivatives and the data term formed in one kernel (k_data_2f_fused).

Every comparison is IEEE `==` on the bit patterns.  The reference is Context.variational_2frame on each pair alone: the host-plane path that the pin tests
(tests/golden/ref_two_frame.npz) hold bit for bit to the compiled reference, and that this feature leaves as it was."""
import ctypes as C

import numpy as np
import pytest

import slowflow_amd as sfa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


def params(**kw):
    p = sfa.Params2f()
    sfa.lib().sfa_params_2frame_default(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def box5(a):
    """5 x 5 box filter over the last two axes (valid part)"""
    h, w = a.shape[-2] - 4, a.shape[-1] - 4
    return sum(a[..., dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)) / 25.0


def make_pairs(w, h, B, seed):
    """B different pairs: frames [B,2,3,h,w] fp32 holding 8-bit pixel values (a band-limited texture and its translate by 1 .. 3 pixels), and a start
    flow [B,2,h,w] near the translation"""
    rng = np.random.default_rng(seed)
    m = 4
    big = box5(box5(rng.uniform(0, 1, size=(B, 3, h + 2 * m + 8, w + 2 * m + 8))))
    lo, hi = big.min(axis=(2, 3), keepdims=True), big.max(axis=(2, 3), keepdims=True)
    big = np.round((big - lo) / (hi - lo) * 255.0)
    frames = np.zeros((B, 2, 3, h, w), np.float32)
    flow = np.zeros((B, 2, h, w), np.float32)
    for b in range(B):
        dx, dy = 1 + b % 3, 1 + (b // 3) % 2
        frames[b, 0] = big[b, :, m:m + h, m:m + w]
        frames[b, 1] = big[b, :, m - dy:m - dy + h, m - dx:m - dx + w]
        flow[b, 0] = dx + rng.uniform(-0.5, 0.5, size=(h, w))
        flow[b, 1] = dy + rng.uniform(-0.5, 0.5, size=(h, w))
    return frames, flow


def padded(a, stride):
    """(..., h, w) -> (..., h, stride) fp32 C-contiguous, padding NaN: columns >= w are never read"""
    out = np.full(a.shape[:-1] + (stride,), np.nan, np.float32)
    out[..., :a.shape[-1]] = a
    return out


def single(ctx, frames, flow, p=None, stride=None):
    """the reference: Context.variational_2frame on one pair alone.  frames [2,3,h,w], flow [2,h,w] -> [2,h,w]"""
    h, w = frames.shape[-2:]
    stride = sfa.stride_of(w) if stride is None else stride
    fl, fr = padded(flow, stride), padded(frames, stride)
    ctx.variational_2frame(fl[0], fl[1], fr[0], fr[1], w, p)
    return np.ascontiguousarray(fl[:, :, :w])


def upload(job, frames, flow, slots=None, stride=None):
    stride = sfa.stride_of(job.w) if stride is None else stride
    for b in (range(frames.shape[0]) if slots is None else slots):
        fl, fr = padded(flow[b], stride), padded(frames[b], stride)
        job.upload(b, fl[0], fl[1], fr[0], fr[1])


def download(job, slots=None, stride=None):
    return np.stack([np.stack(job.download(b, stride))[:, :, :job.w] for b in (range(job.n) if slots is None else slots)])


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def job_result(ctx, frames, flow, p=None, stride=None):
    B, h, w = frames.shape[0], frames.shape[-2], frames.shape[-1]
    job = sfa.PairJob(ctx, w, h, B, p)
    try:
        upload(job, frames, flow, stride=stride)
        job.run()
        return download(job, stride=None if stride is None else stride + 4)
    finally:
        job.close()


# ---- 1. the tile boundaries of the 64 x 16 / halo-4 kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,extra", [(2, 5, 0), (7, 5, 4), (64, 16, 0), (65, 17, 0), (63, 15, 0), (131, 37, 8), (253, 131, 0)])
def test_tile_boundaries(ctx, w, h, extra):
    """B = 3, so that a pair index other than 0 always takes part; `extra`: a host stride that is not the width rounded up"""
    frames, flow = make_pairs(w, h, 3, 100 * w + h)
    got = job_result(ctx, frames, flow, stride=sfa.stride_of(w) + extra if extra else None)
    for b in range(3):
        assert same(got[b], single(ctx, frames[b], flow[b])), (w, h, b)


# ---- 2. the batch index ---------------------------------------------------------------------------------------------------------------------
def test_128_pairs_each_equal_their_single_call(ctx):
    w, h, B = 70, 21, 128
    frames, flow = make_pairs(w, h, B, 2)
    assert len({frames[b].tobytes() for b in range(B)}) == B
    got = job_result(ctx, frames, flow)
    for b in (0, 63, 64, 127):
        assert same(got[b], single(ctx, frames[b], flow[b])), b


# ---- 3. parameters --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(delta=0.5), dict(niter_inner=2), dict(niter_outer=1), dict(niter_solver=7)],
                         ids=["defaults", "delta", "inner2", "outer1", "solver7"])
def test_parameters(ctx, kw):
    """delta = 0.5 enters the colour-constancy branch the default delta = 0 skips; 7 sweeps: a count no chain shape divides, the task-kernel fallback"""
    w, h = 65, 17
    frames, flow = make_pairs(w, h, 3, 3)
    p = params(**kw)
    got = job_result(ctx, frames, flow, p)
    for b in range(3):
        assert same(got[b], single(ctx, frames[b], flow[b], p)), (kw, b)


# ---- 4. warps that leave the image ----------------------------------------------------------------------------------------------------------
def test_out_of_image_warps(ctx):
    """a start flow of +-(w + 3) on part of the field: pixels with mask == 0 and clamped taps; 1e12 on a few pixels: memory-safe, and still `==`"""
    w, h = 131, 37
    frames, flow = make_pairs(w, h, 3, 4)
    flow[0, 0, :, :40] = w + 3
    flow[0, 1, 20:, :] = -(w + 3)
    flow[1, 0, 10:20, 60:] = -(w + 3)
    flow[2, 0, 5, 7] = 1e12; flow[2, 1, 5, 7] = -1e12; flow[2, 1, 30, 100] = 1e12; flow[2, 0, 36, 130] = 1e12
    got = job_result(ctx, frames, flow)
    for b in range(3):
        assert same(got[b], single(ctx, frames[b], flow[b])), b


# ---- 5. the fused kernel against the stored stack -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(65, 17), (131, 37)])
def test_fused_against_unfused(ctx, switches, w, h):
    """the same job with SFA_PAIR_UNFUSED = 1 (launch_deriv_stack + k_data_2f on a stack allocated for it) and 0 (k_data_2f_fused): the five planes of
    the linear system after one outer iteration, and the flow; then the flow of a default run"""
    frames, flow = make_pairs(w, h, 3, 5)
    flow[1, 0, :, :9] = -(w + 3)                                   # masked pixels in one of the pairs
    for p in (params(niter_outer=1, delta=0.5), None):
        job = sfa.PairJob(ctx, w, h, 3, p)
        try:
            res = {}
            for unfused in (1, 0):
                switches.set("SFA_PAIR_UNFUSED", unfused)
                upload(job, frames, flow)
                job.run()
                res[unfused] = (download(job), [job.download_system(b) for b in range(3)])
            assert same(res[0][0], res[1][0]), "flow"
            if p is not None:
                for b in range(3):
                    for name, x, y in zip(("a11", "a12", "a22", "b1", "b2"), res[0][1][b], res[1][1][b]):
                        assert same(x[:, :w], y[:, :w]), (name, b)
                    assert np.abs(res[0][1][b][0][:, :w]).max() > 0                    # (the hook returns the system, not the zeros of a fresh job)
        finally:
            job.close()


# ---- 6. reuse -------------------------------------------------------------------------------------------------------------------------------
def test_reuse_across_runs_and_uploads(ctx):
    w, h, B = 70, 21, 4
    frames, flow = make_pairs(w, h, B, 6)
    other, oflow = make_pairs(w, h, 2, 7)
    job = sfa.PairJob(ctx, w, h, B)
    try:
        upload(job, frames, flow)
        job.run()
        first = download(job)
        upload(job, frames, flow)                                  # the same data once more: the same bits
        job.run()
        assert same(download(job), first)
        upload(job, other, oflow, slots=(0, 1))                    # half the slots anew; slots 2, 3 keep their result and are refined further
        job.run()
        second = download(job)
        for b in range(2):
            assert same(second[b], single(ctx, other[b], oflow[b])), b
        for b in (2, 3):
            assert same(first[b], single(ctx, frames[b], flow[b])), b
            assert same(second[b], single(ctx, frames[b], first[b])), b
    finally:
        job.close()


def test_host_calls_between_the_runs_of_a_live_job(ctx):
    """The host calls build and free a pair job of their own on the caller's context: a single call and a batch of other sizes between two runs of a live
    job leave that job's planes, parameters and solver workspace alone.  The second run has nothing uploaded before it, so it refines the first run's
    result further (run() updates the resident flow in place, as test_reuse_across_runs_and_uploads holds): its outcome is compared with the single call
    on (frames, first result), not with the first result itself."""
    w, h, B = 65, 17, 3
    frames, flow = make_pairs(w, h, B, 12)
    small, sflow = make_pairs(7, 5, 1, 13)
    wide, wflow = make_pairs(131, 37, 2, 14)
    job = sfa.PairJob(ctx, w, h, B)
    try:
        upload(job, frames, flow)
        job.run()
        first = download(job)
        single(ctx, small[0], sflow[0])
        st = sfa.stride_of(131)
        fl, fr = padded(wflow, st), padded(wide, st)
        ctx.variational_2frame_batch([fl[i, 0] for i in range(2)], [fl[i, 1] for i in range(2)], [fr[i, 0] for i in range(2)], [fr[i, 1] for i in range(2)], 131)
        job.run()
        second = download(job)
        for b in range(B):
            assert same(first[b], single(ctx, frames[b], flow[b])), b
            assert same(second[b], single(ctx, frames[b], first[b])), b
        for i in range(2):
            assert same(fl[i, :, :, :131], single(ctx, wide[i], wflow[i])), i
    finally:
        job.close()


# ---- 7. the device seam -------------------------------------------------------------------------------------------------------------------------
torch = None


@pytest.fixture(scope="module")
def dev():
    global torch
    torch = pytest.importorskip("torch")
    return torch.device("cuda", 0)


def seam_run(ctx, job, frames_t, flow_t, channels_last=None):
    """upload_device / set_flow_device / run / download_device on torch's default stream -> [B,2,h,w] numpy"""
    B = job.n
    ctx.wait_stream()
    job.upload_device(frames_t, channels_last=channels_last)
    job.set_flow_device(flow_t, 0, B)
    job.run()
    out = torch.full((B, 2, job.h, job.w), -7.0, device="cuda:0")
    ctx.wait_stream()
    job.download_device(out)
    ctx.signal_stream()
    ctx.sync()
    return out.cpu().numpy()


class U16Frames:
    """uint16 frames through int16 storage that holds the bit patterns (torch's own uint16 support varies with its version)"""

    def __init__(self, raw):
        self.raw, self.shape, self.device = raw, tuple(raw.shape), raw.device

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": "<u2", "data": (self.raw.data_ptr(), False), "version": 3, "strides": tuple(2 * s for s in self.raw.stride())}


def test_device_seam_equals_the_host_upload(ctx, dev):
    w, h, B = 131, 37, 3
    frames, flow = make_pairs(w, h, B, 8)                          # 8-bit pixel values: exact in uint8, uint16 and fp32
    job = sfa.PairJob(ctx, w, h, B)
    try:
        upload(job, frames, flow)
        job.run()
        host = download(job)
        upload(job, frames, np.zeros_like(flow))
        job.run()
        host0 = download(job)
        assert not same(host, host0)
        ft, fl = torch.from_numpy(frames).to(dev), torch.from_numpy(flow).to(dev)
        assert same(seam_run(ctx, job, ft, fl), host), "planar fp32"
        u8 = ft.to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous()
        assert u8.shape == (B, 2, h, w, 3)
        assert same(seam_run(ctx, job, u8, fl), host), "interleaved uint8"
        raw = torch.from_numpy(frames.astype(np.uint16).view(np.int16)).to(dev)
        assert same(seam_run(ctx, job, U16Frames(raw), fl), host), "planar uint16"
        big = torch.full((B, 2, 3, h + 9, w + 14), float("nan"), device=dev)
        crop = big[..., 3:3 + h, 5:5 + w]
        crop.copy_(ft)
        assert not crop.is_contiguous()
        assert same(seam_run(ctx, job, crop, fl), host), "a crop of a larger tensor"
        assert same(seam_run(ctx, job, ft, None), host0), "flow None"
        assert same(seam_run(ctx, job, ft, torch.zeros_like(fl)), host0), "an explicit zero field"
        # download into a [B,2,H,W] slice of a larger tensor: the surroundings keep their sentinel
        ctx.wait_stream()
        job.upload_device(ft)
        job.set_flow_device(fl)
        job.run()
        for x0, wide in ((5, w + 11), (8, w + 17)):                # the element kernel; the 128-bit kernel
            sent = torch.full((B, 4, h + 6, wide), -777.0, device=dev)
            dst = sent[:, 1:3, 2:2 + h, x0:x0 + w]
            ctx.wait_stream()
            job.download_device(dst)
            ctx.sync()
            got = sent.cpu().numpy()
            assert same(got[:, 1:3, 2:2 + h, x0:x0 + w], host)
            outside = np.ones(got.shape, bool)
            outside[:, 1:3, 2:2 + h, x0:x0 + w] = False
            assert (got[outside] == -777.0).all(), "bytes outside the slice were written"
        part = torch.zeros((2, 2, h, w), device=dev)               # pairs b0 .. into a destination of their own
        ctx.wait_stream()
        job.download_device(part, b0=1)
        ctx.sync()
        assert same(part.cpu().numpy(), host[1:3])
    finally:
        job.close()


# ---- 8. asynchrony ------------------------------------------------------------------------------------------------------------------------------
def test_refine_pairs_on_a_side_stream_without_synchronisation(ctx, dev):
    """a torch kernel writes the frames right before refine_pairs() and a torch op reads the result right after, all on one non-default stream and with
    no synchronisation in between; the outcome equals the single calls"""
    from slowflow_amd import device
    w, h, B = 253, 131, 4
    frames, flow = make_pairs(w, h, B, 9)
    want = np.stack([single(ctx, frames[b], flow[b]) for b in range(B)])
    px, fl = torch.from_numpy(frames).to(dev), torch.from_numpy(flow).to(dev)
    device.refine_pairs(ctx, px, fl)                              # the job of this shape exists from here on: creating one waits, refining does not
    side = torch.cuda.Stream(device=dev)
    buf = torch.zeros_like(px)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        buf.copy_(px * 2.0)
        buf.mul_(0.5)                                             # the producer: the last kernel before refine_pairs writes the frames
        got = device.refine_pairs(ctx, buf, fl)
        total = got.double().sum(dim=(2, 3))                      # the consumer, on the same stream
        buf.zero_()                                               # and a reuse of the input, ordered after the library's reads
    side.synchronize()
    assert got.shape == (B, 2, h, w) and got.dtype == torch.float32
    assert same(got.cpu().numpy(), want)
    assert np.array_equal(total.cpu().numpy(), torch.from_numpy(want).to(dev).double().sum(dim=(2, 3)).cpu().numpy())      # the same reduction on the expected field
    device.release_jobs(ctx)
    assert "_refine_pair_jobs" not in ctx.__dict__


def test_refine_pairs_splits_a_large_batch(ctx, dev):
    from slowflow_amd import device
    w, h, B = 70, 21, 130
    frames, flow = make_pairs(w, h, B, 10)
    p = params(niter_outer=2)
    px, fl = torch.from_numpy(frames).to(dev), torch.from_numpy(flow).to(dev)
    got = device.refine_pairs(ctx, px, fl, p)
    torch.cuda.synchronize()
    assert [j.n for j in ctx.__dict__["_refine_pair_jobs"].values()] == [65]          # two jobs of 65 pairs: one shape, created once
    halves = [device.refine_pairs(ctx, px[b0:b0 + 65], fl[b0:b0 + 65], p) for b0 in (0, 65)]
    torch.cuda.synchronize()
    assert same(got.cpu().numpy(), torch.cat(halves).cpu().numpy())
    for b in (0, 64, 65, 129):
        assert same(got[b].cpu().numpy(), single(ctx, frames[b], flow[b], p)), b
    device.release_jobs(ctx)


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------------
class HostArray:
    """a host array that claims to be a device array"""

    def __init__(self, a):
        self.a = a
        self.__cuda_array_interface__ = {"shape": a.shape, "typestr": "<f4", "data": (a.ctypes.data, False), "version": 3, "strides": None}


def test_refusals_name_the_argument_and_leave_the_job_alone(ctx, dev):
    from slowflow_amd import device
    w, h, B = 65, 17, 2
    frames, flow = make_pairs(w, h, B, 11)
    want = np.stack([single(ctx, frames[b], flow[b]) for b in range(B)])
    ft = torch.from_numpy(frames).to(dev)
    job = sfa.PairJob(ctx, w, h, B)
    try:
        upload(job, frames, flow)
        torch.cuda.synchronize()

        def refused(call, *words):
            with pytest.raises(sfa.SlowflowError) as e:
                call()
            assert all(word in str(e.value) for word in words), str(e.value)

        host = np.zeros((B, 2, 3, h, w), np.float32)
        refused(lambda: job.upload_device(host), "frames", "__cuda_array_interface__")
        refused(lambda: job.upload_device(HostArray(host)), "sfa_pair_job_upload_device", "frames_dev", "not device memory")
        refused(lambda: job.set_flow_device(HostArray(np.zeros((B, 2, h, w), np.float32))), "flow_dev", "not device memory")
        refused(lambda: job.download_device(HostArray(np.zeros((B, 2, h, w), np.float32))), "flow_dev", "not device memory")
        refused(lambda: job.upload_device(ft[0]), "frames", "rank 4")                                       # wrong rank
        refused(lambda: device.refine_pairs(ctx, ft[0]), "frames", "rank 4")
        three = torch.zeros((B, 3, 3, h, w), device=dev)
        refused(lambda: job.upload_device(three), "frames", "neither")                                      # three frames
        refused(lambda: device.refine_pairs(ctx, three), "frames", "3 frames")
        refused(lambda: job.upload_device(ft.half()), "frames", "<f2")
        refused(lambda: device.refine_pairs(ctx, ft, torch.zeros((B, 2, h, w), device=dev).half()), "flow0", "<f2")
        refused(lambda: job.upload_device(ft, b0=1), "b0 = 1", "n = 2", "batch of 2")
        refused(lambda: job.set_flow_device(None, b0=1, n=2), "b0 = 1", "batch of 2")
        refused(lambda: job.download_device(torch.zeros((B, 2, h, w), device=dev), b0=1), "b0 = 1", "batch of 2")
        refused(lambda: sfa.PairJob(ctx, w, h, 129), "sfa_pair_job_create", "n out of range")
        refused(lambda: sfa.PairJob(ctx, w, 4, 1), "sfa_pair_job_create", "h >= 5")
        refused(lambda: sfa.PairJob(ctx, 1, h, 1), "sfa_pair_job_create", "w >= 2")
        refused(lambda: sfa.PairJob(ctx, 64 * 4097, 5, 128), "sfa_pair_job_create", "kRedDoubles")
        one = torch.zeros((1, 2, h, w), device=dev)
        refused(lambda: job.download_device(one.expand(B, 2, h, w)), "flow_dev", "overlap")                 # both pairs into one
        refused(lambda: job.download_device(torch.zeros((B, 1, h, w), device=dev).expand(B, 2, h, w)), "overlap")   # u onto v
        L = sfa.lib()
        st = sfa.stride_of(w)
        pl = np.zeros((3, h, st), np.float32)
        assert L.sfa_pair_job_upload(job.h_, 2, sfa.fptr(pl[0]), sfa.fptr(pl[0]), st, sfa.fptr(pl), sfa.fptr(pl)) == -1 and "b outside" in L.sfa_last_error(ctx.h).decode()
        assert L.sfa_pair_job_upload(job.h_, 0, sfa.fptr(pl[0]), None, st, sfa.fptr(pl), sfa.fptr(pl)) == -1 and "null plane" in L.sfa_last_error(ctx.h).decode()
        assert L.sfa_pair_job_download(job.h_, -1, sfa.fptr(pl[0]), sfa.fptr(pl[1]), st) == -1 and "b outside" in L.sfa_last_error(ctx.h).decode()
        # nothing was launched and nothing was changed: the job still holds its upload
        job.run()
        assert same(download(job), want)
    finally:
        job.close()
        device.release_jobs(ctx)
