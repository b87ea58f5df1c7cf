"""The device seam (include/slowflow_amd.h: sfa_job_upload_device, sfa_job_set_flow_device, sfa_job_download_device, sfa_sequence_upload_device,
sfa_ctx_wait_stream / sfa_ctx_signal_stream; slowflow_amd/device.py) on torch tensors that live on the GPU.  The new kernels only convert and move, so the
condition throughout is bit identity with the host path (Job.upload / run / download on the numpy copies of the same data): `==` on every valid pixel of
the flow and the occlusion labels, and on the change norms."""
import ctypes as C

import numpy as np
import pytest

import slowflow_amd as sfa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def config2_params(S=2, occ=False, layers=5):
    """BASELINE config 2's schedule (5 levels, 5 outer x 1 inner x 30 sweeps, thresholds off: fixed work); with occlusion reasoning two alternations, so that
    the discrete step runs once; S = 3 with cfgs/slow_flow.cfg's rho 1/1, omega 0/2"""
    p = sfa.default_params()
    p.S = S; p.layers = layers; p.niter_alter = 2 if occ else 1; p.niter_outer = 5; p.niter_inner = 1; p.niter_solver = 30
    p.thres_outer = 0; p.thres_inner = 0; p.occlusion_reasoning = int(occ); p.hbit = 0
    for i in range(S - 1):
        p.rho[i] = 1
        p.omega[i] = (0, 2)[i] if i < 2 else 1
    for k in range(3):
        p.norm_avg[k] = 127.0; p.norm_std[k] = 0.2
    return p


def pixels(B, F, h, w, dev, seed):
    """8-bit pixel values [B,F,3,h,w] (fp32): per window a band-limited texture, frame f the crop shifted by (2 f, f)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    m = 2 * F
    base = torch.rand((B, 3, h + 2 * m, w + 2 * m), generator=g, device=dev)
    for _ in range(2):
        base = torch.nn.functional.avg_pool2d(base, 5, 1, 2)
    lo, hi = base.amin(dim=(2, 3), keepdim=True), base.amax(dim=(2, 3), keepdim=True)
    base = torch.round((base - lo) / (hi - lo) * 255.0)
    return torch.stack([base[:, :, m - f:m - f + h, m - 2 * f:m - 2 * f + w] for f in range(F)], dim=1).contiguous()


def normalized(px):
    return ((px - 127.0) / 0.2).contiguous()


def start_flow(B, h, w, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    f = torch.rand((B, 2, h // 8 + 2, w // 8 + 2), generator=g, device=dev)
    f = torch.nn.functional.interpolate(f, size=(h, w), mode="bilinear", align_corners=False)
    return (f + torch.tensor([1.5, 0.5], device=dev).view(1, 2, 1, 1)).contiguous()


def host_planes(a, w):
    """(..., h, w) numpy -> (..., h, stride_of(w)) fp32, padding zero"""
    out = np.zeros(a.shape[:-1] + (sfa.stride_of(w),), np.float32)
    out[..., :w] = a
    return out


def host_run(job, frames_np, flow_np, w, want_occ):
    """the host path on `job`: frames_np [B,F,3,h,w] fp32, flow_np [B,2,h,w] or None -> flow [B,2,h,w], occ [B,h,w] or None, change [B,2]"""
    B, F = frames_np.shape[:2]
    for b in range(B):
        fr = [host_planes(frames_np[b, f], w) for f in range(F)]
        if flow_np is None:
            job.upload(b, fr)
        else:
            fl = host_planes(flow_np[b], w)
            job.upload(b, fr, fl[0], fl[1])
    job.run()
    flow = np.zeros((B, 2) + frames_np.shape[3:], np.float32)
    occ = np.zeros((B,) + frames_np.shape[3:], np.float32) if want_occ else None
    ch = np.zeros((B, 2), np.float32)
    for b in range(B):
        wx, wy, c = job.download(b)
        flow[b, 0], flow[b, 1], ch[b] = wx[:, :w], wy[:, :w], c
        if want_occ:
            occ[b] = job.download_occlusions(b)[:, :w]
    return flow, occ, ch


def device_run(ctx, job, frames, flow, want_occ, channels_last=None):
    """the device path on `job` from torch tensors on torch's default stream, ordered with wait_stream / signal_stream"""
    B = frames.shape[0]
    h, w = job.h, job.w
    ctx.wait_stream()                                             # torch's default stream (the null stream) produced the inputs
    job.upload_device(frames, channels_last=channels_last)
    job.set_flow_device(flow, 0, B)
    job.run()
    out = torch.full((B, 2, h, w), -7.0, device=frames.device)
    occ = torch.full((B, h, w), -7.0, device=frames.device) if want_occ else None
    ctx.wait_stream()                                             # ... and fills the outputs: the download is ordered after the fill
    job.download_device(out, occ)
    ctx.signal_stream()
    ctx.sync()
    return out.cpu().numpy(), occ.cpu().numpy() if want_occ else None, job.changes()


def assert_same(a, b, what):
    for x, y, name in zip(a, b, ("flow", "occlusions", "change norms")):
        if x is None and y is None:
            continue
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{what}: {name} differ in {np.count_nonzero(x != y)} values"


# ---- 1. equal to the host path -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 128])
@pytest.mark.parametrize("occ", [False, True])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("w,h", [(1024, 436), (253, 131)])
def test_equal_to_the_host_path(ctx, dev, w, h, S, occ, B):
    """config-2 parameters at 1024 x 436 and at an odd size; upload_device + set_flow_device against Job.upload of the numpy copies, on the same job"""
    F = 2 * S - 1
    D = min(B, 4)                                                 # distinct windows; a larger batch repeats them (window b holds window b % D)
    fr = normalized(pixels(D, F, h, w, dev, seed=w + S))
    fl = start_flow(D, h, w, dev, seed=h + S)
    idx = torch.arange(B, device=dev) % D
    frames, flow = fr[idx].contiguous(), fl[idx].contiguous()
    job = sfa.Job(ctx, config2_params(S, occ), w, h, B)
    try:
        got = device_run(ctx, job, frames, flow, occ)
        del frames, flow
        want = host_run(job, fr.cpu().numpy()[np.arange(B) % D], fl.cpu().numpy()[np.arange(B) % D], w, occ)
    finally:
        job.close()
    assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 0.5          # (a refined flow, not the -7 the outputs were filled with)
    assert_same(got, want, f"{w}x{h} S={S} occ={occ} B={B}")


# ---- 2. layouts ----------------------------------------------------------------------------------------------------------------------------
def small_job(ctx, w, h, B, S=2, occ=False):
    return sfa.Job(ctx, config2_params(S, occ, layers=3), w, h, B)


def test_interleaved_u8_and_planar_u16(ctx, dev):
    """[B,F,H,W,3] uint8 and [B,F,3,H,W] uint16 equal the host path fed the astype(float32) planes ((float) of the element, no scaling)"""
    w, h, B, F = 253, 131, 3, 3
    px = pixels(B, F, h, w, dev, seed=1)                          # 0 .. 255
    job = small_job(ctx, w, h, B)
    try:
        u8 = px.to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous()
        assert u8.shape == (B, F, h, w, 3)
        got8 = device_run(ctx, job, u8, None, False)
        want8 = host_run(job, px.cpu().numpy().astype(np.uint8).astype(np.float32), None, w, False)
        assert_same(got8, want8, "interleaved uint8")
        # uint16 through a hand-made view of int16 storage holding the uint16 bit patterns (torch's own uint16 support varies with its version)
        from slowflow_amd import device
        v16 = (px.cpu().numpy() * 257.0).astype(np.uint16)        # 0 .. 65535
        raw = torch.from_numpy(v16.view(np.int16)).to(dev)
        view = device.DeviceView(raw.data_ptr(), device.DTYPES["u2"], 2, raw.shape, raw.stride(), raw)
        got16 = device_run(ctx, job, view_as_frames(view, raw), None, False)
        want16 = host_run(job, v16.astype(np.float32), None, w, False)
        assert_same(got16, want16, "planar uint16")
        assert not np.array_equal(got8[0], got16[0])
    finally:
        job.close()


class view_as_frames:
    """a DeviceView that device_run can pass on (it needs .shape and .device of the frames)"""

    def __init__(self, view, owner):
        self.view, self.shape, self.device = view, tuple(owner.shape), owner.device

    @property
    def __cuda_array_interface__(self):
        v = self.view
        return {"shape": v.shape, "typestr": "<u2", "data": (v.ptr, False), "version": 3, "strides": tuple(s * v.itemsize for s in v.strides)}


def test_cropped_view_and_shared_frames(ctx, dev):
    """a crop of a larger tensor (not contiguous, rows not 16-byte aligned) equals its contiguous copy; a window stride of 0 equals B separate uploads"""
    w, h, B, F = 253, 131, 3, 3
    big = torch.full((B, F, 3, h + 9, w + 14), float("nan"), device=dev)
    fr = normalized(pixels(B, F, h, w, dev, seed=2))
    crop = big[..., 3:3 + h, 5:5 + w]
    crop.copy_(fr)
    assert not crop.is_contiguous() and (crop.data_ptr() % 16 != 0 or crop.stride(3) % 4 != 0)
    fl = start_flow(B, h, w, dev, seed=3)
    job = small_job(ctx, w, h, B)
    try:
        got = device_run(ctx, job, crop, fl, False)
        want = device_run(ctx, job, fr, fl, False)
        host = host_run(job, fr.cpu().numpy(), fl.cpu().numpy(), w, False)
        assert_same(got, want, "cropped view against its contiguous copy")
        assert_same(got, host, "cropped view against the host path")
        # an aligned crop whose surroundings are NaN, through the 128-bit kernel (x0 and the big row a multiple of four floats): the quad that straddles
        # the width must not carry its neighbours into the job
        big4 = torch.full((B, F, 3, h + 8, w + 15), float("nan"), device=dev)
        crop4 = big4[..., 4:4 + h, 8:8 + w]
        crop4.copy_(fr)
        assert crop4.data_ptr() % 16 == 0 and all(s % 4 == 0 for s in crop4.stride()[:4])
        assert_same(device_run(ctx, job, crop4, fl, False), host, "aligned crop among NaN")
        shared = fr[:1].expand(B, F, 3, h, w)
        assert shared.stride(0) == 0
        got0 = device_run(ctx, job, shared, fl, False)
        want0 = host_run(job, np.repeat(fr[:1].cpu().numpy(), B, axis=0), fl.cpu().numpy(), w, False)
        assert_same(got0, want0, "window stride 0")
    finally:
        job.close()


def test_channel_weights_through_upload_device(ctx, dev):
    """sfa_job_upload_device with host channel weights (pinned staging copy) equals Job.upload with the same weights; called twice with different weights,
    so that the second call waits for the first one's copies out of the staging planes"""
    w, h, B, F = 253, 131, 2, 3
    fr = normalized(pixels(B, F, h, w, dev, seed=13))
    rng = np.random.default_rng(13)
    job = small_job(ctx, w, h, B)
    try:
        for _ in range(2):
            chw = [np.ascontiguousarray(rng.uniform(0.25, 1.75, size=(h, sfa.stride_of(w))).astype(np.float32)) for _ in range(3)]
            ctx.wait_stream()
            job.upload_device(fr, chw=chw)
            job.set_flow_device(None)
            job.run()
            out = torch.zeros((B, 2, h, w), device=dev)
            ctx.wait_stream()
            job.download_device(out)
            ctx.sync()
            got = (out.cpu().numpy(), None, job.changes())
            frn = fr.cpu().numpy()
            for b in range(B):
                job.upload(b, [host_planes(frn[b, f], w) for f in range(F)], chw=chw)
            job.run()
            want = np.stack([np.stack(job.download(b)[:2])[:, :, :w] for b in range(B)])
            assert np.array_equal(got[0], want), "channel weights through upload_device"
            assert np.array_equal(got[2], np.array([job.download(b)[2] for b in range(B)], np.float32))
        ones = device_run(ctx, job, fr, None, False)                                # and back to all ones without them
        assert not np.array_equal(ones[0], got[0])
        assert_same(ones, host_run(job, frn, None, w, False), "weights dropped again")
    finally:
        job.close()


# ---- 3. padding lanes ----------------------------------------------------------------------------------------------------------------------
def test_neighbours_of_a_view_do_not_reach_the_valid_pixels(ctx, dev):
    """What this checks: the memory AROUND a source view never enters a job's valid pixels.  Width 253 leaves 3 lanes of the last quad free; the source is a
    view whose neighbours in memory are NaN and 1e30, through the element, interleaved and 128-bit kernels, and the run that follows equals the host path.
    What it does NOT check: that columns >= width of the job's planes are left unwritten.  That rule cannot be observed through the existing API -- no entry
    point reads a job's or a sequence's padding lanes back (the downloads copy `width` columns), and no kernel of the path reads them either: the pyramid's
    staging clamps its columns to width - 1, the data-term and presmoothing kernels replicate the clamped column, the normalisation sums guard x < width --
    so a lane written by mistake would change nothing this or any other test can see.  The rule rests on the guards of device_io.hip alone (`x >= d.w`
    returns, and the quad that straddles the width is stored element by element up to the width)."""
    w, h, B, F = 253, 131, 2, 3
    fr = normalized(pixels(B, F, h, w, dev, seed=4))
    job = small_job(ctx, w, h, B)
    try:
        host = host_run(job, fr.cpu().numpy(), None, w, False)
        for name, fill in (("NaN", float("nan")), ("1e30", 1e30)):
            big = torch.full((B, F, 3, h + 4, w + 11), fill, device=dev)
            for x0 in (8, 5):                                                    # the 128-bit kernel, the element kernel
                crop = big[..., 2:2 + h, x0:x0 + w]
                crop.copy_(fr)
                assert_same(device_run(ctx, job, crop, None, False), host, f"crop at x0 = {x0} among {name}")
            bigi = torch.full((B, F, h + 4, w + 11, 3), fill, device=dev)
            cropi = bigi[:, :, 2:2 + h, 5:5 + w, :]
            cropi.copy_(fr.permute(0, 1, 3, 4, 2))
            assert_same(device_run(ctx, job, cropi, None, False, channels_last=True), host, f"interleaved crop among {name}")
    finally:
        job.close()


# ---- 4. download ---------------------------------------------------------------------------------------------------------------------------
def test_download_into_a_slice_of_a_larger_tensor(ctx, dev):
    w, h, B, F = 253, 131, 3, 3
    fr = normalized(pixels(B, F, h, w, dev, seed=5))
    job = small_job(ctx, w, h, B, occ=True)
    try:
        host = host_run(job, fr.cpu().numpy(), None, w, True)
        torch.cuda.synchronize()
        job.upload_device(fr)
        job.set_flow_device(None)
        job.run()
        for x0, wide in ((5, w + 11), (8, w + 15)):                              # the element kernel; the 128-bit kernel
            big = torch.full((B, 4, h + 6, wide), -777.0, device=dev)
            flow, occ = big[:, 1:3, 2:2 + h, x0:x0 + w], big[:, 3, 2:2 + h, x0:x0 + w]
            torch.cuda.synchronize()
            job.download_device(flow, occ)
            ctx.sync()
            got = big.cpu().numpy()
            assert np.array_equal(got[:, 1:3, 2:2 + h, x0:x0 + w], host[0]) and np.array_equal(got[:, 3, 2:2 + h, x0:x0 + w], host[1])
            outside = np.ones(got.shape, bool)
            outside[:, 1:4, 2:2 + h, x0:x0 + w] = False
            assert (got[outside] == -777.0).all(), "bytes outside the slice were written"
        # windows b0 .. of the job into a destination of their own
        part = torch.zeros((2, 2, h, w), device=dev)
        ctx.wait_stream()
        job.download_device(part, None, b0=1)
        ctx.sync()
        assert np.array_equal(part.cpu().numpy(), host[0][1:3])
        assert np.array_equal(job.changes(1, 2), host[2][1:3])
    finally:
        job.close()


# ---- 5. sequence ---------------------------------------------------------------------------------------------------------------------------
def test_sequence_upload_device_and_normalize(ctx, dev):
    w, h, N = 253, 131, 5
    px = pixels(1, N, h, w, dev, seed=6)[0]                                      # [N,3,h,w], 8-bit values
    a, b = sfa.Sequence(ctx, w, h, N), sfa.Sequence(ctx, w, h, N)
    try:
        rest = px[2:].to(torch.uint8).permute(0, 2, 3, 1).contiguous()                      # the rest as interleaved uint8
        ctx.wait_stream()
        a.upload_device(px[:2])
        a.upload_device(rest, f0=2)
        hp = host_planes(px.cpu().numpy(), w)
        for f in range(N):
            b.upload(f, hp[f])
        sa, sb = a.normalize(), b.normalize()
        assert sa == sb
        for f in range(N):
            assert np.array_equal(a.download(f).view(np.uint32), b.download(f).view(np.uint32))
    finally:
        a.close(); b.close()


# ---- 6. stream ordering --------------------------------------------------------------------------------------------------------------------
def test_refine_on_a_side_stream_without_synchronisation(ctx, dev):
    """a torch kernel writes the frames right before refine() and a torch op reads the result right after, all on one non-default stream and with no
    synchronisation in between: wait_stream / signal_stream order the library's stream; the outcome equals the fully synchronised run"""
    from slowflow_amd import device
    w, h, B, F = 1024, 436, 4, 3
    p = config2_params(2, False)
    px = pixels(B, F, h, w, dev, seed=7)
    fl = start_flow(B, h, w, dev, seed=8)
    torch.cuda.synchronize()
    want_flow, _, want_ch = device.refine(ctx, p, normalized(px), fl)
    torch.cuda.synchronize()
    want_sum = want_flow.double().sum(dim=(2, 3)).cpu().numpy()
    want = want_flow.cpu().numpy()
    side = torch.cuda.Stream(device=dev)
    frames = torch.zeros_like(px)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        frames.copy_(px)
        frames.sub_(127.0).div_(0.2)                              # the producer: the last kernels before refine write the frames
        got_flow, _, got_ch = device.refine(ctx, p, frames, fl)
        got_sum = got_flow.double().sum(dim=(2, 3))               # the consumer, on the same stream
        frames.zero_()                                            # and a reuse of the input, ordered after the library's reads
    side.synchronize()
    assert np.array_equal(got_sum.cpu().numpy(), want_sum)
    assert np.array_equal(got_flow.cpu().numpy(), want) and np.array_equal(got_ch, want_ch)
    device.release_jobs(ctx)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
class HostArray:
    """a host array that claims to be a device array"""

    def __init__(self, a):
        self.a = a
        self.__cuda_array_interface__ = {"shape": a.shape, "typestr": "<f4", "data": (a.ctypes.data, False), "version": 3, "strides": None}


def test_refusals_name_the_argument_and_launch_nothing(ctx, dev):
    from slowflow_amd import device
    w, h, B, F = 96, 64, 2, 3
    fr = normalized(pixels(B, F, h, w, dev, seed=9))
    job = small_job(ctx, w, h, B)
    try:
        want = host_run(job, fr.cpu().numpy(), None, w, False)
        torch.cuda.synchronize()

        def refused(call, *words):
            with pytest.raises(sfa.SlowflowError) as e:
                call()
            assert all(word in str(e.value) for word in words), str(e.value)

        host = np.zeros((B, F, 3, h, w), np.float32)
        refused(lambda: job.upload_device(host), "frames", "__cuda_array_interface__")                       # numpy: no interface at all
        refused(lambda: job.upload_device(HostArray(host)), "sfa_job_upload_device", "frames_dev", "not device memory")
        refused(lambda: job.set_flow_device(HostArray(np.zeros((B, 2, h, w), np.float32))), "flow_dev", "not device memory")
        refused(lambda: job.download_device(HostArray(np.zeros((B, 2, h, w), np.float32))), "flow_dev", "not device memory")
        refused(lambda: job.upload_device(fr.half()), "frames", "<f2")
        if torch.cuda.device_count() > 1:
            refused(lambda: job.upload_device(fr.to(torch.device("cuda", 1))), "frames_dev", "GPU 1")
        refused(lambda: job.upload_device(fr, b0=1), "b0 = 1", "n = 2", "batch of 2")
        refused(lambda: job.download_device(torch.zeros((B, 2, h, w), device=dev), b0=1), "b0 = 1", "batch of 2")
        one = torch.zeros((1, 2, h, w), device=dev)
        refused(lambda: job.download_device(one.expand(B, 2, h, w)), "flow_dev", "overlap")                 # both windows into one
        both = torch.zeros((B, 2, h, w), device=dev)
        refused(lambda: job.download_device(both, both[:, 0]), "occ_dev", "overlap")                        # the labels onto u
        refused(lambda: job.download_device(torch.zeros((B, 1, h, w), device=dev).expand(B, 2, h, w)), "overlap")   # u onto v
        # through the C-ABI: an element type that does not exist, a column stride of 0, a negative row stride
        L = device._lib()
        lay = device.default_layout(w, h, F)
        for field, value, word in (("dtype", 7, "layout.dtype"), ("column", 0, "layout.column"), ("row", -w, "negative stride")):
            bad = device.DevLayout.from_buffer_copy(lay)
            setattr(bad, field, value)
            rc = L.sfa_job_upload_device(job.h_, 0, B, C.c_void_p(fr.data_ptr()), C.byref(bad), None)
            assert rc == -1 and word in L.sfa_last_error(ctx.h).decode(), L.sfa_last_error(ctx.h).decode()
        st = (C.c_longlong * 4)(2 * h * w, h * w, w, 0)
        assert L.sfa_job_set_flow_device(job.h_, 0, B, C.c_void_p(both.data_ptr()), st) == -1 and "column stride of flow_dev" in L.sfa_last_error(ctx.h).decode()
        # a view that leaves its allocation
        big = device.DevLayout.from_buffer_copy(lay)
        big.window = 1 << 40
        assert L.sfa_job_upload_device(job.h_, 0, B, C.c_void_p(fr.data_ptr()), C.byref(big), None) == -1 and "beyond its allocation" in L.sfa_last_error(ctx.h).decode()
        wrap = device.DevLayout.from_buffer_copy(lay)
        wrap.window = 1 << 62                                     # 4 * window leaves the 64-bit range: refused, not wrapped into a small extent
        job4 = small_job(ctx, w, h, 5)
        try:
            assert L.sfa_job_upload_device(job4.h_, 0, 5, C.c_void_p(fr.data_ptr()), C.byref(wrap), None) == -1 and "64-bit range" in L.sfa_last_error(ctx.h).decode()
        finally:
            job4.close()
        # nothing was launched and nothing was changed: the job still holds the host path's upload, and the context refines a good job
        job.run()
        ctx.sync()
        again = np.stack([np.stack(job.download(b)[:2])[:, :, :w] for b in range(B)])
        assert np.array_equal(again, want[0])
        assert_same(device_run(ctx, job, fr, None, False), want, "a good job after the refusals")
    finally:
        job.close()


# ---- 8. a batch beyond one job ---------------------------------------------------------------------------------------------------------
def test_refine_splits_a_large_batch(ctx, dev):
    from slowflow_amd import device
    w, h, B, F = 96, 64, 130, 3
    p = config2_params(2, True, layers=2)
    fr = normalized(pixels(B, F, h, w, dev, seed=10))
    fl = start_flow(B, h, w, dev, seed=11)
    torch.cuda.synchronize()
    flow, occ, change = device.refine(ctx, p, fr, fl, want_occ=True)
    torch.cuda.synchronize()
    jobs = ctx.__dict__["_refine_jobs"]
    assert [j.batch for j in jobs.values()] == [65]                                # two jobs of 65 windows: one shape, created once
    device.release_jobs(ctx)
    got = (flow.cpu().numpy(), occ.cpu().numpy(), change)
    frn, fln = fr.cpu().numpy(), fl.cpu().numpy()
    job = sfa.Job(ctx, p, w, h, 65)
    try:
        parts = [host_run(job, frn[b0:b0 + 65], fln[b0:b0 + 65], w, True) for b0 in (0, 65)]
    finally:
        job.close()
    assert_same(got, tuple(np.concatenate([a[i] for a in parts]) for i in range(3)), "130 windows")


def test_refine_normalize_goes_through_a_sequence(ctx, dev):
    """normalize=True: the bits of Sequence.normalize over the frames as passed, then the refinement with those statistics as the parameters' norm_avg / norm_std"""
    from slowflow_amd import device
    w, h, B, F = 96, 64, 2, 3
    p = config2_params(2, False, layers=2)
    px = pixels(B, F, h, w, dev, seed=12)
    torch.cuda.synchronize()
    flow, _, change = device.refine(ctx, p, px.to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous(), normalize=True)
    torch.cuda.synchronize()
    device.release_jobs(ctx)
    seq = sfa.Sequence(ctx, w, h, B * F)
    hp = host_planes(px.cpu().numpy().reshape(B * F, 3, h, w), w)
    for f in range(B * F):
        seq.upload(f, hp[f])
    avg, std = seq.normalize()
    q = type(p).from_buffer_copy(p)
    for k in range(3):
        q.norm_avg[k], q.norm_std[k] = avg[k], std[k]
    job = sfa.Job(ctx, q, w, h, B)
    try:
        want = host_run(job, np.stack([seq.download(f)[:, :, :w] for f in range(B * F)]).reshape(B, F, 3, h, w), None, w, False)
    finally:
        job.close(); seq.close()
    assert_same((flow.cpu().numpy(), None, change), want, "refine(normalize=True)")
