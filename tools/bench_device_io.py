"""The device seam (sfa_job_upload_device ...; slowflow_amd/device.py) at 1024 x 436, config 2.  Prints the record kept as profiles/device_io_bench.txt.

  bench_device_io.py [reps]     (default 10 timed repeats after 2 warm-ups)

  1. pack: 128 windows x 3 frames, contiguous planar fp32, one launch of k_pack_frames -- against the same bytes copied the way the library did it before,
     in the same process, two ways: (a) like for like through the library: 128 whole sfa_job_upload_resident calls out of a resident sequence (each 3
     hipMemcpyAsync device-to-device of 3 planes at the pitch AND two hipMemsetAsync of the initial flow) against upload_device + set_flow_device(None),
     which do the same work; HIP events on the context's stream (sfa_timer_start / stop); (b) the copies alone: the same 384 hipMemcpyAsync
     device-to-device calls of 3 planes each, issued straight at the HIP runtime between two buffers of the sequence's size on a stream of their own
     (HIP events on it), against the k_pack_frames launch alone.  Both sides of (a) and the copies of (b) are issued from Python, one ctypes call each.
  2. the same launch for interleaved uint8 [B,F,H,W,3] and for a cropped, unaligned view of a larger fp32 tensor: rate per OUTPUT byte as a fraction of 1.
  3. end to end at B = 1 and B = 16: refine() on device tensors against the host path on the same data (.cpu().numpy(), Job.upload / run / download, back
     to a device tensor), wall clock from the caller's side around a synchronised device.
"""
import ctypes as C
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import slowflow_amd as sfa  # noqa: E402
from slowflow_amd import device  # noqa: E402

W, H, S, F = 1024, 436, 2, 3
WARM = 2


def params():
    p = sfa.default_params()
    p.S = S; p.layers = 5; p.niter_alter = 1; p.niter_outer = 5; p.niter_inner = 1; p.niter_solver = 30
    p.thres_outer = 0; p.thres_inner = 0; p.occlusion_reasoning = 0; p.hbit = 0
    p.rho[0] = 1; p.omega[0] = 0
    for k in range(3):
        p.norm_avg[k] = 127.0; p.norm_std[k] = 0.2
    return p


def textures(B, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    base = torch.rand((B, 3, H + 16, W + 16), generator=g, device=dev)
    for _ in range(2):
        base = torch.nn.functional.avg_pool2d(base, 5, 1, 2)
    base = torch.round((base - base.amin()) / (base.amax() - base.amin()) * 255.0)
    return torch.stack([base[:, :, 8 - f:8 - f + H, 8 - 2 * f:8 - 2 * f + W] for f in range(F)], dim=1).contiguous()


def timed(ctx, fn, reps):
    """ms of `fn` (work enqueued on the context's stream) between two events on that stream: minimum, median, maximum of `reps` after WARM warm-ups"""
    ts = []
    for i in range(WARM + reps):
        ctx.sync()
        ctx.timer_start()
        fn()
        ms = ctx.timer_stop()
        if i >= WARM:
            ts.append(ms)
    return min(ts), float(np.median(ts)), max(ts)


def wall(fn, reps):
    ts = []
    for i in range(WARM + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts), float(np.median(ts)), max(ts)


def fmt(t):
    return "min %.3f  median %.3f  max %.3f ms" % t


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    dev = torch.device("cuda", 0)
    ctx = sfa.Context(0)
    p = params()
    print("# tools/bench_device_io.py: 1024 x 436, S = 2 (3 frames), config 2; %d timed repeats after %d warm-ups" % (reps, WARM))
    print("# library sha256 %s" % hashlib.sha256(open(sfa.LIB_PATH, "rb").read()).hexdigest())
    # ---- 1, 2: the pack launch ---------------------------------------------------------------------------------------------
    B = 128
    px = textures(4, dev)[torch.arange(B, device=dev) % 4].contiguous()               # [B,F,3,H,W] fp32, 8-bit values
    out_bytes = B * F * 3 * H * W * 4
    job = sfa.Job(ctx, p, W, H, B)
    seq = sfa.Sequence(ctx, W, H, B * F)
    torch.cuda.synchronize()
    seq.upload_device(px.view(B * F, 3, H, W))
    ctx.sync()
    t_pack = timed(ctx, lambda: job.upload_device(px), reps)

    def device_both():
        job.upload_device(px)
        job.set_flow_device(None)

    def resident():
        for b in range(B):
            job.upload_resident(b, seq, [b * F + f for f in range(F)])
    t_both = timed(ctx, device_both, reps)
    t_res = timed(ctx, resident, reps)
    # (b) the bare copies: what sfa_job_upload_resident issues for the frames, and nothing else
    pitch = (W + 63) // 64 * 64
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    src = torch.zeros((B * F, 3, H, pitch), device=dev)
    dst = torch.zeros((B * F, 3, H, pitch), device=dev)
    side = torch.cuda.Stream(device=dev)
    nbytes = 3 * H * pitch * 4
    calls = [(dst.data_ptr() + i * nbytes, src.data_ptr() + i * nbytes) for i in range(B * F)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for i in range(WARM + reps):
        torch.cuda.synchronize()
        e0.record(side)
        for d, s_ in calls:
            rc = hip.hipMemcpyAsync(d, s_, nbytes, 3, side.cuda_stream)              # 3 = hipMemcpyDeviceToDevice
            assert rc == 0
        e1.record(side)
        e1.synchronize()
        if i >= WARM:
            ts.append(e0.elapsed_time(e1))
    t_copy = (min(ts), float(np.median(ts)), max(ts))
    del src, dst
    print("1. pack, %d windows x %d frames, contiguous planar fp32 (%.2f GB of valid pixels out):" % (B, F, out_bytes / 1e9))
    print(" (a) like for like through the library (frames + zero initial flow of every window):")
    print("   upload_device + set_flow_device(None)           %s" % fmt(t_both))
    print("   %d sfa_job_upload_resident calls               %s   (%d hipMemcpyAsync of 3 planes at pitch %d + %d hipMemsetAsync)" % (
        B, fmt(t_res), B * F, pitch, 2 * B))
    print("   ratio (medians) %.3f; spread max / min: resident %.3f, device %.3f" % (t_both[1] / t_res[1], t_res[2] / t_res[0], t_both[2] / t_both[0]))
    print(" (b) the frame copies alone:")
    print("   k_pack_frames (one launch, 128-bit)            %s   %.0f GB/s out" % (fmt(t_pack), out_bytes / t_pack[1] / 1e6))
    print("   %d hipMemcpyAsync device-to-device, 3 planes   %s   %.0f GB/s out (%.2f us per copy)" % (
        B * F, fmt(t_copy), out_bytes / t_copy[1] / 1e6, 1e3 * t_copy[1] / (B * F)))
    print("   ratio kernel / copies (medians) %.3f; spread max / min: copies %.3f, kernel %.3f" % (
        t_pack[1] / t_copy[1], t_copy[2] / t_copy[0], t_pack[2] / t_pack[0]))
    u8 = px.to(torch.uint8).permute(0, 1, 3, 4, 2).contiguous()
    big = torch.zeros((B, F, 3, H + 9, W + 14), device=dev)
    crop = big[..., 3:3 + H, 5:5 + W]
    crop.copy_(px)
    torch.cuda.synchronize()
    t_u8 = timed(ctx, lambda: job.upload_device(u8), reps)
    t_crop = timed(ctx, lambda: job.upload_device(crop), reps)
    print("2. the same windows from other layouts (rate per output byte as a fraction of 1.):")
    print("   interleaved uint8 [B,F,H,W,3]                  %s   %.2f" % (fmt(t_u8), t_pack[1] / t_u8[1]))
    print("   cropped fp32 view (row stride %d, unaligned)  %s   %.2f" % (crop.stride(3), fmt(t_crop), t_pack[1] / t_crop[1]))
    fl = torch.zeros((B, 2, H, W), device=dev)
    torch.cuda.synchronize()
    t_flow = timed(ctx, lambda: job.set_flow_device(fl), reps)
    t_down = timed(ctx, lambda: job.download_device(fl), reps)
    print("   k_pack_flow, %d windows                        %s" % (B, fmt(t_flow)))
    print("   k_unpack_planes (u, v), %d windows             %s" % (B, fmt(t_down)))
    job.close(); seq.close()
    del px, u8, big, crop, fl
    # ---- 3: end to end --------------------------------------------------------------------------------------------------------
    print("3. end to end, wall clock from the caller's side (device synchronised before and after):")
    for B in (1, 16):
        frames = ((textures(B, dev) - 127.0) / 0.2).contiguous()
        flow0 = torch.zeros((B, 2, H, W), device=dev)
        hjob = sfa.Job(ctx, p, W, H, B)
        st = sfa.stride_of(W)

        def host_path():
            fn, f0 = frames.cpu().numpy(), flow0.cpu().numpy()
            for b in range(B):
                hjob.upload(b, [np.ascontiguousarray(fn[b, f]) for f in range(F)], np.ascontiguousarray(f0[b, 0]), np.ascontiguousarray(f0[b, 1]))
            hjob.run()
            out = np.zeros((B, 2, H, st), np.float32)
            for b in range(B):
                out[b, 0], out[b, 1], _ = hjob.download(b)
            return torch.from_numpy(out).to(dev)
        assert st == W
        t_host = wall(host_path, reps)
        t_dev = wall(lambda: device.refine(ctx, p, frames, flow0), reps)
        same = torch.equal(host_path(), device.refine(ctx, p, frames, flow0)[0])
        print("   B = %-2d  host path  %s" % (B, fmt(t_host)))
        print("           refine()   %s   difference of the medians %.3f ms (%.1f %%); results equal: %s" % (
            fmt(t_dev), t_host[1] - t_dev[1], 100 * (t_host[1] - t_dev[1]) / t_host[1], same))
        hjob.close()
        device.release_jobs(ctx)
    ctx.close()


if __name__ == "__main__":
    main()
