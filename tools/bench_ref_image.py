"""Times dense_tracking's reference-image stage (slowflow_amd/csrc/ref_image.hip) on the GPU and writes profiles/ref_image_bench.txt.

Per start_jet (one frame 0 of 1024 x 436), acc_skip_pixel 0 / 1 / 3, batches of 1 and 16 frames:
  device   sfa_reference_lab_device on frames already in GPU memory (device.reference_lab into preallocated outputs), HIP events around `inner` calls
  route    what accumulate -fill ran before at acc_skip_pixel 0, the only value it served: rgb8_to_lab on the host, then the upload of the three Lab planes
           and a wait (tools/ref_image_route.cpp, a host clock around work that ends in a synchronise)
Each figure is the median over `--reps` repetitions after a warm-up, with the smallest and largest beside it.  The outputs of skip 1 and 3 are compared
with tests/ref_image_ref.py at the timed size before anything is timed.  Needs a GPU; there is no fallback.

    python tools/bench_ref_image.py [--reps 20] [--inner 50] [--out profiles/ref_image_bench.txt]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
W, H = 1024, 436


def build_route(exe):
    """the route's program, built where it is missing or older than its source (a build made beforehand is used as it is)"""
    src = os.path.join(ROOT, "tools", "ref_image_route.cpp")
    if os.path.exists(exe) and os.path.getmtime(exe) >= os.path.getmtime(src):
        return exe
    host = os.path.join(ROOT, "slowflow_amd", "host")
    r = subprocess.run(["make", "-C", host], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-pthread", "-I", host, os.path.join(ROOT, "tools", "ref_image_route.cpp"), os.path.join(host, "libslowflow_host.a"),
                        "-L", os.path.join(ROOT, "slowflow_amd"), "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "slowflow_amd"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def stats(v):
    v = sorted(v)
    return "%.4f (%.4f .. %.4f)" % (float(np.median(v)), v[0], v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ref_image_bench.txt"))
    a = ap.parse_args()
    import torch

    import ref_image_ref as R
    import slowflow_amd as sfa
    from slowflow_amd import device
    assert torch.cuda.is_available(), "no GPU: nothing is measured"
    ctx, dev = sfa.Context(0), torch.device("cuda", 0)
    lines = ["reference image stage, %d x %d, ms per FRAME: median (min .. max) over %d repetitions of %d calls after a warm-up" % (W, H, a.reps, a.inner), ""]
    for batch in (1, 16):
        rgb = np.random.default_rng(batch).integers(0, 256, (batch, 3, H, W)).astype(np.float32)
        src = torch.from_numpy(rgb).to(dev)
        for skip in (0, 1, 3):
            gw, gh = sfa.reference_grid(W, H, skip)
            out = torch.empty((batch, 3, gh, gw), dtype=torch.float32, device=dev)
            out8 = torch.empty((batch, 3, gh, gw), dtype=torch.uint8, device=dev)
            device.reference_lab(ctx, src, skip, out=out, out_rgb8=out8)                     # warm-up, and the check at the timed size
            torch.cuda.synchronize()
            assert np.array_equal(out8[0].cpu().numpy(), R.reference_rgb8(rgb[0], skip)), "the kernel's image is not the restatement's"
            for with8 in (False, True):
                ms = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.inner):
                        device.reference_lab(ctx, src, skip, out=out, out_rgb8=out8 if with8 else None)
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1) / (a.inner * batch))
                lines.append("device  batch %2d  skip %d  %-14s %s" % (batch, skip, "Lab + rgb8" if with8 else "Lab", stats(ms)))
    ctx.close()
    exe = build_route(os.path.join(ROOT, "tools", "_ref_image_route"))
    for batch in (1, 16):
        r = subprocess.run([exe, str(W), str(H), str(batch), str(a.reps)], capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, r.stdout + r.stderr
        cols = np.array([[float(v) for v in line.split()[1:]] for line in r.stdout.splitlines() if line.startswith("route_ms")])
        for k, name in enumerate(("host rgb8_to_lab", "upload + wait", "both")):
            lines.append("route   batch %2d  skip 0  %-18s %s" % (batch, name, stats(cols[:, k].tolist())))
    lines += ["", "The route exists at skip 0 only: before this stage accumulate -fill refused every other acc_skip_pixel.",
              "The wall time of accumulate -fill at acc_skip_pixel 1 on full frames: not measured."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
