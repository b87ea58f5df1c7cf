"""adaptiveFR's flow-magnitude quantile on flows in GPU memory: device.flow_quantiles (sfa_flow_magnitude_quantiles_device, G groups in one launch
sequence) against what a caller had to do before it, G sequential Context.flow_magnitude_quantile calls on the same values in host memory.

  bench_quantile.py [--out FILE]
      G = 1, 16 and 64 groups of n = 8 fields of 256 x 109 (adaptiveFR's quarter-size samples), and G = 1 of 8 fields of 1024 x 436.
      Grouped call: wall time from the call to the end of a synchronise (host clock, median of 5 after a warm-up), the time the call itself takes to
      return, and its GPU time from HIP events on the context's stream (sfa_timer_start / stop) for planar [G,n,2,h,w], channels-last [G,n,h,w,2] and
      rows padded to a pitch of w + 11.  Host path: wall time of the G calls (host planes in hand), the download of the flows that precedes them
      for a caller whose flows are on the GPU, and the stream time of the calls from the same events, which holds their 2 n uploads and their kernels.
      Each measurement runs in a child process of its own, three runs each, the two ways alternating; both children return their results, which must
      be equal.  Writes FILE (profiles/quantile_device_bench.txt)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

N_FIELDS, REPS, RUNS, Q, SCALE = 8, 5, 3, 0.99, 0.25
CONFIGS = [(1, 256, 109), (16, 256, 109), (64, 256, 109), (1, 1024, 436)]


def flows(G, w, h):
    """[G,n,2,h,w] fp32: each group at a magnitude of its own"""
    rng = np.random.default_rng(G * 1000 + w)
    f = rng.standard_normal((G, N_FIELDS, 2, h, w), dtype=np.float32)
    return f * (1.0 + np.arange(G, dtype=np.float32)).reshape(G, 1, 1, 1, 1)


def child_device(G, w, h):
    import torch

    import slowflow_amd as sfa
    from slowflow_amd import device
    ctx = sfa.Context(0)
    dev = torch.device("cuda", 0)
    t = torch.from_numpy(flows(G, w, h)).to(dev)
    last = t.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    padded = torch.zeros((G, N_FIELDS, 2, h, w + 11), device=dev)[..., :w]
    padded.copy_(t)
    out = torch.empty((G, 2), dtype=torch.float64, device=dev)
    res, gpu = {}, {}
    for name, x in (("planar", t), ("channels_last", last), ("padded", padded)):
        ms = []
        for _ in range(REPS + 1):
            torch.cuda.synchronize()
            ctx.timer_start()
            device.flow_quantiles(ctx, x, Q, SCALE, out=out)
            ms.append(ctx.timer_stop())
        gpu[name] = float(np.median(ms[1:]))
        res[name] = out.cpu().numpy().tolist()
    assert res["planar"] == res["channels_last"] == res["padded"]
    wall, enq = [], []
    for _ in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device.flow_quantiles(ctx, t, Q, SCALE, out=out)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0)); enq.append(1e3 * (t1 - t0))
    print(json.dumps(dict(wall_ms=float(np.median(wall[1:])), enqueue_ms=float(np.median(enq[1:])), gpu_ms=gpu, result=res["planar"])))


def child_host(G, w, h):
    import torch

    import slowflow_amd as sfa
    ctx = sfa.Context(0)
    f = flows(G, w, h)
    t = torch.from_numpy(f).to(torch.device("cuda", 0))
    us = [[np.ascontiguousarray(f[g, i, 0]) for i in range(N_FIELDS)] for g in range(G)]
    vs = [[np.ascontiguousarray(f[g, i, 1]) for i in range(N_FIELDS)] for g in range(G)]
    wall, down, stream = [], [], []
    for _ in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.cpu()
        down.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        res = [ctx.flow_magnitude_quantile(us[g], vs[g], w, SCALE, Q) for g in range(G)]
        wall.append(1e3 * (time.perf_counter() - t0))
        ctx.timer_start()
        for g in range(G):
            ctx.flow_magnitude_quantile(us[g], vs[g], w, SCALE, Q)
        stream.append(ctx.timer_stop())
    print(json.dumps(dict(wall_ms=float(np.median(wall[1:])), download_ms=float(np.median(down[1:])), stream_ms=float(np.median(stream[1:])), result=[list(r) for r in res])))


def spawn(args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit("child %s failed (%d):\n%s%s" % (args, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def spread(v):
    return "%s (median %.3f, spread %.3f)" % (" / ".join("%.3f" % x for x in v), float(np.median(v)), max(v) - min(v))


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child-device"]:
        return child_device(*[int(a) for a in args[1:4]])
    if args[:1] == ["--child-host"]:
        return child_host(*[int(a) for a in args[1:4]])
    out = os.path.join(ROOT, "profiles", "quantile_device_bench.txt")
    if "--out" in args:
        out = args[args.index("--out") + 1]
    lines = ["# tools/bench_quantile.py on one MI355X (gfx950); n = %d fields per group, q = %g, flow_scale = %g; every row a process of its own, median of %d calls after a warm-up;"
             % (N_FIELDS, Q, SCALE, REPS),
             "# %d runs each, the grouped device call and the host path alternating; all times in ms; the two ways returned equal bits in every run" % RUNS,
             "# GPU time: HIP events on the context's stream around the call(s).  The host entry point uploads and selects inside one call, so its stream time holds the",
             "# 2 n uploads with the kernels; packed against strided reads is the comparison of the grouped call's three layouts (planar is what the packed kernel reads)"]
    verdict = None
    for G, w, h in CONFIGS:
        d, p = [], []
        for _ in range(RUNS):
            d.append(spawn(["--child-device", G, w, h]))
            p.append(spawn(["--child-host", G, w, h]))
            if d[-1]["result"] != p[-1]["result"]:
                raise SystemExit("G = %d, %d x %d: the grouped call and the host path differ" % (G, w, h))
            print("G = %d, %d x %d: device %s | host %s" % (G, w, h, {k: v for k, v in d[-1].items() if k != "result"}, {k: v for k, v in p[-1].items() if k != "result"}), flush=True)
        values = G * N_FIELDS * w * h
        lines += ["G = %d groups of %d fields of %d x %d (%d values)" % (G, N_FIELDS, w, h, values),
                  "  grouped device call, wall to the end of a synchronise:   " + spread([x["wall_ms"] for x in d]),
                  "  grouped device call, until the call returns:            " + spread([x["enqueue_ms"] for x in d]),
                  "  %d host-path calls, host planes in hand, wall:           " % G + spread([x["wall_ms"] for x in p]),
                  "  the download of the flows that precedes them, wall:      " + spread([x["download_ms"] for x in p])]
        for name in ("planar", "channels_last", "padded"):
            v = [x["gpu_ms"][name] for x in d]
            lines.append("  grouped call, GPU time, %-14s                  %s = %.3f ns per value" % (name + ":", spread(v), 1e6 * float(np.median(v)) / values))
        v = [x["stream_ms"] for x in p]
        lines.append("  host path, stream time of the %d calls (uploads + kernels): %s = %.3f ns per value" % (G, spread(v), 1e6 * float(np.median(v)) / values))
        if G == 16:
            faster = [x["wall_ms"] < y["wall_ms"] for x, y in zip(d, p)]
            verdict = "# condition: at G = 16 the grouped device call is faster than the 16 host-path calls (without their download) in %d of %d runs: %s" % (
                sum(faster), RUNS, "met" if all(faster) else "NOT met")
            lines.append("  " + verdict[2:])
    lines.append(verdict)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
