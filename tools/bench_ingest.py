#!/usr/bin/env python3
"""Ingest of raw Bayer frames, host route against GPU route (cfg gpu_ingest 0 / 1), on 32 frames of 2048 x 1024 u16 mosaics:
  method 2 at scale 0.25 (the reference cfg's camera setting) and method 0 at scale 1.
(a), (b): the slow_flow driver with gpu_ingest 0 and 1 on the same PGM files, `ingest_seconds` of run.json: the wall time from the start of the run to
    the normalised resident sequence.  That figure INCLUDES reading and decoding the files, the same work in both routes, so the ratio (b) / (a) is
    diluted by it: it understates what the routes differ by.  `decode_seconds` is printed beside it (files decoded; with gpu_ingest 0 also demosaiced and
    cropped on the host, in the io pool, so it is not the same work in (a) and (b)), and so is `ingest_seconds - decode_seconds`: what remains after the
    last file is decoded -- for (a) the rescale round trips and the uploads, for (b) whatever of upload + demosaic + rescale the decoding did not hide.
    The refinement is cut to one sweep per window: it is not part of the figure.
(k): the kernels of route (b) alone, per launch, from HIP events on the context's stream (sfa_timer_start / stop): one upload_mosaic_device of all 32 frames,
    one rescale, after a warm-up launch of each; three repetitions, every value printed.
Three repetitions of everything, in the order a b a b a b; every value is printed, with the median.  Clocks and power are the machine's own at the time
(no pinning): compare (a) and (b) of one run only.

usage: tools/bench_ingest.py [--frames 32] [--width 2048] [--height 1024] [--reps 3] [--out profiles/ingest_bench.txt]"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slowflow_amd as sfa  # noqa: E402

SETTINGS = [(2, 0.25), (0, 1.0)]


def mosaics(n, w, h):
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:h, 0:w]
    base = 2000 + 1500 * np.sin(0.013 * x + 0.007 * y) + 300 * np.cos(0.11 * x - 0.05 * y)
    return [np.clip(base + 40 * k + rng.normal(0, 20, (h, w)), 1, 65535).astype(np.uint16) for k in range(n)]


def driver(folder, frames, method, scale, gpu_ingest, rep):
    out = os.path.join(folder, "out_%d_%g_%d_%d" % (method, scale, gpu_ingest, rep))
    cfg = os.path.join(folder, "run.cfg")
    jets = frames - 3
    with open(cfg, "w") as f:
        f.write("file\t%s/m_%%04i.pgm\noutput\t%s\nJets\t%d\nstart\t2\nmax_fps\t200\n16bit\t1\nraw\t1\nraw_demosaicing\t%d\nraw_red_loc\t1,0\nraw_weight\t1\nscale\t%g\n"
                "deep_matching\t0\nslow_flow_S\t2\nslow_flow_layers\t1\nslow_flow_niter_alter\t1\nslow_flow_niter_outer\t1\nslow_flow_niter_solver\t1\n"
                "slow_flow_occlusion_reasoning\t0\nslow_flow_output_occlusions\t0\ngpus\t1\ngpu_batch\t8\ngpu_ingest\t%d\n" % (folder, out, jets, method, scale, gpu_ingest))
    r = subprocess.run([os.path.join(ROOT, "slowflow_amd", "host", "slow_flow"), cfg, "-overwrite"], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit("slow_flow failed:\n" + r.stdout[-2000:] + r.stderr[-2000:])
    print("driver: raw_demosaicing %d scale %g gpu_ingest %d rep %d done" % (method, scale, gpu_ingest, rep), flush=True)
    run = json.load(open(os.path.join(out, "run.json")))
    shutil.rmtree(out)
    return run["ingest_seconds"], run["decode_seconds"], run["per_gpu"][0]["upload_bytes"]


def kernels(ms, method, scale, reps):
    """per-launch kernel times (ms) of route (b): demosaic of all frames from device memory, rescale"""
    import torch
    from slowflow_amd import device
    ctx = sfa.Context(0)
    n, h, w = len(ms), ms[0].shape[0], ms[0].shape[1]
    dev_m = torch.from_numpy(np.stack(ms)).to("cuda:0")
    torch.cuda.synchronize()
    full = sfa.Sequence(ctx, w, h, n)
    dw, dh = int(np.rint(w * float(np.float32(scale)))), int(np.rint(h * float(np.float32(scale))))
    small = sfa.Sequence(ctx, dw, dh, n) if scale != 1 else None
    out = []
    for rep in range(reps + 1):                                  # the first pass warms up
        ctx.timer_start(); full.upload_mosaic_device(dev_m, (1, 0), method); t_dem = ctx.timer_stop()
        t_res = None
        if small is not None:
            ctx.timer_start(); small.rescale_from(full, scale); t_res = ctx.timer_stop()
        if rep:
            out.append((t_dem, t_res))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.txt"))
    a = ap.parse_args()
    lines = ["ingest of %d raw frames of %d x %d u16 (tools/bench_ingest.py), %s" % (a.frames, a.width, a.height, time.strftime("%Y-%m-%d")),
             "clocks and power: the machine's own at the time, not pinned; (a) and (b) alternate within one run and are to be compared with each other only"]
    folder = tempfile.mkdtemp(prefix="ingest_bench_")
    try:
        ms = mosaics(a.frames, a.width, a.height)
        for k, m in enumerate(ms):
            with open(os.path.join(folder, "m_%04d.pgm" % (1 + k)), "wb") as f:
                f.write(b"P5\n%d %d\n65535\n" % (a.width, a.height) + m.astype(">u2").tobytes())
        driver(folder, a.frames, 2, 0.25, 1, 99)                 # warm-up: the file cache, the runtime's first start
        for method, scale in SETTINGS:
            res = {0: [], 1: []}
            for rep in range(a.reps):
                for gi in (0, 1):
                    res[gi].append(driver(folder, a.frames, method, scale, gi, rep))
            lines.append("")
            lines.append("raw_demosaicing %d, scale %g" % (method, scale))
            for gi, name in ((0, "(a) gpu_ingest 0: host demosaic + rescale round trips + upload of 3 fp32 planes"), (1, "(b) gpu_ingest 1: mosaic upload + GPU demosaic + GPU rescale")):
                ing = [r[0] for r in res[gi]]
                lines.append("  %s" % name)
                lines.append("    ingest_seconds %s  median %.3f  spread max / min %.3f  (decode_seconds %s; bytes sent %.0f)" % (
                    " ".join("%.3f" % v for v in ing), statistics.median(ing), max(ing) / min(ing), " ".join("%.3f" % r[1] for r in res[gi]), res[gi][0][2]))
                rest = [r[0] - r[1] for r in res[gi]]
                lines.append("    ingest_seconds - decode_seconds %s  median %.3f" % (" ".join("%.3f" % v for v in rest), statistics.median(rest)))
            lines.append("  (b) / (a) of the medians: %.2f" % (statistics.median([r[0] for r in res[1]]) / statistics.median([r[0] for r in res[0]])))
            for t_dem, t_res in kernels(ms, method, scale, a.reps):
                px = a.frames * a.width * a.height
                lines.append("  (k) demosaic launch, %d frames: %.3f ms (%.0f GB/s counting 2 bytes read + 12 written per pixel; the halo re-reads, 1.19 x the tile, are not counted)%s" % (
                    a.frames, t_dem, px * 14 / t_dem / 1e6,
                    "" if t_res is None else "; rescale (blur + resize, %d chunk(s) of up to 8 frames): %.3f ms" % ((a.frames + 7) // 8, t_res)))
            with open(a.out, "w") as f:                             # (after every setting: a run cut short leaves what it measured)
                f.write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(folder, ignore_errors=True)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
