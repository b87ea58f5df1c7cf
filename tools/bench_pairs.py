#!/usr/bin/env python3
"""Times the two-frame refinement of 1, 16 and 128 pairs of 1024 x 436 with default parameters, three ways:
  (a) Context.variational_2frame_batch on host planes -- staging, host copies and the wait included: what a caller pays without a resident job,
  (b) a resident PairJob with SFA_PAIR_UNFUSED=1: the stored 24-plane derivative stack and k_data_2f,
  (c) a resident PairJob as it runs by default: k_data_2f_fused.
A call is timed on the host clock from its first statement to the return of the wait that ends it ((b), (c): run() + Context.sync(); the pairs are
resident, nothing is copied).  Per case 3 warm-up calls, then 10 timed ones: median, minimum and maximum in ms.  The work of a call does not depend on the
data (fixed iteration counts), so (b) and (c) keep refining the flow the job holds instead of uploading it again.
Not part of bench.py.  Usage: python tools/bench_pairs.py [--out profiles/pair_job_bench.txt] [--pairs 1,16,128] [--size 1024x436]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import slowflow_amd as sfa  # noqa: E402

WARMUP, TIMED = 3, 10


def make_pairs(w, h, n, seed=0):
    """n pairs that differ (one band-limited texture rolled by a different offset per pair, the second frame its translate by (2, 1)) as host planes"""
    rng = np.random.default_rng(seed)
    stride = sfa.stride_of(w)
    base = rng.uniform(0, 255, size=(3, h + 8, w + 8)).astype(np.float32)
    for ax in (1, 2):
        base = sum(np.roll(base, s, axis=ax) for s in range(-2, 3)) / 5.0
    out = []
    for i in range(n):
        b = np.roll(base, (3 * i, 7 * i), axis=(1, 2))
        im1, im2 = np.zeros((3, h, stride), np.float32), np.zeros((3, h, stride), np.float32)
        im1[:, :, :w] = b[:, 4:4 + h, 4:4 + w]
        im2[:, :, :w] = b[:, 3:3 + h, 2:2 + w]
        wx, wy = np.full((h, stride), 1.75, np.float32), np.full((h, stride), 0.75, np.float32)
        out.append((im1, im2, wx, wy))
    return out


def timed(call):
    for _ in range(WARMUP):
        call()
    ms = []
    for _ in range(TIMED):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_job_bench.txt"))
    ap.add_argument("--pairs", default="1,16,128")
    ap.add_argument("--size", default="1024x436")
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    counts = [int(v) for v in a.pairs.split(",")]
    ctx = sfa.Context(0)
    pairs = make_pairs(w, h, max(counts))
    lines = [f"tools/bench_pairs.py: two-frame refinement, {w} x {h}, default parameters (5 outer x 1 inner x 30 sweeps); ms per call, host clock, "
             f"{WARMUP} warm-up + {TIMED} timed calls: median [min .. max]",
             "(a) variational_2frame_batch on host planes, copies and wait included   (b) resident PairJob, SFA_PAIR_UNFUSED=1   (c) resident PairJob, fused",
             f"{'pairs':>5} {'(a) ms':>28} {'(b) ms':>28} {'(c) ms':>28} {'a/c':>7} {'b/c':>7} {'(c) MB resident':>16}"]
    print("\n".join(lines), flush=True)
    for n in counts:
        sel = pairs[:n]
        wxs, wys = [p[2].copy() for p in sel], [p[3].copy() for p in sel]
        ta = timed(lambda: ctx.variational_2frame_batch(wxs, wys, [p[0] for p in sel], [p[1] for p in sel], w))
        job = sfa.PairJob(ctx, w, h, n)
        for b, (im1, im2, wx, wy) in enumerate(sel):
            job.upload(b, wx, wy, im1, im2)

        def run():
            job.run()
            ctx.sync()
        sfa.debug_set("SFA_PAIR_UNFUSED", 1)
        tb = timed(run)
        sfa.debug_set("SFA_PAIR_UNFUSED", None)
        tc = timed(run)
        job.close()
        resident = 24.0 * n * ((w + 63) // 64 * 64) * h * 4 / 1e6
        fmt = lambda t: f"{t[0]:10.2f} [{t[1]:7.2f} .. {t[2]:7.2f}]"
        line = f"{n:>5} {fmt(ta):>28} {fmt(tb):>28} {fmt(tc):>28} {ta[0] / tc[0]:7.2f} {tb[0] / tc[0]:7.2f} {resident:16.0f}"
        print(line, flush=True)
        lines.append(line)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
