#!/usr/bin/env python3
"""EpicFlow's geodesic k nearest seeds, host function against the batched GPU call, on the same machine in the same run.
  scene: 1024 x 436, 5000 seeds, the synthetic cost map of tests/test_epic.py::scene (every image of a batch its own random seed)
  (h): host/epic.cpp epic_nearest_seeds, one thread, g++ -O2 (libslowflow_host.a), timed inside tests/host/epic_nn_tool.cpp (`time` mode), per call
  (g): Context.epic_nearest_seeds = sfa_epic_nearest_seeds_batch at batch 1, 16 and 128: wall time of the call (uploads, kernels, the waits between its
       stages, downloads) divided by the batch = per image; beside it the kernels' own time by group from HIP events (sfa_epic_nn_stage_ms)
  nn 26 (the consistency filter's pref_nn + 1) and nn 160 (the driver's interpolation).
Three repetitions after one warm-up call per setting; every value is printed, with the median and the spread (min .. max).  Clocks and power are the
machine's own at the time (no pinning): compare (h) and (g) of one run only.  The outputs of batch 1 are compared with the host's before anything is timed.

usage: tools/bench_epic_nn.py [--width 1024] [--height 436] [--seeds 5000] [--batches 1,16,128] [--nns 26,160] [--reps 3] [--out profiles/epic_nn_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import slowflow_amd as sfa  # noqa: E402
from test_epic import scene  # noqa: E402

HOST = os.path.join(ROOT, "slowflow_amd", "host")


def build_tool(folder):
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stdout + r.stderr)
    exe = os.path.join(folder, "epic_nn_tool")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-pthread", "-I", HOST, os.path.join(ROOT, "tests", "host", "epic_nn_tool.cpp"), os.path.join(HOST, "libslowflow_host.a"),
                        "-L", os.path.join(ROOT, "slowflow_amd"), "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "slowflow_amd"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    return exe


def image(w, h, seeds, k):
    _, edges, m = scene(w, h, 100 + k, n_matches=seeds, outliers=0)
    cost = edges + np.float32(0.001)
    x = np.clip(m[:, 0], 0, np.float32(w - 1)).astype(np.int32)
    y = np.clip(m[:, 1], 0, np.float32(h - 1)).astype(np.int32)
    return cost, np.ascontiguousarray(np.stack([x, y], 1))


def spread(v):
    return "median %.2f (%.2f .. %.2f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--seeds", type=int, default=5000)
    ap.add_argument("--batches", default="1,16,128")
    ap.add_argument("--nns", default="26,160")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epic_nn_bench.txt"))
    a = ap.parse_args()
    w, h = a.width, a.height
    batches = [int(x) for x in a.batches.split(",")]
    nns = [int(x) for x in a.nns.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    folder = tempfile.mkdtemp(prefix="bench_epic_nn_")
    exe = build_tool(folder)
    images = [image(w, h, a.seeds, k) for k in range(max(batches))]
    ctx = sfa.Context(0)
    say("epic_nearest_seeds: %d x %d, %d seeds per image; ms per image, %d repetitions after a warm-up" % (w, h, a.seeds, a.reps))
    images[0][0].tofile(os.path.join(folder, "cost.bin"))
    images[0][1].tofile(os.path.join(folder, "seeds.bin"))
    for nn in nns:
        r = subprocess.run([exe, "time", folder, str(w), str(h), str(nn), str(a.reps + 1)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stdout + r.stderr)
        host = [float(x) for x in r.stdout.split()[1:]][1:]                     # the first call is the warm-up
        say("nn %3d  (h) host, one thread          : %s   [%s]" % (nn, spread(host), " ".join("%.2f" % x for x in host)))
        want = [np.fromfile(os.path.join(folder, n), t) for n, t in (("labels.bin", np.int32), ("index.bin", np.int32), ("dist.bin", np.uint32))]
        got = ctx.epic_nearest_seeds([images[0][0]], [images[0][1]], nn)
        same = (np.array_equal(got[0][0].ravel(), want[0]) and np.array_equal(got[1][0].ravel(), want[1]) and np.array_equal(got[2][0].view(np.uint32).ravel(), want[2]))
        say("nn %3d  batch 1 equals the host bit for bit: %s" % (nn, same))
        if not same:
            raise SystemExit("the GPU's lists differ from the host's")
        for nb in batches:
            costs, seeds = [c for c, _ in images[:nb]], [s for _, s in images[:nb]]
            wall, stage = [], []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                ctx.epic_nearest_seeds(costs, seeds, nn)
                wall.append((time.perf_counter() - t0) * 1e3 / nb)
                stage.append(ctx.epic_nn_stage_ms())
            wall, stage = wall[1:], stage[1:]
            med = statistics.median(wall)
            say("nn %3d  (g) GPU, batch %3d            : %s   [%s]   host / GPU = %.2f%s" % (nn, nb, spread(wall), " ".join("%.2f" % x for x in wall), statistics.median(host) / med,
                                                                                             "   SLOWER per image than the host" if med > statistics.median(host) else ""))
            say("          kernels per image (events) : " + ", ".join("%s %.3f" % (k, statistics.median([s[k] for s in stage]) / nb) for k in stage[0]))
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
