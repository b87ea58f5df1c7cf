#!/usr/bin/env python3
"""epic_batch as a whole -- matches, Lab image and edge costs in, flow fields out -- on this tree, where it goes through sfa_epic_batch (one chain on the GPU),
against epic_batch of the parent commit, where everything between the two graph searches and the fit runs on the host; on the same machine in the same run.
  scene: 1024 x 436, 5000 matches, the synthetic scene of tests/test_epic.py::scene (every image of a batch its own random seed)
  settings: LA nn 160 and NW nn 26, saliency filter on (0.045), pref_nn 25
  batches 1, 16 and 128: wall milliseconds of the call inside tests/host/epic_batch_tool.cpp (`time` mode), divided by the batch = per image
  --parent DIR: a built checkout of the parent commit (its libslowflow_amd.so and libslowflow_host.a); the tool of THIS tree is compiled against it
Each (setting, batch) is run `--reps` times per tree, the trees taking turns (this, parent, this, parent ...), every run a fresh process with one warm-up call
before its timed one; the medians are compared.  Beside them the eight stage times of the chain (HIP events, sfa_epic_batch_stage_ms) of this tree's timed
calls, per image.  Clocks and power are the machine's own at the time (no pinning): compare lines of one run only.

usage: tools/bench_epic_batch.py [--width 1024] [--height 436] [--matches 5000] [--batches 1,16,128] [--reps 3] [--parent DIR] [--out profiles/epic_batch_bench.txt]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_epic import scene, stride_of  # noqa: E402

SETTINGS = (("LA", 160), ("NW", 26))
STAGES = ("saliency", "filters", "nn #1", "weights+estimate", "nn #2", "weights", "fit", "apply")


def build_tool(root, folder, name, flags=()):
    """tests/host/epic_batch_tool.cpp of THIS tree against the host library and the GPU library of the tree at `root`"""
    host = os.path.join(root, "slowflow_amd", "host")
    if not os.path.exists(os.path.join(host, "libslowflow_host.a")):
        r = subprocess.run(["make", "-C", host, "libslowflow_host.a"], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(r.stdout + r.stderr)
    exe = os.path.join(folder, name)
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-pthread", *flags, "-I", host, os.path.join(ROOT, "tests", "host", "epic_batch_tool.cpp"), os.path.join(host, "libslowflow_host.a"),
                        "-L", os.path.join(root, "slowflow_amd"), "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(root, "slowflow_amd"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    return exe


def spread(v):
    return "median %.2f (%.2f .. %.2f)" % (statistics.median(v), min(v), max(v))


def lines_of(stdout, key):
    out = [[float(x) for x in line.split()[1:]] for line in stdout.splitlines() if line.startswith(key + " ")]
    if not out:
        raise SystemExit("no %s line in:\n%s" % (key, stdout))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--matches", type=int, default=5000)
    ap.add_argument("--batches", default="1,16,128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its libraries built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epic_batch_bench.txt"))
    a = ap.parse_args()
    w, h = a.width, a.height
    batches = [int(x) for x in a.batches.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    folder = tempfile.mkdtemp(prefix="bench_epic_batch_")
    trees = [("this tree", build_tool(ROOT, folder, "epic_batch_tool"))]
    if a.parent:
        trees.append(("parent   ", build_tool(os.path.abspath(a.parent), folder, "epic_batch_tool_parent", flags=("-DEPIC_BATCH_TOOL_NO_STAGES",))))
    with open(os.path.join(folder, "sizes.txt"), "w") as sizes:
        for k in range(max(batches)):
            rgb, edges, m = scene(w, h, 100 + k, n_matches=a.matches, outliers=a.matches // 50)
            sizes.write("%d %d\n" % (w, h))
            rgb.tofile(os.path.join(folder, "rgb_%d.bin" % k))
            edges.tofile(os.path.join(folder, "edges_%d.bin" % k))
            m.tofile(os.path.join(folder, "matches_%d.bin" % k))
    assert rgb.shape == (3, h, stride_of(w))
    say("epic_batch, saliency 0.045, pref_nn 25: %d x %d, %d matches per image; wall ms per image, %d runs per tree taking turns, one warm-up call in each" % (
        w, h, a.matches, a.reps))
    for method, nn in SETTINGS:
        for nb in batches:
            wall = {name: [] for name, _ in trees}
            stages = []
            for rep in range(a.reps):
                for name, tool in trees:
                    r = subprocess.run([tool, "time", folder, str(nb), method, "0.045", "25", "5.0", str(nn), "0.8", "0.001", "0", "2"], capture_output=True, text=True,
                                       timeout=1800)
                    if r.returncode != 0:
                        raise SystemExit(r.stdout + r.stderr)
                    wall[name].append(lines_of(r.stdout, "batch_ms")[0][1] / nb)
                    if name == trees[0][0]:
                        stages.append(lines_of(r.stdout, "stage_ms")[1])
            tag = "%s nn %3d, batch %3d" % (method, nn, nb)
            for name, _ in trees:
                say("%s  %s : %s   [%s]" % (tag, name, spread(wall[name]), " ".join("%.2f" % x for x in wall[name])))
            if a.parent:
                t, p = statistics.median(wall[trees[0][0]]), statistics.median(wall[trees[1][0]])
                say("%s  parent / this tree = %.2f%s" % (tag, p / t, "" if t < p else "   NOT FASTER per image than the parent"))
            med = [statistics.median([s[k] for s in stages]) / nb for k in range(8)]
            say("%s  kernels per image (events): %s; sum %.3f" % (tag, ", ".join("%s %.3f" % (n, v) for n, v in zip(STAGES, med)), sum(med)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
