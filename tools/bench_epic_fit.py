#!/usr/bin/env python3
"""EpicFlow's model fit and dense application, host code against the batched GPU call, and epic_batch as a whole, on the same machine in the same run.
  scene: 1024 x 436, 5000 seeds, the synthetic scene of tests/test_epic.py::scene (every image of a batch its own random seed); the lists are the GPU
  search's (Context.epic_nearest_seeds), the weights exp(-0.8 d) + 1e-8
  (h): host/epic.cpp, one thread, g++ -O2 (libslowflow_host.a), timed inside tests/host/epic_fit_tool.cpp (`fit` mode with repetitions) on image 0: kernel()'s
       expf loop, epic_fit_localaffine / epic_fit_nadarayawatson, epic()'s apply loop
  (g): Context.epic_interpolate = sfa_epic_interpolate_batch at batch 1, 16 and 128: wall time of the call (uploads, kernels, downloads) divided by the batch
       = per image; beside it the fit and apply kernels' own time from HIP events (sfa_epic_fit_stage_ms), and the fit kernel's time in its plain form
       (SFA_EPIC_FIT_PLAIN=1: every lane reads its row of the lists from global memory, no LDS tiles)
  (e): epic_batch (LA and NW, no saliency filter, pref_nn 25, nn 160) per image, wall time inside the tool's `epic` mode, on this tree and -- with --parent DIR, a
       built checkout of the parent commit -- on the parent's libraries, where fit and application run on the host
  LA at nn 160 (the driver's interpolation) and NW at nn 26.
Three repetitions after one warm-up per setting; every value is printed, with the median and the spread (min .. max).  Clocks and power are the machine's
own at the time (no pinning): compare lines of one run only.  Batch 1 is compared with the host bit for bit before anything is timed.

usage: tools/bench_epic_fit.py [--width 1024] [--height 436] [--seeds 5000] [--batches 1,16,128] [--reps 3] [--parent DIR] [--out profiles/epic_fit_bench.txt]"""
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
from test_epic import scene, stride_of  # noqa: E402

SETTINGS = (("LA", 160), ("NW", 26))


def build_tool(root, folder, name, flags=()):
    """tests/host/epic_fit_tool.cpp of THIS tree against the host library and the GPU library of the tree at `root`"""
    host = os.path.join(root, "slowflow_amd", "host")
    if not os.path.exists(os.path.join(host, "libslowflow_host.a")):
        r = subprocess.run(["make", "-C", host, "libslowflow_host.a"], capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(r.stdout + r.stderr)
    exe = os.path.join(folder, name)
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-pthread", *flags, "-I", host, os.path.join(ROOT, "tests", "host", "epic_fit_tool.cpp"), os.path.join(host, "libslowflow_host.a"),
                        "-L", os.path.join(root, "slowflow_amd"), "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(root, "slowflow_amd"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    return exe


def spread(v):
    return "median %.2f (%.2f .. %.2f)" % (statistics.median(v), min(v), max(v))


def values(stdout, key):
    for line in stdout.splitlines():
        if line.startswith(key + " "):
            return [float(x) for x in line.split()[1:]]
    raise SystemExit("no %s line in:\n%s" % (key, stdout))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--seeds", type=int, default=5000)
    ap.add_argument("--batches", default="1,16,128")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its libraries built: epic_batch is timed on it too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epic_fit_bench.txt"))
    a = ap.parse_args()
    w, h = a.width, a.height
    batches = [int(x) for x in a.batches.split(",")]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    folder = tempfile.mkdtemp(prefix="bench_epic_fit_")
    exe = build_tool(ROOT, folder, "epic_fit_tool")
    nmax = max(batches)
    lim = np.array([w - 1, h - 1, w - 1, h - 1], np.float32)
    costs, seeds, vects = [], [], []
    with open(os.path.join(folder, "sizes.txt"), "w") as sizes:
        for k in range(nmax):                                         # the scenes, written for the `epic` mode as they are made
            rgb, edges, m = scene(w, h, 100 + k, n_matches=a.seeds, outliers=0)
            sizes.write("%d %d\n" % (w, h))
            rgb.tofile(os.path.join(folder, "rgb_%d.bin" % k))
            edges.tofile(os.path.join(folder, "edges_%d.bin" % k))
            np.savetxt(os.path.join(folder, "matches_%d.txt" % k), m, fmt="%.9g")
            mc = np.clip(m, 0, lim)
            costs.append(edges + np.float32(0.001))
            seeds.append(np.ascontiguousarray(mc[:, :2].astype(np.int32)))
            vects.append(np.ascontiguousarray(mc[:, 2:4] - mc[:, 0:2], np.float32))
    assert rgb.shape == (3, h, stride_of(w))
    ctx = sfa.Context(0)
    say("EpicFlow fit and dense application: %d x %d, %d seeds per image; ms per image, %d repetitions after a warm-up" % (w, h, a.seeds, a.reps))
    for method, nn in SETTINGS:
        tag = "%s nn %3d" % (method, nn)
        labels, index, dist = ctx.epic_nearest_seeds(costs, seeds, nn)
        with np.errstate(under="ignore"):
            weight = [(np.exp(np.float32(-0.8) * d) + np.float32(1e-8)).astype(np.float32) for d in dist]
        for name, arr in (("labels", labels[0]), ("seeds", seeds[0]), ("vects", vects[0]), ("index", index[0]), ("weight", weight[0]), ("dist", dist[0])):
            arr.tofile(os.path.join(folder, name + ".bin"))
        r = subprocess.run([exe, "fit", folder, str(w), str(h), str(a.seeds), str(nn), method, str(w), str(a.reps + 1)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stdout + r.stderr)
        host = {k: values(r.stdout, k + "_ms")[1:] for k in ("expf", "fit", "apply")}          # the first round is the warm-up
        for k in ("expf", "fit", "apply"):
            say("%s  (h) host %-5s, one thread       : %s   [%s]" % (tag, k, spread(host[k]), " ".join("%.2f" % x for x in host[k])))
        host_stage = statistics.median(host["fit"]) + statistics.median(host["apply"])
        want = [np.fromfile(os.path.join(folder, n + ".bin"), np.uint32) for n in ("fx", "fy", "model")]
        got = ctx.epic_interpolate(labels[:1], seeds[:1], vects[:1], index[:1], weight[:1], method=method)
        same = all(np.array_equal(g[0].view(np.uint32).ravel(), x) for g, x in zip(got, want))
        say("%s  batch 1 equals the host bit for bit: %s" % (tag, same))
        if not same:
            raise SystemExit("the GPU's models or flows differ from the host's")
        for nb in batches:
            args = (labels[:nb], seeds[:nb], vects[:nb], index[:nb], weight[:nb])
            wall, stage, plain = [], [], []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                ctx.epic_interpolate(*args, method=method)
                wall.append((time.perf_counter() - t0) * 1e3 / nb)
                stage.append(ctx.epic_fit_stage_ms())
            sfa.debug_set("SFA_EPIC_FIT_PLAIN", 1)
            for rep in range(a.reps + 1):
                ctx.epic_interpolate(*args, method=method)
                plain.append(ctx.epic_fit_stage_ms()["fit"] / nb)
            sfa.debug_set("SFA_EPIC_FIT_PLAIN", None)
            wall, stage, plain = wall[1:], stage[1:], plain[1:]
            med = statistics.median(wall)
            say("%s  (g) GPU, batch %3d              : %s   [%s]   host fit + apply / GPU = %.2f%s" % (
                tag, nb, spread(wall), " ".join("%.2f" % x for x in wall), host_stage / med, "   SLOWER per image than the host's fit + apply" if med > host_stage else ""))
            say("           kernels per image (events) : fit %.3f, apply %.3f; the fit in its plain form (no LDS tiles) %.3f" % (
                statistics.median([s["fit"] for s in stage]) / nb, statistics.median([s["apply"] for s in stage]) / nb, statistics.median(plain)))
    ctx.close()
    trees = [("this tree", exe)]
    if a.parent:
        trees.append(("parent   ", build_tool(os.path.abspath(a.parent), folder, "epic_fit_tool_parent", flags=("-DEPIC_FIT_TOOL_EPIC_ONLY",))))
    for method in ("LA", "NW"):
        for nb in batches:
            for name, tool in trees:
                r = subprocess.run([tool, "epic", folder, str(nb), method, "0.0", "25", "5.0", "160", "0.8", "0.001", "0", str(a.reps + 1)], capture_output=True, text=True,
                                   timeout=1800)
                if r.returncode != 0:
                    raise SystemExit(r.stdout + r.stderr)
                t = [x / nb for x in values(r.stdout, "batch_ms")[1:]]
                say("%s nn 160  (e) epic_batch, batch %3d, %s : %s   [%s]" % (method, nb, name, spread(t), " ".join("%.2f" % x for x in t)))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
