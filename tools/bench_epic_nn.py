#!/usr/bin/env python3
"""EpicFlow's geodesic k nearest seeds, host function against the batched GPU call, on the same machine in the same run.
  scene: 1024 x 436, 5000 seeds, the synthetic cost map of tests/test_epic.py::scene (every image of a batch its own random seed); --grid-skip S puts the
         seeds on the fill-in's sample grid instead (sfa_fill_samples of acc_epic_skip S in both directions: 512 x 218 = 111 616 seeds for S = 2)
  (h): host/epic.cpp epic_nearest_seeds, one thread, g++ -O2 (libslowflow_host.a), timed inside tests/host/epic_nn_tool.cpp (`time` mode), per call; skipped
       above --host-max-seeds seeds, where one call takes minutes
  (g): Context.epic_nearest_seeds = sfa_epic_nearest_seeds_batch at batch 1, 16 and 128: wall time of the call (uploads, kernels, the waits between its
       stages, downloads) divided by the batch = per image; beside it the kernels' own time by group from HIP events (sfa_epic_nn_stage_ms) and, per call,
       the slices, forms and workspace of the search (sfa_epic_nn_search_info)
  nn 26 (the consistency filter's pref_nn + 1) and nn 160 (the driver's interpolation).
--search picks the context's mode: dense (the default mode), compact, or both after each other.  --variants lists them in full instead, each
`default` or `compact[/dense|/sparse][/<seeds per slice>]` (the switches SFA_EPIC_NN_SET and SFA_EPIC_NN_SLICE).  The outputs of every variant are compared bit
for bit with the first variant's (and that one with the host's, where the host runs); a SHA-1 of all outputs of a call is printed, so that runs of different
builds (SFA_LIB) can be compared.
Three repetitions after one warm-up call per setting; every value is printed, with the median and the spread (min .. max).  Clocks and power are the
machine's own at the time (no pinning): compare the rows of one run only.

usage: tools/bench_epic_nn.py [--width 1024] [--height 436] [--seeds 5000 | --grid-skip S] [--batches 1,16,128] [--nns 26,160] [--reps 3]
                              [--search dense|compact|both] [--variants LIST] [--host-max-seeds 20000] [--workspace BYTES] [--out profiles/epic_nn_bench.txt]"""
import argparse
import hashlib
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


def image(w, h, seeds, k, grid_skip):
    _, edges, m = scene(w, h, 100 + k, n_matches=16 if grid_skip else seeds, outliers=0)
    cost = edges + np.float32(0.001)
    if grid_skip:                                                     # the fill-in's samples: every grid point a seed
        xs, ys = sfa.fill_samples(w, grid_skip), sfa.fill_samples(h, grid_skip)
        return cost, np.ascontiguousarray(np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2).astype(np.int32))
    x = np.clip(m[:, 0], 0, np.float32(w - 1)).astype(np.int32)
    y = np.clip(m[:, 1], 0, np.float32(h - 1)).astype(np.int32)
    return cost, np.ascontiguousarray(np.stack([x, y], 1))


def spread(v):
    return "median %.2f (%.2f .. %.2f)" % (statistics.median(v), min(v), max(v))


class Variant:
    """`default`, or `compact[/dense|/sparse][/<seeds per slice>]`"""

    def __init__(self, spec):
        parts = spec.split("/")
        if parts[0] not in ("default", "compact") or (parts[0] == "default" and len(parts) > 1):
            raise SystemExit("variant %r: default, or compact[/dense|/sparse][/<seeds per slice>]" % spec)
        self.spec, self.mode, self.form, self.slice = spec, "dense" if parts[0] == "default" else "compact", None, None
        for p in parts[1:]:
            if p in ("dense", "sparse"):
                self.form = p
            else:
                self.slice = int(p)

    def apply(self, ctx):
        if self.mode == "compact" or hasattr(sfa.lib(), "sfa_ctx_set_epic_search"):      # (an SFA_LIB build from before the compact search has the default mode only)
            ctx.set_epic_search(self.mode)
        if self.mode == "compact":
            sfa.debug_set("SFA_EPIC_NN_SET", self.form)
            sfa.debug_set("SFA_EPIC_NN_SLICE", self.slice)


def digest(out):
    s = hashlib.sha1()
    for group in out:
        for a in group:
            s.update(np.ascontiguousarray(a).tobytes())
    return s.hexdigest()[:16]


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for ga, gb in zip(a, b) for x, y in zip(ga, gb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--seeds", type=int, default=5000)
    ap.add_argument("--grid-skip", type=float, default=0)
    ap.add_argument("--batches", default="1,16,128")
    ap.add_argument("--nns", default="26,160")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--search", choices=("dense", "compact", "both"), default="dense")
    ap.add_argument("--variants", default="")
    ap.add_argument("--host-max-seeds", type=int, default=20000)
    ap.add_argument("--workspace", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epic_nn_bench.txt"))
    a = ap.parse_args()
    w, h = a.width, a.height
    batches = [int(x) for x in a.batches.split(",")]
    nns = [int(x) for x in a.nns.split(",")]
    variants = [Variant(v) for v in (a.variants.split(",") if a.variants else {"dense": ["default"], "compact": ["compact"], "both": ["default", "compact"]}[a.search])]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    folder = tempfile.mkdtemp(prefix="bench_epic_nn_")
    images = [image(w, h, a.seeds, k, a.grid_skip) for k in range(max(batches))]
    ns = len(images[0][1])
    with_host = ns <= a.host_max_seeds
    exe = build_tool(folder) if with_host else None
    ctx = sfa.Context(0)
    say("epic_nearest_seeds: %d x %d, %d seeds per image%s; ms per image, %d repetitions after a warm-up; library %s" %
        (w, h, ns, " (the sample grid of acc_epic_skip %g)" % a.grid_skip if a.grid_skip else "", a.reps, os.path.relpath(sfa.LIB_PATH, ROOT)))
    if not with_host:
        say("(h) the host's search is skipped: %d seeds are more than --host-max-seeds %d, one call would take minutes; the variants are compared with each other" % (ns, a.host_max_seeds))
    images[0][0].tofile(os.path.join(folder, "cost.bin"))
    images[0][1].tofile(os.path.join(folder, "seeds.bin"))
    for nn in nns:
        host = None
        if with_host:
            r = subprocess.run([exe, "time", folder, str(w), str(h), str(nn), str(a.reps + 1)], capture_output=True, text=True, timeout=1800)
            if r.returncode != 0:
                raise SystemExit(r.stdout + r.stderr)
            host = [float(x) for x in r.stdout.split()[1:]][1:]                     # the first call is the warm-up
            say("nn %3d  (h) host, one thread          : %s   [%s]" % (nn, spread(host), " ".join("%.2f" % x for x in host)))
            want = [np.fromfile(os.path.join(folder, n), t) for n, t in (("labels.bin", np.int32), ("index.bin", np.int32), ("dist.bin", np.uint32))]
            variants[0].apply(ctx)
            got = ctx.epic_nearest_seeds([images[0][0]], [images[0][1]], nn, workspace_bytes=a.workspace)
            same = (np.array_equal(got[0][0].ravel(), want[0]) and np.array_equal(got[1][0].ravel(), want[1]) and np.array_equal(got[2][0].view(np.uint32).ravel(), want[2]))
            say("nn %3d  %s, batch 1 equals the host bit for bit: %s" % (nn, variants[0].spec, same))
            if not same:
                raise SystemExit("the GPU's lists differ from the host's")
        for nb in batches:
            costs, seeds = [c for c, _ in images[:nb]], [s for _, s in images[:nb]]
            first = None
            for v in variants:
                v.apply(ctx)
                wall, stage, out = [], [], None
                for rep in range(a.reps + 1):
                    t0 = time.perf_counter()
                    out = ctx.epic_nearest_seeds(costs, seeds, nn, workspace_bytes=a.workspace)
                    wall.append((time.perf_counter() - t0) * 1e3 / nb)
                    stage.append(ctx.epic_nn_stage_ms())
                wall, stage = wall[1:], stage[1:]
                med = statistics.median(wall)
                ratio = "" if host is None else "   host / GPU = %.2f%s" % (statistics.median(host) / med, "   SLOWER per image than the host" if med > statistics.median(host) else "")
                say("nn %3d  (g) GPU, batch %3d, %-22s: %s   [%s]%s" % (nn, nb, v.spec, spread(wall), " ".join("%.2f" % x for x in wall), ratio))
                say("          kernels per image (events) : " + ", ".join("%s %.3f" % (k, statistics.median([s[k] for s in stage]) / nb) for k in stage[0]) +
                    "   [search: %s]" % " ".join("%.3f" % (s["search"] / nb) for s in stage))
                info = ctx.epic_nn_search_info() if hasattr(sfa.lib(), "sfa_epic_nn_search_info") else None
                if first is None:
                    first = out
                    equal = "the first variant"
                else:
                    equal = "equals %s bit for bit: %s" % (variants[0].spec, same_bits(out, first))
                say("          outputs sha1 %s, %s%s" % (digest(out), equal, "" if info is None else
                                                          "; slices %(slices)d, images dense %(dense)d / sparse %(sparse)d, largest search workspace %(workspace_bytes)d bytes" % info))
                if first is not out and not same_bits(out, first):
                    raise SystemExit("variant %s differs from %s" % (v.spec, variants[0].spec))
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
