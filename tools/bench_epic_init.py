#!/usr/bin/env python3
"""The initialisation of one batch of windows with deep_matching 1, from the matches and edge maps of the files to the job's initial flow, per window, on two routes
over the same inputs in one process:
  resident  sfa_sequence_rescale (dm_scale != 1) and sfa_sequence_lab of the reference frames, sfa_epic_job (upload, set_lab, run), sfa_job_upload_resident with
            NULL flow planes, sfa_job_set_flow_epic
  parent    what the driver's gpu_epic 1 route did before: per frame the host's blur and resize through sfa_gaussian_blur / sfa_resize_linear_fx (dm_scale != 1)
            and rgb8_to_lab of host/epic.cpp (through a shim compiled here against libslowflow_host.a), sfa_epic_batch on host planes, sfa_resize_linear per plane
            and the fp32 multiplication on the host, sfa_job_upload_resident with the planes
  scene: 1024 x 436 frames, 5000 matches per window (tests/test_epic.py::scene at the interpolation's size), LA nn 160, pref_nn 25, saliency 0.045
  batches 1, 16 and 128; dm_scale 1 and 0.5
Wall clock around each route, ending in a wait for the context's stream (both routes have host work between their GPU calls, so no pair of HIP events spans them);
one warm-up of each route per setting, then `--reps` timed repetitions (half of them, at least 3, from batch 64 on), the routes taking turns; medians and ranges are reported.  Clocks and power are the
machine's own at the time: compare lines of one run only.

usage: tools/bench_epic_init.py [--width 1024] [--height 436] [--matches 5000] [--batches 1,16,128] [--dm 1,0.5] [--reps 5] [--out profiles/epic_init_bench.txt]"""
import argparse
import ctypes as C
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
from test_epic import scene, stride_of  # noqa: E402

SHIM = r"""
#include <cstring>
#include "epic.h"
extern "C" void lab_shim(const float *rgb, int w, int h, int stride, float norm, float *out) {
    color_image_t im;
    im.width = w; im.height = h; im.stride = stride;
    im.c1 = const_cast<float *>(rgb); im.c2 = im.c1 + (size_t)stride * h; im.c3 = im.c2 + (size_t)stride * h;
    color_image_t *lab = rgb8_to_lab(&im, norm);
    memcpy(out, lab->c1, sizeof(float) * 3 * (size_t)stride * h);
    color_image_delete(lab);
}
"""


def build_shim(folder):
    host = os.path.join(ROOT, "slowflow_amd", "host")
    r = subprocess.run(["make", "-C", host, "libslowflow_host.a"], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stdout + r.stderr)
    src, so = os.path.join(folder, "lab_shim.cpp"), os.path.join(folder, "liblab_shim.so")
    open(src, "w").write(SHIM)
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-fPIC", "-shared", "-pthread", "-I", host, src, os.path.join(host, "libslowflow_host.a"), "-L", os.path.join(ROOT, "slowflow_amd"),
                        "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "slowflow_amd"), "-o", so], capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr)
    L = C.CDLL(so)
    L.lab_shim.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]
    L.lab_shim.restype = None
    return L


def spread(v):
    return "median %.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--height", type=int, default=436)
    ap.add_argument("--matches", type=int, default=5000)
    ap.add_argument("--batches", default="1,16,128")
    ap.add_argument("--dm", default="1,0.5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epic_init_bench.txt"))
    a = ap.parse_args()
    if sfa.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without the GPU")
    w, h = a.width, a.height
    st = stride_of(w)
    ctx = sfa.Context(0)
    shim = build_shim(tempfile.mkdtemp(prefix="epic_init_"))
    lines = ["# tools/bench_epic_init.py: %d x %d, %d matches, LA nn 160, pref_nn 25, saliency 0.045; ms per window, wall clock to the stream's end, %d repetitions (batches of 64 and more: see each line)" %
             (w, h, a.matches, a.reps), "# libslowflow_amd.so sha256 " + hashlib.sha256(open(sfa.LIB_PATH, "rb").read()).hexdigest()]
    p = sfa.epic_params(method="LA", saliency_th=0.045, pref_nn=25, nn=160, coef_kernel=1.1, euc=0.001)
    vp = sfa.default_params()
    vp.S = 2; vp.layers = 1
    steps = 1
    for dm in [float(x) for x in a.dm.split(",")]:
        ew, eh = (int(round(w * dm)), int(round(h * dm))) if dm != 1 else (w, h)
        est = stride_of(ew)
        mul = np.float32(np.float32(w // ew) / np.float32(steps))
        for nb in [int(x) for x in a.batches.split(",")]:
            frames = [scene(w, h, 100 + k, n_matches=8, outliers=0)[0] for k in range(nb + 2)]                     # (3, h, st), 0 .. 255, not normalised
            inputs = [scene(ew, eh, 500 + k, n_matches=a.matches, outliers=a.matches // 20)[1:] for k in range(nb)]
            seq, labseq = sfa.Sequence(ctx, w, h, nb + 2), sfa.Sequence(ctx, ew, eh, nb)
            small = sfa.Sequence(ctx, ew, eh, nb) if dm != 1 else None
            for f, fr in enumerate(frames):
                seq.upload(f, fr)
            job, ej = sfa.Job(ctx, vp, w, h, nb), ctx.epic_job(p, ew, eh, nb)
            idx = [[b, b + 1, b + 2] for b in range(nb)]
            ctx.sync()

            def resident():
                if small is not None:
                    small.rescale_from(seq, dm, 0, 1, nb)
                labseq.lab_from(small if small is not None else seq, 1.0, 0, 0 if small is not None else 1, nb)
                for i, (edges, m) in enumerate(inputs):
                    ej.upload(i, m, edges)
                ej.set_lab(labseq, list(range(nb)))
                rc, _ = ej.run()
                for b in range(nb):
                    job.upload_resident(b, seq, idx[b])
                job.set_flow_epic(ej, float(mul), float(mul))
                ctx.sync()
                return rc

            def parent():
                labs = []
                for b in range(nb):
                    fr = frames[b + 1]
                    if dm != 1:
                        sm = np.zeros((3, eh, est), np.float32)
                        for c in range(3):
                            sm[c] = ctx.resize_linear_fx(ctx.gaussian_blur(fr[c], w, float(np.float32(1 / np.sqrt(2 * dm)))), w, dm, dm)[0]
                        fr = sm
                    lab = np.zeros_like(fr)
                    shim.lab_shim(fr.ctypes.data, ew, eh, est, 1.0, lab.ctypes.data)
                    labs.append(lab)
                costs = [e + np.float32(p.euc) for e, _ in inputs]
                fx, fy, rc, _, _ = ctx.epic_batch(labs, costs, [m for _, m in inputs], p, stride=est)
                for b in range(nb):
                    if dm != 1:
                        wx, wy = ctx.resize_linear(fx[b], ew, w, h) * mul, ctx.resize_linear(fy[b], ew, w, h) * mul
                    else:
                        wx, wy = fx[b] * mul, fy[b] * mul
                    job.upload_resident(b, seq, idx[b], np.ascontiguousarray(wx), np.ascontiguousarray(wy))
                ctx.sync()
                return rc

            routes = (("resident", resident), ("parent", parent))
            times = {name: [] for name, _ in routes}
            rcs = {name: fn() for name, fn in routes}                                                 # the warm-up of both
            if rcs["resident"] != rcs["parent"] or any(rcs["resident"]):
                raise SystemExit("the routes disagree or a window has no match left: rc %s against %s" % (rcs["resident"], rcs["parent"]))
            reps = a.reps if nb < 64 else max(3, a.reps // 2)
            for _ in range(reps):
                for name, fn in routes:
                    t0 = time.perf_counter()
                    fn()
                    times[name].append((time.perf_counter() - t0) * 1e3 / nb)
            ratio = statistics.median(times["resident"]) / statistics.median(times["parent"])
            lines.append("dm_scale %-4g batch %-3d  resident %s   parent %s   resident / parent %.2f  (%d repetitions)" %
                         (dm, nb, spread(times["resident"]), spread(times["parent"]), ratio, reps))
            print(lines[-1], flush=True)
            for o in (job, ej, seq, labseq, small):
                if o is not None:
                    o.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
