#!/usr/bin/env python3
"""dense_tracking's EpicFlow fill-in of one start_jet, measured on one GPU: the library's fill calls and epic_fill_rate against the plain chain on the host
(tests/host/epic_fill_tool.cpp), and bench.py's headline figure for two builds of the library, alternating.

    python tools/bench_epic_fill.py [--size 1024 436] [--rates 16 32] [--epic-skip 2] [--reps 3] [--program | --program-only]
                                    [--parent-program PATH [--group 4]] [--parent-lib PATH [--steps 10 --warmup 2]] [--out FILE]

--parent-program (with --program-only): an `accumulate` built from the parent commit, beside its own library.  Its `-fill` and this tree's run alternately
on the same tree (wall clock of the whole process and run.json's timings_s; their output files are compared byte for byte), and this tree's `-fill` runs
--group start_jets with acc_gpu_batch 1 and with acc_gpu_batch --group, alternately.

Per repetition the tool runs, rate by rate, the host's region growing, sfa_consistent_regions, the chain (one epic() per step) and epic_fill_rate (one
epic_batch per rate) on the same inputs, so the two sides of every comparison alternate within a run; the table gives medians with the spread and every
sample.  Times are wall-clock milliseconds of the calls, copies included (each call takes host memory and waits).  The first repetition is a warm-up and
is not counted."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def build_tool(d):
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = os.path.join(d, "epic_fill_tool")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-pthread", "-I", HOST, os.path.join(ROOT, "tests", "host", "epic_fill_tool.cpp"), os.path.join(HOST, "libslowflow_host.a"),
                        "-L", os.path.join(ROOT, "slowflow_amd"), "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "slowflow_amd"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def trajectories(w, h, J, seed):
    """a piecewise-affine motion growing with the step; tracked == J except in blocks of 32 x 32 (a quarter of them) and 5 % of salt"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    right = xx > w * 0.55
    u = np.where(right, 3.0 + 0.002 * (xx - w / 2), -1.5 + 0.001 * yy)
    v = np.where(right, -2.0 + 0.0015 * yy, 0.5 - 0.001 * (xx - 10))
    acc_u = np.stack([(j + 1) / J * u + rng.normal(0, 0.05, (h, w)) for j in range(J)])
    acc_v = np.stack([(j + 1) / J * v + rng.normal(0, 0.05, (h, w)) for j in range(J)])
    blocks = rng.random(((h + 31) // 32, (w + 31) // 32)) < 0.25
    lost = np.kron(blocks, np.ones((32, 32), bool))[:h, :w] | (rng.random((h, w)) < 0.05)
    tracked = np.where(lost, rng.integers(0, J, (h, w)), J).astype(np.int32)
    return acc_u, acc_v, tracked


def make_tree(a, d, w, h, starts=1):
    """the jets and frames of `starts` start_jets under d: rates of a.rates steps (the last one is acc_min_fps, Jets = its steps), corrupted blocks that no
    rate tracks.  -> (fps, the first frame of every start_jet)"""
    import struct
    from synth import texture_frame
    from test_accumulate import smooth_flows
    lo, hi = a.rates
    assert hi % lo == 0 and hi <= 32, "--program: two rates, the second a multiple of the first and at most 32 steps"
    rng = np.random.default_rng(3)
    fps = {"low": 25 * 2 * lo, "high": 25 * 2 * hi}
    first = [10 + 2 * hi * j for j in range(starts)]
    for name, FF in (("low", lo), ("high", hi)):
        os.makedirs(os.path.join(d, name))
        with open(os.path.join(d, name, "config.cfg"), "w") as f:
            f.write("slow_flow_S\t3\njet_fps\t%d\n" % fps[name])
        step = 2 * (hi // FF)
        for base in first:
            fu, fv, _, _ = smooth_flows(rng, FF, h, w, 0.8)
            bu = -fu + (rng.standard_normal(fu.shape) * 0.05).astype(np.float32)
            bv = -fv
            blocks = np.kron(rng.random(((h + 31) // 32, (w + 31) // 32)) < 0.25, np.ones((32, 32), bool))[:h, :w]
            bu[:, blocks] += np.float32(5)                                   # no rate tracks a quarter of the 32 x 32 blocks: the holes -fill closes
            for k in range(FF):
                for path, u, v in ((os.path.join(d, name, "frame_%d.flo" % (base + k * step)), fu[k], fv[k]),
                                   (os.path.join(d, name, "frame_%d_back.flo" % (base + (k + 1) * step)), bu[k], bv[k])):
                    with open(path, "wb") as f:
                        f.write(struct.pack("<fii", 202021.25, w, h))
                        f.write(np.stack([u, v], -1).astype("<f4").tobytes())
    os.makedirs(os.path.join(d, "seq"))
    for k in range(starts * hi + 1):
        rgb = np.clip(np.rint(texture_frame(w, h, k)[:, :, :w]), 0, 255).astype(np.uint8)
        with open(os.path.join(d, "seq", "frame_%d.ppm" % (10 + 2 * k)), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (w, h))
            f.write(np.ascontiguousarray(rgb.transpose(1, 2, 0)).tobytes())
    return fps, first


def write_cfg(a, d, out, fps, starts=1, extra=()):
    cfg = os.path.join(d, "run.cfg")
    with open(cfg, "w") as f:
        f.write("\n".join(["jet_estimation\t%s/low/" % d, "jet_estimation\t%s/high/" % d, "flow_format\tframe_%i", "output\t%s" % out, "start\t10",
                           "file\t%s/seq/frame_%%i.ppm" % d, "ref_fps\t25", "ref_fps_F\t%d" % starts, "max_fps\t%d" % fps["high"], "acc_min_fps\t1",
                           "acc_skip_pixel\t0", "acc_discard_inconsistent\t0", "acc_consistency_threshold\t0.5", "acc_epic_skip\t%g" % a.epic_skip] + list(extra)) + "\n")
    return cfg


class Lines(list):
    """the report's lines; each is printed, and appended to the --out file, as soon as it exists, so that a run that is cut short leaves what it measured"""
    def __init__(self, out=None):
        super().__init__()
        self.out = out
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            open(out, "w").close()

    def append(self, line):
        super().append(line)
        print(line, flush=True)
        if self.out:
            with open(self.out, "a") as f:
                f.write(line + "\n")


def progress(*what):
    print("[bench_epic_fill]", *what, file=sys.stderr, flush=True)


def run_fill(program, a, d, out, fps, first, edges, extra=()):
    """one `accumulate -fill -resume` into a fresh `out`: (seconds of the whole process, run.json, {relative name: bytes} of every output but run.json)"""
    os.makedirs(os.path.join(out, "accumulated", "tmp"))
    for start in first:
        edges.tofile(os.path.join(out, "accumulated", "tmp", "edges_%d.dat" % start))
    cfg = write_cfg(a, d, out, fps, len(first), extra)
    t0 = time.perf_counter()
    r = subprocess.run([program, cfg, "-fill", "-resume"], capture_output=True, text=True, timeout=a.run_timeout)
    t = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    progress(program, " ".join(extra), "%.2f s" % t)
    acc = os.path.join(out, "accumulated")
    files = {}
    for base, _, names in os.walk(acc):
        for n in names:
            if n != "run.json" and os.path.basename(base) != "tmp":
                files[os.path.relpath(os.path.join(base, n), acc)] = open(os.path.join(base, n), "rb").read()
    return t, json.load(open(os.path.join(acc, "run.json"))), files


def parent_program_bench(a, w, h, lines):
    """the parent's `accumulate -fill` against this tree's on one start_jet, alternating; then this tree's on a.group start_jets, one per run and all in one"""
    import shutil
    program = os.path.join(HOST, "accumulate")
    edges = np.random.default_rng(40).uniform(0.01, 0.5, (h, w)).astype(np.float32)
    lo, hi = a.rates
    with tempfile.TemporaryDirectory() as d:
        fps, first = make_tree(a, d, w, h, 1)
        progress("tree of 1 start_jet written")
        times, inner, files = {"parent": [], "change": []}, {"parent": [], "change": []}, {}
        for rep in range(a.reps + 1):
            for side, exe in (("parent", a.parent_program), ("change", program)):
                out = os.path.join(d, "out_%s_%d" % (side, rep))
                t, run, files[side] = run_fill(exe, a, d, out, fps, first, edges)
                shutil.rmtree(out)
                if rep:
                    times[side].append(t)
                    inner[side].append(run["timings_s"])
            assert sorted(files["parent"]) == sorted(files["change"]) and all(files["parent"][k] == files["change"][k] for k in files["parent"]), "outputs differ"
        lines.append("accumulate -fill on one start_jet of %d x %d, rates of %d and %d steps, Jets %d, acc_skip_pixel 0, acc_epic_skip %g; seconds of the whole process,"
                     % (w, h, lo, hi, hi, a.epic_skip))
        lines.append("%d alternating repetitions after a warm-up; the %d output files of the two are equal byte for byte in every repetition" % (a.reps, len(files["change"])))
        lines.append("  parent (the stage calls, start_jet by start_jet) : " + med(times["parent"]))
        lines.append("  change (the track job that fills in)           : " + med(times["change"]))
        spread = max(times["parent"]) - min(times["parent"])
        over = statistics.median(times["change"]) - statistics.median(times["parent"])
        lines.append("  change's median - parent's median = %+.2f s; the parent's own spread is %.2f s: %s" % (over, spread, "no regression" if over <= spread else "REGRESSION"))
        for key in ("frames", "accumulate", "epic_fill", "energy_call", "fuse", "write", "total"):
            for side in ("parent", "change"):
                lines.append("    %s, run.json timings_s[%-11s] : " % (side, key) + med([t[key] for t in inner[side]]))
        lines.append("    (the parent's timings_s are host wall clock around its calls, copies included; the change's accumulate, epic_fill, energy_call and fuse are")
        lines.append("     the job's HIP events, and epic_fill includes the interpolation's host reads)")
    with tempfile.TemporaryDirectory() as d:
        fps, first = make_tree(a, d, w, h, a.group)
        progress("tree of %d start_jets written" % a.group)
        times, inner, files = {1: [], a.group: []}, {1: [], a.group: []}, {}
        for rep in range(a.reps + 1):
            for batch in (1, a.group):
                out = os.path.join(d, "out_%d_%d" % (batch, rep))
                t, run, files[batch] = run_fill(program, a, d, out, fps, first, edges, ["acc_gpu_batch\t%d" % batch])
                shutil.rmtree(out)
                assert run["fill_path"] == "track_job" and run["gpu_batch"] == batch
                if rep:
                    times[batch].append(t)
                    inner[batch].append(run["timings_s"])
            assert all(files[1][k] == files[a.group][k] for k in files[1]), "outputs differ between the group sizes"
        lines.append("this tree's accumulate -fill on %d start_jets of that size; seconds of the whole process, %d alternating repetitions after a warm-up; equal output files"
                     % (a.group, a.reps))
        for batch in (1, a.group):
            lines.append("  acc_gpu_batch %-2d : " % batch + med(times[batch]))
            for key in ("epic_fill", "energy_call", "fuse"):
                lines.append("    run.json timings_s[%-11s] : " % key + med([t[key] for t in inner[batch]]))


def program_bench(a, w, h, lines):
    """`accumulate -fill` against `accumulate -fuse` on one start_jet of the same synthetic tree, alternating: rates of a.rates steps (the last one is
    acc_min_fps, Jets = its steps), acc_skip_pixel 0, corrupted blocks that no rate tracks"""
    program = os.path.join(HOST, "accumulate")
    lo, hi = a.rates
    with tempfile.TemporaryDirectory() as d:
        fps, _ = make_tree(a, d, w, h)
        edges = np.random.default_rng(40).uniform(0.01, 0.5, (h, w)).astype(np.float32)
        times = {"-fuse": [], "-fill": []}
        inner = {"-fuse": [], "-fill": []}
        holes = {}
        for rep in range(a.reps + 1):
            for flag in ("-fuse", "-fill"):
                out = os.path.join(d, "out_%s_%d" % (flag[1:], rep))
                os.makedirs(os.path.join(out, "accumulated", "tmp"))
                edges.tofile(os.path.join(out, "accumulated", "tmp", "edges_10.dat"))
                cfg = write_cfg(a, d, out, fps)
                t0 = time.perf_counter()
                r = subprocess.run([program, cfg, flag, "-resume"], capture_output=True, text=True, timeout=3000)
                t = time.perf_counter() - t0
                assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
                run = json.load(open(os.path.join(out, "accumulated", "run.json")))
                uv = np.fromfile(os.path.join(out, "accumulated", "frame_10.flo"), "<f4")[3:]
                holes[flag] = int((np.abs(uv[0::2]) > 1e9).sum())
                if rep:
                    times[flag].append(t)
                    inner[flag].append(run["timings_s"])
                last = run
        lines.append("accumulate on one start_jet of %d x %d, rates of %d and %d steps, Jets %d, acc_skip_pixel 0, acc_epic_skip %g; seconds, %d alternating repetitions after a warm-up"
                     % (w, h, lo, hi, hi, a.epic_skip, a.reps))
        lines.append("  -fuse (2 slots, the track job)  : " + med(times["-fuse"]) + "   pixels left UNKNOWN_FLOW: %d" % holes["-fuse"])
        lines.append("  -fill (4 slots, the fill job)    : " + med(times["-fill"]) + "   pixels left UNKNOWN_FLOW: %d" % holes["-fill"])
        for key in ("frames", "accumulate", "epic_fill", "energy_call", "fuse", "write"):
            lines.append("    -fill, run.json timings_s[%-11s] : " % key + med([t[key] for t in inner["-fill"]]))
        lines.append("    -fuse, run.json timings_s[fuse       ] : " + med([t["fuse"] for t in inner["-fuse"]]))
        lines.append("    -fill's fill-in per rate: " + ", ".join("rate %d kept %d matches %d filled %s" % (f["rate"], f["kept_pixels"], f["matches"], f["filled"]) for f in last["fill"]))


def bench_py(a, lines):
    """bench.py's headline figure with the parent's library (SFA_LIB) and with this tree's, alternating"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)]
    vals = {"parent": [], "change": []}
    for rep in range(a.reps):
        for side in ("parent", "change"):
            env = dict(os.environ)
            if side == "parent":
                env["SFA_LIB"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("SFA_LIB", None)
            r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=1500)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            out = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and '"value"' in l]
            vals[side].append(float(out[-1]["value"]))
            progress("bench.py", side, vals[side][-1])
    lines.append("bench.py --gpus 1 --steps %d --warmup %d, the parent's library and this tree's, alternating (%s):" % (a.steps, a.warmup, out[-1]["unit"]))
    for side in ("parent", "change"):
        lines.append("  %-6s : " % side + med(vals[side]))


def med(xs):
    return "median %8.2f (%.2f .. %.2f)  [%s]" % (statistics.median(xs), min(xs), max(xs), " ".join("%.2f" % x for x in xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=(1024, 436))
    ap.add_argument("--rates", type=int, nargs="+", default=(16, 32))
    ap.add_argument("--epic-skip", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit's library: bench.py runs with it and with the tree's, alternating")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--program", action="store_true", help="also run the accumulate program with -fuse and with -fill on one synthetic start_jet")
    ap.add_argument("--program-only", action="store_true", help="only that")
    ap.add_argument("--parent-program", default=None, help="the parent commit's accumulate (beside its own library): its -fill and this tree's alternate")
    ap.add_argument("--run-timeout", type=float, default=600, help="seconds one run of the program may take (with --parent-program)")
    ap.add_argument("--group", type=int, default=4, help="the start_jets of the group run (with --parent-program)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = a.size
    from test_epic import scene
    import slowflow_amd as sfa
    lines = ["EpicFlow fill-in of one start_jet: %d x %d, rates of %s steps, acc_epic_skip %g, acc_skip_pixel 0; wall-clock ms of the calls, %d repetitions after a warm-up"
             % (w, h, " and ".join(str(J) for J in a.rates), a.epic_skip, a.reps)]
    if a.program_only:
        lines = Lines(a.out)
    with tempfile.TemporaryDirectory() as d:
        if a.program_only:
            build_tool(d)                                                    # (make -C host)
            if a.parent_program:
                parent_program_bench(a, w, h, lines)
            else:
                program_bench(a, w, h, lines)
            if a.parent_lib:
                bench_py(a, lines)
            return
        exe = build_tool(d)
        rgb, _, _ = scene(w, h, 0)
        rgb.tofile(os.path.join(d, "rgb.bin"))
        np.random.default_rng(40).uniform(0.01, 0.5, (h, w)).astype(np.float32).tofile(os.path.join(d, "edges.bin"))
        inputs = [trajectories(w, h, J, 10 + J) for J in a.rates]
        for r, (au, av, tr) in enumerate(inputs):
            au.tofile(os.path.join(d, "acc_u_%d.bin" % r)); av.tofile(os.path.join(d, "acc_v_%d.bin" % r)); tr.tofile(os.path.join(d, "tracked_%d.bin" % r))
        ms = {}
        info = {}
        for rep in range(a.reps + 1):
            r = subprocess.run([exe, d, str(w), str(h), "0", repr(a.epic_skip), "0.001"] + [str(J) for J in a.rates], capture_output=True, text=True, timeout=3000)
            assert r.returncode == 0, r.stdout + r.stderr
            for k, g, rg, c, f in re.findall(r"^ms (\d+) grow (\S+) regions (\S+) chain (\S+) fill (\S+)$", r.stdout, flags=re.M):
                if rep:
                    for name, v in (("grow", g), ("regions", rg), ("chain", c), ("fill", f)):
                        ms.setdefault((int(k), name), []).append(float(v))
            for m in re.findall(r"^rate (\d+) chain (\d) (\d+) (\d+) fill (\d) (\d+) (\d+) index (\d+)$", r.stdout, flags=re.M):
                info[int(m[0])] = m
            for k, J in enumerate(a.rates):                                  # the two sides computed the same thing in this very run
                for name in ("u", "v"):
                    x, y = (np.fromfile(os.path.join(d, "%s_%s_%d.bin" % (side, name, k)), np.uint64) for side in ("chain", "fill"))
                    assert np.array_equal(x, y), "rate %d: epic_fill_rate and the chain differ" % k
        for k, J in enumerate(a.rates):
            m = info[k]
            lines.append("rate %d, %d steps: %s kept pixels, %s matches per step, filled %s; fill-in trajectories equal the chain's bit for bit" % (k, J, m[5], m[6], m[4]))
            g, rg, c, f = (ms[(k, n)] for n in ("grow", "regions", "chain", "fill"))
            lines.append("  region growing on the host (C++)        : " + med(g))
            lines.append("  sfa_consistent_regions (1 map)          : " + med(rg) + "   host / GPU = %.2f%s"
                         % (statistics.median(g) / statistics.median(rg), "" if statistics.median(rg) <= statistics.median(g) else "   SLOWER than the host"))
            lines.append("  chain: %2d x epic(), one by one          : " % J + med(c))
            lines.append("  epic_fill_rate: one epic_batch of %2d    : " % J + med(f) + "   chain / fill = %.2f%s"
                         % (statistics.median(c) / statistics.median(f), "" if statistics.median(f) <= statistics.median(c) else "   SLOWER than the chain"))
        # the library calls from Python: all rates' maps in one sfa_consistent_regions, and the matches call per rate
        ctx = sfa.Context(0)
        tracked = np.stack([t for _, _, t in inputs])
        xs, ys = sfa.fill_samples(w, a.epic_skip), sfa.fill_samples(h, a.epic_skip)
        t_reg, t_match = [], {k: [] for k in range(len(a.rates))}
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            mask, kept = ctx.consistent_regions(tracked, list(a.rates), 100)
            t = (time.perf_counter() - t0) * 1e3
            if rep:
                t_reg.append(t)
            for k, (au, av, _) in enumerate(inputs):
                t0 = time.perf_counter()
                ctx.fill_matches(au[None], av[None], mask[k:k + 1], xs, ys, 1)
                t = (time.perf_counter() - t0) * 1e3
                if rep:
                    t_match[k].append(t)
        lines.append("sfa_consistent_regions, the %d maps in one call : " % len(a.rates) + med(t_reg))
        for k, J in enumerate(a.rates):
            lines.append("sfa_fill_matches, rate %d (%2d steps, %d x %d samples; the call uploads %d MB of trajectories) : " % (k, J, len(xs), len(ys), 2 * J * w * h * 8 >> 20)
                         + med(t_match[k]))
        ctx.close()
    if a.program:
        program_bench(a, w, h, lines)
    if a.parent_lib:
        bench_py(a, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
