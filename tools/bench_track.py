"""dense_tracking's accumulation, energies and fusion chained: the resident track job (sfa_track_job) against today's staged call sequence with n = 1.

  bench_track.py [--parent-lib FILE] [--out FILE]
      1024 x 436 frames, acc_skip_pixel 1 (a 512 x 218 grid), K 2 rates, Jets 16 with r_Jets 16 and 32, default keys, every grid pixel a hypothesis.
      The job with B = 1, 4 and 16 start_jets: wall time per start_jet from the first upload to the last download (host clock around a synchronise,
      median of 3 after a warm-up) and the job's eight stage times.  The staged sequence (accumulate_consistent_scaled -> hypothesis_energies_scaled
      per rate -> dt_smoothness_weight -> fuse_hypotheses, n = 1) the same way, with the time of its energies and fusion calls alone.
      Each measurement runs in a child process of its own, the staged ones alternating with the job's.  --parent-lib: a build of the parent commit's
      library (the same C-ABI without the track job), loaded by the staged children through SFA_LIB: the baseline, measured three times, each time
      followed by the same sequence on this tree's library, so that the refactored wrappers are compared within the parent's own spread.  Without it
      the staged sequence runs on this tree's library only.  Writes FILE (profiles/track_bench.txt).

  bench_track.py --occlusions [--parent-lib FILE] [--out FILE]
      The same job with use_occlusions (one rectangle of 255 per occlusion image), at B = 1, 4 and 16, wall time per start_jet as above, with the inputs
      (a) as host planes through upload_flows(occ=) and (b) with the flows and the 8-bit occlusion images already in GPU memory (torch tensors, one
      start_jet's repeated B times through a zero segment stride) through upload_flows_device and upload_occlusions_device.  The frames come from the
      host and the results go to the host in both.  Three repetitions that alternate (a) and (b), each measurement a process of its own; after its
      timed runs a child times the uploads alone (to a synchronise).  --parent-lib: (a) also on the parent commit's library, in the same alternation:
      the comparison point.  Writes FILE (profiles/track_occlusions_device.txt) with the medians, the ranges and the sha256 of each library."""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

W, H, SKIP, JETS, R_JETS, REPS = 1024, 436, 1, 16, (16, 32), 3


def inputs():
    """one start_jet: per rate (fu, fv, bu, bv) fp32 (r_Jets, H, W) and frames fp32 (JETS + 1, 3, H, W).  The flows vanish on the image border and the
    backward flow undoes the forward one, so every grid pixel is tracked through every step"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    flows = []
    for r, rJ in enumerate(R_JETS):
        u = np.stack([(0.8 + 0.1 * r) / rJ * np.sin(2 * np.pi * x / W) * np.cos(2 * np.pi * y / H + 0.1 * k) for k in range(rJ)]).astype(np.float32)
        v = np.stack([(0.6 - 0.1 * r) / rJ * np.sin(2 * np.pi * y / H) * np.cos(2 * np.pi * x / W - 0.1 * k) for k in range(rJ)]).astype(np.float32)
        flows.append((u, v, -u, -v))
    rng = np.random.default_rng(0)
    frames = np.stack([np.stack([np.sin(0.11 * (x - 0.05 * t) + c) * np.cos(0.07 * y - c) for c in range(3)]) for t in range(JETS + 1)]).astype(np.float32)
    frames += 0.05 * rng.standard_normal(frames.shape).astype(np.float32)
    return flows, frames


def child_staged():
    import slowflow_amd as sfa
    ctx = sfa.Context(0)
    flows, frames = inputs()
    src = sfa.jet_source(W, H, W)
    gw, gh = sfa.accumulate_grid(W, H, SKIP)
    fp = sfa.fuse_params(skip=SKIP)
    total, t_energy, t_fuse = [], [], []
    for _ in range(REPS + 1):
        ctx.sync()
        t0 = time.perf_counter()
        U, V = np.zeros((1, 2, JETS, gh, gw)), np.zeros((1, 2, JETS, gh, gw))
        E, O = np.zeros((1, 2, gh, gw)), np.zeros((1, 2, gh, gw), np.uint64)
        te = 0.0
        for r, rJ in enumerate(R_JETS):
            au, av, tr = ctx.accumulate_consistent(*[a[None] for a in flows[r]], W, 1.0, SKIP, True, True, source=src)
            ta = time.perf_counter()
            E[0, r], O[0, r], U[0, r], V[0, r] = [a[0] for a in ctx.hypothesis_energies(sfa.energy_params(skip=SKIP, weight=float(r)), rJ, au, av, tr, frames[None], W,
                                                                                     flows=tuple(a[None] for a in flows[0]), adapted=True, flow_source=src)]
            te += time.perf_counter() - ta
        weight = ctx.smoothness_weight(frames[0], W)
        tf = time.perf_counter()
        out = ctx.fuse_hypotheses(fp, U, V, E, O, weight[None], W, H)
        ctx.sync()
        t1 = time.perf_counter()
        total.append(1e3 * (t1 - t0)); t_energy.append(1e3 * te); t_fuse.append(1e3 * (t1 - tf))
    print(json.dumps(dict(total_ms=float(np.median(total[1:])), energies_ms=float(np.median(t_energy[1:])), fuse_ms=float(np.median(t_fuse[1:])),
                          iters=int(out["iters"][0]), hypotheses=float(np.isfinite(E).mean()))))


def child_job(B):
    import slowflow_amd as sfa
    ctx = sfa.Context(0)
    flows, frames = inputs()
    p = sfa.track_params(W, H, JETS, R_JETS, n=B, sources=[sfa.jet_source(W, H, W)] * 2, skip=SKIP)
    job = sfa.TrackJob(ctx, p)
    per, stages = [], []
    for _ in range(REPS + 1):
        ctx.sync()
        t0 = time.perf_counter()
        for s in range(B):
            for r in range(2):
                job.upload_flows(s, r, *flows[r])
            job.upload_frames(s, frames)
        job.run(B)
        for s in range(B):
            rates = [job.download_rate(s, r) for r in range(2)]
            fused = job.download_fused(s)
        ctx.sync()
        per.append(1e3 * (time.perf_counter() - t0) / B)
        stages.append(job.stage_ms())
    print(json.dumps(dict(per_start_ms=float(np.median(per[1:])), stage_ms=[float(v) for v in np.median(np.array(stages[1:]), 0)], iters=int(fused["iters"]),
                          hypotheses=float(np.mean([np.isfinite(q["energy"]).mean() for q in rates])), bytes=sfa.track_job_bytes(p))))


def occlusion_images():
    """per rate raw uint8 images (r_Jets, H, W): one 128 x 64 rectangle of 255 per step, seeded"""
    rng = np.random.default_rng(1)
    out = []
    for rJ in R_JETS:
        o = np.zeros((rJ, H, W), np.uint8)
        for k in range(rJ):
            x0, y0 = int(rng.integers(0, W - 128)), int(rng.integers(0, H - 64))
            o[k, y0:y0 + 64, x0:x0 + 128] = 255
        out.append(o)
    return out


def child_occlusions(route, B):
    if route == "device":
        import torch                                # before the library is loaded, as the other tools do: one HIP runtime in the process
    import slowflow_amd as sfa
    ctx = sfa.Context(0)
    flows, frames = inputs()
    occ = occlusion_images()
    p = sfa.track_params(W, H, JETS, R_JETS, n=B, sources=[sfa.jet_source(W, H, W)] * 2, skip=SKIP, use_occlusions=1)
    job = sfa.TrackJob(ctx, p)
    if route == "device":
        dev = torch.device("cuda", 0)
        t_flows = [tuple(torch.from_numpy(np.stack([f[a], f[a + 1]], 1)).to(dev)[None].expand(B, -1, -1, -1, -1) for a in (0, 2)) for f in flows]
        t_occ = [torch.from_numpy(o).to(dev)[None].expand(B, -1, -1, -1) for o in occ]
        torch.cuda.synchronize()

    def uploads():
        if route == "device":
            for r in range(2):
                job.upload_flows_device(r, *t_flows[r])
                job.upload_occlusions_device(r, t_occ[r])
        for s in range(B):
            if route == "host":
                for r in range(2):
                    job.upload_flows(s, r, *flows[r], occ=occ[r])
            job.upload_frames(s, frames)

    per = []
    for _ in range(REPS + 1):
        ctx.sync()
        t0 = time.perf_counter()
        uploads()
        job.run(B)
        for s in range(B):
            rates = [job.download_rate(s, r) for r in range(2)]
            fused = job.download_fused(s)
        ctx.sync()
        per.append(1e3 * (time.perf_counter() - t0) / B)
    ctx.sync()
    t0 = time.perf_counter()
    uploads()
    ctx.sync()
    up = 1e3 * (time.perf_counter() - t0) / B
    print(json.dumps(dict(per_start_ms=float(np.median(per[1:])), upload_ms=up, stage_ms=job.stage_ms(), iters=int(fused["iters"]),
                          tracked=[float((q["tracked"] > 0).mean()) for q in rates], sha256=hashlib.sha256(open(sfa.LIB_PATH, "rb").read()).hexdigest())))


def main_occlusions(out, parent):
    routes = ([("parent", "host", parent)] if parent else []) + [("a", "host", None), ("b", "device", None)]
    got = {(name, B): [] for name, _, _ in routes for B in (1, 4, 16)}
    for rep in range(3):
        for B in (1, 4, 16):
            for name, route, lib in routes:
                got[name, B].append(spawn(["--child-occlusions", route, str(B)], lib))
                print("repetition %d, B = %d, %s: %s" % (rep, B, name, got[name, B][-1]), flush=True)
    first = got["a", 1][0]
    lines = ["# tools/bench_track.py --occlusions on one MI355X (gfx950); %d x %d, acc_skip_pixel %d, K 2, Jets %d, r_Jets %s, use_occlusions 1, default keys; tracked at %s of the grid pixels, %d TRW-S iterations"
             % (W, H, SKIP, JETS, R_JETS, " / ".join("%.1f %%" % (100 * t) for t in first["tracked"]), first["iters"]),
             "# wall time per start_jet from the first upload to the last download, frames from the host and results to the host; each figure the median of %d runs after a warm-up in a process of its own;" % REPS,
             "# three such processes per row, alternating: (a) flows and occlusion images as host planes (upload_flows(occ=)), (b) flows and 8-bit occlusion images already in GPU memory",
             "# (upload_flows_device + upload_occlusions_device)%s; upload_ms: the uploads alone up to a synchronise, per start_jet" % ("; parent: (a) on the parent commit's library" if parent else ""),
             "# library sha256: this tree %s%s" % (first["sha256"], "; parent %s" % got["parent", 1][0]["sha256"] if parent else ""),
             "#  route   B  per_start_ms median (min .. max)   upload_ms median (min .. max)"]
    for B in (1, 4, 16):
        for name, _, _ in routes:
            v, u = [g["per_start_ms"] for g in got[name, B]], [g["upload_ms"] for g in got[name, B]]
            lines.append("%8s %3d %12.2f (%.2f .. %.2f) %16.2f (%.2f .. %.2f)" % (name, B, float(np.median(v)), min(v), max(v), float(np.median(u)), min(u), max(u)))
        a, b = [float(np.median([g["per_start_ms"] for g in got[n, B]])) for n in ("a", "b")]
        lines.append("#        B = %d: (b) / (a) = %.3f" % (B, b / a))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def spawn(args, lib=None):
    env = dict(os.environ)
    if lib:
        env["SFA_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit("child %s failed (%d):\n%s%s" % (args, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child-staged"]:
        return child_staged()
    if args[:1] == ["--child-job"]:
        return child_job(int(args[1]))
    if args[:1] == ["--child-occlusions"]:
        return child_occlusions(args[1], int(args[2]))
    out, parent = os.path.join(ROOT, "profiles", "track_occlusions_device.txt" if "--occlusions" in args else "track_bench.txt"), None
    if "--out" in args:
        out = args[args.index("--out") + 1]
    if "--parent-lib" in args:
        parent = os.path.abspath(args[args.index("--parent-lib") + 1])
    if "--occlusions" in args:
        return main_occlusions(out, parent)
    base, ours, jobs = [], [], {}
    for B in (1, 4, 16):                                            # alternating: the parent's staged sequence, this tree's, the job
        base.append(spawn(["--child-staged"], parent))
        print("staged (%s): %s" % ("parent library" if parent else "this tree", base[-1]), flush=True)
        if parent:
            ours.append(spawn(["--child-staged"]))
            print("staged (this tree): %s" % ours[-1], flush=True)
        jobs[B] = spawn(["--child-job", str(B)])
        print("job B = %d: %s" % (B, jobs[B]), flush=True)
    who = "the parent commit's library" if parent else "this tree's library (no --parent-lib: NOT the parent baseline)"
    b_ms = float(np.median([b["total_ms"] for b in base]))
    lines = ["# tools/bench_track.py on one MI355X (gfx950); %d x %d, acc_skip_pixel %d, K 2, Jets %d, r_Jets %s, default keys; hypotheses at %.1f %% of the grid pixels"
             % (W, H, SKIP, JETS, R_JETS, 100 * jobs[1]["hypotheses"]),
             "# wall time per start_jet from the first upload to the last download, host planes in and out, median of %d after a warm-up; each row a process of its own" % REPS,
             "# staged sequence, n = 1, %s, three runs alternating with the job's: %s ms per start_jet (median %.2f), %d TRW-S iterations"
             % (who, " / ".join("%.2f" % b["total_ms"] for b in base), b_ms, base[0]["iters"]),
             "#   B  per_start_ms  speedup  job_MB | stage ms per run: records accumulate energies weight labels pairwise trws output (records: frame derivatives + records; the flows are packed at upload)"]
    for B, j in jobs.items():
        lines.append("%5d %13.2f %8.2f %7.0f | %s" % (B, j["per_start_ms"], b_ms / j["per_start_ms"], j["bytes"] / 2 ** 20, " ".join("%.3f" % v for v in j["stage_ms"])))
    if ours:
        for key, name in (("energies_ms", "hypothesis_energies_scaled, both rates"), ("fuse_ms", "fuse_hypotheses"), ("total_ms", "the whole staged sequence")):
            pv, ov = [b[key] for b in base], [b[key] for b in ours]
            inside = abs(float(np.median(ov)) - float(np.median(pv))) <= max(pv) - min(pv)     # the medians differ by no more than the parent's own spread
            lines.append("# wrapper check, %s (n = 1), three runs each, alternating: parent %s ms (spread %.2f), this tree %s ms (median %.2f): %s" % (
                name, " / ".join("%.2f" % v for v in pv), max(pv) - min(pv), " / ".join("%.2f" % v for v in ov), float(np.median(ov)),
                "within the parent's spread" if inside else "OUTSIDE the parent's spread"))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
