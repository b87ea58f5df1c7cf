"""sfa_hypothesis_energies (dense_tracking's unary hypothesis energies) at 1024 x 436, skip 1: Jets in {4, 8, 16, 32}, 1 and 2 rates (r_Jets = Jets, and
r_Jets = Jets plus r_Jets = 2 Jets, one call per rate), every grid pixel a hypothesis.

  bench_hypothesis_energy.py time [reps]   each configuration timed end to end through the C-ABI (uploads of frames, flows and trajectories, the
                                           derivatives, the three energy kernels, the downloads), median of `reps` after one warm-up; plus the numpy
                                           restatement (tests/energy_ref.py, one core) on a 128 x 64 crop with Jets 4.  Prints one JSON line.
  bench_hypothesis_energy.py trace         every configuration once, no warm-up, in the order of `time`: run it under rocprofv3 --kernel-trace.
  bench_hypothesis_energy.py report TIME.json KERNEL_TRACE.csv
                                           the table: end-to-end ms, and the GPU time of the call's kernels (uploads and downloads excluded), split into
                                           k_hyp_bcgc and the rest.  Writes nothing itself: redirect to profiles/hypothesis_energy_bench.txt."""
import csv
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import slowflow_amd as sfa  # noqa: E402

W, H, SKIP = 1024, 436, 1
CONFIGS = [(J, rates) for J in (4, 8, 16, 32) for rates in (1, 2)]
KERNELS = ("k_interleave", "k_convolve", "k_energy_records", "k_hyp_serial", "k_hyp_bcgc", "k_hyp_sum")


def inputs(J, rJ, rng):
    st = sfa.stride_of(W)
    gw, gh = sfa.accumulate_grid(W, H, SKIP)
    frames = np.zeros((1, J + 1, 3, H, st), np.float32)
    frames[..., :W] = rng.standard_normal((J + 1, 3, H, W)).astype(np.float32)
    y, x = np.mgrid[0:gh, 0:gw].astype(np.float64)
    bu, bv = 1.5 * np.sin(x / 37.0), 1.0 * np.cos(y / 23.0)
    acc_u = np.stack([(f + 1) * bu * J / rJ for f in range(rJ)])[None]
    acc_v = np.stack([(f + 1) * bv * J / rJ for f in range(rJ)])[None]
    tracked = np.full((1, gh, gw), rJ, np.int32)
    fl = []
    for k in range(4):
        a = np.zeros((1, J, H, st), np.float32)
        a[..., :W] = rng.standard_normal((J, H, W)).astype(np.float32) * 0.3 + (1.5 if k % 2 == 0 else 1.0) * (1 if k < 2 else -1)
        fl.append(a)
    return frames, acc_u, acc_v, tracked, fl


def runner(ctx, J, rates):
    rng = np.random.default_rng(J)
    calls = []
    for r in range(rates):
        rJ = J * (r + 1)
        frames, au, av, tr, fl = inputs(J, rJ, rng)
        p = sfa.energy_params(skip=SKIP, weight=float(r))
        calls.append((p, rJ, au, av, tr, frames, fl))

    def run():
        for p, rJ, au, av, tr, frames, fl in calls:
            ctx.hypothesis_energies(p, rJ, au, av, tr, frames, W, fl)
    return run, int(tracked_count(calls))


def tracked_count(calls):
    return sum(int((c[4] == c[1]).sum()) for c in calls)


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    if mode == "report":
        return report(sys.argv[2], sys.argv[3])
    reps = int(sys.argv[2]) if len(sys.argv) > 2 and mode == "time" else 1
    ctx = sfa.Context(0)
    res = {"size": [W, H], "skip": SKIP, "reps": reps, "configs": []}
    for J, rates in CONFIGS:
        run, nh = runner(ctx, J, rates)
        if mode == "trace":
            run()
            continue
        run()                                                                      # warm-up
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e3)
        res["configs"].append({"Jets": J, "rates": rates, "hypotheses": nh, "e2e_ms": float(np.median(ts))})
    if mode == "time":
        from energy_ref import Params, energies
        rng = np.random.default_rng(0)
        J, h, w = 4, 64, 128
        frames = rng.standard_normal((J + 1, 3, h, w)).astype(np.float32)
        gw, gh = sfa.accumulate_grid(w, h, SKIP)
        au = np.stack([(f + 1) * np.full((gh, gw), 0.7) for f in range(J)])
        fl = tuple((rng.standard_normal((J, h, w)) * 0.3).astype(np.float32) for _ in range(4))
        d = np.zeros_like(frames)
        t0 = time.perf_counter()
        energies(Params(skip=SKIP), J, au, au, np.full((gh, gw), J, np.int32), frames, d, d, fl)
        res["numpy_jets4_128x64_ms"] = (time.perf_counter() - t0) * 1e3
        res["numpy_jets4_128x64_hypotheses"] = gw * gh
        res["library_sha256"] = hashlib.sha256(open(sfa.LIB_PATH, "rb").read()).hexdigest()
        print(json.dumps(res))
    ctx.close()


def report(time_json, trace_csv):
    res = json.loads(open(time_json).read().strip().splitlines()[-1])
    calls, cur = [], {}
    with open(trace_csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda row: int(row["Start_Timestamp"]))          # the file is not in dispatch order
    for row in rows:
        k = next((k for k in KERNELS if k in row["Kernel_Name"]), None)
        if k is None:
            continue
        cur[k] = cur.get(k, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6
        if k == "k_hyp_sum":                                                       # the last launch of a call
            calls.append(cur)
            cur = {}
    per = []
    for c in res["configs"]:
        got = calls[:c["rates"]]
        calls = calls[c["rates"]:]
        per.append((sum(sum(x.values()) for x in got), sum(x.get("k_hyp_bcgc", 0.0) for x in got)))
    assert not calls, "more traced calls than configurations"
    print("# tools/bench_hypothesis_energy.py on one MI355X (gfx950): 'time 3', then 'trace' under rocprofv3 --kernel-trace, then 'report'")
    print("# %d x %d, acc_skip_pixel %d (r = 1: 9 neighbours), every grid pixel a hypothesis; rates: r_Jets = Jets, and r_Jets = 2 Jets in a second call"
          % (W, H, SKIP))
    print("# e2e: the C-ABI calls of all rates, uploads and downloads included (median of %d); kernels: GPU time of the calls' kernels alone" % res["reps"])
    print("# %-4s %-5s %11s %10s %11s %13s" % ("Jets", "rates", "hypotheses", "e2e_ms", "kernels_ms", "k_hyp_bcgc_ms"))
    for c, (k, b) in zip(res["configs"], per):
        print("  %-4d %-5d %11d %10.2f %11.3f %13.3f" % (c["Jets"], c["rates"], c["hypotheses"], c["e2e_ms"], k, b))
    print("# numpy restatement (tests/energy_ref.py, one core), Jets 4, 128 x 64, skip 1 (%d hypotheses): %.0f ms"
          % (res["numpy_jets4_128x64_hypotheses"], res["numpy_jets4_128x64_ms"]))
    print("# library sha256 %s" % res["library_sha256"])


if __name__ == "__main__":
    main()
