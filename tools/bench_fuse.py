"""dense_tracking's fusion on the GPU: sfa_dt_smoothness_weight and sfa_fuse_hypotheses at 1024 x 436, skip 1 (a 512 x 218 grid), K in {2, 4, 8} rates,
Jets in {16, 32}, n in {1, 16, 64} segments, synthetic hypotheses (tests/test_fuse.py synth: 20 % holes, slots near a copy of slot 0), default keys.

  bench_fuse.py [reps] [--out FILE]   each configuration end to end through the C-ABI (uploads, the four kernels, downloads), median of `reps` after one
                                      warm-up, with the kernels' own times from the library's HIP events (stage_ms); TRW-S per iteration is the TRW-S
                                      kernel's time over the largest iteration count of the call's segments (the segments run concurrently, one
                                      workgroup each).  Plus the smoothness weight alone and the numpy restatement (tests/fuse_ref.py, one core) on a
                                      64 x 32 grid.  Configurations whose inputs exceed 4 GB are listed as not run.  Writes FILE (profiles/fuse_bench.txt)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import fuse_ref as fr  # noqa: E402
import slowflow_amd as sfa  # noqa: E402
from test_fuse import synth  # noqa: E402

W, H, SKIP = 1024, 436, 1
CONFIGS = [(K, J, n) for K in (2, 4, 8) for J in (16, 32) for n in (1, 16, 64)]
MAX_BYTES = 4 << 30


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "fuse_bench.txt")
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 3
    ctx = sfa.Context(0)
    gw, gh = sfa.accumulate_grid(W, H, SKIP)
    lines = ["# tools/bench_fuse.py %d on one MI355X (gfx950); %d x %d, acc_skip_pixel %d: grid %d x %d; default keys (acc_trws_max_iter 10)" % (
        reps, W, H, SKIP, gw, gh),
        "# e2e: the C-ABI call, uploads and downloads included (median of %d after a warm-up); kernels from the library's HIP events" % reps]
    rng = np.random.default_rng(0)
    frame = rng.uniform(0, 255, (3, H, W)).astype(np.float32)
    ts = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        ctx.smoothness_weight(frame, W)
        ts.append(time.perf_counter() - t0)
    lines.append("# smoothness weight (sfa_dt_smoothness_weight, one frame, upload and download included): %.3f ms" % (1e3 * np.median(ts[1:])))
    lines.append("#  K Jets   n   e2e_ms  labels_ms pairwise_ms  trws_ms iters trws_ms/iter output_ms")
    p = sfa.fuse_params(skip=SKIP)
    for K, J, n in CONFIGS:
        nbytes = 2 * n * K * J * gw * gh * 8
        if nbytes > MAX_BYTES:
            lines.append("%4d %4d %3d   not run: %.1f GB of adapted flows" % (K, J, n, nbytes / 2 ** 30))
            continue
        U1, V1, E1, O1, W1 = synth(np.random.default_rng(K * 100 + J), K, J, W, H, SKIP, 0.2)
        U, V = np.ascontiguousarray(np.broadcast_to(U1, (n,) + U1.shape[1:])), np.ascontiguousarray(np.broadcast_to(V1, (n,) + V1.shape[1:]))
        E, O = np.ascontiguousarray(np.broadcast_to(E1, (n,) + E1.shape[1:])), np.ascontiguousarray(np.broadcast_to(O1, (n,) + O1.shape[1:]))
        Wt = np.ascontiguousarray(np.broadcast_to(W1, (n,) + W1.shape[1:]))
        ts, st = [], []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            r = ctx.fuse_hypotheses(p, U, V, E, O, Wt, W, H, stage_ms=True)
            ts.append(time.perf_counter() - t0)
            st.append(r["stage_ms"])
        ms = np.median(np.array(st[1:]), 0)
        it = int(r["iters"].max())
        lines.append("%4d %4d %3d %8.2f %10.3f %11.3f %8.2f %5d %12.3f %9.3f" % (K, J, n, 1e3 * np.median(ts[1:]), ms[0], ms[1], ms[2], it, ms[2] / it, ms[3]))
        print(lines[-1], flush=True)
        del U, V, E, O, Wt
    # the numpy restatement on one core
    w2, h2 = 128, 64
    U1, V1, E1, O1, W1 = synth(np.random.default_rng(1), 2, 16, w2, h2, SKIP, 0.2)
    t0 = time.perf_counter()
    want = fr.fuse(U1[0], V1[0], E1[0], O1[0], W1[0], fr.Params(skip=SKIP), w2)
    t = time.perf_counter() - t0
    g2 = sfa.accumulate_grid(w2, h2, SKIP)
    lines.append("# numpy restatement (tests/fuse_ref.py, trws_diag, one core): %d x %d grid, K 2, Jets 16, %d iterations: %.2f s" % (g2[0], g2[1], want["iters"], t))
    ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
