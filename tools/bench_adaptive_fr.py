"""The adaptiveFR program's two GPU steps at its default shape (a 1024 x 436 sequence at scale 0.25: pairs of 256 x 109, 40 samples):
  - 40 pairs refined in one sfa_variational_2frame_batch against 40 sfa_variational_2frame calls (adaptiveFR's parameters: alpha 1, gamma 0.72, delta 0,
    5 outer x 1 inner x 30 SOR sweeps), each timed end to end through the C-ABI (uploads and downloads included), median of `reps`;
  - sfa_flow_magnitude_quantile against numpy.sort of the same magnitudes (float32, the host form), for 1 M and 9.2 M values (uploads included).
Prints one JSON line, with the library's sha256 (which build it ran on).  usage: bench_adaptive_fr.py [reps]"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import oracle as orc  # noqa: E402
import slowflow_amd as sfa  # noqa: E402
from synth import noise_plane, smooth_noise_color  # noqa: E402


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    W, H, N = 256, 109, 40
    ctx = sfa.Context(0)
    rng = np.random.default_rng(0)
    pairs = []
    for i in range(N):
        big = smooth_noise_color(rng, W + 8, H + 8, 40)
        a, b = orc.aligned_zeros((3, H, orc.stride_of(W))), orc.aligned_zeros((3, H, orc.stride_of(W)))
        a[:, :, :W] = big[:, 4:4 + H, 4:4 + W]
        b[:, :, :W] = big[:, 3:3 + H, 2:2 + W]
        pairs.append((a, b, noise_plane(rng, W, H, 1.5, 2.5), noise_plane(rng, W, H, 0.5, 1.5)))
    p = sfa.Params2f(1.0, 0.72, 0.0, 1.1, 5, 1, 30, 1.9)

    def singles():
        for a, b, x, y in pairs:
            ctx.variational_2frame(x.copy(), y.copy(), a, b, W, p)

    def batch():
        ctx.variational_2frame_batch([q[2].copy() for q in pairs], [q[3].copy() for q in pairs], [q[0] for q in pairs], [q[1] for q in pairs], W, p)

    singles(); batch()                                                         # warm-up: module load, allocations
    rec = {"pairs": N, "size": [W, H], "reps": reps, "single_calls_ms": median_ms(singles, reps), "batch_ms": median_ms(batch, reps)}
    rec["batch_speedup"] = rec["single_calls_ms"] / rec["batch_ms"]
    for n in (1 << 20, 9_200_000):
        u = rng.uniform(-20, 20, size=(1, n)).astype(np.float32)
        v = rng.uniform(-20, 20, size=(1, n)).astype(np.float32)
        ctx.flow_magnitude_quantile([u], [v], n, 2.0, 0.9)

        def host():
            s = np.float32(2.0)
            a, b = u * s, v * s
            m = np.sort(np.sqrt(a * a + b * b).ravel())
            return m[int(np.ceil(np.float32(0.9) * np.float32(n) - 1))]

        rec[f"quantile_gpu_ms_{n}"] = median_ms(lambda: ctx.flow_magnitude_quantile([u], [v], n, 2.0, 0.9), reps)
        rec[f"quantile_numpy_sort_ms_{n}"] = median_ms(host, reps)
    rec["library_sha256"] = hashlib.sha256(open(sfa.LIB_PATH, "rb").read()).hexdigest()
    ctx.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
