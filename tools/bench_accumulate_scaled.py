"""sfa_accumulate_consistent_scaled on quarter-size jets: a 256 x 109 source brought to 1024 x 436 (slow_flow.cfg's scale 0.25 against
dense_tracking.cfg's scale 1.0), skip 0, FF 4 and 16, 1 and 16 segments per call.

  bench_accumulate_scaled.py [repeats]   per configuration, after one warm-up of each call, `repeats` (default 3) rounds of
      scaled     the call on the quarter-size planes: end to end (host clock around the synchronous C-ABI call: uploads, resampling, kernel, download of
                 the last step), the two k_jet_resample launches and k_accumulate<double2> (HIP events inside the library, stage_ms)
      identity   the same call on full-size float planes (the resampled flows rounded to fp32, so the trajectories are the same to fp32) with an
                 identity source: end to end, the two k_interleave launches and k_accumulate<float2> -- the kernel sfa_accumulate_consistent runs
      the two alternate within a round.  The last lines repeat the figures profiles/accumulate_bench.txt recorded for sfa_accumulate_consistent at
      the same FF, skip and n, and the library's sha256.
All segments of a call share one host copy of the flows (the pointers repeat)."""
import ctypes as C
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import slowflow_amd as sfa  # noqa: E402

SW, SH, W, H = 256, 109, 1024, 436
CONFIGS = [(FF, n) for FF in (4, 16) for n in (1, 16)]
_f = C.POINTER(C.c_float)


def padded(a, stride):
    out = np.zeros(a.shape[:-1] + (stride,), np.float32)
    out[..., :a.shape[-1]] = a
    return out


def inputs(ctx, FF):
    """quarter-size planes of a smooth flow of ~1.5 source pixels, and the full-size float planes of the same flow"""
    from test_accumulate import smooth_flows
    small = smooth_flows(np.random.default_rng(FF), FF, SH, SW, 1.5)
    src = sfa.jet_source(SW, SH, sfa.stride_of(SW), w=W)
    assert src.target() == (W, H)
    sp = [padded(a, src.stride) for a in small]
    fu, fv = ctx.jet_flow_resample(sp[0], sp[1], src)
    bu, bv = ctx.jet_flow_resample(sp[2], sp[3], src)
    full = [padded(a.astype(np.float32), sfa.stride_of(W)) for a in (fu, fv, bu, bv)]
    return src, sp, sfa.jet_source(W, H, sfa.stride_of(W)), full


def runner(ctx, src, planes, FF, n):
    L = sfa.lib()
    L.sfa_accumulate_consistent_scaled.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(sfa.JetSource)] + [C.POINTER(_f)] * 4 + [
        C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
    ptrs = [(_f * (n * FF))(*[sfa.fptr(a[f]) for _ in range(n) for f in range(FF)]) for a in planes]
    gw, gh = sfa.accumulate_grid(W, H, 0)
    au, av, tr = np.zeros(n * gw * gh), np.zeros(n * gw * gh), np.zeros(n * gw * gh, np.int32)
    ms = (C.c_float * 2)()

    def run():
        t0 = time.perf_counter()
        rc = L.sfa_accumulate_consistent_scaled(ctx.h, n, FF, W, H, C.byref(src), *ptrs, None, 1.0, 0, 0, 0, au.ctypes.data, av.ctypes.data, tr.ctypes.data, ms)
        e2e = (time.perf_counter() - t0) * 1e3
        if rc != 0:
            raise sfa.SlowflowError(L.sfa_last_error(ctx.h).decode())
        return e2e, ms[0], ms[1], int((tr == FF).sum())
    return run


def parent_figures():
    """(FF, n) -> (e2e_ms, kernel_ms) of skip 0 as profiles/accumulate_bench.txt recorded them for sfa_accumulate_consistent"""
    out = {}
    path = os.path.join(ROOT, "profiles", "accumulate_bench.txt")
    if os.path.exists(path):
        for line in open(path):
            t = line.split()
            if len(t) >= 5 and not line.startswith("#") and t[1] == "0":
                out[int(t[0]), int(t[2])] = (float(t[3]), float(t[4]))
    return out


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    ctx = sfa.Context(0)
    print("# tools/bench_accumulate_scaled.py on one MI355X (gfx950): %d x %d jets -> %d x %d, skip 0; ms; e2e = host clock around the C-ABI call, kernels = HIP events" % (SW, SH, W, H))
    print("# %-3s %-3s %-3s %-9s %10s %12s %14s %10s" % ("FF", "n", "rep", "call", "e2e_ms", "prepare_ms", "k_accumulate", "tracked"))
    med = {}
    for FF, n in CONFIGS:
        src, sp, ident, full = inputs(ctx, FF)
        calls = [("scaled", runner(ctx, src, sp, FF, n)), ("identity", runner(ctx, ident, full, FF, n))]
        for _, run in calls:
            run()                                                                  # warm-up of every shape the timed rounds use
        for rep in range(repeats):
            for name, run in calls:
                e2e, prep, acc, tracked = run()
                med.setdefault((FF, n, name), []).append((e2e, prep, acc))
                print("  %-3d %-3d %-3d %-9s %10.3f %12.4f %14.4f %10d" % (FF, n, rep, name, e2e, prep, acc, tracked))
    print("# medians; prepare = 2 x k_jet_resample (scaled: float planes -> double2 at the target) or 2 x k_interleave (identity: float planes -> float2);")
    print("# k_accumulate = <double2> (scaled) or <float2> (identity, the kernel of sfa_accumulate_consistent); parent = profiles/accumulate_bench.txt's record")
    print("# %-3s %-3s %12s %12s %12s %12s %12s %12s %14s %14s" % ("FF", "n", "scaled_e2e", "resample", "acc_double2", "ident_e2e", "interleave", "acc_float2",
                                                                  "parent_e2e", "parent_kernel"))
    parent = parent_figures()
    for FF, n in CONFIGS:
        s = np.median(np.array(med[FF, n, "scaled"]), axis=0)
        i = np.median(np.array(med[FF, n, "identity"]), axis=0)
        pe, pk = parent.get((FF, n), (float("nan"), float("nan")))
        print("  %-3d %-3d %12.3f %12.4f %12.4f %12.3f %12.4f %12.4f %14.2f %14.3f" % (FF, n, s[0], s[1], s[2], i[0], i[1], i[2], pe, pk))
    print("# library sha256 %s" % hashlib.sha256(open(sfa.LIB_PATH, "rb").read()).hexdigest())
    ctx.close()


if __name__ == "__main__":
    main()
