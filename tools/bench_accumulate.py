"""sfa_accumulate_consistent (dense_tracking's consistent accumulation) at 1024 x 436: FF in {4, 16, 32}, skip in {0, 1}, 1 / 16 / 64 segments per call.

  bench_accumulate.py time [reps]        each configuration timed end to end through the C-ABI (uploads of the flows, the interleave, the kernel, the
                                         download of the last step), median of `reps` after one warm-up; plus the numpy restatement (tests/accum_ref.py,
                                         one core) on one segment of FF 4.  Prints one JSON line.
  bench_accumulate.py trace              every configuration once, no warm-up, in the order of `time`: run it under rocprofv3 --kernel-trace; dispatch k of
                                         k_accumulate is configuration k.
  bench_accumulate.py report TIME.json KERNEL_TRACE.csv
                                         the table: end-to-end ms, k_accumulate ms (uploads excluded), and the bytes each step gathers per grid pixel
                                         (4 + 4 taps of 8 bytes, forward and backward; + 16 bytes of output per pixel) over kernel time against the HBM peak.
All segments of a call share one host copy of the flows (the pointers repeat), so 64 x 32 planes need no host memory of their own."""
import csv
import ctypes as C
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

W, H = 1024, 436
CONFIGS = [(FF, skip, n) for FF in (4, 16, 32) for skip in (0, 1) for n in (1, 16, 64)]
HBM_PEAK = 8.0e12                                                                  # MI355X_MICROARCH: 8 TB/s spec


def flows(FF):
    from test_accumulate import smooth_flows
    fu, fv, bu, bv = smooth_flows(np.random.default_rng(FF), FF, H, W, 6.0)
    st = sfa.stride_of(W)
    out = []
    for a in (fu, fv, bu, bv):
        p = np.zeros((FF, H, st), np.float32)
        p[:, :, :W] = a
        out.append(p)
    return out


def runner(ctx, FF, skip, n):
    L = sfa.lib()
    _f = C.POINTER(C.c_float)
    L.sfa_accumulate_consistent.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(_f)] * 4 + [
        C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    planes = flows(FF)
    ptrs = [(_f * (n * FF))(*[sfa.fptr(a[f]) for _ in range(n) for f in range(FF)]) for a in planes]
    gw, gh = sfa.accumulate_grid(W, H, skip)
    au, av, tr = np.zeros(n * gw * gh), np.zeros(n * gw * gh), np.zeros(n * gw * gh, np.int32)

    def run():
        rc = L.sfa_accumulate_consistent(ctx.h, n, FF, W, H, planes[0].shape[2], *ptrs, None, 1.0, skip, 0, 0, au.ctypes.data, av.ctypes.data, tr.ctypes.data)
        if rc != 0:
            raise sfa.SlowflowError(L.sfa_last_error(ctx.h).decode())
    return run, gw * gh


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "time"
    if mode == "report":
        return report(sys.argv[2], sys.argv[3])
    reps = int(sys.argv[2]) if len(sys.argv) > 2 and mode == "time" else 1
    ctx = sfa.Context(0)
    res = {"size": [W, H], "reps": reps, "configs": []}
    for FF, skip, n in CONFIGS:
        run, npx = runner(ctx, FF, skip, n)
        if mode == "trace":
            run()
            continue
        run()                                                                      # warm-up
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e3)
        res["configs"].append({"FF": FF, "skip": skip, "n": n, "grid_pixels": npx, "e2e_ms": float(np.median(ts))})
    if mode == "time":
        from accum_ref import accumulate
        fu, fv, bu, bv = (a[:, :, :W] for a in flows(4))
        t0 = time.perf_counter()
        accumulate(fu, fv, bu, bv, None, 1.0, 0, False)
        res["numpy_ff4_skip0_one_segment_ms"] = (time.perf_counter() - t0) * 1e3
        res["library_sha256"] = hashlib.sha256(open(sfa.LIB_PATH, "rb").read()).hexdigest()
        print(json.dumps(res))
    ctx.close()


def report(time_json, trace_csv):
    res = json.loads(open(time_json).read().strip().splitlines()[-1])
    ks = []
    with open(trace_csv) as f:
        for row in csv.DictReader(f):
            if "k_accumulate" in row["Kernel_Name"]:
                ks.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    assert len(ks) == len(res["configs"]), (len(ks), len(res["configs"]))
    print("# 1024 x 436, uploads included: e2e (C-ABI call, median of %d); uploads excluded: k_accumulate alone (rocprofv3 --kernel-trace, one dispatch)" % res["reps"])
    print("# gathered bytes: per grid pixel and step 64 B of flow taps (forward + backward, 4 taps x 8 B each) + 16 B of output per pixel; rate = bytes / kernel time")
    print("# %-3s %-4s %-3s %10s %12s %14s %12s" % ("FF", "skip", "n", "e2e_ms", "kernel_ms", "gathered_GB/s", "of_8TB/s"))
    for c, k in zip(res["configs"], ks):
        b = c["n"] * c["grid_pixels"] * (64.0 * c["FF"] + 16)
        print("  %-3d %-4d %-3d %10.2f %12.3f %14.0f %11.1f%%" % (c["FF"], c["skip"], c["n"], c["e2e_ms"], k, b / (k * 1e-3) / 1e9, 100 * b / (k * 1e-3) / HBM_PEAK))
    print("# numpy restatement (tests/accum_ref.py, one core), FF 4, skip 0, one segment: %.0f ms" % res["numpy_ff4_skip0_one_segment_ms"])
    print("# library sha256 %s" % res["library_sha256"])


if __name__ == "__main__":
    main()
