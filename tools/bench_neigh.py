"""dense_tracking's alternation stages on the GPU: sfa_prune_hypotheses, sfa_neighbour_proposals and the fusion of the lists they leave, at a 512 x 218
grid, Jets 32, two rates with fill-in (4 slots in lists of 16 positions), one start_jet, default keys, acc_perturb_keep 3.

  bench_neigh.py [reps] [--out FILE]   round 0 (proposals from the consistent pixels, then the fusion) and round 1 (prune by the fusion's selection,
                                       proposals, the fusion with position 0 pinned), the accepted proposals rescored
                                       on random frames and flows of the grid's size before each fusion: each kernel's time from the library's HIP events, median of
                                       `reps` calls after one warm-up.  Synthetic flows: constant over 8 x 8 blocks plus a slot offset, so that a draw
                                       from the pixel's own block is discarded as similar and the others are accepted; 15 % of the pixels hold no
                                       hypothesis, 70 % are consistent.  Beside each row stands the TRW-S time of profiles/fuse_bench.txt (K 4, Jets 32,
                                       one segment: 10 iterations).  Writes FILE (profiles/neigh_bench.txt) with the library's SHA-256."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import slowflow_amd as sfa  # noqa: E402

GW, GH, J, SLOTS, KEEP = 512, 218, 32, 4, 3
FUSE_RECORD = os.path.join(ROOT, "profiles", "fuse_bench.txt")


def trws_of_record():
    """the TRW-S time per round and per iteration of the K 4, Jets 32, n 1 row of profiles/fuse_bench.txt, and that file's SHA-256"""
    raw = open(FUSE_RECORD, "rb").read()
    for line in raw.decode().splitlines():
        f = line.split()
        if len(f) == 10 and f[:3] == ["4", "32", "1"]:
            return float(f[6]), float(f[8]), hashlib.sha256(raw).hexdigest()
    raise SystemExit("profiles/fuse_bench.txt holds no row for K 4, Jets 32, n 1")


TRWS_ROUND_MS, TRWS_ITER_MS, FUSE_SHA = trws_of_record()


def synth(rng):
    by, bx = (GH + 7) // 8, (GW + 7) // 8
    U, V = np.zeros((1, SLOTS, J, GH, GW)), np.zeros((1, SLOTS, J, GH, GW))
    for k in range(SLOTS):
        for a in (U, V):
            b = np.cumsum(rng.normal(0, 0.5, (J, by, bx)), 0) + 0.3 * k
            a[0, k] = np.repeat(np.repeat(b, 8, 1), 8, 2)[:, :GH, :GW]
    e = rng.uniform(0, 50, (1, SLOTS, GH, GW)).astype(np.float32).astype(np.float64)
    e[rng.random(e.shape) < 0.3] = np.inf
    e[:, :, rng.random((GH, GW)) < 0.15] = np.inf
    occ = rng.integers(0, 2, (1, SLOTS, GH, GW)).astype(np.uint64)
    return sfa.hyp_lists(U, V, e, occ)


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "neigh_bench.txt")
    if "--out" in args:
        i = args.index("--out")
        out = args[i + 1]
        del args[i:i + 2]
    reps = int(args[0]) if args else 3
    ctx = sfa.Context(0)
    rng = np.random.default_rng(0)
    lists = synth(rng)
    cons = (rng.random((1, GH, GW)) < 0.7).astype(np.uint8)
    weight = rng.uniform(0.01, 0.5, (1, GH, GW)).astype(np.float32)
    p = sfa.neigh_params(perturb_keep=KEEP)
    ep = sfa.energy_params(skip=0)                                              # the grid is the image
    frames = rng.normal(0, 1, (1, J + 1, 3, GH, GW)).astype(np.float32)
    flows = [rng.normal(0, 1.5, (1, J, GH, GW)).astype(np.float32) for _ in range(4)]
    sha = hashlib.sha256(open(sfa.LIB_PATH, "rb").read()).hexdigest()
    lines = ["# tools/bench_neigh.py %d on one MI355X (gfx950); grid %d x %d, Jets %d, %d slots in lists of 16 positions, 1 start_jet; default keys," % (
        reps, GW, GH, J, SLOTS),
        "# acc_perturb_keep %d, acc_trws_max_iter 10; kernel times from the library's HIP events, median of %d calls after a warm-up" % (KEEP, reps),
        "# libslowflow_amd.so sha256 %s" % sha,
        "# beside each row: TRW-S of profiles/fuse_bench.txt (sha256 %s) at K 4, Jets 32, n 1:" % FUSE_SHA,
        "# %.2f ms per round (10 iterations), %.3f ms per iteration" % (TRWS_ROUND_MS, TRWS_ITER_MS),
        "# round stage                      ms   share of a TRW-S round   of one iteration"]

    def row(rnd, name, ms):
        lines.append("  %5d %-22s %9.3f %12.1f %% %18.1f %%" % (rnd, name, ms, 100 * ms / TRWS_ROUND_MS, 100 * ms / TRWS_ITER_MS))
        print(lines[-1], flush=True)

    def fuse(l, pin):
        fp = sfa.fuse_params(skip=0, pin_first=pin)
        st = []
        for _ in range(reps + 1):
            r = ctx.fuse_hypotheses(fp, l["U"], l["V"], l["energy"], l["occ"], weight, GW, GH, stage_ms=True)
            st.append(r["stage_ms"])
        return r, np.median(np.array(st[1:]), 0)

    def propose(l, rnd):
        st = []
        for _ in range(reps + 1):
            r = ctx.neighbour_proposals(p, l, rnd, [1], cons if rnd == 0 else None, stage_ms=True)
            st.append(r[4])
        return r, np.median(np.array(st[1:]), 0)

    cur = lists
    for rnd in (0, 1):
        if rnd > 0:
            st = []
            for _ in range(reps + 1):
                pr, ms = ctx.prune_hypotheses(cur, sel, KEEP, stage_ms=True)
                st.append(ms)
            ms = np.median(np.array(st[1:]), 0)
            row(rnd, "prune: map", ms[0])
            row(rnd, "prune: gather", ms[1])
            cur = pr
        (cur, pix, _, acc, _), ms = propose(cur, rnd)
        row(rnd, "propose: flags", ms[0])
        row(rnd, "propose: search+accept", ms[1])
        row(rnd, "propose: gather", ms[2])
        lines.append("#       accepted proposals: %d (%.2f per pixel)" % (acc[0], acc[0] / (GW * GH)))
        st = []
        for _ in range(reps + 1):
            rs, ms = ctx.rescore_proposals(ep, cur, pix, frames, GW, flows, [0.0, 0.0, 1.0, 1.0], stage_ms=True)
            st.append(ms)
        row(rnd, "rescore (energies)", float(np.median(st[1:])))
        cur = rs
        r, ms = fuse(cur, int(rnd > 0))
        it = int(r["iters"].max())
        row(rnd, "fuse: labels", ms[0])
        row(rnd, "fuse: pairwise", ms[1])
        row(rnd, "fuse: TRW-S (K 16)", ms[2])
        lines.append("#       TRW-S over the 16 positions: %d iterations, %.3f ms each" % (it, ms[2] / it))
        sel = r["slot"]
    lines += ["# reading: the search-draw-accept kernel stays under one TRW-S iteration at K 4, so it was left as first written (one wave per pixel, 16 of",
              "# its 64 lanes comparing).  What a round costs is the fusion of lists of 16 positions: k_trws<16> takes five to six times the K 4 iteration."]
    ctx.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
