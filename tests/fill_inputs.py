"""Seeded inputs of the fill-job tests (tests/test_track_fill.py, test_track_fill_host.py): segments whose accumulation leaves what the fill-in is for.

A segment is, per rate, forward flows of tests/test_epic_fill.py's piecewise-affine motion (the trajectories() of that file, spread evenly over the rate's
steps), backward flows that undo them, and a first step whose backward flow is off by three pixels wherever no trajectory shall survive: a hole in the
middle, a strip that cuts the right edge off, and everything behind the strip but one island of 8 x 8 frame pixels.  The motion's own discontinuity at
0.55 w is a second strip nothing crosses.  `islands` names the rates of a segment whose consistent pixels are three such islands only: fewer than
removeSmallSegments' 100 pixels each, so no region is kept, no sample has a match and the rate is not filled.  tests/test_track_fill_host.py shows both
claims (Case.filled) on the restatements tests/accum_ref.py and tests/fill_ref.py.  The image the Lab planes come from is tests/test_epic.py's scene at
the grid's size; the edge map is noise of 0.01 .. 0.5, where one addition of euc 0.25 more moves region borders (tests/test_epic_fill.py)."""
import numpy as np

import slowflow_amd as sfa
from accum_ref import grid

F32 = np.float32
PAD = F32(1e30)                                     # what the stride padding holds: never read
RATES, JETS, MIN_FPS = (2, 4), 4, 1
EPSILON = 0.75
WEIGHTS = (0.0, 0.5)
EUC = 0.25
EPIC_SKIP = 2.0


class Case:
    def __init__(self, name, w, h, skip, runs, islands=()):
        """runs: the seeds of each run of one job, in order; islands: {seed: rates without a consistent region}"""
        self.name, self.w, self.h, self.skip, self.runs, self.islands = name, w, h, skip, tuple(tuple(r) for r in runs), dict(islands)
        self.stride = sfa.stride_of(w)
        self.gw, self.gh, self.incr, self.start = grid(w, h, skip)
        self.K, self.n = len(RATES), max(len(r) for r in self.runs)

    def params(self, **kw):
        return sfa.track_params(self.w, self.h, JETS, RATES, n=self.n, weights=WEIGHTS, fuse=sfa.fuse_params(trws_max_iter=8), min_fps_idx=MIN_FPS,
                                skip=self.skip, epsilon=EPSILON, discard=1, **kw)

    def fill(self, **kw):
        kw.setdefault("epic_skip", EPIC_SKIP)
        kw.setdefault("epic", sfa.epic_params(pref_nn=25, nn=160, coef_kernel=1.1, euc=kw.pop("euc", EUC)))
        return sfa.track_fill_params(**kw)

    def filled(self, seed, r):
        return 0 if r in self.islands.get(seed, ()) else 1


# the base case: three segments, of which seed 32 keeps only islands on rate 0; then two new segments on the same job, where position 0 (filled in the
# first run) is the one that is not filled
BASE = Case("base", 96, 64, 0, [(31, 32, 33), (34, 35)], islands={32: (0,), 34: (0,)})
SKIP1 = Case("skip1", 96, 64, 1, [(41,)])           # the grid is 48 x 32
TAIL = Case("tail", 99, 65, 0, [(51, 52)])          # 6435 pixels: no multiple of 4, nor of the advance kernel's 1024 pixels per block


def segment(case, seed):
    """-> dict: flows[r] = (fu, fv, bu, bv) fp32 (r_Jets, h, stride), frames fp32 (Jets + 1, 3, h, stride), rgb fp32 (3, gh, stride_of(gw)) of 8-bit values
    (the image the Lab planes are made of), edges fp32 (gh, gw)"""
    from test_epic import scene
    rng = np.random.default_rng(seed)
    w, h = case.w, case.h
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    gain = rng.uniform(0.85, 1.15)
    right = xx > w * 0.55
    u = gain * np.where(right, 3.0 + 0.02 * (xx - w / 2), -1.5 + 0.01 * yy)
    v = gain * np.where(right, -2.0 + 0.015 * yy, 0.5 - 0.01 * (xx - 10))
    fx, fy = xx / w, yy / h
    dx, dy = rng.uniform(-0.03, 0.03, 2)
    island = lambda cx, cy: (xx >= int(cx * w)) & (xx < int(cx * w) + 8) & (yy >= int(cy * h)) & (yy < int(cy * h) + 8)
    bad = ((fx >= 0.31 + dx) & (fx < 0.73 + dx) & (fy >= 0.31 + dy) & (fy < 0.69 + dy)) | ((fx >= 0.83) & ~island(0.875, 0.8))
    lonely = ~(island(0.875, 0.8) | island(0.05, 0.06) | island(0.42, 0.47))
    flows = []
    for r, rJ in enumerate(RATES):
        f = np.full((4, rJ, h, case.stride), PAD, F32)
        wrong = lonely if r in case.islands.get(seed, ()) else bad
        for k in range(rJ):
            su, sv = u / rJ, v / rJ
            bu = np.where(wrong, -su + 3.0, -su) if k == 0 else -su
            f[0, k, :, :w], f[1, k, :, :w], f[2, k, :, :w], f[3, k, :, :w] = su, sv, bu, -sv
        flows.append(tuple(f))
    frames = np.full((JETS + 1, 3, h, case.stride), PAD, F32)
    tex = rng.uniform(0.15, 0.45, (3, 2))
    for t in range(JETS + 1):
        sx, sy = xx - gain * 1.0 * t / JETS, yy + gain * 0.5 * t / JETS
        for c in range(3):
            frames[t, c, :, :w] = np.sin(tex[c, 0] * sx + c) * np.cos(tex[c, 1] * sy - c) + 0.05 * rng.standard_normal((h, w))
    rgb = scene(case.gw, case.gh, seed)[0]
    edges = np.random.default_rng(seed + 40).uniform(0.01, 0.5, (case.gh, case.gw)).astype(F32)
    return dict(flows=flows, frames=frames, rgb=rgb, edges=edges)


def advanced(edges, additions, euc):
    """the edge map after `additions` sequential fp32 additions of euc (host/epic_fill.cpp:47-56): repeated additions, never a product"""
    out, e = np.array(edges, F32), F32(euc)
    for _ in range(additions if e != 0 else 0):
        out = (out + e).astype(F32)
    return out
