"""Inputs whose MAGNITUDES vary (pure numpy): planes scaled by a ladder of powers of two in bands of eight columns, and a fixed sprinkle of IEEE special values.
Everything else the suite feeds the kernels is O(1) noise; these reach the data-term kernel's guard branches, subnormal operands and overflow.

guard_classes restates num_ok3 / den_ok3 of slowflow_amd/csrc/kernels.hip on an oracle derivative stack, so that a test can prove on the CPU which of a kernel's
branches its input takes before anything runs on the GPU."""
import numpy as np

from oracle import aligned_zeros, stride_of
from synth import smooth_noise_color

W, H = 136, 24                                   # three 64-wide tile columns (the last 8 px wide), three 8-row tiles: a partial tile column, an interior wave, all three row groups
LOW = dict(exps=[-70, -45, -20, 0], top=-45)     # rows 0-7 mixed waves, rows 8-15 admitted, rows 16 ... rejected (low numerators only)
FULL = dict(exps=[-70, -45, -20, 0, 14, 27], top=None)   # every row banded: low numerators, high numerators and high denominators in every wave
HIGH = dict(exps=[-45, 0, 14, 27], top=27)       # reaches 2^27: the reference's own level is not finite there

FLT_MIN = np.float32(2.0 ** -126)
FLT_MAX = np.finfo(np.float32).max
SUB_MIN = np.float32(2.0 ** -149)
SUB_MAX = np.nextafter(FLT_MIN, np.float32(0))
SPECIALS = np.array([0.0, -0.0, SUB_MIN, SUB_MAX, FLT_MIN, FLT_MAX, np.inf, -np.inf, np.nan], np.float32)
FINITE_SPECIALS = SPECIALS[:6]


def ladder_scale(w, h, exps, band=8, top=None):
    """(h, w) fp32: rows 0-7 hold 2^exps[(x // band) % len(exps)], rows 8-15 hold 1, rows 16 ... hold 2^top; top=None: every row carries the bands"""
    bands = np.exp2(np.asarray(exps, np.float64))[(np.arange(w) // band) % len(exps)].astype(np.float32)
    s = np.empty((h, w), np.float32)
    s[:] = bands
    if top is not None:
        s[8:16] = 1.0
        s[16:] = np.float32(2.0 ** top)
    return s


def ladder_plane(plane, w, exps, band=8, top=None):
    """a copy of a (..., h, stride) plane with its valid columns multiplied by the ladder"""
    out = aligned_zeros(plane.shape)
    out[...] = plane
    out[..., :w] *= ladder_scale(w, plane.shape[-2], exps, band, top)
    return out


def ladder_frames(oracle, w, h, n, exps, top, seed):
    """n colour frames: integer-shifted crops ((2, 1) px per frame, as test_gpu_parity.normalized_frames shifts them) of one band-limited texture, each multiplied by
    the ladder.  NOT normalised: subtracting a mean would absorb the small bands; use them with the statistics (0, 1)"""
    rng = np.random.default_rng(seed)
    m = max(8, 2 * n)
    base = smooth_noise_color(rng, w + 2 * m, h + 2 * m, scale=10)
    scale = ladder_scale(w, h, exps, top=top)
    frames = []
    for k in range(n):
        f = aligned_zeros((3, h, stride_of(w)))
        f[:, :, :w] = base[:, m - k:m - k + h, m - 2 * k:m - 2 * k + w] * scale
        frames.append(f)
    return frames


def sprinkle(plane, seed, w=None, values=SPECIALS):
    """writes each of `values` (by default +0, -0, the smallest and the largest subnormal, FLT_MIN, FLT_MAX, +Inf, -Inf, NaN) at three seeded positions of the
    valid columns of every leading plane (once each where a plane has fewer than 54 pixels), in place; returns the plane"""
    rng = np.random.default_rng(seed)
    h = plane.shape[-2]
    w = plane.shape[-1] if w is None else w
    flat = plane.reshape(-1, h, plane.shape[-1])
    for p in flat:
        pos = rng.choice(h * w, (3 if h * w >= 6 * len(values) else 1) * len(values), replace=False)
        for i, q in enumerate(pos):
            p[q // w, q % w] = values[i % len(values)]
    return plane


def is_subnormal(a):
    a = np.asarray(a, np.float32)
    return (a != 0) & (np.abs(a) < FLT_MIN)


def value_sets(a):
    """the positions of NaN, +Inf, -Inf and subnormal values, as four boolean arrays"""
    a = np.asarray(a, np.float32)
    return np.isnan(a), a == np.inf, a == -np.inf, is_subnormal(a)


def num_ok(a):
    """kernels.hip num_ok: +0 (not -0), or 2^-87 <= a < 2^53"""
    a = np.asarray(a, np.float32)
    bits = a.view(np.uint32)
    return (bits == 0) | ((a >= np.float32(2.0 ** -87)) & (a < np.float32(2.0 ** 53)))


def den_ok(n):
    """kernels.hip den_ok3: fmaxf(...) < 2^33 (fmaxf drops a NaN operand; a denominator here is a sum of squares + 0.01 and NaN only where an image value is)"""
    n = np.asarray(n, np.float32)
    return n < np.float32(2.0 ** 33)


def guard_terms(D, w=None):
    """numerators and denominators of a successive term's first inner iteration (du = dv = 0, s = 0, no channel weights) from an oracle derivative stack
    (8, 3, h, stride: Ix Iy Iz Ixx Ixy Iyy Ixz Iyz), in fp32 as the kernel forms them: a (9, h, w), n (9, h, w)"""
    f = np.float32
    w = D.shape[-1] if w is None else w
    Ix, Iy, Iz, Ixx, Ixy, Iyy, Ixz, Iyz = (D[k][..., :w].astype(f) for k in range(8))
    dn = f(0.1) * f(0.1)
    a = np.concatenate([Iz * Iz, Ixz * Ixz, Iyz * Iyz])
    n = np.concatenate([Ix * Ix + Iy * Iy + dn, Ixx * Ixx + Ixy * Ixy + dn, Iyy * Iyy + Ixy * Ixy + dn])
    return a, n


def guard_pass(D, w=None):
    """per pixel: (colour group admitted, gradient group admitted, low-numerator failure, high-numerator failure, denominator failure)"""
    with np.errstate(all="ignore"):
        a, n = guard_terms(D, w)
        nok, dok = num_ok(a), den_ok(n)
        col = nok[:3].all(0) & dok[:3].all(0)
        grd = nok[3:].all(0) & dok[3:].all(0)
        low = (~nok & (a < np.float32(2.0 ** -87))).any(0)
        high = (~nok & ~(a < np.float32(2.0 ** 53))).any(0)
    return col, grd, low, high, ~dok.all(0)


def guard_classes(D, w=None):
    """per 64-column segment of every row one of 'all', 'none', 'mixed': whether all, none or some of its pixels pass num_ok3 / den_ok3 in both groups of
    quotients.  Returns an (h, ceil(w / 64)) array of str"""
    col, grd, _, _, _ = guard_pass(D, w)
    ok = col & grd
    h, w = ok.shape
    nseg = (w + 63) // 64
    out = np.empty((h, nseg), dtype=object)
    for y in range(h):
        for s in range(nseg):
            seg = ok[y, 64 * s:min(w, 64 * s + 64)]
            out[y, s] = "all" if seg.all() else "none" if not seg.any() else "mixed"
    return out


def class_counts(classes):
    return {k: int((classes == k).sum()) for k in ("mixed", "all", "none")}


# ------------------------------------------------------------------------------------------------------
# the tracking stage (tests/test_track_value_ranges.py): flows whose trajectories take every branch of the position guards of accumulate.hip and energy.hip,
# double-precision special values for accumulated flows and energies, and the classes an input reaches, computed from the restatements' intermediates
# ------------------------------------------------------------------------------------------------------
SMALL = (5, 4)                                  # smaller than every tile and block
TRAJ_MAGS = np.array([2.0 ** -140, 2.0 ** -20, 1.0, 2.0 ** 31, 2.0 ** 63, FLT_MAX, 1e10, -1e10], np.float32)   # eight bands: all of them in any 64 columns
F64_SPECIALS = np.array([0.0, -0.0, 5e-324, 2.0 ** -1022, 1e9, np.nextafter(1e9, np.inf), 1e10, -1e10, float(FLT_MAX), np.inf, -np.inf, np.nan])
INT_RANGE = 2.0 ** 31                           # from here on (int) of a double is no index at all


def traj_flows(FF, h, w, seed, band=8, sprinkle_seed=None, mags=TRAJ_MAGS):
    """the flow ladder for trajectories: (fu, fv, bu, bv), fp32 (FF, h, w).  A smooth field of a pixel or two (the backward one its negative plus noise) times
    TRAJ_MAGS in bands of `band` columns, the bands moving on by one per step, so that a trajectory that stays in the image at step f meets the next magnitude at
    step f + 1: subnormal, 2^-20, O(1), 2^31, 2^63, +-FLT_MAX, and exactly +-1e10 (UNKNOWN_FLOW).  sprinkle_seed: SPECIALS sprinkled into every plane;
    mags: other magnitudes (one of 1: the smooth field alone, whose trajectories stay in the image and meet the sprinkle)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.zeros((4, FF, h, w), np.float32)
    with np.errstate(all="ignore"):
        for f in range(FF):
            a, p = rng.uniform(0.5, 3, 4), rng.uniform(0, 6.3, 4)
            u = 1.5 * np.sin(a[0] * x / w * 6.3 + p[0]) * np.cos(a[1] * y / h * 6.3 + p[1])
            v = 1.5 * np.cos(a[2] * x / w * 6.3 + p[2]) * np.sin(a[3] * y / h * 6.3 + p[3])
            noise = rng.standard_normal((2, h, w)) * rng.choice([0.01, 0.3])
            mag = np.asarray(mags, np.float32)[((np.arange(w) // band) + f) % len(mags)][None, :]
            for k, (fld, sign) in enumerate(((u, 1.0), (v, 1.0), (-u + noise[0], -1.0), (-v + noise[1], -1.0))):
                val = (fld * mag.astype(np.float64)).astype(np.float32)
                val = np.where(np.abs(mag) == FLT_MAX, np.where(fld < 0, -FLT_MAX, FLT_MAX), val)
                out[k, f] = np.where(np.abs(mag) == np.float32(1e10), np.float32(sign) * mag, val)
    if sprinkle_seed is not None:
        for k in range(4):
            sprinkle(out[k], sprinkle_seed + k)
    return out[0], out[1], out[2], out[3]


def ulp_below(n):
    """n - the largest double below n"""
    return float(n) - float(np.nextafter(np.float64(n), 0.0))


def _landing(n, band):
    """step 0's flow along one axis of extent n, by bands of `band` pixels: the pixel c lands on c + 1 (an integer; n from the last pixel), n - 1, n - 1.5,
    +0.0 (c + (-c)), c itself (the flow is -0.0), -1, n, c + 0.5; pixel 0 lands on -2^-149, the negative value nearest zero"""
    c = np.arange(n, dtype=np.float64)
    kind = (np.arange(n) // band) % 8
    t = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5, kind == 6, kind == 7],
                  [np.ones(n), (n - 1) - c, (n - 1.5) - c, -c, np.full(n, -0.0), -c - 1, n - c, np.full(n, 0.5)])
    t = np.where(kind == 4, -0.0, t)                                           # np.select keeps the sign; so does this
    t[0] = -float(SUB_MIN)
    assert np.array_equal(t.astype(np.float32).astype(np.float64), t)
    return t.astype(np.float32)


def edge_landing(FF, h, w, band_x=8, band_y=3):
    """the edge-landing field: (fu, fv, bu, bv), fp32 (FF, h, w), FF >= 3.  Step 0 moves pixel (x, y) by _landing(w)[x], _landing(h)[y]: positions that are an
    integer, exactly w - 1 / h - 1, exactly +0.0, w and h themselves (outside by one ulp), -1, and -2^-149 from pixel 0.
    An integer pixel plus an fp32 flow is exact in a double, so neither -0.0 (a sum is -0.0 only when both terms are) nor the largest double below w can be a
    position after step 0.  The second comes after step 1: the pixels that landed on w - 1.5 interpolate step 1's columns w - 2 (3.0) and w - 1 (-2 ulp) with
    weight 1/2 each, 1.5 - ulp, and land on w - ulp; those on +0.0 read column 0 (-2^-149) and land on the negative value nearest zero.  Rows alike.
    The backward flows are the exact negatives, except on alternate groups of four columns of step 2"""
    assert FF >= 3 and w >= 3 and h >= 3
    fu, fv = np.zeros((FF, h, w), np.float32), np.zeros((FF, h, w), np.float32)
    fu[0], fv[0] = _landing(w, band_x)[None, :], _landing(h, band_y)[:, None]
    fu[1], fv[1] = 0.25, 0.125
    fu[1][:, 0], fu[1][:, w - 2], fu[1][:, w - 1] = -SUB_MIN, 3.0, -2 * ulp_below(w)
    fv[1][0, :], fv[1][h - 2, :], fv[1][h - 1, :] = -SUB_MIN, 3.0, -2 * ulp_below(h)
    fu[2:], fv[2:] = 0.25, 0.125
    bu, bv = -fu, -fv
    bu[2][:, (np.arange(w) // 4) % 2 == 1] += 2.0
    return fu, fv, bu, bv


def specials64(a, seed, values=F64_SPECIALS):
    """F64_SPECIALS (+-0, 5e-324, 2^-1022, 1e9 and the next double, +-1e10, FLT_MAX, +-Inf, NaN) sprinkled into every (h, w) plane of a float64 array, in place"""
    return sprinkle(a, seed, values=values)


def position_classes(tested, y, x, h, w):
    """what the in-image test `y >= 0 && y < h && x >= 0 && x < w` on doubles meets, as boolean arrays over the positions `tested`:
    fail_nan (a NaN coordinate), fail_magnitude (a coordinate that (int) cannot hold: |c| >= 2^31 or Inf), fail_ulp (outside by the least amount: exactly w or h,
    or the negative fp32 value nearest zero), pass_ulp (the largest double below w or h), pass_zero, pass_last (exactly w - 1 or h - 1), pass_integer"""
    with np.errstate(invalid="ignore"):
        y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
        ok = tested & (y >= 0) & (y < h) & (x >= 0) & (x < w)
        bad = tested & ~ok
        nan = np.isnan(y) | np.isnan(x)
        return dict(fail_nan=bad & nan,
                    fail_magnitude=bad & ~nan & ((np.abs(y) >= INT_RANGE) | (np.abs(x) >= INT_RANGE)),
                    fail_ulp=bad & ~nan & ((x == w) | (y == h) | (x == -float(SUB_MIN)) | (y == -float(SUB_MIN))),
                    pass_ulp=ok & ((x == np.nextafter(np.float64(w), 0)) | (y == np.nextafter(np.float64(h), 0))),
                    pass_zero=ok & ((x == 0) | (y == 0)),
                    pass_last=ok & ((x == w - 1) | (y == h - 1)),
                    pass_integer=ok & (x == np.floor(x)) & (y == np.floor(y)))


def tap_classes(planes, ok, y, x):
    """bilinearInterp's four taps at the in-image positions `ok` of (h, w) planes (utils.h:182-217): where a tap that is Inf or NaN in one of the planes
    carries the weight zero.  edge_zero_tap: on the last row or column, where the weight is zero by rule; zero_tap: anywhere (an integer coordinate as well)"""
    h, w = planes[0].shape
    y, x = np.where(ok, y, 0.0), np.where(ok, x, 0.0)
    x0, y0 = x.astype(np.int64), y.astype(np.int64)
    assert np.all((x0 >= 0) & (x0 < w) & (y0 >= 0) & (y0 < h))
    wx, wy = np.where(x0 + 1 < w, x - x0, 0.0), np.where(y0 + 1 < h, y - y0, 0.0)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    hit = np.zeros(np.shape(ok), bool)
    for p in planes:
        p = np.asarray(p, np.float64)
        for wgt, val in (((1 - wy) * (1 - wx), p[y0, x0]), ((1 - wy) * wx, p[y0, x1]), (wy * (1 - wx), p[y1, x0]), (wy * wx, p[y1, x1])):
            hit |= (wgt == 0) & ~np.isfinite(val)
    hit &= ok
    return dict(zero_tap=hit, edge_zero_tap=hit & ((x0 == w - 1) | (y0 == h - 1)))


def float_overflow(a):
    """finite doubles whose conversion to float is not: |a| rounds beyond FLT_MAX"""
    a = np.asarray(a, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.isfinite(a) & ~np.isfinite(a.astype(np.float32))


def segments_reached(mask, columns):
    """the 64-column segments in which a class occurs: mask over positions whose image column is `columns` (broadcast against it)"""
    mask = np.asarray(mask, bool)
    cols = np.broadcast_to(np.asarray(columns), mask.shape)
    return sorted(set((cols[mask] // 64).tolist()))


def accumulate_classes(trace, flows, h, w, gw, incr, start):
    """the classes one accumulate() call reached, from its trace (accum_ref.accumulate(trace=[...])): {class: sorted 64-column segments of the start pixel}.
    Positions (the test before a step) and targets (the test before the backward lookup) are classified alike, under 'pos_' and 'tgt_'; 'fwd_' and 'bwd_'
    carry the zero-weight taps of the forward lookup at the position and of the backward one at the target"""
    fu, fv, bu, bv = flows
    col = (np.arange(len(trace[0]["cx"])) % gw) * incr + start
    out = {}

    def note(prefix, classes):
        for k, m in classes.items():
            out.setdefault(prefix + k, set()).update(segments_reached(m, col))

    for f, t in enumerate(trace):
        note("pos_", position_classes(t["act"], t["cy"], t["cx"], h, w))
        note("tgt_", position_classes(t["tgt"], t["ny"], t["nx"], h, w))
        note("fwd_", tap_classes((fu[f], fv[f]), t["ins"], t["cy"], t["cx"]))
        note("bwd_", tap_classes((bu[f], bv[f]), t["tgt_in"], t["ny"], t["nx"]))
    return {k: sorted(v) for k, v in out.items()}


def energy_classes(terms, flows, frames, h, w, incr, start):
    """the classes one energies() call reached, from its terms: {class: sorted 64-column segments of the hypothesis' pixel}.  'pos_': the positions p + U[t - 1] that
    setOcclusions, addJC and addBCGC test (the latter at the hypothesis' own pixel); 'tgt_': p + U[t]; 'break': addJC's `> 1e9`; 'flow_' / 'frame_': zero-weight
    taps of the flow lookups (flows given) and of the frame lookups"""
    U, V = terms["U"], terms["V"]
    J, H = U.shape
    px, py = (terms["hx"] * incr + start).astype(np.float64), (terms["hy"] * incr + start).astype(np.float64)
    out = {}

    def note(prefix, classes):
        for k, m in classes.items():
            out.setdefault(prefix + k, set()).update(segments_reached(m, px.astype(np.int64)))

    every = np.ones(H, bool)
    with np.errstate(invalid="ignore"):
        note("", dict(unknown_break=((U > 1e9) | (V > 1e9)).any(0)))
        for t in range(J):
            xm, ym = (px + U[t - 1], py + V[t - 1]) if t > 0 else (px + 0, py + 0)
            xt, yt = px + U[t], py + V[t]
            note("pos_", position_classes(every, ym, xm, h, w))
            note("tgt_", position_classes(every, yt, xt, h, w))
            ok_t = (yt >= 0) & (yt < h) & (xt >= 0) & (xt < w)
            note("frame_", tap_classes(tuple(frames[t + 1]), ok_t, yt, xt))
            if flows is not None:
                ok_m = (ym >= 0) & (ym < h) & (xm >= 0) & (xm < w) & ~terms["occ"][t]
                note("flow_", tap_classes((flows[0][t], flows[1][t]), ok_m, ym, xm))
    return {k: sorted(v) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------------
# the EpicFlow chain (tests/test_epic_value_ranges.py): edge-cost planes over the whole domain +0 ... +Inf of sfa_epic_nearest_seeds_batch / sfa_epic_batch,
# the seeds that meet their special pixels, and matches at the edges of the clamp
# ------------------------------------------------------------------------------------------------------
EPIC_SIZES = ((136, 24, 300), (12, 10, 26), SMALL + (6,))      # (w, h, seeds): one sweep workgroup each, diagonals of 24, 10 and 4 cells
EPIC_EXPS = (-140, -70, -20, 0, 14, 40, 60)                     # capped at 2^60: 2 * C * C of arg_sweep's two-sided update overflows from C = 2^64
EPIC_TOP = 127                                                  # the sprinkled plane's extra band: two such costs sum past 0x7F7F7F7F and stay finite
EPIC_SPECIALS = np.array([0.0, np.inf, FLT_MAX, SUB_MIN, SUB_MAX, FLT_MIN], np.float32)      # the domain's own: no -0, -Inf, NaN.  In the order seeds are moved onto them


def cost_plain(w, h, seed):
    """uniform(0.05, 1): the magnitudes the rest of the suite feeds the search"""
    return np.random.default_rng(seed).uniform(0.05, 1, (h, w)).astype(np.float32)


def cost_ladder(w, h, seed, exps=EPIC_EXPS, band=None):
    """uniform(0.05, 1) * 2^e, e from `exps` in bands of `band` columns that move on by one band every eight rows: every diagonal of the sweep and every 64
    consecutive pixels mix the magnitudes.  band: eight columns, or as many as still let a narrower plane hold every exponent (one column at 12 x 10 and
    5 x 4).  The smallest band is subnormal and never 0 (0.05 * 2^-140 > 2^-145)"""
    band = band or min(8, max(1, w // len(exps)))
    e = np.asarray(exps, np.float64)[((np.arange(w)[None, :] // band) + (np.arange(h)[:, None] // 8)) % len(exps)]
    return (cost_plain(w, h, seed).astype(np.float64) * np.exp2(e)).astype(np.float32)


def cost_ladder_sprinkled(w, h, seed):
    """cost_ladder with a further band of 2^127, and EPIC_SPECIALS (+0, +Inf, FLT_MAX, 2^-149, the largest subnormal, FLT_MIN) on one pixel in sixteen -- each of
    them at least once, whatever the size"""
    c = cost_ladder(w, h, seed, EPIC_EXPS + (EPIC_TOP,))
    rng = np.random.default_rng(seed + 1000)
    pos = rng.choice(w * h, max(len(EPIC_SPECIALS), (w * h) // 16), replace=False)
    c.reshape(-1)[pos] = EPIC_SPECIALS[np.arange(len(pos)) % len(EPIC_SPECIALS)]
    return c


def cost_zeros(w, h, seed, zero=0.0):
    """cost_plain with a third of the pixels `zero`"""
    c = cost_plain(w, h, seed)
    c[np.random.default_rng(seed + 2000).uniform(0, 1, (h, w)) < 1.0 / 3] = np.float32(zero)
    return c


def cost_minus_zeros(w, h, seed):
    """cost_zeros with -0.0 for +0.0, from the same random stream"""
    return cost_zeros(w, h, seed, zero=-0.0)


def epic_seeds(w, h, ns, seed, cost=None):
    """(ns, 2) int32 random (x, y).  cost: the leading seeds are moved onto the first pixel of each EPIC_SPECIALS value the plane holds -- of the first
    ns // 2 kinds where the seeds are few"""
    rng = np.random.default_rng(seed + 3000)
    s = np.stack([rng.integers(0, w, ns), rng.integers(0, h, ns)], 1).astype(np.int32)
    if cost is not None:
        bits = np.ascontiguousarray(cost, np.float32).view(np.uint32).reshape(-1)
        k = 0
        for v in EPIC_SPECIALS[:max(1, ns // 2)]:
            at = np.flatnonzero(bits == v.view(np.uint32))
            if len(at):
                s[k] = (at[0] % w, at[0] // w)
                k += 1
    return s


def epic_edge_matches(w, h):
    """matches (x1 y1 x2 y2) at the edges of the clamp to [0, w - 1] x [0, h - 1], all finite: +-FLT_MAX, -0.0 (max(0.f, -0.f) is +0), subnormal coordinates,
    w - 1 and h - 1 and the floats after them"""
    f = np.float32
    wx, hy = f(w - 1), f(h - 1)
    return np.array([[FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX], [-FLT_MAX, FLT_MAX, 3, 2], [FLT_MAX, -FLT_MAX, 1, 1], [-0.0, -0.0, 2.5, 1.5], [-0.0, 3, -0.0, 2],
                     [SUB_MIN, SUB_MAX, 1.25, 0.75], [-SUB_MIN, -SUB_MAX, SUB_MAX, SUB_MIN], [wx, hy, wx - 1, hy - 1], [np.nextafter(wx, f(np.inf)), 1, wx, 2],
                     [2, np.nextafter(hy, f(np.inf)), 3, hy], [np.nextafter(wx, f(0)), np.nextafter(hy, f(0)), wx, hy]], np.float32)


def list_classes(index, dist):
    """what a nearest-seeds result holds, as counts: exact zeros, subnormals, +Inf, absent entries (-1 / 0x7F7F7F7F), and neighbouring entries of a row that tie"""
    bits = np.ascontiguousarray(dist, np.float32).view(np.uint32)
    present = index >= 0
    tie = (bits[:, 1:] == bits[:, :-1]) & present[:, 1:] & present[:, :-1]
    return dict(zero=int((present & (dist == 0)).sum()), subnormal=int((present & is_subnormal(dist)).sum()), inf=int((present & (dist == np.inf)).sum()),
                absent=int((~present).sum()), ties=int(tie.sum()))
