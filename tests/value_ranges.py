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
