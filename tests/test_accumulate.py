"""dense_tracking's first stage: sfa_accumulate_consistent (slowflow_amd/csrc/accumulate.hip) and the accumulate program against tests/accum_ref.py,
a float64 restatement of accumulateConsistentBatches (reference utils/utils.cpp:517-617) and bilinearInterp<double> (utils/utils.h:182-217).

CPU: the vectorised restatement against the scalar one, hand-worked cases, every quirk pinned by at least one case, the grid rule against
sfa_accumulate_grid, the occlusion-mask decoding of a driver-written .pgm.  GPU: the kernel == the restatement (IEEE equality on acc_u, acc_v and
tracked), batching, NaN padding, all_steps, bad arguments, and the program end to end."""
import ctypes as C
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import slowflow_amd as sfa
from accum_ref import QUIRKS, accumulate, accumulate_scalar, decode_occlusion, grid, median3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
PROGRAM = os.path.join(HOST, "accumulate")


@pytest.fixture(scope="module")
def host_build():
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return HOST


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
def uniform(FF, h, w, u, v):
    """FF steps of a constant (u, v) field, fp32 (FF, h, w) planes"""
    return np.full((FF, h, w), u, np.float32), np.full((FF, h, w), v, np.float32)


def smooth_flows(rng, FF, h, w, scale):
    """smooth random forward flows of magnitude ~scale and backward flows near their negatives (some steps consistent, some not)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    fu, fv, bu, bv = (np.zeros((FF, h, w), np.float32) for _ in range(4))
    for f in range(FF):
        a = rng.uniform(0.5, 3, 4)
        p = rng.uniform(0, 6.3, 4)
        fu[f] = scale * np.sin(a[0] * x / max(w, 1) * 6.3 + p[0]) * np.cos(a[1] * y / max(h, 1) * 6.3 + p[1])
        fv[f] = scale * np.cos(a[2] * x / max(w, 1) * 6.3 + p[2]) * np.sin(a[3] * y / max(h, 1) * 6.3 + p[3])
        noise = rng.standard_normal((2, h, w)) * rng.choice([0.01, 0.3, 2.0])
        bu[f] = -fu[f] + noise[0]
        bv[f] = -fv[f] + noise[1]
    return fu, fv, bu, bv


def random_masks(rng, FF, h, w, p=0.1):
    return np.where(rng.random((FF, h, w)) < p, 0, 255).astype(np.uint8)


# ---- CPU: the two restatements agree --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_vectorised_restatement_equals_scalar(seed):
    rng = np.random.default_rng(seed)
    FF, h, w = int(rng.integers(1, 6)), int(rng.integers(1, 14)), int(rng.integers(1, 16))
    skip = int(rng.integers(0, min(3, h, w)))
    fu, fv, bu, bv = smooth_flows(rng, FF, h, w, float(rng.choice([0.4, 2.0, 6.0])))
    masks = random_masks(rng, FF, h, w, 0.2) if seed % 2 else None
    eps, discard = float(rng.choice([0.0, 0.5, 1.0, 1e30])), bool(seed % 3 == 0)
    a = accumulate(fu, fv, bu, bv, masks, eps, skip, discard)
    b = accumulate_scalar(fu, fv, bu, bv, masks, eps, skip, discard)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


# ---- CPU: hand-worked cases.  Each takes `off` (quirks switched off in the restatement) and asserts the reference's behaviour. --------------------
def case_translation(off=()):
    """pure translation: every pixel whose trajectory stays inside accumulates exactly (f + 1) t and stays fully tracked"""
    fu, fv = uniform(4, 12, 12, 0.5, 0.25)
    au, av, tr = accumulate(fu, fv, -fu, -fv, None, 0.0, 0, False, off)
    for f in range(4):
        assert np.all(au[f, :8, :8] == (f + 1) * 0.5) and np.all(av[f, :8, :8] == (f + 1) * 0.25)
    assert np.all(tr[:8, :8] == 4)


def case_broken(k, discard, off=()):
    """the forward flow doubles from step k on while the backward flow stays -t: every step from k fails, tracked == k + 1 (0 with discard) and the
    pixel moves on at constant velocity t (the last consistent vector; forward[0] at the grid point when k == 0)"""
    FF, t = 5, (0.5, 0.5)
    fu, fv = uniform(FF, 16, 16, *t)
    fu[k:] *= 2
    fv[k:] *= 2
    bu, bv = uniform(FF, 16, 16, -t[0], -t[1])
    au, av, tr = accumulate(fu, fv, bu, bv, None, 0.1, 0, discard, off)
    last = (fu[0, 2, 2], fv[0, 2, 2]) if k == 0 else t
    for f in range(FF):
        if k == 0:
            assert au[f, 2, 2] == (f + 1) * last[0] and av[f, 2, 2] == (f + 1) * last[1]
        else:
            assert au[f, 2, 2] == (f + 1) * 0.5 and av[f, 2, 2] == (f + 1) * 0.5
    assert tr[2, 2] == (0 if discard else k + 1)


def case_start_at_first_forward(off=()):
    """k == 0 with a non-uniform first field: constant velocity from step 0 is forward[0] AT the grid point, not zero"""
    fu, fv = uniform(3, 10, 10, 0.5, 0.0)
    fu[0] += np.arange(10, dtype=np.float32)[None, :] * 0.125
    bu, bv = uniform(3, 10, 10, 5.0, 5.0)                                           # never consistent
    au, av, tr = accumulate(fu, fv, bu, bv, None, 0.1, 0, False, off)
    assert au[0, 1, 3] == fu[0, 1, 3] and au[2, 1, 3] == 3 * np.float64(fu[0, 1, 3]) and tr[1, 3] == 1


def case_leaves_image(off=()):
    """t = 3 px right on a 8-wide image: the pixel at x = 6 lands outside after step 0 (diff = vec - last_flow = 0 there: consistent), then moves on at
    constant velocity outside with tracked == 2.  The pixel at x = 0 first fails on the last step: tracked == f + 1 == FF, as if fully tracked"""
    fu, fv = uniform(4, 4, 8, 3.0, 0.0)
    au, av, tr = accumulate(fu, fv, -fu, -fv, None, 0.5, 0, False, off)
    assert [au[f, 1, 6] for f in range(4)] == [3.0, 6.0, 9.0, 12.0]
    assert tr[1, 6] == 2 and tr[1, 0] == 4


def case_leaves_left(off=()):
    """t = -0.75: the pixel at x = 0 reaches -0.75 after step 0, which is outside (>= 0 on the double, not on its truncation)"""
    fu, fv = uniform(3, 4, 6, -0.75, 0.0)
    au, av, tr = accumulate(fu, fv, -fu, -fv, None, 0.5, 0, False, off)
    assert tr[2, 0] == 2 and au[2, 2, 0] == -2.25


def case_occluded(off=()):
    """masks: the pixel (3, 3) seen at step 1 at (3, 3.6) -> truncated to (3, 3), occluded there: tracked == 2, acc[1] still accumulated,
    acc[2:] ZERO; its neighbour (3, 4) reaches (3, 4.6) -- a mask hole at (3, 4) on step 1 would have caught (3, 3) if the lookup rounded"""
    FF = 4
    fu, fv = uniform(FF, 8, 10, 0.6, 0.0)
    masks = np.full((FF, 8, 10), 255, np.uint8)
    masks[1, 3, 3] = 0
    au, av, tr = accumulate(fu, fv, -fu, -fv, masks, 0.5, 0, False, off)
    assert tr[3, 3] == 2 and au[1, 3, 3] == 2 * np.float64(np.float32(0.6))
    assert au[2, 3, 3] == 0 and au[3, 3, 3] == 0 and av[3, 3, 3] == 0
    assert tr[3, 2] == FF and au[3, 3, 2] != 0                                      # (3, 2) is at (3, 2.6) on step 1: (3, 2) is visible
    masks[1, 3, 3] = 255
    masks[1, 3, 4] = 0
    au, av, tr = accumulate(fu, fv, -fu, -fv, masks, 0.5, 0, False, off)
    assert tr[3, 3] == FF and tr[3, 4] == 2


def case_grid_origins(off=()):
    """skip 1, 2, 3: grid pixel (x, y) starts at image pixel (x (skip + 1) + (int)(0.5 skip), ...): origins 0, 1, 1"""
    h, w = 13, 17
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    for skip, origin in ((1, 0), (2, 1), (3, 1)):
        fu = (x * 0.001 + 0.25)[None].astype(np.float32)
        fv = (y * 0.001 + 0.125)[None].astype(np.float32)
        au, av, tr = accumulate(fu, fv, -fu, -fv, None, 1e30, skip, False, off)
        gw, gh = w // (skip + 1), h // (skip + 1)
        assert au.shape == (1, gh, gw)
        assert au[0, 1, 2] == fu[0, 1 * (skip + 1) + origin, 2 * (skip + 1) + origin]
        assert av[0, 1, 2] == fv[0, 1 * (skip + 1) + origin, 2 * (skip + 1) + origin]


def case_last_row_and_column(off=()):
    """at x = w - 1 + 0.5 the weight of the column is 0: the value is the last column's, not a blend with any other"""
    h, w, FF = 3, 4, 2
    fu, fv = uniform(FF, h, w, 0.5, 0.5)
    fu[1, :, 3], fu[1, :, 0] = 0.25, -2.0
    fv[1, 2, :], fv[1, 0, :] = 0.125, -3.0
    au, av, tr = accumulate(fu, fv, -fu, -fv, None, 1e30, 0, False, off)
    assert au[1, 2, 3] == 0.5 + 0.25                                              # at (2.5, 3.5) on step 1: last row and last column
    assert av[1, 2, 3] == 0.5 + 0.125


def case_error_norm(off=()):
    """diff (0.6, 0.6): sqrt(0.72) = 0.85 <= 1 is consistent (an L1 norm, 1.2, would not be)"""
    fu, fv = uniform(3, 8, 8, 0.5, 0.5)
    bu, bv = uniform(3, 8, 8, 0.1, 0.1)
    au, av, tr = accumulate(fu, fv, bu, bv, None, 1.0, 0, False, off)
    assert tr[1, 1] == 3


def case_tracked_once(off=()):
    """the first failure sets tracked; later ones leave it"""
    case_broken(1, False, off)


CASES = [case_translation, lambda off=(): case_broken(2, False, off), lambda off=(): case_broken(2, True, off), lambda off=(): case_broken(0, False, off),
         case_start_at_first_forward, case_leaves_image, case_leaves_left, case_occluded, case_grid_origins, case_last_row_and_column, case_error_norm,
         case_tracked_once]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_hand_worked_case(case):
    CASES[case]()


@pytest.mark.parametrize("quirk", QUIRKS)
def test_each_quirk_is_pinned(quirk):
    """with the quirk switched off in the restatement, at least one hand-worked case fails"""
    failed = []
    for i, c in enumerate(CASES):
        try:
            c(off=(quirk,))
        except AssertionError:
            failed.append(i)
    assert failed, f"no case pins the quirk {quirk}"


def test_grid_rule_matches_the_library():
    for w in (1, 2, 3, 5, 17, 436, 1024, 1025):
        for h in (1, 2, 7, 436):
            for skip in range(0, 6):
                if skip >= min(w, h):
                    with pytest.raises(sfa.SlowflowError):
                        sfa.accumulate_grid(w, h, skip)
                    continue
                gw, gh, incr, start = grid(w, h, skip)
                assert sfa.accumulate_grid(w, h, skip) == (gw, gh)
                assert (gh - 1) * incr + start < h and (gw - 1) * incr + start < w
    for bad in ((0, 5, 0), (5, 0, 0), (5, 5, -1)):
        with pytest.raises(sfa.SlowflowError):
            sfa.accumulate_grid(*bad)


def write_driver_pgm(path, occ):
    """the slow_flow driver's occlusion file (host/slow_flow.cpp: writePGM(offset 1, scale 127.5)) of a label field occ in {-1, +1}"""
    v = np.clip(np.float32(127.5) * (occ.astype(np.float32) + np.float32(1)), 0, 255)
    g = (v + np.float32(0.5)).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (occ.shape[1], occ.shape[0]))
        f.write(g.tobytes())
    return g


def read_pgm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w)


def test_occlusion_decoding_of_a_driver_pgm(host_build, tmp_path):
    """grey 255 = label +1 ("occluded in the future": the forward trajectory disappears) -> 0 after median and 255 - x = occluded; a lone label
    is removed by the median, a block survives; the program decodes as the restatement does"""
    rng = np.random.default_rng(3)
    occ = -np.ones((20, 23), np.int8)
    occ[5:12, 6:15] = 1                                                             # a block occluded in the future
    occ[16, 2] = 1                                                                  # a lone pixel: the median drops it
    occ[0, 0:2] = 1
    occ[rng.integers(0, 20, 6), rng.integers(0, 23, 6)] = 1
    g = write_driver_pgm(tmp_path / "frame_10.pgm", occ)
    assert set(np.unique(g)) <= {0, 255}
    m = decode_occlusion(g)
    assert np.all(m[6:11, 7:14] == 0) and m[16, 2] == 255
    assert np.array_equal(median3(np.full((3, 3), 7, np.uint8)), np.full((3, 3), 7, np.uint8))
    r = subprocess.run([PROGRAM, "-decode_occlusion", str(tmp_path / "frame_10.pgm"), str(tmp_path / "mask.pgm")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_pgm(tmp_path / "mask.pgm"), m)
    # the reference's own form: a P4 bitmap (bit 1 = black = 0 when OpenCV reads it)
    bits = np.packbits(g == 0, axis=1)
    with open(tmp_path / "frame_10.pbm", "wb") as f:
        f.write(b"P4\n%d %d\n" % (g.shape[1], g.shape[0]) + bits.tobytes())
    r = subprocess.run([PROGRAM, "-decode_occlusion", str(tmp_path / "frame_10.pbm"), str(tmp_path / "mask4.pgm")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_pgm(tmp_path / "mask4.pgm"), m)


# ---- GPU: the kernel against the restatement ------------------------------------------------------------------------------------------------------
def gpu_run(ctx, segs, w, eps, skip, discard, all_steps=True, stride=None, pad=0.0):
    """segs: list of (fu, fv, bu, bv, masks) with (FF, h, w) planes -> the library's (acc_u, acc_v, tracked)"""
    FF, h, _ = segs[0][0].shape
    stride = stride or sfa.stride_of(w)
    n = len(segs)
    arrs = [np.full((n, FF, h, stride), pad, np.float32) for _ in range(4)]
    use_m = segs[0][4] is not None
    masks = np.full((n, FF, h, stride), 0 if pad != pad else 255, np.uint8) if use_m else None
    for s, seg in enumerate(segs):
        for k in range(4):
            arrs[k][s, :, :, :w] = seg[k]
        if use_m:
            masks[s, :, :, :w] = seg[4]
    return ctx.accumulate_consistent(*arrs, w, eps, skip, discard, all_steps, masks)


def assert_same(got, ref):
    au, av, tr = got
    ru, rv, rt = ref
    assert au.shape == ru.shape and tr.shape == rt.shape
    assert np.array_equal(au, ru) and np.array_equal(av, rv), f"acc differs at {np.argwhere((au != ru) | (av != rv))[:5]}"
    assert np.array_equal(tr, rt)


SIZES = [(1, 1), (2, 3), (5, 2), (7, 9), (33, 17), (130, 67), (257, 101), (1024, 436)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_kernel_equals_restatement(ctx, size):
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    runs = 0
    for FF in (1, 2, 7, 32):
        for skip in (0, 1, 2):
            if skip >= min(w, h):
                continue
            if w * h > 100000 and (FF, skip) not in ((32, 0), (7, 1), (2, 2), (1, 0)):
                continue                                                            # the restatement's time at 1024 x 436
            eps = [0.0, 1.0, 1e30][runs % 3]
            occ, discard = runs % 2 == 0, runs % 4 in (1, 2)
            scale = [0.5, 3.0, 0.3 * max(w, h)][runs % 3]                           # the last leaves the image within a few steps
            fu, fv, bu, bv = smooth_flows(rng, FF, h, w, scale)
            masks = random_masks(rng, FF, h, w, 0.05) if occ else None
            ref = accumulate(fu, fv, bu, bv, masks, eps, skip, discard)
            got = gpu_run(ctx, [(fu, fv, bu, bv, masks)], w, eps, skip, discard)
            assert_same((got[0][0], got[1][0], got[2][0]), ref)
            runs += 1
    assert runs >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("eps, occ, discard", [(0.0, False, False), (1.0, True, False), (1e30, True, True), (1.0, False, True)])
def test_kernel_parameter_grid(ctx, eps, occ, discard):
    """epsilon 0 / 1 / 1e30, occlusion and discard on and off, on one mid-size case with flows that leave the image"""
    rng = np.random.default_rng(int(eps) % 7 + 3 * occ + 5 * discard)
    w, h, FF = 97, 61, 7
    for skip in (0, 1, 2):
        fu, fv, bu, bv = smooth_flows(rng, FF, h, w, 9.0)
        masks = random_masks(rng, FF, h, w, 0.08) if occ else None
        ref = accumulate(fu, fv, bu, bv, masks, eps, skip, discard)
        got = gpu_run(ctx, [(fu, fv, bu, bv, masks)], w, eps, skip, discard)
        assert_same((got[0][0], got[1][0], got[2][0]), ref)


@pytest.mark.gpu
def test_nan_in_the_stride_padding_changes_nothing(ctx):
    rng = np.random.default_rng(11)
    w, h, FF = 45, 23, 5
    fu, fv, bu, bv = smooth_flows(rng, FF, h, w, 4.0)
    masks = random_masks(rng, FF, h, w, 0.1)
    seg = [(fu, fv, bu, bv, masks)]
    a = gpu_run(ctx, seg, w, 1.0, 1, False, stride=w + 7, pad=0.0)
    b = gpu_run(ctx, seg, w, 1.0, 1, False, stride=w + 7, pad=np.nan)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert_same((a[0][0], a[1][0], a[2][0]), accumulate(fu, fv, bu, bv, masks, 1.0, 1, False))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 64])
def test_segments_in_one_call_equal_single_calls(ctx, n):
    rng = np.random.default_rng(n)
    w, h, FF = 61, 37, 3
    segs = []
    for s in range(n):
        fu, fv, bu, bv = smooth_flows(rng, FF, h, w, [0.5, 3.0, 12.0][s % 3])
        segs.append((fu, fv, bu, bv, random_masks(rng, FF, h, w, 0.05)))
    au, av, tr = gpu_run(ctx, segs, w, 0.5, 1, False)
    for s in range(n):
        one = gpu_run(ctx, [segs[s]], w, 0.5, 1, False)
        assert np.array_equal(au[s], one[0][0]) and np.array_equal(av[s], one[1][0]) and np.array_equal(tr[s], one[2][0])
    assert_same((au[n - 1], av[n - 1], tr[n - 1]), accumulate(*segs[n - 1], 0.5, 1, False))


@pytest.mark.gpu
def test_last_step_only_is_the_last_plane(ctx):
    rng = np.random.default_rng(5)
    w, h, FF = 80, 50, 6
    segs = [(*smooth_flows(rng, FF, h, w, 5.0), random_masks(rng, FF, h, w, 0.05)) for _ in range(2)]
    full = gpu_run(ctx, segs, w, 1.0, 0, True, all_steps=True)
    last = gpu_run(ctx, segs, w, 1.0, 0, True, all_steps=False)
    assert last[0].shape == (2, 1, h, w)
    assert np.array_equal(last[0][:, 0], full[0][:, -1]) and np.array_equal(last[1][:, 0], full[1][:, -1])
    assert np.array_equal(last[2], full[2])


@pytest.mark.gpu
def test_bad_arguments_return_error_codes(ctx):
    L = sfa.lib()
    _f = C.POINTER(C.c_float)
    _u8 = C.POINTER(C.c_ubyte)
    L.sfa_accumulate_consistent.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(_f)] * 4 + [
        C.POINTER(_u8), C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    plane = np.zeros((8, 8), np.float32)
    p = (_f * 4)(*[sfa.fptr(plane)] * 4)
    out = np.zeros(4096, np.float64)
    tr = np.zeros(4096, np.int32)

    def call(n=1, FF=1, w=8, h=8, stride=8, ptrs=p, skip=0, masks=None, outp=True):
        return L.sfa_accumulate_consistent(ctx.h, n, FF, w, h, stride, ptrs, ptrs, ptrs, ptrs, masks, 1.0, skip, 0, 1,
                                           out.ctypes.data if outp else None, out.ctypes.data, tr.ctypes.data)

    assert call() == 0
    for kw in (dict(n=0), dict(FF=0), dict(w=0), dict(h=0), dict(stride=7), dict(skip=-1), dict(skip=8), dict(outp=False), dict(ptrs=None),
               dict(ptrs=(_f * 4)(sfa.fptr(plane), None, None, None), n=2), dict(masks=(_u8 * 1)(None))):
        assert call(**kw) == -1, kw                                                # SFA_ERR_ARG
        assert L.sfa_last_error(ctx.h)


# ---- the program, end to end ----------------------------------------------------------------------------------------------------------------------
def write_flo(path, u, v):
    h, w = u.shape
    with open(path, "wb") as f:
        f.write(struct.pack("<fii", 202021.25, w, h))
        f.write(np.stack([u, v], -1).astype("<f4").tobytes())


def read_flo(path):
    data = open(path, "rb").read()
    tag, w, h = struct.unpack("<fii", data[:12])
    assert tag == np.float32(202021.25)
    uv = np.frombuffer(data[12:], "<f4").reshape(h, w, 2)
    return uv[..., 0], uv[..., 1]


W, H = 53, 29
# two rates as slow_flow writes them: jet_fps 100 and 200 at max_fps 200, slow_flow_S 3 (steps 2); ref_fps 25 -> Jets = 100 / (25 * 2) = 2, skip 2,
# r_Jets 2 and 4, r_skip 2 and 1; start 10, ref_fps_F 2 -> sequence starts 10 and 18
RATES = [dict(name="low", fps=100, S=3), dict(name="high", fps=200, S=3)]


def make_jets(root, seed=0):
    rng = np.random.default_rng(seed)
    truth = {}
    for r, rate in enumerate(RATES):
        d = root / rate["name"]
        (d / "occlusion").mkdir(parents=True)
        (d / "config.cfg").write_text("# slow flow\nslow_flow_S\t%d\njet_fps\t%d\n" % (rate["S"], rate["fps"]))
        r_steps, r_skip = rate["S"] - 1, 200 // rate["fps"]
        FF = int(np.float32(np.float32(rate["fps"]) / np.float32(100)) * np.float32(2))
        for start in (10, 18):
            fu, fv, _, _ = smooth_flows(rng, FF, H, W, 0.8)
            bu = -fu + (rng.standard_normal(fu.shape) * 0.05).astype(np.float32)   # mostly consistent: some pixels fully tracked, others not
            bv = -fv
            masks = []
            for f in range(FF):
                a = start + f * r_steps * r_skip
                write_flo(d / ("frame_%d.flo" % a), fu[f], fv[f])
                write_flo(d / ("frame_%d_back.flo" % (a + r_steps * r_skip)), bu[f], bv[f])
                occ = np.where(rng.random((H, W)) < 0.02, 1, -1).astype(np.int8)
                occ[3:9, 4:12] = 1
                masks.append(decode_occlusion(write_driver_pgm(d / "occlusion" / ("frame_%d.pgm" % a), occ)))
            truth[r, start] = (fu, fv, bu, bv, np.stack(masks))
    return truth


def write_cfg(root, out, extra=""):
    lines = ["jet_estimation\t%s/" % (root / "low"), "jet_estimation\t%s/" % (root / "high"), "flow_format\tframe_%i", "output\t%s" % out, "start\t10",
             "ref_fps\t25", "ref_fps_F\t2", "max_fps\t200", "acc_skip_pixel\t1", "acc_occlusion\t1", "acc_discard_inconsistent\t0",
             "acc_consistency_threshold\t0.5", "acc_epic_interpolation\t1\t# not this stage"]
    cfg = root / "dense_tracking.cfg"
    cfg.write_text("\n".join(lines) + "\n" + extra)
    return cfg


@pytest.mark.gpu
def test_program_end_to_end(host_build, tmp_path):
    truth = make_jets(tmp_path)
    out = tmp_path / "result"
    cfg = write_cfg(tmp_path, out)
    r = subprocess.run([PROGRAM, str(cfg)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    run = json.load(open(out / "accumulated" / "run.json"))
    assert run["Jets"] == 2 and run["steps"] == 2 and run["skip"] == 2 and run["calls"] == 2
    assert len(run["segments"]) == 4
    for seg in run["segments"]:
        fu, fv, bu, bv, masks = truth[seg["rate"], seg["sequence_start"]]
        au, av, tr = accumulate(fu, fv, bu, bv, masks, 0.5, 1, False)
        FF = fu.shape[0]
        assert seg["FF"] == FF
        u, v = read_flo(out / "accumulated" / str(seg["rate"]) / ("frame_%d.flo" % seg["sequence_start"]))
        assert np.array_equal(u, au[-1].astype(np.float32)) and np.array_equal(v, av[-1].astype(np.float32))
        t = read_pgm(out / "accumulated" / str(seg["rate"]) / ("tracked_%d.pgm" % seg["sequence_start"]))
        assert np.array_equal(t, np.where(tr == FF, 255, 255 * tr // FF).astype(np.uint8))
        assert seg["created"] == int((tr == FF).sum()) and seg["rejected"] == tr.size - seg["created"]
        assert 0 < seg["created"] < tr.size
    assert "trajectory hypotheses generated!" in r.stdout


@pytest.mark.gpu
def test_program_select_resume_and_missing_files(host_build, tmp_path):
    make_jets(tmp_path, seed=1)
    out = tmp_path / "result"
    cfg = write_cfg(tmp_path, out)
    r = subprocess.run([PROGRAM, str(cfg), "-select", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    written = sorted(p.name for p in (out / "accumulated").rglob("*.flo"))
    assert written == ["frame_18.flo", "frame_18.flo"]
    before = (out / "accumulated" / "1" / "frame_18.flo").stat().st_mtime_ns
    r = subprocess.run([PROGRAM, str(cfg), "-resume"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("already exists!") == 2
    assert (out / "accumulated" / "1" / "frame_18.flo").stat().st_mtime_ns == before
    run = json.load(open(out / "accumulated" / "run.json"))
    assert sorted((s["rate"], s["sequence_start"]) for s in run["segments"]) == [(0, 10), (1, 10)] and len(run["skipped"]) == 2
    # without -resume the reference never writes into an existing folder: result_1
    r = subprocess.run([PROGRAM, str(cfg), "-select", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and (tmp_path / "result_1" / "accumulated" / "0" / "frame_10.flo").exists()
    # a missing flow names the file and exits with status 2
    missing = tmp_path / "high" / "frame_14_back.flo"
    missing.unlink()
    r = subprocess.run([PROGRAM, str(cfg), "-select", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and str(missing) in r.stderr.replace("//", "/")
