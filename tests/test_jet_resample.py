"""Jets of another size than the tracking frames: sfa_jet_flow_resample, sfa_jet_occlusion_decode (slowflow_amd/csrc/jet_resample.hip) and the
`source=` / `flow_source=` forms of accumulate_consistent and hypothesis_energies, against tests/jet_resample_ref.py, a scalar numpy restatement of
dense_tracking.cpp:1134-1146 and :1171-1189 with cv::resize's documented arithmetic (OpenCV is not in the tree: parity unpinned).

CPU: the size rule, the linear resize on affine fields, the cubic decode on constant images and at rescale 1.  GPU: kernel == restatement with
np.array_equal, the chained calls against accum_ref / energy_ref fed the restatement's doubles, identity sources against the existing calls bit for
bit, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import slowflow_amd as sfa
from accum_ref import accumulate, decode_occlusion
from energy_ref import derivatives, energies
from jet_resample_ref import (crop_rect, decode_occlusion_scaled, resample_flow, rescale_of, resize_cubic_8u, resize_linear_64f, target_size)
from test_accumulate import smooth_flows
from test_hypothesis_energy import random_case, random_params, to_gpu_layout


# ---- CPU -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cw, ch, w, want", [(256, 109, 1024, (1024, 436)), (13, 10, 52, (52, 40)), (9, 7, 30, (30, 23)), (256, 109, 1023, (1023, 436))])
def test_size_rule(cw, ch, w, want):
    """lrint(cw * rescale) x lrint(ch * rescale) with rescale = (1.0f * w) / cw: the first three are consistent with their frames, and 256 x 109
    against a width of 1023 gives 1023 x 436, which the reference accepts"""
    r = rescale_of(w, cw)
    assert r.dtype == np.float32 and target_size(cw, ch, r) == want
    assert sfa.jet_source(cw, ch, w=w).target() == want


def test_size_rule_rounds_halves_to_even():
    assert target_size(12, 5, 0.5) == (6, 2)                                      # 2.5 -> 2 (cvRound), not 3
    assert sfa.jet_source(12, 5, rescale=0.5).target() == (6, 2)


@pytest.mark.parametrize("sw, sh, rescale", [(9, 7, 4.0), (9, 7, 3.0), (9, 7, np.float32(30) / np.float32(9))])
def test_linear_resize_reproduces_an_affine_field(sw, sh, rescale):
    """a field affine in (x, y) is reproduced at the source coordinate (d + 0.5) / rescale - 0.5 wherever no tap is clamped"""
    y, x = np.mgrid[0:sh, 0:sw].astype(np.float64)
    src = 0.75 * x - 1.25 * y + 3.0
    out = resize_linear_64f(src, rescale)
    dw, dh = target_size(sw, sh, rescale)
    assert out.shape == (dh, dw)
    scale = 1.0 / np.float64(np.float32(rescale))
    X, Y = (np.arange(dw) + 0.5) * scale - 0.5, (np.arange(dh) + 0.5) * scale - 0.5
    inner_x, inner_y = (X >= 0) & (X <= sw - 1), (Y >= 0) & (Y <= sh - 1)
    assert inner_x.sum() > dw // 2 and inner_y.sum() > dh // 2
    want = 0.75 * X[None, :] - 1.25 * Y[:, None] + 3.0
    sel = inner_y[:, None] & inner_x[None, :]
    # the float coordinate and weights carry 2^-24 relative to a coordinate below 16: 1e-5 is two orders above that, 0.05 px of slope below
    assert np.abs(out - want)[sel].max() < 1e-5
    # on the clamped border the value is the border pixel's
    assert out[0, 0] == src[0, 0] and out[-1, -1] == src[-1, -1]


@pytest.mark.parametrize("rescale", [4.0, np.float32(30) / np.float32(9), 0.5])
def test_cubic_of_a_constant_image_is_constant(rescale):
    for v in (0, 255):
        img = np.full((7, 9), v, np.uint8)
        assert np.all(resize_cubic_8u(img, rescale) == v)
        assert np.all(decode_occlusion_scaled(img, rescale) == 255 - v)


def test_decode_at_rescale_one_is_todays_decode():
    rng = np.random.default_rng(0)
    img = rng.choice(np.array([0, 127, 255], np.uint8), (11, 14))
    assert np.array_equal(resize_cubic_8u(img, 1.0), img)
    assert np.array_equal(decode_occlusion_scaled(img, 1.0), decode_occlusion(img))


def test_crop_rect_is_the_references_index_rule():
    assert crop_rect((8, 6), (8, 6)) == (4, 3, 8, 6)
    assert crop_rect((8, 6), (7, 5)) == (5, 4, 7, 5)                                # x - 7 / 2 + 8 = x + 5: integer division


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


def padded(a, stride, pad, dtype):
    """(..., h, w) -> (..., h, stride) with the padding filled with `pad`"""
    out = np.full(a.shape[:-1] + (stride,), pad, dtype)
    out[..., :a.shape[-1]] = a
    return out


def random_field(rng, n, sh, sw):
    return (rng.standard_normal((n, sh, sw)) * 3).astype(np.float32), (rng.standard_normal((n, sh, sw)) * 3).astype(np.float32)


FLOW_CASES = [  # source w, h, target width or factor, crop (center, extent), n
    (5, 4, dict(rescale=4.0), None, 1), (7, 5, dict(rescale=3.0), None, 3), (9, 7, dict(w=30), None, 1), (2, 2, dict(rescale=4.0), None, 1),
    (1, 3, dict(rescale=4.0), None, 3), (12, 8, dict(rescale=0.5), None, 1), (16, 12, dict(rescale=4.0), ((8, 6), (8, 6)), 3),
    (16, 12, dict(rescale=4.0), ((8, 6), (7, 5)), 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("sw, sh, factor, crop, n", FLOW_CASES)
def test_flow_resample_equals_restatement(ctx, sw, sh, factor, crop, n):
    rng = np.random.default_rng(sw * 100 + sh + n)
    u, v = random_field(rng, n, sh, sw)
    rect = crop_rect(*crop) if crop else None
    stride = sfa.stride_of(sw) + 4
    src = sfa.jet_source(sw, sh, stride, crop=rect, **factor)
    gu, gv = ctx.jet_flow_resample(padded(u, stride, np.nan, np.float32), padded(v, stride, np.nan, np.float32), src)   # NaN in the padding: never read
    for k in range(n):
        ru, rv = resample_flow(u[k], v[k], src.rescale, rect)
        assert ru.shape == src.target()[::-1]
        assert np.array_equal(gu[k], ru) and np.array_equal(gv[k], rv)


@pytest.mark.gpu
@pytest.mark.parametrize("sw, sh, factor", [(5, 4, dict(rescale=4.0)), (9, 7, dict(w=30)), (70, 9, dict(rescale=1.0))])
def test_occlusion_decode_equals_restatement(ctx, sw, sh, factor):
    rng = np.random.default_rng(sw)
    n = 2
    img = rng.choice(np.array([0, 127, 255], np.uint8), (n, sh, sw))
    stride = sfa.stride_of(sw) + 4
    src = sfa.jet_source(sw, sh, stride, **factor)
    got = ctx.jet_occlusion_decode(padded(img, stride, 77, np.uint8), src)
    for k in range(n):
        assert np.array_equal(got[k], decode_occlusion_scaled(img[k], src.rescale))
        if src.rescale == 1.0:
            assert np.array_equal(got[k], decode_occlusion(img[k]))                  # the bits of today's decode


SW, SH, TW, TH = 13, 10, 52, 40


def quarter_jets(rng, FF, occ):
    """FF steps of 13 x 10 flows whose rescaled steps stay mostly consistent at 52 x 40, raw occlusion images, and both resampled by the restatement"""
    fu, fv, bu, bv = smooth_flows(rng, FF, SH, SW, 0.4)
    raw = rng.choice(np.array([0, 0, 0, 127, 255], np.uint8), (FF, SH, SW)) if occ else None
    r = rescale_of(TW, SW)
    big = [np.stack([resample_flow(a[f], b[f], r)[c] for f in range(FF)]) for a, b, c in ((fu, fv, 0), (fu, fv, 1), (bu, bv, 0), (bu, bv, 1))]
    masks = np.stack([decode_occlusion_scaled(raw[f], r) for f in range(FF)]) if occ else None
    return (fu, fv, bu, bv, raw), big, masks


@pytest.fixture(scope="module")
def quarter_case():
    """one reference per (occ): computed once, shared, left unchanged"""
    out = {}
    for occ in (False, True):
        small, big, masks = quarter_jets(np.random.default_rng(5 + occ), 3, occ)
        ref = {skip: accumulate(big[0], big[1], big[2], big[3], masks, 0.5, skip, False) for skip in (0, 1)}   # the restatement's planes, fed as doubles
        out[occ] = (small, ref)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("occ", [False, True])
@pytest.mark.parametrize("all_steps", [False, True])
def test_accumulate_with_a_source_equals_the_restated_chain(ctx, quarter_case, skip, occ, all_steps):
    (fu, fv, bu, bv, raw), ref = quarter_case[occ]
    stride = sfa.stride_of(SW) + 4
    src = sfa.jet_source(SW, SH, stride, w=TW)
    assert src.rescale == 4.0 and src.target() == (TW, TH)
    planes = [padded(a[None], stride, np.nan, np.float32) for a in (fu, fv, bu, bv)]
    au, av, tr = ctx.accumulate_consistent(*planes, TW, 0.5, skip, False, all_steps=all_steps, masks=padded(raw[None], stride, 9, np.uint8) if occ else None,
                                           source=src)
    ru, rv, rt = ref[skip]
    assert 0 < (rt == 3).sum() < rt.size                                            # some trajectories fully tracked, some not
    sel = slice(None) if all_steps else slice(-1, None)
    assert np.array_equal(au[0], ru[sel]) and np.array_equal(av[0], rv[sel]) and np.array_equal(tr[0], rt)


@pytest.mark.gpu
def test_accumulate_with_an_identity_source_is_the_existing_call(ctx):
    rng = np.random.default_rng(21)
    w, h, FF = 45, 23, 4
    fu, fv, bu, bv = smooth_flows(rng, FF, h, w, 3.0)
    raw = rng.choice(np.array([0, 0, 0, 255], np.uint8), (FF, h, w))
    stride = sfa.stride_of(w)
    planes = [padded(a[None], stride, 0, np.float32) for a in (fu, fv, bu, bv)]
    masks = np.stack([decode_occlusion(raw[f]) for f in range(FF)])
    old = ctx.accumulate_consistent(*planes, w, 0.5, 1, False, masks=padded(masks[None], stride, 0, np.uint8))
    ms = []
    new = ctx.accumulate_consistent(*planes, w, 0.5, 1, False, masks=padded(raw[None], stride, 0, np.uint8), source=sfa.jet_source(w, h, stride), stage_ms=ms)
    for a, b in zip(old, new):
        assert np.array_equal(a, b)
    assert len(ms) == 2 and ms[1] > 0


@pytest.mark.gpu
def test_energies_with_a_flow_source_equal_the_restated_chain(ctx, oracle):
    rng = np.random.default_rng(8)
    J = 4
    frames, au, av, tr, _ = random_case(rng, J, J, TH, TW, 1, with_flows=False)
    fu, fv, bu, bv = smooth_flows(rng, J, SH, SW, 0.5)
    r = rescale_of(TW, SW)
    big = tuple(np.stack([resample_flow(a[f], b[f], r)[c] for f in range(J)]) for a, b, c in ((fu, fv, 0), (fu, fv, 1), (bu, bv, 0), (bu, bv, 1)))
    p = random_params(rng, 1, penalty=1)
    dx, dy = derivatives(oracle, frames, TW)
    e_ref, b_ref, _ = energies(p, J, au, av, tr, frames, dx, dy, big)
    fr, _ = to_gpu_layout(frames, None)
    stride = sfa.stride_of(SW) + 4
    small = [padded(a[None], stride, np.nan, np.float32) for a in (fu, fv, bu, bv)]
    e, b = ctx.hypothesis_energies(p.to_c(sfa), J, au[None], av[None], tr[None], fr, TW, small, flow_source=sfa.jet_source(SW, SH, stride, w=TW))
    assert np.isfinite(e_ref).sum() > 0
    assert np.array_equal(b[0], b_ref) and np.array_equal(e[0], e_ref)


@pytest.mark.gpu
def test_energies_with_an_identity_source_are_the_existing_call(ctx):
    rng = np.random.default_rng(9)
    J, h, w = 4, 17, 33
    frames, au, av, tr, flows = random_case(rng, J, J, h, w, 1)
    p = random_params(rng, 1, penalty=1)
    fr, fl = to_gpu_layout(frames, flows)
    old = ctx.hypothesis_energies(p.to_c(sfa), J, au[None], av[None], tr[None], fr, w, fl, adapted=True)
    new = ctx.hypothesis_energies(p.to_c(sfa), J, au[None], av[None], tr[None], fr, w, fl, adapted=True, flow_source=sfa.jet_source(w, h, fr.shape[-1]))
    for a, b in zip(old, new):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_refusals_name_the_argument_and_leave_the_context_working(ctx):
    L = sfa.lib()
    _f = C.POINTER(C.c_float)
    L.sfa_jet_flow_resample.argtypes = [C.c_void_p, C.c_int, C.POINTER(sfa.JetSource), C.POINTER(_f), C.POINTER(_f), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.sfa_accumulate_consistent_scaled.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(sfa.JetSource)] + [C.POINTER(_f)] * 4 + [
        C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    plane = np.zeros((8, 8), np.float32)
    p = (_f * 1)(sfa.fptr(plane))
    out = np.zeros(64 * 64, np.float64)
    tr = np.zeros(64 * 64, np.int32)
    cases = [(sfa.jet_source(8, 8, rescale=4.0), 32, 31, "is 32 x 32, not the target 32 x 31"),   # size mismatch: both sizes named
             (sfa.jet_source(8, 8, crop=(4, 4, 8, 4), rescale=4.0), 32, 16, "crop"),         # the crop leaves the flow
             (sfa.jet_source(8, 8, crop=(-1, 0, 4, 4), rescale=4.0), 16, 16, "crop"),
             (sfa.jet_source(8, 8, rescale=0.0), 32, 32, "rescale"), (sfa.jet_source(8, 8, rescale=-4.0), 32, 32, "rescale")]
    for src, w, h, word in cases:
        for rc in (L.sfa_jet_flow_resample(ctx.h, 1, C.byref(src), p, p, w, h, out.ctypes.data, out.ctypes.data),
                   L.sfa_accumulate_consistent_scaled(ctx.h, 1, 1, w, h, C.byref(src), p, p, p, p, None, 1.0, 0, 0, 1, out.ctypes.data, out.ctypes.data,
                                                      tr.ctypes.data, None)):
            assert rc == -1                                                          # SFA_ERR_ARG
            msg = L.sfa_last_error(ctx.h).decode()
            assert "source" in msg and word in msg, msg
    # a cropped occlusion image is refused by name
    with pytest.raises(sfa.SlowflowError, match="cropped occlusions"):
        ctx.jet_occlusion_decode(np.zeros((1, 8, 8), np.uint8), sfa.jet_source(8, 8, crop=(2, 2, 4, 4), rescale=2.0))
    # the context still works
    u, v = ctx.jet_flow_resample(np.ones((1, 8, 8), np.float32), np.zeros((1, 8, 8), np.float32), sfa.jet_source(8, 8, rescale=4.0))
    assert np.all(u == 4.0) and np.all(v == 0.0)
