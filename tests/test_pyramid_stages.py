"""The coarse-to-fine pyramid, stage by stage, against the oracle -- bit for bit, no tolerance anywhere but in (e), which is the path's own TOL_UV.

The kernels: k_gauss_h / k_gauss_v (every radius 1 .. 16), k_pyr_down (every shipped instance R1 .. R8, every tile height, the 40-60 KB zone of LDS, the
fall-backs to the two kernels), k_resize and k_resize_flow (up and down, post_x != post_y).  Inputs are white noise, so that every tap and every bilinear weight
shows in the result: a wrong border pixel or tile seam is a different bit, not 1e-3 of a smooth frame.

(a) sfa_gaussian_blur                     vs orc_gaussian_blur_cv
(b) sfa_pyramid_down (hook: one step)     vs orc_resize_linear_cv(orc_gaussian_blur_cv), and fused == SFA_PYRAMID_UNFUSED
(c) sfa_resize_flow (hook)                vs orc_resize_linear_cv * fp32 factor
(d) sfa_job_download_level_frame (hook)   vs orc_variational's own construction (slowflow_oracle.c, the pyramid loop of orc_variational) level by level
(e) a non-zero initial flow through three levels vs orc_variational
(f) refusals: p_scale outside what the kernels hold, bad indices of the hook"""
import ctypes as C

import numpy as np
import pytest

import slowflow_amd as sfa
from synth import noise_color, noise_plane, smooth_noise_color
from test_gpu_parity import TOL_UV, c_, mk_params, normalized_frames, run_both, valid

pytestmark = pytest.mark.gpu
SFA_ERR_ARG = -1        # include/slowflow_amd.h


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


# ---- (a) the blur at every radius -------------------------------------------------------------------------------------------------------
# ksize = cvRound(8 sigma + 1) | 1: radii 1, 2, 3, 4, 5, 6, 7, 8 (what k_pyr_down's instances cover), then 9, 12, 16 (k_gauss_h / k_gauss_v only; 16 is the widest)
SIGMAS = [(0.3, 1), (0.5, 2), (0.745356, 3), (1.0, 4), (1.2, 5), (1.4, 6), (1.7, 7), (2.0, 8), (2.3, 9), (3.0, 12), (3.9, 16)]


@pytest.mark.parametrize("w,h", [(67, 45), (5, 4)])                  # 5 x 4: narrower and lower than every kernel but the first
@pytest.mark.parametrize("sigma,radius", SIGMAS)
def test_gaussian_blur_every_radius(ctx, oracle, w, h, sigma, radius):
    assert (int(np.rint(float(np.float32(sigma)) * 8 + 1)) | 1) // 2 == radius
    src = noise_plane(np.random.default_rng(1000 * radius + w), w, h, 0, 255)
    a = oracle.gaussian_blur_cv(src, w, sigma)
    b = ctx.gaussian_blur(c_(src), w, sigma)
    assert np.array_equal(valid(a, w), valid(b, w))


def test_gaussian_blur_refuses_more_than_33_taps(ctx, oracle):
    src = noise_plane(np.random.default_rng(3), 67, 45, 0, 255)
    with pytest.raises(sfa.SlowflowError) as e:
        ctx.gaussian_blur(c_(src), 67, 4.2)
    assert "-> %d" % SFA_ERR_ARG in str(e.value) and "sigma" in str(e.value)
    assert np.array_equal(valid(oracle.gaussian_blur_cv(src, 67, 3.9), 67), valid(ctx.gaussian_blur(c_(src), 67, 3.9), 67))   # the context goes on working


# ---- (b) one pyramid step -----------------------------------------------------------------------------------------------------------------
# (sw, sh, dw, dh, sigma), then what launch_pyr_down must decide for it: (1, td, LDS bytes) or (0, 0, 0) for the two kernels.  The figures are worked out by hand
# from the launcher's rule, not copied from a run: CM = the tile's 64 columns' footprint ceil(64 sw / dw) + 2, + 3 for the aligned start, rounded up to 4;
# CS = CM + 2 r rounded up to 4, + 4; RM = ceil(td sh / dh) + 2; RS = RM + 2 r; bytes = 4 (RS CS + RS CM + 3 td); td = the first of 32, 16, 8 at <= 40 KB, else 8;
# above 60 KB, or r > 8: the two kernels.
PYR_STEPS = [
    ((131, 97, 118, 87, 0.3), (1, 32, 27264)),          # R1
    ((131, 97, 118, 87, 0.5), (1, 32, 28608)),          # R2
    ((131, 97, 118, 87, 0.745356), (1, 32, 30656)),     # R3
    ((200, 150, 150, 112, 0.9), (1, 16, 25280)),        # R4
    ((97, 61, 48, 30, 1.2), (1, 8, 33504)),             # R5
    ((131, 97, 100, 80, 1.4), (1, 16, 27392)),          # R6
    ((131, 97, 110, 85, 1.7), (1, 32, 40240)),          # R7, 32 rows at 40 240 B: the largest footprint that keeps four blocks per CU
    ((131, 97, 110, 85, 2.0), (1, 16, 28016)),          # R8
    ((131, 97, 110, 85, 2.3), (0, 0, 0)),               # radius 9: no instance
    ((130, 98, 65, 20, 1.0), (1, 8, 56896)),            # R4, td stays 8 between 40 and 60 KB
    ((260, 40, 65, 30, 1.0), (1, 8, 45456)),            # the same zone by the width: 264 columns of footprint
    ((130, 98, 43, 32, 1.2247), (0, 0, 0)),             # 61 664 B > 60 KB
    ((193, 66, 129, 33, 0.9), (1, 16, 37152)),          # three tile columns, the last one pixel wide
    ((70, 200, 60, 33, 0.745356), (1, 8, 39312)),       # six source rows per destination row
    ((130, 98, 130, 98, 0.745356), (1, 32, 25344)),     # scale 1
    ((5, 7, 4, 6, 0.745356), (1, 32, 34976)),           # smaller than the staging quads and the radius
    ((3, 3, 2, 2, 0.745356), (1, 16, 28352)),
]


@pytest.mark.parametrize("case,plan", PYR_STEPS, ids=["%dx%d-to-%dx%d-sigma%g" % c for c, _ in PYR_STEPS])
def test_pyramid_step_is_the_oracles_blur_then_resize(ctx, oracle, switches, case, plan):
    sw, sh, dw, dh, sigma = case
    nb, nplanes = 2, 3
    rng = np.random.default_rng(sw * 1000 + dw)
    src = np.stack([noise_color(rng, sw, sh, 0, 255) for _ in range(nb)])
    want = np.stack([np.stack([oracle.resize_linear_cv(oracle.gaussian_blur_cv(src[b, k], sw, sigma), sw, dw, dh) for k in range(nplanes)]) for b in range(nb)])
    got, info = ctx.pyramid_down(c_(src), sw, dw, dh, sigma)
    print("pyramid step %dx%d -> %dx%d sigma %g: k_pyr_down %d, td %d, LDS %d B" % (sw, sh, dw, dh, sigma, *info))
    assert info == plan
    assert np.array_equal(valid(got, dw), valid(want, dw))
    switches.set("SFA_PYRAMID_UNFUSED", "1")
    two, info2 = ctx.pyramid_down(c_(src), sw, dw, dh, sigma)
    assert info2 == (0, 0, 0)
    assert np.array_equal(valid(two, dw), valid(want, dw)) and np.array_equal(valid(two, dw), valid(got, dw))


# ---- (c) the flow between levels ------------------------------------------------------------------------------------------------------------
# widths on and off the block's 64 columns, heights on and off k_resize_flow's 16 rows per block
FLOW_UP = [(117, 88, 130, 98), (58, 44, 65, 49), (2, 5, 3, 6), (65, 17, 131, 35)]
FLOW_DOWN = [(130, 98, 52, 39), (200, 37, 20, 5), (131, 97, 64, 16), (67, 45, 67, 45)]        # the initial flow's direction (job_initial_flow)


FLOW_CASES = [(s, (0.9, 0.8979592)) for s in FLOW_UP + FLOW_DOWN] + [((117, 88, 130, 98), (1.0, 1.0))]     # the last: the kernel's `!= 1.0f` branch


@pytest.mark.parametrize("shape,post", FLOW_CASES, ids=["%dx%d-to-%dx%d-post%g" % (*c, q[0]) for c, q in FLOW_CASES])
def test_flow_resize_is_the_oracles(ctx, oracle, shape, post):
    sw, sh, dw, dh = shape
    nb = 3
    rng = np.random.default_rng(sw * 1000 + dw)
    wx = np.stack([noise_plane(rng, sw, sh, -20, 20) for _ in range(nb)])
    wy = np.stack([noise_plane(rng, sw, sh, -20, 20) for _ in range(nb)])
    gx, gy = ctx.resize_flow(c_(wx), c_(wy), sw, dw, dh, post[0], post[1])
    for b in range(nb):
        ex = oracle.resize_linear_cv(wx[b], sw, dw, dh) * np.float32(post[0])
        ey = oracle.resize_linear_cv(wy[b], sw, dw, dh) * np.float32(post[1])
        assert ex.dtype == np.float32
        assert np.array_equal(valid(ex, dw), valid(gx[b], dw)) and np.array_equal(valid(ey, dw), valid(gy[b], dw)), b


# ---- (d) the job's pyramid, level by level ----------------------------------------------------------------------------------------------------
def oracle_pyramid(oracle, frame3, w, h, layers, p_scale, presmooth_sigma=0.0):
    """the levels of one frame as orc_variational builds them (slowflow_oracle.c: its pyramid loop, variational_mt.cpp:583-652): level 0 the frame (presmoothed
    if the cfg's sigma > 0), level l = resize(blur(level l - 1, 1 / sqrtf(2 p_scale))) per plane.  Returns [(w_l, h_l, planes (3, h_l, stride_of(w_l)))]"""
    sizes = oracle.pyramid_sizes(w, h, layers, p_scale)
    sigma = float(np.float32(1) / np.sqrt(np.float32(2) * np.float32(p_scale)))
    lv = frame3 if not presmooth_sigma > 0 else np.stack([oracle.gaussian_presmooth(frame3[k], w, presmooth_sigma) for k in range(3)])
    out = [(w, h, lv)]
    for l in range(1, len(sizes)):
        (pw, _), (lw, lh) = sizes[l - 1], sizes[l]
        lv = np.stack([oracle.resize_linear_cv(oracle.gaussian_blur_cv(c_(lv[k]), pw, sigma), pw, lw, lh) for k in range(3)])
        out.append((lw, lh, lv))
    return out


# (w, h, p_scale, layers, presmooth sigma, levels the sizes give).  130 x 98: 0.9 / 0.75 R3 and R4 at td 32; 0.5 R4 at td 16; 0.4 and 0.35 R5 at td 8, 46.5 and
# 57.7 KB; 0.3 R5 beyond 60 KB: the two kernels.  p_scale 0.11 is radius 9 (the two kernels; refused before k_gauss_h / k_gauss_v held 33 taps): at 130 x 98 the
# size break (variational_mt.cpp:647) leaves level 0 alone, so 760 x 750 -- the smallest round size whose second level 83 x 82 survives it -- runs the step itself.
JOB_PYRAMIDS = [(130, 98, 0.9, 4, 0.0, 4), (130, 98, 0.75, 3, 0.0, 3), (130, 98, 0.5, 3, 0.0, 3), (130, 98, 0.4, 3, 0.0, 3), (130, 98, 0.35, 2, 0.0, 2),
                (130, 98, 0.3, 2, 0.0, 2), (130, 98, 0.11, 2, 0.0, 1), (760, 750, 0.11, 2, 0.0, 2), (9, 7, 0.9, 2, 0.0, 2), (130, 98, 0.9, 3, 0.8, 3)]


@pytest.mark.parametrize("w,h,p_scale,layers,presmooth,nlevels", JOB_PYRAMIDS)
def test_job_pyramid_levels_are_the_oracles(ctx, oracle, w, h, p_scale, layers, presmooth, nlevels):
    nb, F = 2, 3
    rng = np.random.default_rng(int(p_scale * 1000) + w)
    windows = [[noise_color(rng, w, h, 0, 255) for _ in range(F)] for _ in range(nb)]
    _, ps = mk_params(oracle, S=2, rho=[1], omega=[0], niter_outer=1, niter_solver=1, layers=layers, p_scale=p_scale, presmooth_sigma=presmooth)
    assert len(oracle.pyramid_sizes(w, h, layers, p_scale)) == nlevels
    j = sfa.Job(ctx, ps, w, h, nb)
    try:
        for b in range(nb):
            j.upload(b, [c_(f) for f in windows[b]])
        j.run()
        for b in range(nb):
            for f in range(F):
                want = oracle_pyramid(oracle, windows[b][f], w, h, layers, p_scale, presmooth)
                assert len(want) == nlevels
                for l, (lw, lh, planes) in enumerate(want):
                    got = j.download_level_frame(b, l, f)
                    assert got.shape == planes.shape
                    assert np.array_equal(valid(got, lw), valid(planes, lw)), (b, f, l, lw, lh)
    finally:
        j.close()


# ---- (e) an initial flow that is not zero, down to the coarsest level and back up -------------------------------------------------------------------
def test_variational_multilevel_from_a_nonzero_initial_flow(ctx, oracle):
    """test_variational_multilevel's configuration (130 x 98, 3 levels) started from a smooth field around the sequence's motion: job_initial_flow's resize to the
    coarsest level (scale > 1, post_x != post_y) feeds the whole path, which every other multi-level test at this size starts from zeros"""
    w, h = 130, 98
    frames, af, sf = normalized_frames(oracle, w, h, 3, seed=11)
    po, ps = mk_params(oracle, S=2, rho=[1], omega=[0], norm_avg=af, norm_std=sf, layers=3, niter_outer=3)
    s = smooth_noise_color(np.random.default_rng(17), w, h, 1.0)                 # box-filtered noise, 127.5 +- 0.5
    init = (2.0 + 2.0 * (s[0] - 127.5), 1.0 + 2.0 * (s[1] - 127.5))          # up to 1.9 px off the sequence's (2, 1)
    for a in init:
        a[:, w:] = 0
    assert 0.3 < np.abs(init[0][:, :w] - 2.0).max() < 3.0 and not np.array_equal(init[0], init[1] + 1.0)
    o, g = run_both(ctx, oracle, po, ps, frames, w, h, level_only=False, init=init)
    d = max(np.abs(valid(o[0], w) - valid(g[0], w)).max(), np.abs(valid(o[1], w) - valid(g[1], w)).max())
    print("max |d(u, v)| from a non-zero start = %g" % d)
    assert d <= TOL_UV, d


# ---- (f) refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_scale", [0.0, -0.5, float("nan"), 1.5, 0.005])
def test_job_create_refuses_a_p_scale_the_pyramid_cannot_take(ctx, oracle, p_scale):
    """0, negative, NaN: sigma = 1 / sqrt(2 p_scale) is no number; above 1 the levels grow; 0.005 is sigma 10, 81 taps against the kernels' 33"""
    _, ps = mk_params(oracle, S=2, rho=[1], omega=[0], layers=2, p_scale=p_scale)
    L = sfa.lib()
    job = C.c_void_p()
    rc = L.sfa_job_create(ctx.h, C.byref(ps), 130, 98, 1, C.byref(job))
    msg = L.sfa_last_error(ctx.h).decode()
    assert rc == SFA_ERR_ARG and "sfa_job_create" in msg and "p_scale" in msg, (rc, msg)
    assert not job.value
    src = noise_plane(np.random.default_rng(5), 19, 11, 0, 255)                   # the context stays usable
    assert np.array_equal(valid(oracle.gaussian_blur_cv(src, 19, 1.0), 19), valid(ctx.gaussian_blur(c_(src), 19, 1.0), 19))


def test_level_frame_hook_refuses_bad_indices(ctx, oracle):
    w, h = 20, 12
    _, ps = mk_params(oracle, S=2, rho=[1], omega=[0], niter_outer=1, niter_solver=1, layers=2, p_scale=0.9)
    sizes = oracle.pyramid_sizes(w, h, 2, 0.9)
    assert sizes == [(20, 12), (18, 10)]
    frames = [noise_color(np.random.default_rng(k), w, h, 0, 255) for k in range(3)]
    j = sfa.Job(ctx, ps, w, h, 2)
    try:
        for b in range(2):
            j.upload(b, [c_(f) for f in frames])
        j.run()
        for (b, level, f, stride, name) in [(-1, 0, 0, None, "b"), (2, 0, 0, None, "b"), (0, -1, 0, None, "level"), (0, 2, 0, None, "level"), (0, 1, -1, None, "f"),
                                            (0, 1, 3, None, "f"), (0, 0, 0, 19, "stride"), (0, 1, 0, 17, "stride")]:
            with pytest.raises(sfa.SlowflowError) as e:
                j.download_level_frame(b, level, f, size=sizes[level] if 0 <= level < 2 else sizes[0], stride=stride)
            assert "-> %d" % SFA_ERR_ARG in str(e.value) and "sfa_job_download_level_frame" in str(e.value) and name + " =" in str(e.value), (name, str(e.value))
        got = j.download_level_frame(1, 1, 2, stride=18)                          # a stride of exactly the level's width is taken
        assert np.array_equal(got, valid(oracle_pyramid(oracle, frames[2], w, h, 2, 0.9)[1][2], 18))
    finally:
        j.close()
