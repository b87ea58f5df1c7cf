"""Value-range parity: what the kernels do with magnitudes the rest of the suite never feeds them -- zero regions, subnormals, values near overflow, Inf and NaN.

tests/value_ranges.py builds the inputs: planes scaled by a ladder of powers of two in bands of eight columns (several magnitudes in any 64 consecutive columns of a
row: every wave is mixed, whatever a kernel's lane mapping), and a sprinkle of IEEE special values.  The first tests run on the CPU and prove on oracle-side data
that the inputs reach what the GPU tests claim (the guard classes of the fused data-term kernel, subnormal residuals, subnormal results); every GPU test repeats the
proof for its own input as asserts before it compares.  The stages and the solver are held to the oracle bit for bit (NaN == NaN) with equal sets of NaN, +Inf, -Inf
and subnormal positions; a level to the suite's bound max(TOL_LEVEL, 3 x the oracle's own sensitivity)."""
import numpy as np
import pytest

import oracle as orc
import slowflow_amd as sfa
import value_ranges as vr
from synth import copy_sys, noise_plane, smooth_noise_color, sor_system
from test_gpu_parity import TOL_LEVEL, c_, mk_params, normalized_frames, oracle_sensitivity, run_both, valid
from value_ranges import FULL, HIGH, LOW, H, W

gpu = pytest.mark.gpu
LOR = (2, 0.05, 0.5)
SIZES = [(W, H), (5, 4)]            # the ladder shape, and one smaller than every tile for the per-pixel kernels


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


def same(o, g, w, what=None):
    """GPU == oracle on the valid columns, NaN == NaN, and the same positions of NaN, +Inf, -Inf and subnormal values"""
    o, g = valid(np.asarray(o), w), valid(np.asarray(g), w)
    for name, so, sg in zip(("nan", "+inf", "-inf", "subnormal"), vr.value_sets(o), vr.value_sets(g)):
        assert np.array_equal(so, sg), (what, name, int(so.sum()), int(sg.sum()))
    bad = ~((o == g) | (np.isnan(o) & np.isnan(g)))
    assert not bad.any(), (what, int(bad.sum()), o[bad][:4], g[bad][:4])


def spans(o, w, seed):
    """the proof that an oracle result reaches what its test claims: on the FULL ladder alone finite values 2^60 apart; with the sprinkle NaN and Inf as well"""
    v = valid(np.asarray(o), w)
    if seed is None:
        m = np.abs(v[v != 0])
        assert np.isfinite(v).all() and m.min() * 2.0 ** 60 < m.max(), (m.min(), m.max())
    else:
        assert np.isnan(v).any() and np.isinf(v).any() and np.isfinite(v).any()


def laddered(a, w, spec=FULL, seed=None, values=vr.SPECIALS):
    """a copy of the plane(s) with the valid columns multiplied by the ladder; seed: with the special values sprinkled in"""
    out = vr.ladder_plane(a, w, spec["exps"], top=spec["top"])
    if seed is not None:
        vr.sprinkle(out, seed, w, values)
    return out


def level_frames(oracle, spec, n, seed=5, w=W, h=H):
    return vr.ladder_frames(oracle, w, h, n, spec["exps"], spec["top"], seed)


def stack01(oracle, frames, w=W):
    return oracle.derivative_stack(frames[0], frames[1], w)


# ------------------------------------------------------------------------------------------------------
# the builders (CPU): the conditions that keep the GPU tests below from passing vacuously
# ------------------------------------------------------------------------------------------------------
def test_ladder_scale_layout():
    s = vr.ladder_scale(W, H, LOW["exps"], top=LOW["top"])
    assert s.dtype == np.float32 and s.shape == (H, W)
    assert s[0, 0] == 2.0 ** -70 and s[7, 8] == 2.0 ** -45 and s[3, 16] == 2.0 ** -20 and s[0, 31] == 1 and s[0, 32] == 2.0 ** -70
    assert (s[8:16] == 1).all() and (s[16:] == np.float32(2.0 ** -45)).all()
    for x0 in range(0, W - 63):                                   # any 64 consecutive columns of a banded row carry every magnitude
        assert len(np.unique(s[0, x0:x0 + 64])) == 4
    f = vr.ladder_scale(W, H, FULL["exps"])
    assert (f == f[0]).all() and len(np.unique(f[0])) == 6


def test_sprinkle_writes_every_special_value_into_the_valid_columns():
    p = np.ones((2, H, orc.stride_of(W) + 4), np.float32)
    q = vr.sprinkle(p.copy(), 3, W)
    assert np.array_equal(vr.sprinkle(p.copy(), 3, W), q, equal_nan=True)                       # fixed, seeded positions
    assert (q[..., W:] == 1).all()
    for k in range(2):
        v = q[k][q[k].view(np.uint32) != np.float32(1).view(np.uint32)]
        assert v.size == 3 * vr.SPECIALS.size
        assert sorted(v.view(np.uint32).tolist()) == sorted(np.tile(vr.SPECIALS, 3).view(np.uint32).tolist())
    assert vr.is_subnormal(vr.SUB_MIN) and vr.is_subnormal(vr.SUB_MAX) and not vr.is_subnormal(vr.FLT_MIN) and not vr.is_subnormal(np.float32(0))


def test_guard_restatement_edges():
    f = np.float32
    lo, hi = f(2.0 ** -87), f(2.0 ** 53)
    a = np.array([0.0, -0.0, np.nextafter(lo, f(0)), lo, 1.0, np.nextafter(hi, f(0)), hi, np.inf, np.nan, -1.0, vr.SUB_MAX], f)
    assert vr.num_ok(a).tolist() == [True, False, False, True, True, True, False, False, False, False, False]
    n = np.array([0.01, np.nextafter(f(2.0 ** 33), f(0)), 2.0 ** 33, np.inf], f)
    assert vr.den_ok(n).tolist() == [True, True, False, False]


def test_low_ladder_has_every_guard_class(oracle):
    """LOW: waves that are mixed, fully admitted and fully rejected, and squared residuals that are subnormal"""
    D = stack01(oracle, level_frames(oracle, LOW, 3))
    counts = vr.class_counts(vr.guard_classes(D, W))
    assert sum(counts.values()) == 72 and min(counts.values()) >= 8, counts
    print("LOW guard classes of 72 segments:", counts)
    banded = vr.ladder_frames(oracle, W, H, 3, LOW["exps"], None, 5)
    a, _ = vr.guard_terms(stack01(oracle, banded), W)
    print("LOW, every row banded: subnormal squared residuals:", int(vr.is_subnormal(a).sum()))
    assert vr.is_subnormal(a).sum() >= 1000
    _, _, low, high, den = vr.guard_pass(D, W)
    assert low.any() and not high.any() and not den.any()                                       # LOW fails on small numerators only


def test_full_ladder_mixes_every_wave(oracle):
    """FULL: every 64-column segment mixed, and each of the three guard terms fails somewhere"""
    D = stack01(oracle, level_frames(oracle, FULL, 3))
    counts = vr.class_counts(vr.guard_classes(D, W))
    assert counts == {"mixed": 72, "all": 0, "none": 0}, counts
    col, grd, low, high, den = vr.guard_pass(D, W)
    print(f"FULL: {1 - (col & grd).mean():.0%} of the pixels fail a guard: {low.mean():.0%} low numerator, {high.mean():.0%} high numerator, {den.mean():.0%} denominator")
    assert low.mean() > 0.1 and high.mean() > 0.05 and den.mean() > 0.1


@pytest.mark.parametrize("dt_norm", [0, 1])
def test_oracle_data_term_on_the_full_ladder_is_finite_and_has_subnormals(oracle, dt_norm):
    """started from zero planes (noise would absorb the tiny terms) the oracle's system entries stay finite for every penalty and contain subnormal values"""
    case = data_case(oracle, W, H)
    for pid in range(5):
        sys_o = data_oracle(oracle, case, case["D"], W, pid, dt_norm, False, 1.0 / 3.0, -1.0)
        assert all(np.isfinite(valid(x, W)).all() for x in sys_o), pid
        assert sum(int(vr.is_subnormal(valid(x, W)).sum()) for x in sys_o) > 0, pid


def test_oracle_level_on_the_low_ladder_is_finite_and_the_high_ladder_is_not(oracle):
    for spec, finite in ((LOW, True), (HIGH, False)):
        frames = level_frames(oracle, spec, 3)
        po, _ = mk_params(oracle, S=2, rho=[1], omega=[0], niter_outer=2)
        wx, wy = orc.plane(H, orc.stride_of(W)), orc.plane(H, orc.stride_of(W))
        rc, _, _ = oracle.compute_one_level(po, wx, wy, frames, W)
        fin = np.isfinite(valid(wx, W)) & np.isfinite(valid(wy, W))
        assert rc == 0 and fin.all() == finite and fin.any()
        if finite:
            s = oracle_sensitivity(oracle, po, frames, W, H)
            print(f"LOW: the oracle's sensitivity to 1-ulp input noise = {s:.3g}")
            assert s < TOL_LEVEL


# ------------------------------------------------------------------------------------------------------
# B. the stage kernels against the oracle at the ladder
# ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("seed", [None, 11])
def test_convolve(ctx, oracle, seed):
    rng = np.random.default_rng(1)
    src = laddered(noise_plane(rng, W, H, -3, 3), W, FULL, seed)
    for order in (1, 2):
        for horiz in (True, False):
            a = oracle.convolve(src, W, order, horiz)
            spans(a, W, seed)
            same(a, ctx.convolve(c_(src), W, order, horiz), W, (order, horiz))


@gpu
@pytest.mark.parametrize("seed", [None, 12])
def test_derivative_stack(ctx, oracle, seed):
    I1, I2 = level_frames(oracle, FULL, 2)
    if seed is not None:
        vr.sprinkle(I1, seed, W); vr.sprinkle(I2, seed + 100, W)
    D = oracle.derivative_stack(I1, I2, W)
    spans(D, W, seed)
    same(D, ctx.derivative_stack(c_(I1), c_(I2), W), W)


@gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seed", [None, 13])
def test_image_warp(ctx, oracle, seed, w, h):
    """extreme values in the IMAGE, ordinary flows (flows beyond the int range: test_gpu_parity.test_image_warp_with_flows_beyond_the_int_range)"""
    rng = np.random.default_rng(2)
    src = laddered(smooth_noise_color(rng, w, h), w, FULL, seed)
    wx, wy = noise_plane(rng, w, h, -4, 4), noise_plane(rng, w, h, -4, 4)
    for factor in (-2, -1, 1, 2):
        a, ma = oracle.image_warp(src, wx, wy, w, factor)
        b, mb = ctx.image_warp(c_(src), c_(wx), c_(wy), w, factor)
        if (w, h) == (W, H):
            spans(a, w, seed)
        same(a, b, w, factor)
        assert np.array_equal(valid(ma, w), valid(mb, w)), factor


@gpu
@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("pid", [0, 1, 2, 3, 4])
def test_smoothness(ctx, oracle, method, pid):
    """the ladder on the flow (uu, vv) and, separately, on the local weight dpsis.  Method 2 compares the column index with (weight - 1) (the shadowed `float w`,
    variational_aux_mt.cpp:100-103): a weight above the width in the LAST column makes the reference read never-written memory -- no defined value -- so for
    method 2 the last column's weights above the width (large bands, FLT_MAX, +Inf) are put back to 0.25; NaN and every other special value stay"""
    eps = 0.001 if pid in (1, 3) else 0.05
    for w, h in SIZES:
        rng = np.random.default_rng(method * 10 + pid)
        uu, vv = noise_plane(rng, w, h, -2, 2), noise_plane(rng, w, h, -2, 2)
        dps = noise_plane(rng, w, h, 0.05, 0.5)
        for on_flow in (True, False):
            for seed in (None, 14):
                u, v, d = (laddered(uu, w, FULL, seed), laddered(vv, w, FULL, seed and seed + 1), dps) if on_flow else (uu, vv, laddered(dps, w, FULL, seed))
                if method == 2 and not on_flow:
                    d[:, w - 1][d[:, w - 1] > w] = 0.25
                a = oracle.smoothness(method, u, v, d, w, 4.0, orc.Penalty(pid, eps, 0.5))
                b = ctx.smoothness(method, c_(u), c_(v), c_(d), w, 4.0, sfa.Penalty(pid, eps, 0.5))
                for x, y, n in zip(a, b, ("horiz", "vert")):
                    same(x, y, w, (w, on_flow, seed, n))


@gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seed", [None, 15])
def test_sub_laplacian(ctx, oracle, seed, w, h):
    rng = np.random.default_rng(4)
    src, wh, wv, d0 = (laddered(p, w, FULL, seed and seed + i) for i, p in
                       enumerate((noise_plane(rng, w, h), noise_plane(rng, w, h, 0, 2), noise_plane(rng, w, h, 0, 2), noise_plane(rng, w, h))))
    a = orc.plane(*d0.shape); a[...] = d0
    oracle.sub_laplacian(a, src, wh, wv, w)
    b = ctx.sub_laplacian(c_(d0).copy(), c_(src), c_(wh), c_(wv), w)
    if (w, h) == (W, H):
        spans(a, w, seed)
    same(a, b, w)


def data_case(oracle, w, h):
    """the inputs of the data-term stage at the FULL ladder: the stack of two laddered frames, O(1) increments, a mask with holes, channel weights"""
    rng = np.random.default_rng(6)
    I1, I2 = level_frames(oracle, FULL, 2, seed=6, w=w, h=h)
    mask = noise_plane(rng, w, h, 0, 1)
    mask[:, :w] = (mask[:, :w] > 0.2) * 0.5
    return dict(D=oracle.derivative_stack(I1, I2, w), du=noise_plane(rng, w, h, -.5, .5), dv=noise_plane(rng, w, h, -.5, .5), mask=mask,
                chw=[noise_plane(rng, w, h, 0.5, 1.5) for _ in range(3)])


def data_oracle(oracle, case, D, w, pid, dt_norm, ref_term, hd, s):
    h, stride = case["du"].shape
    eps = 0.001 if pid in (1, 3) else 0.05
    sys_o = [orc.plane(h, stride) for _ in range(5)]                                             # accumulated from zero: noise would absorb the tiny terms
    rc = oracle.add_data(sys_o, case["mask"], case["du"], case["dv"], D, case["chw"], w, hd, 2.0, s, dt_norm, orc.Penalty(pid, eps, 0.5), orc.Penalty(pid, eps, 0.5), ref_term)
    assert rc in (0, None)
    return sys_o


@pytest.fixture(scope="module")
def data_cases(oracle):
    out = {}
    for w, h in SIZES:
        case = data_case(oracle, w, h)
        Ds = orc.aligned_zeros(case["D"].shape); Ds[...] = case["D"]
        case["D_sprinkled"] = vr.sprinkle(Ds, 16, w)
        out[w, h] = case
    return out


@gpu
@pytest.mark.parametrize("ref_term", [False, True])
@pytest.mark.parametrize("dt_norm", [0, 1])
@pytest.mark.parametrize("pid", [0, 1, 2, 3, 4])
def test_data_terms(ctx, oracle, data_cases, ref_term, dt_norm, pid):
    eps = 0.001 if pid in (1, 3) else 0.05
    for (w, h), case in data_cases.items():
        for key in ("D", "D_sprinkled"):
            for s in (-2.0, 1.0):
                for hd in (0.0, 1.0 / 3.0):
                    sys_o = data_oracle(oracle, case, case[key], w, pid, dt_norm, ref_term, hd, s)
                    if key == "D" and (w, h) == (W, H):
                        assert all(np.isfinite(valid(x, w)).all() for x in sys_o) and sum(int(vr.is_subnormal(valid(x, w)).sum()) for x in sys_o) > 0
                    sys_g = [np.zeros(case["du"].shape, np.float32) for _ in range(5)]
                    rc = ctx.add_data(sys_g, c_(case["mask"]), c_(case["du"]), c_(case["dv"]), c_(case[key]), [c_(x) for x in case["chw"]], w, hd, 2.0, s, dt_norm,
                                      sfa.Penalty(pid, eps, 0.5), sfa.Penalty(pid, eps, 0.5), ref_term)
                    assert rc == 0
                    for x, y, n in zip(sys_o, sys_g, ["a11", "a12", "a22", "b1", "b2"]):
                        same(x, y, w, (w, key, s, hd, n))


@gpu
@pytest.mark.parametrize("pid", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("seed", [None, 17])
def test_occlusion_costs(ctx, oracle, pid, seed):
    w, h, ref = W, H, 1
    rng = np.random.default_rng(pid + 20)
    eps = 0.001 if pid in (1, 3) else 0.05
    po, ps = mk_params(oracle, S=2, rho=[1], omega=[0.5], robust_color=(pid, eps, 0.5), robust_grad=(pid, eps, 0.3))
    imgs = [[laddered(smooth_noise_color(rng, w, h, 10), w, FULL, seed and seed + 4 * i + j) for j in range(4)] for i in range(2 * ref)]
    masks = [noise_plane(rng, w, h, 0, 1) for _ in range(2 * ref)]
    for m in masks:
        m[:, :w] = (m[:, :w] > 0.2).astype(np.float32)
    masks[0][:3, :w] = 0; masks[-1][:3, :w] = 0
    so = orc.aligned_zeros((2 * ref, 8, 3, h, orc.stride_of(w))); to = orc.aligned_zeros(so.shape)
    for i, (a, b, c, d) in enumerate(imgs):
        so[i] = oracle.derivative_stack(a, b, w); to[i] = oracle.derivative_stack(c, d, w)
    mo = orc.aligned_zeros((2 * ref,) + masks[0].shape); mo[...] = np.stack(masks)
    o0, o1 = oracle.occlusion_costs(mo, so, to, ref, list(po.rho)[:ref], list(po.omega)[:ref], po.delta / np.float32(3), po.gamma / np.float32(3),
                                    po.occlusion_penalty, po.robust_color, po.robust_grad, w)
    g0, g1 = ctx.occlusion_costs(ps, [c_(m) for m in masks], [c_(i[0]) for i in imgs], [c_(i[1]) for i in imgs], [c_(i[2]) for i in imgs], [c_(i[3]) for i in imgs], w)
    same(o0, g0, w, "d0"); same(o1, g1, w, "d1")


@gpu
@pytest.mark.parametrize("seed", [None, 18])
def test_pyramid_and_presmoothing(ctx, oracle, seed):
    rng = np.random.default_rng(8)
    src = laddered(noise_plane(rng, W, H, 0, 255), W, FULL, seed)
    for name, a, b in (("blur", oracle.gaussian_blur_cv(src, W, 0.8), ctx.gaussian_blur(c_(src), W, 0.8)),
                       ("presmooth", oracle.gaussian_presmooth(src, W, 0.8), ctx.gaussian_presmooth(c_(src), W, 0.8))):
        spans(a, W, seed)
        same(a, b, W, name)
    a, dwa = oracle.resize_linear_fx(src, W, 0.5, 0.5)
    b, dwb = ctx.resize_linear_fx(c_(src), W, 0.5, 0.5)
    assert dwa == dwb and a.shape == b.shape
    spans(a, dwa, seed)
    same(a, b, dwa, "resize")


def dpsis_case(w, h):
    """a ramp of slope 1 per column under a little texture, with statistics that put -coef |grad lum| around -110 ... -80: expf's underflow branch and its
    subnormal results (0.5 exp(n) is subnormal for n in about (-103.3, -86.6), zero below)"""
    rng = np.random.default_rng(9)
    im = smooth_noise_color(rng, w, h, 1.5)
    im[:, :, :w] += np.arange(w, dtype=np.float32)
    return im, (10.0, 20.0, 30.0), (4900.0, 4800.0, 5000.0)


def test_dpsis_case_reaches_zero_subnormal_and_normal_weights(oracle):
    for w, h in SIZES[:1]:
        im, avg, std = dpsis_case(w, h)
        a = valid(oracle.dpsis_weight(im, w, avg, std, 0), w)
        counts = (int((a == 0).sum()), int(vr.is_subnormal(a).sum()), int((a >= vr.FLT_MIN).sum()))
        print("dpsis weights: zero, subnormal, normal =", counts)
        assert min(counts) >= 50 and sum(counts) == a.size, counts


@gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_dpsis_weight_underflow(ctx, oracle, w, h):
    im, avg, std = dpsis_case(w, h)
    a = oracle.dpsis_weight(im, w, avg, std, 0)
    if (w, h) == (W, H):
        v = valid(a, w)
        assert (v == 0).sum() >= 50 and vr.is_subnormal(v).sum() >= 50 and (v >= vr.FLT_MIN).sum() >= 50
    same(a, ctx.dpsis_weight(c_(im), w, avg, std, 0), w)


@gpu
@pytest.mark.parametrize("seed", [None, 19])
def test_dpsis_weight_on_the_ladder(ctx, oracle, seed):
    im = laddered(smooth_noise_color(np.random.default_rng(10), W, H), W, FULL, seed)
    same(oracle.dpsis_weight(im, W, (0, 0, 0), (1, 1, 1), 0), ctx.dpsis_weight(c_(im), W, (0, 0, 0), (1, 1, 1), 0), W)


# ------------------------------------------------------------------------------------------------------
# C. the fused assembly kernel's guard branches
# ------------------------------------------------------------------------------------------------------
VARIANTS = (("default", {}), ("exact_div", {"SFA_EXACT_DIV": "1"}), ("generic", {"SFA_ASSEMBLE_GENERIC": "1"}), ("unfused", {"SFA_UNFUSED": "1"}), ("plain_grid", {"SFA_ASM_XCD": "0"}))
SWITCHES = ("SFA_EXACT_DIV", "SFA_ASSEMBLE_GENERIC", "SFA_UNFUSED", "SFA_ASM_XCD")
TERMS = {"S2": dict(S=2, rho=[1], omega=[0]), "S3_to_reference": dict(S=3, rho=[1, 0.5], omega=[0.5, 2])}


def level_gpu(ctx, ps, frames, w, h):
    wx, wy = np.zeros((h, sfa.stride_of(w)), np.float32), np.zeros((h, sfa.stride_of(w)), np.float32)
    ctx.compute_one_level(ps, wx, wy, [c_(f) for f in frames], w, None)
    return wx, wy


def level_variants(ctx, switches, ps, frames, w=W, h=H):
    outs = {}
    for name, env in VARIANTS:
        for k in SWITCHES:
            switches.unset(k)
        for k, v in env.items():
            switches.set(k, v)
        outs[name] = level_gpu(ctx, ps, frames, w, h)
    for k in SWITCHES:
        switches.unset(k)
    return outs


def assert_guard_classes_present(oracle, frames):
    counts = vr.class_counts(vr.guard_classes(stack01(oracle, frames), W))
    assert min(counts.values()) >= 8, counts                         # mixed, fully admitted and fully rejected waves, eight rows of segments each at the least


@gpu
@pytest.mark.parametrize("pen", [None, LOR], ids=["modified_l1", "lorentzian"])
@pytest.mark.parametrize("inner", [1, 2])
@pytest.mark.parametrize("terms", sorted(TERMS))
def test_guard_branches_on_the_low_ladder(ctx, oracle, switches, terms, inner, pen):
    """the cfg-default terms (normalised data term, no channel weights; modified L1 -> the FAST == 1 instance, Lorentzian -> FAST == 2) on frames whose squared
    residuals fall below 2^-87 in some bands: waves that take the shared reciprocal, waves that take __fdiv_rn inside the same instance, and waves in which one
    lane's failure sends the others down the exact path.  One set of bits under every variant of the kernel, and the oracle's flow within the suite's bound"""
    kw = dict(TERMS[terms], dataterm_norm=1, niter_outer=2, niter_inner=inner)
    if pen:
        kw.update(robust_color=pen, robust_grad=pen)
    frames = level_frames(oracle, LOW, 2 * kw["S"] - 1)
    assert_guard_classes_present(oracle, frames)
    po, ps = mk_params(oracle, **kw)
    outs = level_variants(ctx, switches, ps, frames)
    for name, (gx, gy) in outs.items():
        assert np.array_equal(valid(gx, W), valid(outs["default"][0], W)) and np.array_equal(valid(gy, W), valid(outs["default"][1], W)), name
    o, g = run_both(ctx, oracle, po, ps, frames, W, H)
    assert np.array_equal(g[0], outs["default"][0]) and np.array_equal(g[1], outs["default"][1])
    d = max(np.abs(valid(o[0], W) - valid(g[0], W)).max(), np.abs(valid(o[1], W) - valid(g[1], W)).max())
    tol = max(TOL_LEVEL, 3 * oracle_sensitivity(oracle, po, frames, W, H))
    print(f"{terms} inner {inner} {'lorentzian' if pen else 'modified L1'}: max|d(u,v)| = {d:.3g}, bound {tol:.3g}")
    assert np.isfinite(valid(o[0], W)).all() and d <= tol, (d, tol)


@gpu
@pytest.mark.parametrize("pen", [None, LOR], ids=["modified_l1", "lorentzian"])
@pytest.mark.parametrize("inner", [1, 2])
@pytest.mark.parametrize("terms", sorted(TERMS))
def test_guard_branches_up_to_2_27(ctx, oracle, switches, terms, inner, pen):
    """a ladder that reaches 2^27: numerators above 2^53 and denominators above 2^33 as well.  The reference's own level is not finite there, so no numeric
    tolerance: the variants give one set of bits (NaN == NaN), and the GPU's finite pixels are the oracle's"""
    kw = dict(TERMS[terms], dataterm_norm=1, niter_outer=2, niter_inner=inner)
    if pen:
        kw.update(robust_color=pen, robust_grad=pen)
    frames = level_frames(oracle, HIGH, 2 * kw["S"] - 1)
    _, _, low, high, den = vr.guard_pass(stack01(oracle, frames), W)
    assert low.any() and high.any() and den.any() and "mixed" in vr.guard_classes(stack01(oracle, frames), W)
    po, ps = mk_params(oracle, **kw)
    outs = level_variants(ctx, switches, ps, frames)
    for name, (gx, gy) in outs.items():
        assert np.array_equal(valid(gx, W), valid(outs["default"][0], W), equal_nan=True) and np.array_equal(valid(gy, W), valid(outs["default"][1], W), equal_nan=True), name
    o, g = run_both(ctx, oracle, po, ps, frames, W, H)
    for k in range(2):
        assert np.array_equal(np.isfinite(valid(o[k], W)), np.isfinite(valid(g[k], W))), (k, int(np.isfinite(valid(o[k], W)).sum()), int(np.isfinite(valid(g[k], W)).sum()))


def flat_frames(oracle):
    """textured (normalised) frames with a saturated block (one constant in every frame) and a block of +0: there every residual and derivative is exactly zero,
    the numerators are +0 -- which the guard admits by a clause of its own -- and the denominators are the bare 0.01"""
    frames, af, sf = normalized_frames(oracle, W, H, 3, seed=7)
    for f in frames:
        f[:, 2:14, 20:90] = 3.0
        f[:, 14:22, 70:130] = 0.0
    return frames, af, sf


def test_flat_regions_have_zero_numerators_that_pass_the_guard(oracle):
    frames, _, _ = flat_frames(oracle)
    D = stack01(oracle, frames)
    a, n = vr.guard_terms(D, W)
    zero = (a.view(np.uint32) == 0).all(0)
    bare = zero & (n == np.float32(0.1) * np.float32(0.1)).all(0)                              # (two pixels further inside: the second derivatives' support)
    assert zero.sum() >= 500 and bare.sum() >= 200                                              # (where the two blocks touch, the mean image has an edge)
    assert vr.class_counts(vr.guard_classes(D, W))["all"] == 72


@gpu
@pytest.mark.parametrize("pen", [None, LOR], ids=["modified_l1", "lorentzian"])
def test_flat_and_saturated_regions(ctx, oracle, switches, pen):
    """zero numerators over the smallest denominator, in whole waves and beside textured lanes: one set of bits under every variant, the oracle's flow within the bound"""
    frames, af, sf = flat_frames(oracle)
    a, _ = vr.guard_terms(stack01(oracle, frames), W)
    assert (a.view(np.uint32) == 0).all(0).sum() >= 500
    kw = dict(S=2, rho=[1], omega=[0], norm_avg=af, norm_std=sf, dataterm_norm=1, niter_outer=2, niter_inner=2)
    if pen:
        kw.update(robust_color=pen, robust_grad=pen)
    po, ps = mk_params(oracle, **kw)
    outs = level_variants(ctx, switches, ps, frames)
    for name, (gx, gy) in outs.items():
        assert np.array_equal(valid(gx, W), valid(outs["default"][0], W)) and np.array_equal(valid(gy, W), valid(outs["default"][1], W)), name
    o, g = run_both(ctx, oracle, po, ps, frames, W, H)
    d = max(np.abs(valid(o[0], W) - valid(g[0], W)).max(), np.abs(valid(o[1], W) - valid(g[1], W)).max())
    tol = max(TOL_LEVEL, 3 * oracle_sensitivity(oracle, po, frames, W, H))
    print(f"flat regions, {'lorentzian' if pen else 'modified L1'}: max|d(u,v)| = {d:.3g}, bound {tol:.3g}")
    assert d <= tol, (d, tol)


@gpu
def test_rejected_waves_leave_the_neighbouring_windows_alone(ctx, oracle, switches):
    """a lockstep job of 9 windows (81 tiles: the XCD tile order, which needs 64) that alternate LOW frames and ordinary ones: each window bit for bit what it
    gives as a single-window job, under the XCD order and the plain grid"""
    nb = 9
    plain, af, sf = normalized_frames(oracle, W, H, 3, seed=7)
    wins = [level_frames(oracle, LOW, 3, seed=30 + b) if b % 2 == 0 else [np.roll(f, 3 * b, axis=1) for f in plain] for b in range(nb)]
    assert_guard_classes_present(oracle, wins[0])
    assert vr.class_counts(vr.guard_classes(stack01(oracle, wins[1]), W))["all"] == 72          # the ordinary windows: every wave on the fast path
    _, ps = mk_params(oracle, S=2, rho=[1], omega=[0], norm_avg=af, norm_std=sf, niter_outer=2, layers=1)

    def run(frames_of):
        job = sfa.Job(ctx, ps, W, H, len(frames_of))
        for b, f in enumerate(frames_of):
            job.upload(b, [c_(x) for x in f])
        job.run()
        out = [job.download(b)[:2] for b in range(len(frames_of))]
        job.close()
        return out

    singles = [run([f])[0] for f in wins]
    for xcd in (None, "0"):
        switches.set("SFA_ASM_XCD", xcd)
        for b, ((bx, by), (sx, sy)) in enumerate(zip(run(wins), singles)):
            assert np.isfinite(bx).all() and np.array_equal(bx, sx) and np.array_equal(by, sy), (xcd, b)
    assert not np.array_equal(singles[0][0], singles[2][0]) and not np.array_equal(singles[1][0], singles[3][0])


# ------------------------------------------------------------------------------------------------------
# D. chain_ok: the scalar limits of launch_assemble_images
# ------------------------------------------------------------------------------------------------------
def _limit_settings():
    """hd = rho delta / 3 and hg = rho gamma / 3 per term, data_norm = sum of rho + omega (job.hip: data_term, data_terms): with S = 2, rho = [r], omega = [0] the
    three scalars are r delta / 3, r gamma / 3 and r, so every limit of launch_assemble_images can be met exactly and missed by one binade.  Limits as read there:
    modified L1 hd, hg in {0} + [2^-16, 2^16], eps in [2^-20, 2^20]; Lorentzian hd, hg in {0} + [2^-12, 2^16], eps in [2^-10, 2^10]; data_norm in [2^-8, 2^8]"""
    out = []
    for name in ("delta", "gamma"):
        for e in (-17, -16, 16, 17):
            out.append((f"{name}=3*2^{e}", {name: 3.0 * 2.0 ** e}))
    for name in ("robust_color", "robust_grad"):
        for e in (-21, -20, 20, 21):
            out.append((f"{name}.eps=2^{e}", {name: (1, 2.0 ** e, 0.5)}))
    for e in (-9, -8, 8, 9):
        out.append((f"data_norm=2^{e}", {"rho": [2.0 ** e]}))
    for e in (-11, -10, 10, 11):
        out.append((f"lorentzian.eps=2^{e}", {"robust_color": (2, 2.0 ** e, 0.5), "robust_grad": (2, 2.0 ** e, 0.5)}))
    for e in (-13, -12):
        out.append((f"lorentzian,delta=3*2^{e}", {"robust_color": LOR, "robust_grad": LOR, "delta": 3.0 * 2.0 ** e}))
    return out


@gpu
@pytest.mark.parametrize("name,kw", _limit_settings(), ids=[n for n, _ in _limit_settings()])
def test_chain_limits(ctx, oracle, switches, name, kw):
    """every scalar limit behind which the host admits the shared-reciprocal divisions (AssembleArgs::chain_ok), on it and one binade outside: the default bits are
    the __fdiv_rn-only bits, and the oracle's flow within the suite's bound.  data_norm is no constant: it is the sum of the rho and omega weights"""
    frames, af, sf = normalized_frames(oracle, W, H, 3, seed=7)
    assert vr.class_counts(vr.guard_classes(stack01(oracle, frames), W))["all"] == 72           # textured frames: the per-pixel guards admit every wave
    args = dict(S=2, rho=[1], omega=[0], norm_avg=af, norm_std=sf, niter_outer=2, dataterm_norm=1)
    args.update(kw)
    po, ps = mk_params(oracle, **args)
    if "delta" in kw:
        assert np.float32(ps.delta) / np.float32(3) == np.float32(kw["delta"] / 3)                # hd lands on the power of two exactly
    if "gamma" in kw:
        assert np.float32(ps.gamma) / np.float32(3) == np.float32(kw["gamma"] / 3)
    switches.set("SFA_EXACT_DIV", "1")
    ex, ey = level_gpu(ctx, ps, frames, W, H)
    switches.unset("SFA_EXACT_DIV")
    o, g = run_both(ctx, oracle, po, ps, frames, W, H)
    assert np.array_equal(valid(g[0], W), valid(ex, W)) and np.array_equal(valid(g[1], W), valid(ey, W)), name
    d = max(np.abs(valid(o[0], W) - valid(g[0], W)).max(), np.abs(valid(o[1], W) - valid(g[1], W)).max())
    tol = max(TOL_LEVEL, 3 * oracle_sensitivity(oracle, po, frames, W, H))
    print(f"{name}: max|d(u,v)| = {d:.3g}, bound {tol:.3g}")
    assert d <= tol, (name, d, tol)


# ------------------------------------------------------------------------------------------------------
# E. the solver
# ------------------------------------------------------------------------------------------------------
SOR_KEYS = ("du", "dv", "a11", "a12", "a22", "b1", "b2", "sh", "sv")
B_SCALE = np.float32(2.0 ** -125)       # the right-hand sides of the LOW case: b / a straddles FLT_MIN where the ladder holds 1, so du, dv and their products with the weights are subnormal there


def sor_case(w, h, spec):
    """a random SPD system whose coefficient planes (a11, a12, a22, b1, b2, sh, sv) are scaled by the ladder: det = a11 a22 - a12^2 carries its square (subnormal in
    the 2^-70 bands of LOW).  LOW: the right-hand sides are 2^-125 times O(1) noise instead (partly subnormal themselves), and one band (columns 8 .. 15, cut off from its neighbours by zero horizontal
    weights) has b1 = b2 = 0: there du, dv stay exactly 0"""
    rng = np.random.default_rng(w + h)
    s = sor_system(rng, w, h)
    scale = vr.ladder_scale(w, h, spec["exps"], top=spec["top"])
    for k in SOR_KEYS[2:]:
        if spec is not LOW or k not in ("b1", "b2"):
            s[k][:, :w] *= scale
    if spec is LOW:
        for k in ("b1", "b2"):
            s[k][:, :w] *= B_SCALE
            s[k][:, 8:16] = 0
        s["sh"][:, 7] = 0; s["sh"][:, 15] = 0
    return s


def sor_oracle(oracle, s0, w, K, red_black):
    a = copy_sys(s0)
    oracle.sor(*[a[k] for k in SOR_KEYS], w, K, 1.9, red_black=red_black)
    return a


@pytest.mark.parametrize("w,h", [(W, H), (67, 45)])
def test_oracle_solver_on_the_low_ladder_is_finite_and_has_subnormals(oracle, w, h):
    s0 = sor_case(w, h, LOW)
    det = valid(s0["a11"], w) * valid(s0["a22"], w) - valid(s0["a12"], w) * valid(s0["a12"], w)
    assert vr.is_subnormal(det).sum() >= 100
    for red_black in (False, True):
        for K in (1, 30):
            a = sor_oracle(oracle, s0, w, K, red_black)
            for k in ("du", "dv"):
                v = valid(a[k], w)
                assert np.isfinite(v).all() and vr.is_subnormal(v).sum() >= 100, (k, K, red_black)
                assert (v[:, 8:16] == 0).all() and (v[:, :8] != 0).any()


@gpu
@pytest.mark.parametrize("red_black", [False, True], ids=["raster", "red_black"])
@pytest.mark.parametrize("K", [1, 30])
@pytest.mark.parametrize("w,h", [(W, H), (67, 45)])
@pytest.mark.parametrize("spec", [LOW, FULL], ids=["low", "full"])
def test_solver(ctx, oracle, spec, w, h, K, red_black):
    """sfa_sor_coupled against the raster-order oracle and sfa_sor_red_black against its CPU twin, bit for bit.  With FULL coefficients the oracle itself may leave
    non-finite values: then their positions are equal, and so is the rest"""
    s0 = sor_case(w, h, spec)
    a = sor_oracle(oracle, s0, w, K, red_black)
    if spec is LOW:
        for k in ("du", "dv"):
            v = valid(a[k], w)
            assert np.isfinite(v).all() and vr.is_subnormal(v).sum() >= 100 and (v[:, 8:16] == 0).all()
    b = {k: c_(v).copy() for k, v in s0.items()}
    ctx.sor_coupled(*[b[k] for k in SOR_KEYS], w, K, 1.9, red_black=red_black)
    for k in ("du", "dv", "a11", "a12", "a22"):
        same(a[k], b[k], w, k)


# ------------------------------------------------------------------------------------------------------
# F. the two-frame path
# ------------------------------------------------------------------------------------------------------
def pair_case(oracle):
    w, h = 65, 17
    im1, im2 = vr.ladder_frames(oracle, w, h, 2, LOW["exps"], LOW["top"], 40)
    rng = np.random.default_rng(41)
    return w, h, im1, im2, noise_plane(rng, w, h, 1.5, 2.5), noise_plane(rng, w, h, 0.5, 1.5)


def pair_oracle(oracle, case, po):
    w, h, im1, im2, wx0, wy0 = case
    wxo, wyo = orc.plane(*wx0.shape), orc.plane(*wx0.shape)
    wxo[...] = wx0; wyo[...] = wy0
    oracle.variational_2frame(wxo, wyo, im1, im2, w, po)
    return wxo, wyo


def test_oracle_two_frame_on_the_low_ladder_is_finite(oracle):
    case = pair_case(oracle)
    wxo, wyo = pair_oracle(oracle, case, orc.params_2f(delta=0.5))
    assert np.isfinite(valid(wxo, 65)).all() and np.isfinite(valid(wyo, 65)).all()
    assert not np.array_equal(valid(wxo, 65), valid(case[4], 65))


@gpu
def test_two_frame_pair_job_on_the_low_ladder(ctx, oracle):
    """one pair job at 65 x 17 on LOW-scaled images (with the colour term, delta = 0.5) against the oracle's two-frame restatement: bit for bit"""
    case = pair_case(oracle)
    w, h, im1, im2, wx0, wy0 = case
    po = orc.params_2f(delta=0.5)
    wxo, wyo = pair_oracle(oracle, case, po)
    assert np.isfinite(valid(wxo, w)).all() and np.isfinite(valid(wyo, w)).all()
    pg = sfa.Params2f(po.alpha, po.gamma, po.delta, po.sigma, po.niter_outer, po.niter_inner, po.niter_solver, po.sor_omega)
    job = sfa.PairJob(ctx, w, h, 1, pg)
    job.upload(0, c_(wx0), c_(wy0), c_(im1), c_(im2))
    job.run()
    wxg, wyg = job.download(0)
    job.close()
    same(wxo, wxg, w, "wx"); same(wyo, wyg, w, "wy")
