"""Pins the CPU restatement (oracle/slowflow_oracle.c) against the reference's own compiled C
(oracle/_ref, built by oracle/Makefile from the reference sources).  Where that library was not built,
the `reflib` fixture answers every call from what the reference produced for exactly those inputs
(tests/golden/ref_pin.npz, tests/ref_replay.py; recorded by tests/golden/make_golden_pin.py): the SHA-256
of every output, met by the oracle's own computation of the same operator, or the outputs themselves where
the oracle has no bit-exact counterpart."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle as orc
from synth import copy_sys, noise_color, noise_plane, smooth_noise_color, sor_system

SIZES = [(67, 45), (64, 48), (130, 98), (5, 4), (2, 2), (9, 33)]


def valid(a, w):
    return a[..., :w]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("order", [1, 2])
def test_convolutions_bit_exact(oracle, reflib, w, h, order):
    if order == 2 and h < 4:
        pytest.skip("5-tap vertical fast path needs h>=4 (image.c:443)")
    rng = np.random.default_rng(w * 1000 + h + order)
    src = noise_plane(rng, w, h, -3, 3)
    for horiz in (True, False):
        a = oracle.convolve(src, w, order, horiz)
        b = reflib.convolve(src, w, order, horiz)
        assert np.array_equal(valid(a, w), valid(b, w)), (order, horiz)


@pytest.mark.parametrize("w,h", [(67, 45), (64, 48), (2, 2), (130, 98), (3, 7)])
@pytest.mark.parametrize("K,omega", [(1, 1.9), (2, 1.9), (30, 1.9), (7, 1.0)])
def test_sor_bit_exact(oracle, reflib, w, h, K, omega):
    rng = np.random.default_rng(w + 31 * h + K)
    sys0 = sor_system(rng, w, h)
    sys0["du"][:, :w] = rng.uniform(-.2, .2, (h, w))
    sys0["dv"][:, :w] = rng.uniform(-.2, .2, (h, w))
    a, b = copy_sys(sys0), copy_sys(sys0)
    oracle.sor(a["du"], a["dv"], a["a11"], a["a12"], a["a22"], a["b1"], a["b2"], a["sh"], a["sv"], w, K, omega)
    reflib.sor(b["du"], b["dv"], b["a11"], b["a12"], b["a22"], b["b1"], b["b2"], b["sh"], b["sv"], w, K, omega)
    for k in ("du", "dv", "a11", "a12", "a22"):
        assert np.array_equal(valid(a[k], w), valid(b[k], w)), k


def test_sor_generic_edge_weights_bit_exact(oracle, reflib):
    """sh[w-1] / sv[h-1] non-zero and non-zero initial guess: the drop-in sor_coupled accepts any planes"""
    w, h = 37, 21
    rng = np.random.default_rng(5)
    sys0 = sor_system(rng, w, h)
    sys0["sh"][:, :] = rng.uniform(0.1, 1, sys0["sh"].shape)
    sys0["sv"][:, :] = rng.uniform(0.1, 1, sys0["sv"].shape)
    sys0["du"][:, :] = rng.uniform(-1, 1, sys0["du"].shape)
    sys0["dv"][:, :] = rng.uniform(-1, 1, sys0["dv"].shape)
    a, b = copy_sys(sys0), copy_sys(sys0)
    oracle.sor(a["du"], a["dv"], a["a11"], a["a12"], a["a22"], a["b1"], a["b2"], a["sh"], a["sv"], w, 5, 1.9)
    reflib.sor(b["du"], b["dv"], b["a11"], b["a12"], b["a22"], b["b1"], b["b2"], b["sh"], b["sv"], w, 5, 1.9)
    for k in ("du", "dv"):
        assert np.array_equal(valid(a[k], w), valid(b[k], w)), k


def test_sor_readable_bit_exact_and_close_to_fast(oracle, reflib):
    w, h = 40, 30
    rng = np.random.default_rng(11)
    sys0 = sor_system(rng, w, h)
    a, b, c = copy_sys(sys0), copy_sys(sys0), copy_sys(sys0)
    oracle.sor(a["du"], a["dv"], a["a11"], a["a12"], a["a22"], a["b1"], a["b2"], a["sh"], a["sv"], w, 30, 1.9, readable=True)
    reflib.sor(b["du"], b["dv"], b["a11"], b["a12"], b["a22"], b["b1"], b["b2"], b["sh"], b["sv"], w, 30, 1.9, readable=True)
    assert np.array_equal(valid(a["du"], w), valid(b["du"], w))
    assert np.array_equal(valid(a["dv"], w), valid(b["dv"], w))
    oracle.sor(c["du"], c["dv"], c["a11"], c["a12"], c["a22"], c["b1"], c["b2"], c["sh"], c["sv"], w, 30, 1.9)
    assert np.max(np.abs(valid(a["du"], w) - valid(c["du"], w))) < 2e-5


@pytest.mark.parametrize("w,h", [(67, 45), (64, 48), (130, 98)])
@pytest.mark.parametrize("factor", [-2, -1, 1, 2, 3])
def test_image_warp_bit_exact(oracle, reflib, w, h, factor):
    rng = np.random.default_rng(w + h + factor + 100)
    src = smooth_noise_color(rng, w, h)
    wx, wy = noise_plane(rng, w, h, -4, 4), noise_plane(rng, w, h, -4, 4)
    # push some samples far outside to exercise clamping and the mask
    wx[0, :5] = 1000; wy[1, :5] = -1000; wx[2, 3] = -0.0
    a, ma = oracle.image_warp(src, wx, wy, w, factor)
    fwx = orc.plane(h, wx.shape[1]); fwy = orc.plane(h, wx.shape[1])
    fwx[...] = np.float32(factor) * wx
    fwy[...] = np.float32(factor) * wy
    b, mb = reflib.image_warp_prescaled(src, fwx, fwy, w)
    assert np.array_equal(valid(a, w), valid(b, w))
    assert np.array_equal(valid(ma, w), valid(mb, w))
    assert 0 < valid(ma, w).mean() < 1


@pytest.mark.parametrize("w,h", [(67, 45), (64, 48)])
def test_sub_laplacian_bit_exact(oracle, reflib, w, h):
    rng = np.random.default_rng(w * h)
    src, wh, wv = noise_plane(rng, w, h), noise_plane(rng, w, h, 0, 2), noise_plane(rng, w, h, 0, 2)
    d0 = noise_plane(rng, w, h)
    a = orc.plane(*d0.shape); a[...] = d0
    b = orc.plane(*d0.shape); b[...] = d0
    oracle.sub_laplacian(a, src, wh, wv, w)
    reflib.sub_laplacian(b, src, wh, wv, w)
    assert np.array_equal(valid(a, w), valid(b, w))


@pytest.mark.parametrize("w,h", [(67, 45), (64, 48)])
def test_dpsis_weight_bit_exact(oracle, reflib, w, h):
    rng = np.random.default_rng(w - h)
    im = smooth_noise_color(rng, w, h)
    a = oracle.dpsis_weight(im, w)
    b = reflib.dpsis_weight(im, w)
    assert np.array_equal(valid(a, w), valid(b, w))
    assert 0 < valid(a, w).min() and valid(a, w).max() <= 0.5


@pytest.mark.parametrize("w,h", [(67, 45), (64, 48)])
def test_derivative_stack_bit_exact(oracle, reflib, w, h):
    """MT stack (variational_mt.cpp:113-133): M=.5*(I2+I1), Iz=I1-I2 == 2-frame get_derivatives(im1=I2, im2=I1)"""
    rng = np.random.default_rng(w + 7 * h)
    I1, I2 = smooth_noise_color(rng, w, h), smooth_noise_color(rng, w, h)
    a = oracle.derivative_stack(I1, I2, w)
    b = reflib.get_derivatives(I2, I1, w)      # dt = im2 - im1 = I1 - I2
    names = ["Ix", "Iy", "Iz", "Ixx", "Ixy", "Iyy", "Ixz", "Iyz"]
    for i, n in enumerate(names):
        assert np.array_equal(valid(a[i], w), valid(b[i], w)), n


@pytest.mark.parametrize("pid", [0, 1, 2, 3, 4, 7])
def test_penalties_bit_exact(oracle, reflib, pid):
    rng = np.random.default_rng(pid)
    x = np.concatenate([rng.uniform(0, 1e-6, 64), rng.uniform(0, 1, 64), rng.uniform(0, 50, 64), [0, 0.25, 0.2499999, 1e-12]]).astype(np.float32)
    for eps, trunc in ((0.001, 0.5), (0.05, 0.5), (0.3, 2.0)):
        xs, s, v = reflib.penalty_derivative(pid, eps, trunc, x)
        pen = orc.Penalty(pid, eps, trunc)
        so, vo = oracle.psi_deriv(pen, xs)
        assert np.array_equal(s, so), (pid, eps, "scalar")
        assert np.array_equal(v, vo), (pid, eps, "vec")


def test_smoothness_method1_near_pinned(oracle, reflib):
    """2-frame compute_smoothness (variational_aux.c:86): same operator with half_alpha/sqrt(x+eps) instead of
    alpha*psi'(x); identical up to rounding order."""
    w, h = 67, 45
    rng = np.random.default_rng(3)
    uu, vv = noise_plane(rng, w, h, -2, 2), noise_plane(rng, w, h, -2, 2)
    dps = noise_plane(rng, w, h, 0.05, 0.5)
    alpha = 4.0
    pen = orc.Penalty(1, 0.001, 0.5)
    sh, sv = oracle.smoothness(1, uu, vv, dps, w, alpha, pen)
    rh, rv = reflib.compute_smoothness(uu, vv, dps, w, alpha / 2)
    for a, b in ((sh, rh), (sv, rv)):
        rel = np.abs(valid(a, w) - valid(b, w)) / np.maximum(np.abs(valid(b, w)), 1e-30)
        assert rel.max() < 4e-7
    assert np.all(sh[:, w - 1:] == 0) and np.all(sv[h - 1] == 0)


def test_data_term_near_pinned(oracle, reflib):
    """2-frame compute_data_and_match (variational_aux.c:226) == MT add_data_and_match with s=-1 (factor -1,
    factor+1 = 0) on the negated temporal derivatives, unit mask/weights, hd = 2*half_delta_over3/... up to
    rounding: MT psi' = 1/(2 sqrt(x+eps)) times hd, 2-frame = half_hd/sqrt(x+eps)."""
    w, h = 67, 45
    rng = np.random.default_rng(9)
    I1, I2 = smooth_noise_color(rng, w, h, 10), smooth_noise_color(rng, w, h, 10)
    D = oracle.derivative_stack(I1, I2, w)
    du, dv = noise_plane(rng, w, h, -.5, .5), noise_plane(rng, w, h, -.5, .5)
    mask = orc.plane(h, du.shape[1], 1.0)
    ones = orc.plane(h, du.shape[1], 1.0)
    delta_over3, gamma_over3 = 1.0 / 3.0, 6.0 / 3.0
    sysm = [orc.plane(h, du.shape[1]) for _ in range(5)]
    pen = orc.Penalty(1, 0.001, 0.5)
    # MT, s = 0: factor 0, factor+1 = 1: r = Iz - Ix*du - Iy*dv, tx = -Ix
    oracle.add_data(sysm, mask, du, dv, D, [ones, ones, ones], w, delta_over3, gamma_over3, 0.0, True, pen, pen)
    # 2-frame operator uses r = Iz' + Ix*du + Iy*dv with Iz' = im2-im1: feed the negated temporal stacks
    Dn = [orc.aligned_zeros(D[i].shape) for i in range(8)]
    for i in range(8):
        Dn[i][...] = D[i]
    for i in (2, 6, 7):
        Dn[i][...] = -D[i]
    ref = reflib.compute_data_and_match(mask, du, dv, Dn, w, delta_over3 / 2, gamma_over3 / 2)
    for a, b, n in zip(sysm, ref, ["a11", "a12", "a22", "b1", "b2"]):
        va, vb = valid(a, w), valid(b, w)
        scale = np.abs(vb).max()
        assert np.max(np.abs(va - vb)) <= 2e-6 * scale, n


def test_expf_restatement():
    """glibc's expf (called by the reference at variational_aux_mt.cpp:700) is not correctly rounded, so the device
    code restates its published algorithm (slowflow_amd/csrc/kernels.hip expf_glibc).  The same restatement in numpy
    must agree with this machine's libm bit for bit."""
    import ctypes
    import struct
    from decimal import Decimal, getcontext
    getcontext().prec = 60
    N = 32
    T = []
    for i in range(N):
        v = float(Decimal(2) ** (Decimal(i) / Decimal(N)))
        T.append((struct.unpack("<Q", struct.pack("<d", v))[0] - (i << 47)) & 0xFFFFFFFFFFFFFFFF)
    T = np.array(T, dtype=np.uint64)
    inv = float.fromhex("0x1.71547652b82fep+0") * N
    C = [float.fromhex("0x1.c6af84b912394p-5") / N / N / N, float.fromhex("0x1.ebfce50fac4f3p-3") / N / N, float.fromhex("0x1.62e42ff0c52d6p-1") / N]
    shift = float.fromhex("0x1.8p+52")
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-8, 0, 150000), rng.uniform(-0.01, 0, 25000), rng.uniform(-80, 5, 25000)]).astype(np.float32)
    z = inv * x.astype(np.float64)
    kd = z + shift
    ki = kd.view(np.uint64)
    kd = kd - shift
    r = z - kd
    t = T[(ki % N).astype(np.int64)] + (ki << np.uint64(47))
    s = t.view(np.float64)
    y = ((C[0] * r + C[1]) * (r * r) + (C[2] * r + 1)) * s
    mine = y.astype(np.float32)
    libm = ctypes.CDLL("libm.so.6")
    libm.expf.restype = ctypes.c_float
    libm.expf.argtypes = [ctypes.c_float]
    ref = np.array([libm.expf(float(v)) for v in x], dtype=np.float32)
    assert (ref != mine).mean() < 1e-5     # 0 here; an FMA build of libm may flip ~1e-9 of them
    # and the kernel's table is this table
    src = open(os.path.join(os.path.dirname(__file__), "..", "slowflow_amd", "csrc", "kernels.hip")).read()
    for v in T:
        assert ("0x%016xull" % int(v)) in src


# ------------------------------------------------------------------------------------------------------
# occlusion step (optimizeOcc): psi itself is pinned; the energies / cut are restated (parity unpinned, oracle header)
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pid,eps,trunc", [(0, .05, .5), (1, .001, .5), (2, .05, .5), (3, .001, .5), (3, .05, .02), (4, .05, .5)])
def test_psi_apply_pinned(oracle, reflib, pid, eps, trunc):
    rng = np.random.default_rng(pid)
    x = np.concatenate([rng.uniform(0, 1e-4, 2000), rng.uniform(0, 2, 2000), rng.uniform(0, 1e4, 2000), [0, 0, 0, 0]]).astype(np.float32)
    xx, v = reflib.penalty_apply(pid, eps, trunc, x)
    assert np.array_equal(v, oracle.psi_apply(orc.Penalty(pid, eps, trunc), xx))


def test_grid_cut_is_the_exact_minimum(oracle):
    """the oracle's Dinic cut against exhaustive search on 4x3 grids"""
    rng = np.random.default_rng(0)
    w, h = 4, 3
    st = orc.stride_of(w)
    for trial in range(40):
        d0, d1 = orc.plane(h, st), orc.plane(h, st)
        d0[:, :w] = rng.uniform(0, 2, (h, w)); d1[:, :w] = rng.uniform(0, 2, (h, w))
        alpha = float(rng.uniform(0, 1))
        occ, e = oracle.grid_cut(d0, d1, alpha, w)
        best = min(np.where(lab, d1[:, :w], d0[:, :w]).astype(np.float64).sum() + alpha * ((lab[:, 1:] != lab[:, :-1]).sum() + (lab[1:] != lab[:-1]).sum())
                   for lab in (np.array([(bits >> i) & 1 for i in range(w * h)]).reshape(h, w) for bits in range(1 << (w * h))))
        assert abs(best - e) < 1e-6
        assert abs(oracle.grid_cut_energy(occ, d0, d1, alpha, w) - e) < 1e-12


@pytest.mark.parametrize("w,h", [(67, 45), (64, 48), (130, 98)])
@pytest.mark.parametrize("kw", [dict(), dict(delta=0.5, niter_outer=3, niter_inner=2), dict(alpha=3.0, gamma=0.2, niter_solver=7, sor_omega=1.5)])
def test_two_frame_variational_end_to_end(oracle, reflib, w, h, kw):
    """the original two-frame refinement (variational.c:101): the restatement against the REAL compiled entry point, bit for bit
    on the whole output -- warp, derivative stack, smoothness, data term, laplacian, SOR, updates, all iterations"""
    rng = np.random.default_rng(w + h)
    im1 = smooth_noise_color(rng, w + 8, h + 8, 40)
    a, b = orc.aligned_zeros((3, h, orc.stride_of(w))), orc.aligned_zeros((3, h, orc.stride_of(w)))
    a[:, :, :w] = im1[:, 4:4 + h, 4:4 + w]
    b[:, :, :w] = im1[:, 3:3 + h, 2:2 + w]                       # translated by (2, 1)
    wx0, wy0 = noise_plane(rng, w, h, 1.5, 2.5), noise_plane(rng, w, h, 0.5, 1.5)
    p = orc.params_2f(**kw)
    wxr, wyr = orc.plane(*wx0.shape), orc.plane(*wx0.shape)
    wxr[...] = wx0; wyr[...] = wy0
    wxo, wyo = wxr.copy(), wyr.copy()
    wxo2, wyo2 = orc.plane(*wx0.shape), orc.plane(*wx0.shape)
    wxo2[...] = wx0; wyo2[...] = wy0
    reflib.variational_2frame(wxr, wyr, a, b, w, p)
    oracle.variational_2frame(wxo2, wyo2, a, b, w, p)
    assert np.array_equal(valid(wxr, w), valid(wxo2, w)) and np.array_equal(valid(wyr, w), valid(wyo2, w))
    assert np.abs(valid(wxr, w) - valid(wx0, w)).max() > 1e-3      # it did move


@pytest.mark.parametrize("w,h", [(67, 45), (64, 48), (130, 98)])
@pytest.mark.parametrize("sigma", [0.5, 0.8, 1.0, 2.3])
def test_gaussian_presmooth_bit_exact(oracle, reflib, w, h, sigma):
    """cfg sigma > 0 (variational_mt.cpp:590-597): gaussian_filter + the generic convolve_horiz / convolve_vert of image.c"""
    rng = np.random.default_rng(int(sigma * 10) + w)
    src = noise_plane(rng, w, h, 0, 255)
    assert np.array_equal(valid(oracle.gaussian_presmooth(src, w, sigma), w), valid(reflib.gaussian_presmooth(src, w, sigma), w))


# ------------------------------------------------------------------------------------------------------
# transitive pins of the MT-only pieces (variational_mt.cpp / variational_aux_mt.cpp need GCO + OpenCV headers and cannot be built
# here): each is tied to something the compiled reference DOES pin
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(67, 45), (64, 48), (130, 98)])
@pytest.mark.parametrize("kw", [dict(), dict(delta=0.5, niter_outer=3), dict(alpha=3.0, gamma=2.0, delta=0.7, niter_solver=7, sor_omega=1.5)])
def test_compute_one_level_forward_is_the_two_frame_variational(oracle, reflib, w, h, kw):
    """orc_compute_one_level (variational_mt.cpp:169-493) with S=2, method forward, modified-L1 everywhere, smoothing 1, normalised data
    term, rho_0 = 1, omega_0 = 0, image statistics (0, 1), one inner iteration IS the reference's two-frame refinement (variational.c:19-84
    through variational():101, compiled as is): same warp of the second frame, same derivative stack up to the sign of the temporal
    derivatives (which only enter squared or in pairs), the same weights written as alpha*psi'(x) = alpha/(2 sqrt(x+eps^2)) instead of
    half_alpha/sqrt(x+eps), mask weights 1 (occ = -1, data_norm = 1), sub_laplacian on uu == wx.  The two differ by rounding order only
    (near-pins of smoothness 4e-7 and data term 2e-6, amplified through the outer iterations: SURVEY H3 measured <= 2e-5 for 5e-7
    per solve).  Measured on these nine cases: 9.5e-7 .. 1.2e-5; the bound asserted is 2.5e-5, a quarter of north_star's 1e-4 on (u, v), so that a
    restatement slip of half the acceptance tolerance in the level's glue does not pass."""
    rng = np.random.default_rng(w + h)
    base = smooth_noise_color(rng, w + 8, h + 8, 40)
    st = orc.stride_of(w)
    im1, im2, dummy = orc.aligned_zeros((3, h, st)), orc.aligned_zeros((3, h, st)), orc.aligned_zeros((3, h, st))
    im1[:, :, :w] = base[:, 4:4 + h, 4:4 + w]
    im2[:, :, :w] = base[:, 3:3 + h, 2:2 + w]                     # translated by (2, 1)
    dummy[:, :, :w] = rng.uniform(0, 255, (3, h, w))              # frame 0 is never read with method forward
    wx0, wy0 = noise_plane(rng, w, h, 1.5, 2.5), noise_plane(rng, w, h, 0.5, 1.5)
    p2 = orc.params_2f(**kw)
    wxr, wyr = orc.plane(h, st), orc.plane(h, st)
    wxr[...] = wx0; wyr[...] = wy0
    reflib.variational_2frame(wxr, wyr, im1, im2, w, p2)
    p = oracle.default_params()
    p.S = 2; p.one_direction = 1; p.smoothing = 1; p.dataterm_norm = 1; p.niter_alter = 1; p.niter_outer = p2.niter_outer; p.niter_inner = 1
    p.niter_solver = p2.niter_solver; p.sor_omega = p2.sor_omega; p.thres_outer = 0; p.thres_inner = 0
    p.alpha = p2.alpha; p.gamma = p2.gamma; p.delta = p2.delta
    for pen in (p.robust_color, p.robust_grad, p.robust_reg):
        pen.id = 1; pen.eps = 0.001; pen.trunc = 0.5
    p.rho[0] = 1; p.omega[0] = 0; p.hbit = 0; p.occlusion_reasoning = 0; p.layers = 1
    for k in range(3):
        p.norm_avg[k] = 0; p.norm_std[k] = 1
    wxo, wyo = orc.plane(h, st), orc.plane(h, st)
    wxo[...] = wx0; wyo[...] = wy0
    rc, _, _ = oracle.compute_one_level(p, wxo, wyo, [dummy, im1, im2], w)
    assert rc == 0
    d = max(np.abs(valid(wxo, w) - valid(wxr, w)).max(), np.abs(valid(wyo, w) - valid(wyr, w)).max())
    moved = np.abs(valid(wxr, w) - valid(wx0, w)).max()
    assert moved > 1e-3 and d <= 2.5e-5, (d, moved)
    # and the whole entry point with one layer is that level
    wxv, wyv = orc.plane(h, st), orc.plane(h, st)
    wxv[...] = wx0; wyv[...] = wy0
    rc, _ = oracle.variational(p, wxv, wyv, [dummy, im1, im2], w)
    assert rc == 0 and np.array_equal(valid(wxv, w), valid(wxo, w)) and np.array_equal(valid(wyv, w), valid(wyo, w))


@pytest.mark.parametrize("dt_norm", [1, 0])
@pytest.mark.parametrize("pid", [1, 2, 0])
def test_ref_term_is_the_successive_term(oracle, pid, dt_norm):
    """add_data_and_match_ref (variational_aux_mt.cpp:408-634) one frame from the reference frame (|s| = 1: g = -1, F2 = 1) forms the same
    residuals r = w(Iz - Ix du - Iy dv), norms Ix^2 + Iy^2 + dn and accumulations as add_data_and_match (:166-403) with s = 0 (f = 0,
    p = 1) -- every extra factor is an exact +-1 -- and two frames away (|s| = 2: g = -2, F2 = 4) the same as one frame away on spatial
    derivatives scaled by 2 (powers of two: exact in fp32).  That ties the restated ref term to the successive term, which is near-pinned to
    the compiled reference (test_data_term_near_pinned).  The unnormalised branch (slow_flow_dataterm 0) carries the reference's quirks
    (channel 3 drops its weight, an extra factor on channel 1) and divides its residuals by s^2: only the sign symmetry holds there;
    that branch stays parity unpinned."""
    w, h = 67, 45
    rng = np.random.default_rng(17 + pid)
    I1, I2 = smooth_noise_color(rng, w, h, 10), smooth_noise_color(rng, w, h, 10)
    D = oracle.derivative_stack(I1, I2, w)
    st = D.shape[-1]
    du, dv = noise_plane(rng, w, h, -.5, .5), noise_plane(rng, w, h, -.5, .5)
    mask = orc.plane(h, st)
    mask[:, :w] = rng.uniform(0, 1, (h, w)).astype(np.float32)
    chw = [noise_plane(rng, w, h, 0.5, 1.5) for _ in range(3)]
    pen = orc.Penalty(pid, 0.01, 0.5)
    hd, hg = 1.0 / 3.0, 6.0 / 3.0

    def run(Dx, s, ref_term, hg=hg):
        sysm = [orc.plane(h, st) for _ in range(5)]
        for a in sysm:
            a[:, :w] = rng0.uniform(-1, 1, (h, w)).astype(np.float32)      # the terms ACCUMULATE: start from a common non-zero state
        rc = oracle.add_data(sysm, mask, du, dv, Dx, chw, w, hd, hg, s, dt_norm, pen, pen, ref_term=ref_term)
        assert rc in (0, None)
        return sysm

    D2 = orc.aligned_zeros(D.shape)
    D2[...] = D
    for i in (0, 1, 3, 4, 5):                                             # Ix, Iy, Ixx, Ixy, Iyy doubled; Iz, Ixz, Iyz as they are
        D2[i] *= 2
    rng0 = np.random.default_rng(5); ref1 = run(D, 1.0, True)
    rng0 = np.random.default_rng(5); refm1 = run(D, -1.0, True)
    rng0 = np.random.default_rng(5); ref2 = run(D, -2.0, True)
    rng0 = np.random.default_rng(5); ref1_scaled = run(D2, 1.0, True)
    for a, b, c_, d, n in zip(ref1, refm1, ref2, ref1_scaled, ["a11", "a12", "a22", "b1", "b2"]):
        assert np.array_equal(valid(a, w), valid(b, w)), n                 # only |s| enters (:416-425)
        if dt_norm:                                                       # the unnormalised residuals are divided by s^2 (:447): no such identity
            assert np.array_equal(valid(c_, w), valid(d, w)), n           # |s| = 2 == |s| = 1 on doubled derivatives
    if dt_norm:
        # colour part alone: bit for bit (x - (-y) == x + y).  With the gradient part the right-hand sides associate their products
        # differently -- (ta*Ixz)*X at :352-353 against (ta*Ixx)*Ixz at :584-585 -- so b1, b2 agree to rounding, the matrix entries exactly.
        rng0 = np.random.default_rng(5); r_c = run(D, 1.0, True, hg=0.0)
        rng0 = np.random.default_rng(5); s_c = run(D, 0.0, False, hg=0.0)
        for a, b, n in zip(r_c, s_c, ["a11", "a12", "a22", "b1", "b2"]):
            assert np.array_equal(valid(a, w), valid(b, w)), n
        rng0 = np.random.default_rng(5); succ0 = run(D, 0.0, False)
        for a, b, n in zip(ref1, succ0, ["a11", "a12", "a22", "b1", "b2"]):
            if n[0] == "a":
                assert np.array_equal(valid(a, w), valid(b, w)), n
            else:
                assert np.abs(valid(a, w) - valid(b, w)).max() <= 1e-6 * np.abs(valid(b, w)).max(), n


@pytest.mark.parametrize("ref,one_direction", [(1, 0), (2, 0), (2, 1), (3, 0)])
def test_mask_weighting_against_numpy(oracle, ref, one_direction):
    """variational_mt.cpp:293-320 evaluated directly: fac = (1 + [occ == 0]) * N, past slots *= [occ >= 0] / fac, future slots *= [occ <= 0] / fac"""
    w, h = 67, 45
    st = orc.stride_of(w)
    rng = np.random.default_rng(ref)
    masks = orc.aligned_zeros((2 * ref, h, st))
    masks[:, :, :w] = (rng.uniform(0, 1, (2 * ref, h, w)) > 0.2).astype(np.float32)
    occ = orc.plane(h, st)
    occ[:, :w] = rng.integers(-1, 2, (h, w)).astype(np.float32)
    rho, omega = rng.uniform(0.5, 2, ref).astype(np.float32), rng.uniform(0, 2, ref).astype(np.float32)
    N = np.float32(0)
    for a in range(ref):
        N = np.float32(N + np.float32(rho[a] + omega[a]))             # :223-226
    want = masks.copy()
    fac = (np.float32(1) + (occ == 0).astype(np.float32)) * N
    back, fwd = (occ >= 0).astype(np.float32) / fac, (occ <= 0).astype(np.float32) / fac
    for s in range(ref if one_direction else 0, 2 * ref):
        want[s] = np.float32(1) * (back if s < ref else fwd) * want[s]
    got = oracle.mask_weight(masks, occ, ref, float(N), one_direction, w)
    assert got.dtype == np.float32 and np.array_equal(valid(got, w), valid(want, w))
    if one_direction:
        assert np.array_equal(got[:ref], masks[:ref])                  # past slots untouched


def test_normalize_against_numpy_fp64(oracle):
    """variational_mt.cpp:17-85: per-channel mean of per-frame means and of per-frame E[x^2] in double over the valid pixels,
    std = sqrt(E[x^2] - mean^2) / 255, I <- (I - mean) / std stored as float; publish = 6 significant digits (:71-84)"""
    w, h, F = 67, 45, 5
    st = orc.stride_of(w)
    rng = np.random.default_rng(0)
    frames = []
    for f in range(F):
        a = orc.aligned_zeros((3, h, st))
        a[:, :, :w] = rng.uniform(0, 255, (3, h, w)).astype(np.float32) * np.float32(0.5 + 0.2 * f)
        a[:, :, w:] = 1e9                                             # padding must not enter the statistics
        frames.append(a)
    src = [f.copy() for f in frames]
    avg, std, af, sf = oracle.normalize(frames, w)
    for k in range(3):
        m = np.mean([s[k, :, :w].astype(np.float64).sum() / (h * w) for s in src])
        q = np.mean([(s[k, :, :w] * s[k, :, :w]).astype(np.float64).sum() / (h * w) for s in src])   # the product is a FLOAT product (:35)
        sd = np.sqrt(q - m * m) / 255
        assert abs(avg[k] - m) <= 1e-9 * abs(m) and abs(std[k] - sd) <= 1e-9 * sd          # summation order is the only freedom
        assert af[k] == np.float32(float("%g" % avg[k])) and sf[k] == np.float32(float("%g" % std[k]))
        for s, f in zip(src, frames):
            want = ((s[k, :, :w].astype(np.float64) - avg[k]) / std[k]).astype(np.float32)
            assert np.array_equal(f[k, :, :w], want)


def test_dpsis_weight_with_statistics_is_the_pinned_weight_of_the_denormalised_image(oracle, reflib):
    """the MT form c*std + avg (variational_aux_mt.cpp:688-690) against the compiled 2-frame compute_dpsis_weight fed the image that was
    de-normalised with the same fp32 operations -- pins non-trivial statistics, not only avg 0 / std 1"""
    w, h = 67, 45
    rng = np.random.default_rng(2)
    im = smooth_noise_color(rng, w, h)
    avg, std = (101.5, 97.25, 88.0), (0.31, 0.29, 0.4)
    den = orc.aligned_zeros(im.shape)
    for k in range(3):
        den[k] = im[k] * np.float32(std[k]) + np.float32(avg[k])
    a = oracle.dpsis_weight(im, w, avg=avg, std=std)
    b = reflib.dpsis_weight(den, w)
    assert np.array_equal(valid(a, w), valid(b, w))


# ---- the pyramid operators (OpenCV arithmetic, absent here: SURVEY 8c says they stay unpinned) get a SECOND, independent derivation: the documented
#      semantics written with numpy / scipy in double precision.  Not a pin (no OpenCV output behind it) -- it guards kernel size, normalisation, border
#      mode and the coordinate mapping against a slip in the C restatement.
def _cv_gaussian_kernel(sigma):
    ksize = int(np.rint(sigma * 4 * 2 + 1)) | 1                      # cv::GaussianBlur with ksize = Size(): cvRound(sigma * 8 + 1) | 1 for CV_32F
    x = np.arange(ksize) - (ksize - 1) * 0.5
    k = np.exp(-0.5 * x * x / (sigma * sigma))
    return k / k.sum()


@pytest.mark.parametrize("w,h,sigma", [(67, 45, 0.745356), (130, 98, 1.0), (64, 48, 1.4142135)])
def test_gaussian_blur_cv_against_scipy(oracle, w, h, sigma):
    from scipy.ndimage import correlate1d
    rng = np.random.default_rng(w)
    src = orc.plane(h, orc.stride_of(w))
    src[:, :w] = rng.uniform(0, 255, (h, w)).astype(np.float32)
    got = oracle.gaussian_blur_cv(src, w, sigma)[:, :w]
    k = _cv_gaussian_kernel(sigma)
    want = correlate1d(correlate1d(src[:, :w].astype(np.float64), k, axis=1, mode="nearest"), k, axis=0, mode="nearest")     # BORDER_REPLICATE
    assert np.abs(got - want).max() < 2e-4 * 255


@pytest.mark.parametrize("sw,sh,dw,dh", [(1024 // 8, 436 // 4, 921 // 8, 392 // 4), (67, 45, 60, 40), (60, 40, 67, 45), (130, 98, 117, 88)])
def test_resize_linear_cv_against_numpy(oracle, sw, sh, dw, dh):
    rng = np.random.default_rng(sw + dw)
    src = orc.plane(sh, orc.stride_of(sw))
    src[:, :sw] = rng.uniform(-3, 3, (sh, sw)).astype(np.float32)
    got = oracle.resize_linear_cv(src, sw, dw, dh)[:, :dw]

    def coords(n_dst, n_src):                                         # cv::resize INTER_LINEAR: src = (dst + .5) * (n_src / n_dst) - .5, clamped
        f = (np.arange(n_dst) + 0.5) * (n_src / n_dst) - 0.5
        i = np.floor(f).astype(int)
        a = f - i
        a = np.where(i < 0, 0.0, a); i = np.maximum(i, 0)
        a = np.where(i >= n_src - 1, 0.0, a); i = np.minimum(i, n_src - 1)
        return i, np.minimum(i + 1, n_src - 1), a
    x0, x1, ax = coords(dw, sw)
    y0, y1, ay = coords(dh, sh)
    s = src[:, :sw].astype(np.float64)
    top = s[y0][:, x0] * (1 - ax) + s[y0][:, x1] * ax
    bot = s[y1][:, x0] * (1 - ax) + s[y1][:, x1] * ax
    want = top * (1 - ay)[:, None] + bot * ay[:, None]
    assert np.abs(got - want).max() < 2e-4                             # the coordinate is a float in cv::resize: ~1e-5 px of rounding times a slope of a few units per pixel
    dst_fx, dwx = oracle.resize_linear_fx(src, sw, dw / sw, dh / sh)   # the Size(0,0), fx, fy form maps coordinates with 1 / f instead
    if dwx == dw and dst_fx.shape[0] == dh:
        assert np.abs(dst_fx[:, :dw] - want).max() < 1e-3


def test_pyramid_sizes_are_float_floor(oracle):
    """variational_mt.cpp:609-610: floor(w * p) with p a float, in float arithmetic, level by level"""
    for (w, h, layers, p) in [(1024, 436, 5, 0.9), (2048, 2048, 6, 0.9), (640, 480, 8, 0.75)]:
        want, cw, ch = [(w, h)], w, h
        for _ in range(1, layers):
            cw, ch = int(np.floor(np.float32(cw) * np.float32(p))), int(np.floor(np.float32(ch) * np.float32(p)))
            want.append((cw, ch))
        assert oracle.pyramid_sizes(w, h, layers, p)[:layers] == want[:len(oracle.pyramid_sizes(w, h, layers, p))]
