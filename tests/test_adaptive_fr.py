"""The adaptiveFR program (step 1 of the pipeline: <sequence>/quantil.dat for slow_flow's `adaptive 1`) and the two library entries it runs on:
sfa_variational_2frame_batch (n pairs in one launch sequence, each bit-identical to the single call) and sfa_flow_magnitude_quantile (an exact radix
select on the GPU, against a numpy restatement of adaptiveFR.cpp:645-668)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import oracle as orc
import slowflow_amd as sfa
from synth import noise_plane, smooth_noise_color, texture_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
PROGRAM = os.path.join(HOST, "adaptiveFR")


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


# ---- the rank rule and the quantile, restated in numpy ---------------------------------------------------------------------------------------
def rank_rule(N, q):
    """adaptiveFR.cpp:660-666 in float32: (k0, k1, average), or None where the reference indexes outside its array"""
    if N == 0 or not (0 < q <= 1):
        return None
    npf = np.float32(np.float32(q) * np.float32(N)) - np.float32(1)
    if npf < np.float32(N - 1) and np.fmod(npf, np.float32(2)) == 0:
        k0, k1, av = int(npf), int(npf) + 1, True
    else:
        k0 = k1 = int(np.ceil(npf)); av = False
    return None if k0 < 0 or k1 >= N else (k0, k1, av)


def np_quantile(us, vs, w, s, q):
    """float32 scale (image_mul_scalar), float32 magnitude, a full sort of the bit patterns with the sign bit cleared (NaN above +Inf), the rule"""
    s = np.float32(s)
    m = []
    for u, v in zip(us, vs):
        a, b = u[:, :w] * s, v[:, :w] * s
        m.append(np.sqrt(a * a + b * b).ravel())
    keys = np.sort(np.concatenate(m).view(np.uint32) & np.uint32(0x7fffffff))
    vals = keys.view(np.float32)
    k0, k1, av = rank_rule(len(vals), q)
    quant = 0.5 * (float(vals[k0]) + float(vals[k1])) if av else float(vals[k0])
    return quant, float(vals[-1])


def same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("N", [1, 2, 3, 5, 10, 11, 40, 97, 1000, 12345, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 7])
@pytest.mark.parametrize("q", [0.5, 0.6, 0.9, 0.99, 1.0, 0.25, 1e-9])
def test_rank_rule_is_the_reference_statement(N, q):
    """the library's one statement of the rule (sfa_quantile_ranks, host only) against the float32 restatement, N through float included"""
    want = rank_rule(N, q)
    if want is None:
        with pytest.raises(sfa.SlowflowError):
            sfa.quantile_ranks(N, q)
    else:
        assert sfa.quantile_ranks(N, q) == want


def test_rank_rule_refusals_and_the_averaging_branch():
    for N, q in ((0, 0.5), (10, 0.0), (10, -0.5), (10, 1.5), (10, float("nan"))):
        with pytest.raises(sfa.SlowflowError):
            sfa.quantile_ranks(N, q)
    assert sfa.quantile_ranks(10, 0.9) == (8, 9, True) and sfa.quantile_ranks(5, 0.6) == (2, 3, True)
    assert sfa.quantile_ranks(2 ** 24 + 3, 0.5) == (2 ** 23 + 1, 2 ** 23 + 1, False)       # N -> float 2^24 + 4


def test_make_builds_the_program_and_unknown_arguments_print_usage(host_build):
    assert os.access(PROGRAM, os.X_OK)
    r = subprocess.run([PROGRAM, "-no_such_option"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "unknown argument -no_such_option" in r.stderr
    assert "usage:" in r.stdout and "./adaptiveFR -path" in r.stdout and "-quantil" in r.stdout


# ---- GPU: the quantile ------------------------------------------------------------------------------------------------------------------------
def fields(rng, n, w, h, lo=-3.0, hi=3.0):
    return [noise_plane(rng, w, h, lo, hi) for _ in range(n)], [noise_plane(rng, w, h, lo, hi) for _ in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,w,h", [(1, 1, 1), (1, 2, 1), (1, 5, 1), (3, 7, 5), (40, 256, 109), (4, 1000, 3)])
@pytest.mark.parametrize("q", [0.5, 0.9, 0.99, 1.0])
@pytest.mark.parametrize("s", [2.0, float(np.float32(1.0 / (0.3 * 3)))])
def test_quantile_is_exact(ctx, n, w, h, q, s):
    rng = np.random.default_rng(n * 1000 + w + h)
    us, vs = fields(rng, n, w, h)
    if rank_rule(n * w * h, q) is None:
        with pytest.raises(sfa.SlowflowError):
            ctx.flow_magnitude_quantile(us, vs, w, s, q)
        return
    got = ctx.flow_magnitude_quantile(us, vs, w, s, q)
    assert got == np_quantile(us, vs, w, s, q)
    assert ctx.flow_magnitude_quantile(us, vs, w, s, q) == got                      # integer counts: the same bits every run


@pytest.mark.gpu
@pytest.mark.parametrize("N,q", [(10, 0.9), (5, 0.6), (12, 0.25), (1002, 0.5), (3, 1.0)])
def test_quantile_averaging_branch(ctx, N, q):
    k0, k1, av = rank_rule(N, q)
    assert av or N == 3
    rng = np.random.default_rng(N)
    us, vs = fields(rng, 1, N, 1)
    assert ctx.flow_magnitude_quantile(us, vs, N, 1.0, q) == np_quantile(us, vs, N, 1.0, q)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2 ** 20, 2 ** 24 + 3])
@pytest.mark.parametrize("q", [0.5, 0.9, 0.99, 1.0])
def test_quantile_large_n(ctx, N, q):
    """N past 2^24: the rule sees N rounded to float (q = 1 at 2^24 + 3 selects past the array and is refused, as the reference would overrun)"""
    rng = np.random.default_rng(7)
    us, vs = fields(rng, 1, N, 1, -20, 20)
    if rank_rule(N, q) is None:
        with pytest.raises(sfa.SlowflowError):
            ctx.flow_magnitude_quantile(us, vs, N, 0.5, q)
        return
    assert ctx.flow_magnitude_quantile(us, vs, N, 0.5, q) == np_quantile(us, vs, N, 0.5, q)


@pytest.mark.gpu
def test_quantile_ties_zeros_and_non_finite(ctx):
    w, h = 64, 20
    z = [orc.plane(h, orc.stride_of(w)) for _ in range(3)]
    for q in (0.5, 0.9, 1.0):
        assert ctx.flow_magnitude_quantile(z, z, w, 2.0, q) == (0.0, 0.0)                # all zero
    rng = np.random.default_rng(3)
    us, vs = fields(rng, 3, w, h)
    for u, v in zip(us, vs):                                                            # heavily tied: four distinct vectors
        u[:, :w] = rng.choice(np.float32([0, 1, -1, 0.5]), size=(h, w)); v[:, :w] = 0
    for q in (0.5, 0.9, 0.99, 1.0):
        assert ctx.flow_magnitude_quantile(us, vs, w, 2.0, q) == np_quantile(us, vs, w, 2.0, q)
    us, vs = fields(rng, 2, w, h)
    us[0][3, 5] = np.inf; vs[1][7, 9] = -np.inf; us[1][0, 0] = 3e38                   # overflow to +Inf in the square
    for q in (0.5, 0.9, 1.0):
        got, want = ctx.flow_magnitude_quantile(us, vs, w, 2.0, q), np_quantile(us, vs, w, 2.0, q)
        assert got == want and got[1] == np.inf
    us[0][1, 1] = np.nan; vs[0][2, 2] = -np.nan                                         # NaN sorts above +Inf, whatever its sign bit
    N = 2 * w * h
    for q in (0.5, (N - 2.0) / N, (N - 1.0) / N, 1.0):
        got, want = ctx.flow_magnitude_quantile(us, vs, w, 2.0, q), np_quantile(us, vs, w, 2.0, q)
        assert same(got[0], want[0]) and np.isnan(got[1]) and np.isnan(want[1]), (q, got, want)


@pytest.mark.gpu
def test_quantile_refusals(ctx):
    rng = np.random.default_rng(0)
    us, vs = fields(rng, 2, 8, 8)
    for q in (0.0, -0.1, 1.01):
        with pytest.raises(sfa.SlowflowError):
            ctx.flow_magnitude_quantile(us, vs, 8, 1.0, q)
    with pytest.raises(sfa.SlowflowError):
        ctx.flow_magnitude_quantile([], [], 8, 1.0, 0.5)


# ---- GPU: the batched two-frame refinement ------------------------------------------------------------------------------------------------------
PARAM_SETS = {"default": dict(), "color_inner": dict(delta=0.5, niter_outer=3, niter_inner=2), "weights": dict(alpha=3.0, gamma=0.2, niter_solver=7, sor_omega=1.5),
              "adaptiveFR": dict(alpha=1.0, gamma=0.72, delta=0.0, sigma=1.1, niter_outer=5)}


def p2f(kw):
    po = orc.params_2f(**kw)
    return po, sfa.Params2f(po.alpha, po.gamma, po.delta, po.sigma, po.niter_outer, po.niter_inner, po.niter_solver, po.sor_omega)


def make_pairs(w, h, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        big = smooth_noise_color(rng, w + 8, h + 8, 40)
        a, b = orc.aligned_zeros((3, h, orc.stride_of(w))), orc.aligned_zeros((3, h, orc.stride_of(w)))
        dx, dy = 1 + i % 4, 1 + (i // 4) % 3
        a[:, :, :w] = big[:, 4:4 + h, 4:4 + w]
        b[:, :, :w] = big[:, 4 - dy:4 - dy + h, 4 - dx:4 - dx + w]
        out.append((a, b, noise_plane(rng, w, h, dx - 0.5, dx + 0.5), noise_plane(rng, w, h, dy - 0.5, dy + 0.5)))
    return out


_single = {}


def singles(ctx, w, h, case):
    """every pair refined alone by sfa_variational_2frame (cached per size and parameter set)"""
    key = (w, h, case)
    if key not in _single:
        pairs = make_pairs(w, h, 128, w * h)
        _, pg = p2f(PARAM_SETS[case])
        res = []
        for a, b, wx0, wy0 in pairs:
            wx, wy = wx0.copy(), wy0.copy()
            ctx.variational_2frame(wx, wy, a, b, w, pg)
            res.append((wx, wy))
        _single[key] = (pairs, res)
    return _single[key]


def run_batch(ctx, pairs, w, pg):
    wxs, wys = [p[2].copy() for p in pairs], [p[3].copy() for p in pairs]
    ctx.variational_2frame_batch(wxs, wys, [p[0] for p in pairs], [p[1] for p in pairs], w, pg)
    return wxs, wys


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(PARAM_SETS))
@pytest.mark.parametrize("w,h", [(67, 45), (256, 109)])
@pytest.mark.parametrize("n", [1, 2, 5, 40, 128])
def test_batch_is_the_single_call(ctx, n, w, h, case):
    pairs, want = singles(ctx, w, h, case)
    po, pg = p2f(PARAM_SETS[case])
    sel = list(range(n)) if n < 128 else list(range(128))
    wxs, wys = run_batch(ctx, [pairs[i] for i in sel], w, pg)
    for k, i in enumerate(sel):
        assert np.array_equal(wxs[k][:, :w], want[i][0][:, :w]) and np.array_equal(wys[k][:, :w], want[i][1][:, :w]), (n, k)
    if n in (5, 40):                                                                     # the position of a pair in the batch does not matter
        rev = sel[::-1]
        rxs, rys = run_batch(ctx, [pairs[i] for i in rev], w, pg)
        for k, i in enumerate(rev):
            assert np.array_equal(rxs[k][:, :w], want[i][0][:, :w]) and np.array_equal(rys[k][:, :w], want[i][1][:, :w]), ("reversed", n, k)
    if orc.ref_available() and n <= 5:                                                   # and against the compiled reference where it travelled along
        for k, i in enumerate(sel):
            a, b, wx0, wy0 = pairs[i]
            wxr, wyr = orc.plane(*wx0.shape), orc.plane(*wx0.shape)
            wxr[...] = wx0; wyr[...] = wy0
            orc.RefLib().variational_2frame(wxr, wyr, a, b, w, po)
            assert np.array_equal(wxr[:, :w], wxs[k][:, :w]) and np.array_equal(wyr[:, :w], wys[k][:, :w])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["default", "color_inner", "weights"])
def test_batch_carries_the_golden_pair(ctx, case):
    """the committed outputs of the compiled reference's own variational() (tests/golden/ref_two_frame.npz), as pair 17 of a batch of 40"""
    T = np.load(os.path.join(os.path.dirname(__file__), "golden", "ref_two_frame.npz"))
    w, h = (int(v) for v in T["size"])
    _, pg = p2f(PARAM_SETS[case])
    c_ = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    others = make_pairs(w, h, 40, 5)
    pairs = [(c_(a), c_(b), c_(x), c_(y)) for a, b, x, y in others]
    pairs[17] = (c_(T["im1"]), c_(T["im2"]), c_(T["wx0"]), c_(T["wy0"]))
    wxs, wys = run_batch(ctx, pairs, w, pg)
    assert np.array_equal(wxs[17][:, :w], T[f"{case}_wx"]) and np.array_equal(wys[17][:, :w], T[f"{case}_wy"])


@pytest.mark.gpu
def test_batch_refusals(ctx):
    a, b, wx, wy = make_pairs(67, 45, 1, 0)[0]
    with pytest.raises(sfa.SlowflowError):
        ctx.variational_2frame_batch([], [], [], [], 67)
    with pytest.raises(sfa.SlowflowError):
        ctx.variational_2frame_batch([wx] * 129, [wy] * 129, [a] * 129, [b] * 129, 67)


# ---- GPU: the program end to end ------------------------------------------------------------------------------------------------------------
def write_ppm(path, img):
    h, w = img.shape[1:]
    data = np.clip(np.round(img[:, :, :w]), 0, 255).astype(np.uint8).transpose(1, 2, 0).tobytes()
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(data)


def read_flo(path):
    with open(path, "rb") as f:
        tag, w, h = struct.unpack("<fii", f.read(12))
        d = np.frombuffer(f.read(), np.float32).reshape(h, w, 2)
    assert tag == 202021.25
    return d[..., 0].copy(), d[..., 1].copy()


def adaptive_rates_keyframes(quantil, hfr_quantil, lfr_factor, keyframes, steps):
    """slow_flow's rates with keyframes (the reference's slow_flow.cpp:340-351)"""
    hfr = int(max(1.0, round(hfr_quantil / quantil)))
    while hfr < keyframes and keyframes % (hfr * steps) != 0:
        hfr += 1
    lfr = min(keyframes, hfr * lfr_factor)
    while ((lfr * steps < keyframes and (keyframes % (lfr * steps) != 0 or (keyframes % (lfr * steps) == 0 and (lfr * steps) % (hfr * steps) != 0)))
           or (lfr * steps >= keyframes and (lfr * steps) % (hfr * steps) != 0)):
        lfr += 1
    return hfr, min(keyframes // steps, lfr)


@pytest.mark.gpu
def test_program_end_to_end(host_build, tmp_path):
    W, H, DX, DY = 256, 192, 2.0, -1.0                    # per recorded frame, full resolution
    scale, skip, step, samples = 0.25, 2, 3, 4
    seq = tmp_path / "data" / "seqA"
    seq.mkdir(parents=True)
    for k in range(step * (samples - 1) + skip + 1):
        write_ppm(str(seq / ("%07i.ppm" % k)), texture_frame(W, H, k, DX, DY))
    sw, sh = int(W * scale), int(H * scale)
    fu, fv = DX * skip * scale, DY * skip * scale            # the motion of a sample at the scaled size
    tmpd = seq / "adaptiveFR" / "tmp"
    tmpd.mkdir(parents=True)
    ys, xs = np.mgrid[2:sh - 2:3, 2:sw - 2:3]
    for i in range(samples):
        a = i * step
        with open(str(tmpd / ("matches_%d_%d.dat" % (a, a + skip))), "w") as f:
            for x, y in zip(xs.ravel(), ys.ravel()):
                f.write("%d %d %g %g 1.0 0\n" % (x, y, x + fu, y + fv))
        np.ones(sw * sh, np.float32).tofile(str(tmpd / ("edges_%d.dat" % a)))
    base = str(tmp_path / "data") + "/"
    cmd = [PROGRAM, "-path", base, "-folder", "seqA", "-format", "%07i.ppm", "-samples", str(samples), "-step", str(step), "-skip", str(skip),
           "-scale", str(scale)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = seq / "adaptiveFR"
    us, vs = [], []
    for i in range(samples):
        a = i * step
        assert (out / "sequence" / ("frame_epic_%d.png" % a)).exists() and (out / "sequence" / ("frame_epic_%d.png" % (a + skip))).exists()
        assert open(str(out / "tmp" / ("frame_%d.png" % a)), "rb").read(8) == b"\x89PNG\r\n\x1a\n"
        u, v = read_flo(str(out / ("%07i.flo" % a)))
        assert u.shape == (sh, sw)
        inner = (slice(6, sh - 6), slice(6, sw - 6))
        assert abs(u[inner] - fu).mean() < 0.2 and abs(v[inner] - fv).mean() < 0.2, (i, abs(u[inner] - fu).mean(), abs(v[inner] - fv).mean())
        us.append(u); vs.append(v)
    assert (out / "results.info").read_text().startswith("Adaptive Frame rate\n\nsamples\t4\n")
    assert "seqA\t0.9 quantil\t" in (tmp_path / "data" / "results.info").read_text()
    assert (out / "config.cfg").exists()
    quant, mx = np_quantile(us, vs, sw, np.float32(1.0 / (scale * skip)), np.float32(0.9))
    qtext = (seq / "quantil.dat").read_text()
    assert qtext == "%g\n%g\n" % (quant, mx), (qtext, quant, mx)
    # a second run reads the .flo files back and refines nothing
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.count("already exist") == samples and "finished" not in r.stdout, r.stdout + r.stderr
    assert (seq / "quantil.dat").read_text() == qtext
    # slow_flow with `adaptive 1` reads the quantile that was written and picks the rates it implies
    (tmp_path / "adaptiveFR.dat").write_text("opt_hfr_quantil\t2\nopt_lfr_quantil\t8\nopt_lfr_rate\t4\n")
    cfg = tmp_path / "run.cfg"
    cfg.write_text("file\t%s/%%07i.ppm\noutput\t%s/out\nJets\t1\nstart\t0\nmax_fps\t200\nref_fps\t20\nadaptive\t1\nadaptive_fr_file\t%s/adaptiveFR.dat\n"
                   "16bit\t0\nraw\t0\nscale\t0.25\ndeep_matching\t0\ngpus\t1\nslow_flow_S\t2\nslow_flow_layers\t1\nslow_flow_niter_alter\t1\n"
                   "slow_flow_niter_outer\t1\nslow_flow_occlusion_reasoning\t0\n" % (seq, tmp_path, tmp_path))
    hfr, lfr = adaptive_rates_keyframes(float(qtext.split()[0]), 2.0, 4, 10, 1)
    r = subprocess.run([os.path.join(HOST, "slow_flow"), str(cfg), "-overwrite", "-fr", "0"], capture_output=True, text=True, timeout=600)
    assert ("hfr_rate %d" % hfr) in r.stdout and ("lfr_rate %d" % lfr) in r.stdout, r.stdout + r.stderr
    # a missing match file: listed by name, exit status 2, nothing refined
    missing = tmpd / ("matches_%d_%d.dat" % (step, step + skip))
    missing.unlink()
    r = subprocess.run(cmd + ["-overwrite"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and str(missing) in r.stderr.replace("//", "/") and "finished" not in r.stdout, r.stdout + r.stderr
