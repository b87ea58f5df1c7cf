"""The three operators whose parity with the reference is not pinned -- compute_smoothness,
add_data_and_match / _ref and optimizeOcc's data costs -- against the independent float64 derivations of
tests/indep_ref.py: the oracle on the CPU, the HIP kernels on the GPU (through the C-ABI), with NaN in the stride
padding of every input as well.  Every reference quirk the two implementations reproduce, and a few
plausible slips, are switched on in the derivation one at a time and must then be rejected by the same tolerance:
that shows the inputs reach the branch the quirk lives in.

Tolerance: an fp32 result x passes against the derivation r when |x - r| <= K * 2^-24 * m + TINY, m being r's
magnitude companion (indep_ref.py).  Each rounding of the fp32 chain contributes at most 2^-24 times the magnitude of
the quantity it rounds, and the magnitudes only grow along the chain, so K is the number of roundings on the longest
path from the inputs to one output, plus the factor 2 a square puts on the relative error of its operand:
  - smoothness: difference (1), squared (x2), method 1's central difference (2) and mean (2) squared (x2), sum of
    four squares (3), psi' (<= 4 inside, its argument's error is in m), weight sum (1), * alpha (1), * psi' (1):
    about 20.  K_SMOOTH = 32.
  - data terms: residual (4 products + 4 sums + the channel weight, ~9) squared (x2) over a normaliser (~5 roundings,
    1 division), a sum of up to 6 (5), psi' (4), then mask * delta * psi' / n * w (5), the matrix factor (2-3) and an
    accumulation of up to 9 contributions onto the incoming value (9): about 50.  K_DATA = 64.
  - occlusion costs: a sum of 6 squares (5), psi (3), * rho * delta * mask (3), 4 terms per slot and up to 2*8 slots
    into a label (up to 31 sums), the normaliser's own chain (up to 31 sums, its error enters through the quotient
    rule), * 0.01 (1), / norm (1), + penalty (1): about 80 for S = 9.  K_OCC = 128.
TINY absorbs results that are 0 in fp64 and a flushed subnormal in fp32.

The truncated modified L1 penalty (id 3) jumps at its truncation; elements whose fp64 argument lies within 1e-5 of it
(relative to the argument's magnitude) may take the other branch in fp32 and are excluded -- fewer than 0.1 %.
"""
import numpy as np
import pytest

import indep_ref as ir
import oracle as orc
from synth import noise_color, noise_plane, smooth_noise_color

U = 2.0 ** -24
TINY = 1e-30
K_SMOOTH, K_DATA, K_OCC = 32, 64, 128
MAX_EXCLUDED = 1e-3


def _eps(pid):
    return 0.001 if pid in (1, 3) else 0.05


def verdict(x, ref, K, w):
    """-> (pass mask over the valid region, exclusion mask)"""
    x = np.asarray(x, np.float32)[..., :w].astype(np.float64)
    ex = np.broadcast_to(np.asarray(ref.k, bool), x.shape)
    with np.errstate(invalid="ignore"):
        ok = np.abs(x - ref.v) <= K * U * ref.m + TINY
    return ok | ex, ex


class Excluded:
    """counts the elements excluded near a kink over one test: fewer than MAX_EXCLUDED of them"""

    def __init__(self):
        self.n_ex = self.n = 0

    def check(self):
        assert self.n_ex < MAX_EXCLUDED * self.n, f"{self.n_ex} of {self.n} elements lie near a kink"


def assert_accepts(outs, refs, K, w, what, excluded=None):
    excluded = excluded or Excluded()
    for i, (x, r) in enumerate(zip(outs, refs)):
        ok, ex = verdict(x, r, K, w)
        excluded.n_ex += int(np.count_nonzero(ex))
        excluded.n += ex.size
        if not ok.all():
            y, xx = np.argwhere(~ok)[0]
            xv = float(np.asarray(x)[..., :w][y, xx])
            raise AssertionError(f"{what}: output {i} at (x={xx}, y={y}): {xv!r} vs derivation {r.v[y, xx]!r} "
                                 f"(bound {K * U * r.m[y, xx]:.3g}); {np.count_nonzero(~ok)} elements fail")


def rejects(outs, refs, K, w):
    return any(not verdict(x, r, K, w)[0].all() for x, r in zip(outs, refs))


def assert_variants_rejected(outs, variants, K, w, what):
    """variants: {keyword: derivation with that keyword on}"""
    for name, refs in variants.items():
        assert rejects(outs, refs, K, w), f"{what}: the variant {name} is accepted -- the inputs do not exercise it"


def nan_padded(a, w):
    """a copy of a (..., h, stride) array with NaN in the stride padding"""
    b = np.array(a, np.float32, copy=True)
    b[..., w:] = np.nan
    return b


def bits(a, w):
    return np.ascontiguousarray(np.asarray(a, np.float32)[..., :w]).view(np.int32)


# ------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------
def smooth_inputs(method, pid, w, h):
    rng = np.random.default_rng(1000 * method + 100 * pid + w * 7 + h)
    uu, vv = noise_plane(rng, w, h, -2, 2), noise_plane(rng, w, h, -2, 2)
    if pid == 3:       # the truncation at 0.5: flow differences of a few tenths put arguments on both sides of it
        uu[:, :w] *= 0.15
        vv[:, :w] *= 0.15
    dps = noise_plane(rng, w, h, 0.05, 0.5)
    if method == 2:
        # weights above 1 on every third pixel so that the shadowed test `i < w - 1` (w = the weight) passes there and
        # fails elsewhere; capped at the width, so that the last column never passes: there the reference would read
        # a never-written difference and the next row's weight (no defined value, and the stride padding)
        yy, xx = np.mgrid[0:h, 0:w]
        big = (xx + yy) % 3 == 0
        dps[:, :w] = np.where(big, rng.uniform(1.0, max(1.0, min(float(w), 12.0)), (h, w)), dps[:, :w]).astype(np.float32)
    return uu, vv, dps, orc.Penalty(pid, _eps(pid), 0.5)


def smooth_derivations(method, uu, vv, dps, pen, w, alpha=4.0):
    p = (pen.id, pen.eps, pen.trunc)
    ref = ir.smoothness(method, uu, vv, dps, alpha, p, w)
    var = {}
    if method == 2 and w >= 2:
        var["method2_uses_width"] = ir.smoothness(method, uu, vv, dps, alpha, p, w, method2_uses_width=True)
    return ref, var


DATA_S = {False: (-2.0, -1.0, 0.0, 1.0), True: (-2.0, -1.0, 1.0, 2.0)}        # the values test_data_terms uses
DATA_HD = (0.0, 1.0 / 3.0)


def data_inputs(pid, dt_norm, ref_term, w, h):
    rng = np.random.default_rng(pid + 7 * dt_norm + 13 * ref_term + 31 * w + h)
    # scale 10: residuals of a few units, so that every penalty works away from its quadratic zone
    hh = max(h, 4)            # the pair is at least 4 rows high (the 5-tap vertical filter); _data_stack cuts its stack to h
    I1 = smooth_noise_color(rng, w, hh, 10)
    I2 = smooth_noise_color(rng, w, hh, 10)
    if pid == 3:
        # the truncated L1 (truncation 0.5 for colour, 0.3 for the gradient): a second frame close to the first puts
        # the arguments on both sides of the truncation, and so does a smaller flow increment
        I2 = I1 + noise_color(rng, w, hh, -0.15, 0.15)
    fl = 0.05 if pid == 3 else 0.5
    du, dv = noise_plane(rng, w, h, -fl, fl), noise_plane(rng, w, h, -fl, fl)
    yy, xx = np.mgrid[0:h, 0:w]
    mask = orc.plane(h, I1.shape[-1])
    mask[:, :w] = np.where((xx + 2 * yy) % 5 == 4, 0.0, 0.5)       # occluded on every fifth pixel, never at (0, 0)
    chw = [noise_plane(rng, w, h, 0.5, 1.5) for _ in range(3)]
    sysm = [noise_plane(rng, w, h) for _ in range(5)]
    return dict(I1=I1, I2=I2, du=du, dv=dv, mask=mask, chw=chw, sys=sysm,
                color=orc.Penalty(pid, _eps(pid), 0.5), grad=orc.Penalty(pid, _eps(pid), 0.3))


def data_derivations(inp, D, w, hd, s, dt_norm, ref_term, hg=2.0):
    c, g = inp["color"], inp["grad"]
    args = (inp["sys"], inp["mask"], inp["du"], inp["dv"], D, inp["chw"], hd, hg, s, dt_norm,
            (c.id, c.eps, c.trunc), (g.id, g.eps, g.trunc), ref_term, w)
    ref = ir.data_term(*args)
    var = {}
    if ref_term and not dt_norm:
        if hd != 0:
            var["ch3_keeps_weight"] = ir.data_term(*args, ch3_keeps_weight=True)
        if s * s != 1:                # factorsq == 1 makes the quirk invisible
            var["no_extra_factorsq"] = ir.data_term(*args, no_extra_factorsq=True)
    return ref, var


OCC_RHO = [1.0, 0.5, 2.0, 0.25, 1.5, 0.75, 3.0, 0.125]
OCC_OMEGA = [0.0, 2.0, 0.5, 1.0, 0.0, 0.25, 1.25, 4.0]     # omega = 0 at idx 0 and 4


def occ_inputs(S, pid, w, h):
    ref = S - 1
    rng = np.random.default_rng(pid + 10 * S + 3 * w + h)
    imgs = [[smooth_noise_color(rng, w, h, 10) for _ in range(4)] for _ in range(2 * ref)]     # per slot: succ1, succ2, ref1, ref2
    if pid == 3:
        # with every argument beyond the truncation psi is one constant and the costs no longer depend on rho, omega
        # or idx: second images close to the first put the arguments on both sides of it
        for im in imgs:
            im[1] = im[0] + noise_color(rng, w, h, -0.4, 0.4)
            im[3] = im[2] + noise_color(rng, w, h, -0.4, 0.4)
    yy, xx = np.mgrid[0:h, 0:w]
    masks = []
    for s in range(2 * ref):
        m = noise_plane(rng, w, h, 0, 1)
        m[:, :w] = (m[:, :w] > 0.2).astype(np.float32)
        # rows 0..2 without any support for one label -- label 0 (slots s >= ref) in the even columns, label 1 in the odd
        # ones -- for the norm guard; the last row fully supported for both
        m[:, :w][(yy < 3) & (xx % 2 == (0 if s >= ref else 1))] = 0
        m[h - 1, :w] = 1
        masks.append(m)
    return imgs, masks, (pid, _eps(pid), 0.5), (pid, _eps(pid), 0.3)


OCC_VARIANTS = ("labels_swapped", "idx_off_by_one", "no_norm_guard", "no_dt_scale", "penalty_on_label0")


def occ_derivations(masks, succ, toref, ref, hd, hg, penalty, color, grad, w):
    args = (np.stack(masks), succ, toref, ref, OCC_RHO[:ref], OCC_OMEGA[:ref], hd, hg, penalty, color, grad, w)
    res = ir.occlusion_costs(*args)
    var = {}
    for name in OCC_VARIANTS:
        if name == "idx_off_by_one" and ref < 2:          # one idx only: nothing to be off by
            continue
        var[name] = ir.occlusion_costs(*args, **{name: True})
    return res, var


def occ_params(S, pid):
    hd = float(np.float32(1.0) / np.float32(3.0))             # delta / 3 and gamma / 3 in float, as variational_mt.cpp forms them
    hg = float(np.float32(6.0) / np.float32(3.0))
    return hd, hg, 0.1


# ------------------------------------------------------------------------------------------------------------------
# the derivation itself
# ------------------------------------------------------------------------------------------------------------------
def test_penalties_match_their_closed_forms_and_derivatives():
    """psi' is the derivative of psi away from the kinks (Geman-McClure excepted: its `apply` has no epsilon, its
    `derivative` has), and the ids follow the switch of variational_aux_mt.cpp:909-925"""
    x = ir.V(np.geomspace(1e-4, 50, 400))
    for pid in (0, 1, 2, 3):
        pen = (pid, _eps(pid), 0.5)
        h = 1e-6 * x.v
        num = (ir.psi(pen, ir.V(x.v + h)).v - ir.psi(pen, ir.V(x.v - h)).v) / (2 * h)
        sel = np.abs(np.sqrt(x.v) - 0.5) > 1e-3 if pid == 3 else np.ones_like(x.v, bool)
        assert np.allclose(num[sel], ir.dpsi(pen, x).v[sel], rtol=1e-5), pid
    e2 = float(np.float32(0.05) * np.float32(0.05))
    assert np.allclose(ir.dpsi((4, 0.05, 0.5), x).v, (e2 + 2 * x.v) / (e2 + x.v) ** 2)
    assert np.allclose(ir.psi((4, 0.05, 0.5), x).v, x.v / (x.v + 1) ** 2)
    assert ir.psi((3, 0.001, 0.5), ir.V(np.array([0.3]))).v[0] == np.sqrt(0.5 + float(np.float32(0.001) ** 2))
    assert ir.dpsi((3, 0.001, 0.5), ir.V(np.array([0.3]))).v[0] == 0.0
    assert ir.dpsi((7, 0.001, 0.5), x).v[0] == ir.dpsi((1, 0.001, 0.5), x).v[0]      # any other id: modified L1


def test_penalties_against_the_oracle():
    """the pinned psi / psi' of the oracle inside the same tolerance (the scalar and vector overloads differ only in
    the precision of their arithmetic)"""
    o = orc.Oracle()
    x = np.concatenate([np.geomspace(1e-6, 100, 300), [0.0, 0.2499, 0.2501, 0.09]]).astype(np.float32)
    for pid in range(5):
        pen = orc.Penalty(pid, _eps(pid), 0.5)
        p = (pid, _eps(pid), 0.5)
        xv = ir.V(x.astype(np.float64))
        ds, dv = o.psi_deriv(pen, x)
        for got, ref in ((ds, ir.dpsi(p, xv)), (dv, ir.dpsi(p, xv)), (o.psi_apply(pen, x), ir.psi(p, xv))):
            ok = np.abs(got.astype(np.float64) - ref.v) <= 8 * U * ref.m
            assert ok.all(), (pid, x[~ok], got[~ok], ref.v[~ok])


# ------------------------------------------------------------------------------------------------------------------
# CPU: the oracle against the derivation
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(67, 45), (5, 2)])
@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("pid", [0, 1, 2, 3, 4])
def test_smoothness_oracle(oracle, method, pid, w, h):
    uu, vv, dps, pen = smooth_inputs(method, pid, w, h)
    out = oracle.smoothness(method, uu, vv, dps, w, 4.0, pen)
    ref, var = smooth_derivations(method, uu, vv, dps, pen, w)
    excluded = Excluded()
    assert_accepts(out, ref, K_SMOOTH, w, f"smoothness method {method}", excluded)
    assert_variants_rejected(out, var, K_SMOOTH, w, f"smoothness method {method}")
    excluded.check()
    if method == 2:
        assert "method2_uses_width" in var


def _oracle_data(oracle, inp, D, w, hd, s, dt_norm, ref_term, hg=2.0):
    sysm = [orc.plane(*x.shape) for x in inp["sys"]]
    for a, b in zip(sysm, inp["sys"]):
        a[...] = b
    rc = oracle.add_data(sysm, inp["mask"], inp["du"], inp["dv"], D, inp["chw"], w, hd, hg, s, dt_norm,
                         inp["color"], inp["grad"], ref_term)
    assert rc in (0, None)
    return sysm


@pytest.mark.parametrize("ref_term", [False, True])
@pytest.mark.parametrize("dt_norm", [0, 1])
@pytest.mark.parametrize("pid", [0, 1, 2, 3, 4])
def test_data_terms_oracle(oracle, ref_term, dt_norm, pid):
    w, h = 67, 45
    inp = data_inputs(pid, dt_norm, ref_term, w, h)
    D = oracle.derivative_stack(inp["I1"], inp["I2"], w)
    seen, excluded = set(), Excluded()
    for s in DATA_S[ref_term]:
        for hd in DATA_HD:
            out = _oracle_data(oracle, inp, D, w, hd, s, dt_norm, ref_term)
            ref, var = data_derivations(inp, D, w, hd, s, dt_norm, ref_term)
            what = f"data term dt_norm={dt_norm} ref={ref_term} s={s} hd={hd:.3f}"
            assert_accepts(out, ref, K_DATA, w, what, excluded)
            assert_variants_rejected(out, var, K_DATA, w, what)
            seen |= set(var)
    excluded.check()
    if ref_term and not dt_norm:
        assert seen == {"ch3_keeps_weight", "no_extra_factorsq"}


@pytest.mark.parametrize("S", [2, 3, 5, 9])
@pytest.mark.parametrize("pid", [0, 1, 2, 3, 4])
def test_occlusion_costs_oracle(oracle, S, pid):
    w, h = 37, 21
    ref = S - 1
    imgs, masks, color, grad = occ_inputs(S, pid, w, h)
    hd, hg, penalty = occ_params(S, pid)
    succ = np.stack([oracle.derivative_stack(a, b, w) for a, b, _, _ in imgs])
    toref = np.stack([oracle.derivative_stack(c, d, w) for _, _, c, d in imgs])
    mo = orc.aligned_zeros((2 * ref,) + masks[0].shape); mo[...] = np.stack(masks)
    so = orc.aligned_zeros(succ.shape); so[...] = succ
    to = orc.aligned_zeros(toref.shape); to[...] = toref
    out = oracle.occlusion_costs(mo, so, to, ref, OCC_RHO[:ref], OCC_OMEGA[:ref], hd, hg, penalty,
                                 orc.Penalty(*color), orc.Penalty(*grad), w)
    res, var = occ_derivations(masks, succ, toref, ref, hd, hg, penalty, color, grad, w)
    excluded = Excluded()
    assert_accepts(out, res, K_OCC, w, f"occlusion costs S={S}", excluded)
    assert_variants_rejected(out, var, K_OCC, w, f"occlusion costs S={S}")
    excluded.check()
    assert len(var) == len(OCC_VARIANTS) - (ref < 2)


# ------------------------------------------------------------------------------------------------------------------
# GPU: the HIP kernels against the derivation, zero-padded and NaN-padded
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


def c_(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def sfa_pen(p):
    import slowflow_amd as sfa
    return sfa.Penalty(*p) if isinstance(p, tuple) else sfa.Penalty(p.id, p.eps, p.trunc)


def assert_nan_padding_is_not_read(zero_run, nan_run, w, what):
    for i, (a, b) in enumerate(zip(zero_run, nan_run)):
        assert np.array_equal(bits(a, w), bits(b, w)), f"{what}: output {i} changes with NaN in the stride padding"


# each entry point's smallest accepted shapes (sfa_smoothness h >= 2, sfa_add_data_and_match h >= 1,
# sfa_occlusion_costs h >= 4), then odd, tile-straddling and wide shapes
SMOOTH_SHAPES = [(1, 2), (2, 2), (3, 7), (5, 2), (63, 5), (65, 17), (67, 45), (130, 98)]
DATA_SHAPES = [(1, 1), (1, 6), (5, 1), (63, 5), (65, 17), (67, 45), (130, 98)]
OCC_SHAPES = [(1, 4), (2, 4), (3, 7), (63, 5), (65, 17), (67, 45), (130, 98)]


def _gpu_smooth(ctx, method, uu, vv, dps, pen, w):
    # method 2 reads a neighbour's padding only in the last column and only for a weight above the width: the inputs
    # keep the weights below it there (smooth_inputs), so the whole valid region must be independent of the padding
    zero = ctx.smoothness(method, c_(uu), c_(vv), c_(dps), w, 4.0, sfa_pen(pen))
    nan = ctx.smoothness(method, nan_padded(uu, w), nan_padded(vv, w), nan_padded(dps, w), w, 4.0, sfa_pen(pen))
    assert_nan_padding_is_not_read(zero, nan, w, f"smoothness method {method}")
    return zero


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SMOOTH_SHAPES)
@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("pid", [0, 1, 2, 3, 4])
def test_smoothness_gpu(ctx, method, pid, w, h):
    uu, vv, dps, pen = smooth_inputs(method, pid, w, h)
    out = _gpu_smooth(ctx, method, uu, vv, dps, pen, w)
    ref, var = smooth_derivations(method, uu, vv, dps, pen, w)
    excluded = Excluded()
    assert_accepts(out, ref, K_SMOOTH, w, f"smoothness method {method}", excluded)
    assert_variants_rejected(out, var, K_SMOOTH, w, f"smoothness method {method}")
    excluded.check()


@pytest.mark.gpu
def test_smoothness_gpu_full_size(ctx):
    w, h = 1024, 436
    uu, vv, dps, pen = smooth_inputs(2, 1, w, h)
    out = _gpu_smooth(ctx, 2, uu, vv, dps, pen, w)
    ref, var = smooth_derivations(2, uu, vv, dps, pen, w)
    assert_accepts(out, ref, K_SMOOTH, w, "smoothness method 2, 1024x436")
    assert_variants_rejected(out, var, K_SMOOTH, w, "smoothness method 2, 1024x436")


def _data_stack(inp, w, h):
    """the derivative stack of the pair (at least four rows high, data_inputs) cut to h rows: for the data term the
    stack is only an input"""
    return c_(orc.Oracle().derivative_stack(inp["I1"], inp["I2"], w)[:, :, :h])


def _gpu_data(ctx, inp, D, w, hd, s, dt_norm, ref_term, hg=2.0):
    runs = []
    for pad in (lambda a: c_(a).copy(), lambda a: nan_padded(a, w)):
        sysm = [pad(x) for x in inp["sys"]]
        rc = ctx.add_data(sysm, pad(inp["mask"]), pad(inp["du"]), pad(inp["dv"]), pad(D), [pad(x) for x in inp["chw"]], w, hd, hg, s,
                          dt_norm, sfa_pen(inp["color"]), sfa_pen(inp["grad"]), ref_term)
        assert rc == 0
        runs.append(sysm)
    assert_nan_padding_is_not_read(runs[0], runs[1], w, f"data term dt_norm={dt_norm} ref={ref_term} s={s}")
    return runs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", DATA_SHAPES)
@pytest.mark.parametrize("ref_term", [False, True])
@pytest.mark.parametrize("dt_norm", [0, 1])
@pytest.mark.parametrize("pid", [0, 1, 2, 3, 4])
def test_data_terms_gpu(ctx, ref_term, dt_norm, pid, w, h):
    inp = data_inputs(pid, dt_norm, ref_term, w, h)
    D = _data_stack(inp, w, h)
    excluded = Excluded()
    for s in DATA_S[ref_term]:
        for hd in DATA_HD:
            out = _gpu_data(ctx, inp, D, w, hd, s, dt_norm, ref_term)
            ref, var = data_derivations(inp, D, w, hd, s, dt_norm, ref_term)
            what = f"data term dt_norm={dt_norm} ref={ref_term} s={s} hd={hd:.3f}"
            assert_accepts(out, ref, K_DATA, w, what, excluded)
            assert_variants_rejected(out, var, K_DATA, w, what)
    excluded.check()


@pytest.mark.gpu
def test_data_terms_gpu_full_size(ctx):
    w, h = 1024, 436
    inp = data_inputs(1, 0, True, w, h)
    D = _data_stack(inp, w, h)
    out = _gpu_data(ctx, inp, D, w, 1.0 / 3.0, 2.0, 0, True)
    ref, var = data_derivations(inp, D, w, 1.0 / 3.0, 2.0, 0, True)
    excluded = Excluded()
    assert_accepts(out, ref, K_DATA, w, "data term, 1024x436", excluded)
    excluded.check()
    assert_variants_rejected(out, var, K_DATA, w, "data term, 1024x436")
    assert set(var) == {"ch3_keeps_weight", "no_extra_factorsq"}


def _gpu_occ(ctx, S, imgs, masks, color, grad, w):
    import slowflow_amd as sfa
    ref = S - 1
    p = sfa.default_params()
    p.S, p.delta, p.gamma, p.occlusion_penalty = S, 1.0, 6.0, 0.1
    for i in range(ref):
        p.rho[i], p.omega[i] = OCC_RHO[i], OCC_OMEGA[i]
    p.robust_color.id, p.robust_color.eps, p.robust_color.trunc = color
    p.robust_grad.id, p.robust_grad.eps, p.robust_grad.trunc = grad
    runs = []
    for pad in (c_, lambda a: nan_padded(a, w)):
        runs.append(ctx.occlusion_costs(p, [pad(m) for m in masks], *[[pad(i[k]) for i in imgs] for k in range(4)], w))
    assert_nan_padding_is_not_read(runs[0], runs[1], w, f"occlusion costs S={S}")
    return runs[0]


def _occ_case(ctx, S, pid, w, h):
    ref = S - 1
    imgs, masks, color, grad = occ_inputs(S, pid, w, h)
    hd, hg, penalty = occ_params(S, pid)
    out = _gpu_occ(ctx, S, imgs, masks, color, grad, w)
    o = orc.Oracle()
    succ = np.stack([o.derivative_stack(a, b, w) for a, b, _, _ in imgs])
    toref = np.stack([o.derivative_stack(c, d, w) for _, _, c, d in imgs])
    res, var = occ_derivations(masks, succ, toref, ref, hd, hg, penalty, color, grad, w)
    excluded = Excluded()
    assert_accepts(out, res, K_OCC, w, f"occlusion costs S={S}", excluded)
    assert_variants_rejected(out, var, K_OCC, w, f"occlusion costs S={S}")
    excluded.check()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", OCC_SHAPES)
@pytest.mark.parametrize("S", [2, 3, 5, 9])
@pytest.mark.parametrize("pid", [0, 1, 2, 3, 4])
def test_occlusion_costs_gpu(ctx, S, pid, w, h):
    _occ_case(ctx, S, pid, w, h)


@pytest.mark.gpu
def test_occlusion_costs_gpu_full_size(ctx):
    _occ_case(ctx, 3, 1, 1024, 436)
