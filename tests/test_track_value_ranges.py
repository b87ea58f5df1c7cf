"""Value-range parity of the tracking stage: what accumulate.hip, jet_resample.hip, energy.hip, fill.hip, fuse.hip and the resident job of track.hip do with
values the rest of the suite never feeds them -- subnormal and huge flows, the UNKNOWN_FLOW trajectories of the fill-in, positions on and one ulp off the image's
edges, Inf and NaN.  tests/value_ranges.py builds the inputs and names the classes an input reaches; the references are the restatements (accum_ref, jet_resample_ref,
energy_ref, fill_ref, fuse_ref, track_inputs.restate), which assert that every index they form lies inside its plane.

The CPU tests run first and without a GPU: the two restatements of a stage agree on every input, every class a GPU test claims is reached in more than one
64-column segment, and each value rule (the product with a zero-weight tap, addJC's `> 1e9` break, NaN fails the bounds, a NaN energy is absent) changes the
restatement's result on these inputs when it is switched off.  Every GPU comparison is bit for bit with NaN == NaN and equal sets of NaN, +Inf, -Inf (fp32:
subnormal) positions.

  accumulate   accumulate_consistent == accum_ref.accumulate on the ladder, the edge-landing field and the sprinkle; float2 and (half-size source) double2 path
  resample     jet_flow_resample == jet_resample_ref.resample_flow with Inf / NaN under the zero weights of the clamped last row and column
  energies     hypothesis_energies == energy_ref.energies with the fp64 specials in the accumulated flows, laddered flows and frames, three penalties, three regimes
  fill         fill_matches / fill_trajectories == fill_ref with the fp64 / fp32 specials, conversions beyond FLT_MAX and float * int overflow
  fusion       fuse_hypotheses == fuse_ref.fuse on finite energies of any magnitude, on float overflow, and with NaN energies and flows in one segment of three
  resident job TrackJob on T1 with the sprinkle in one segment's flows == track_inputs.restate; the other segments are those of the run without it"""
import numpy as np
import pytest

import fill_ref
import fuse_ref as fr
import slowflow_amd as sfa
import track_inputs as ti
import value_ranges as vr
from accum_ref import accumulate, accumulate_scalar, grid
from energy_ref import Params as EnergyParams, derivatives, energies, energies_scalar
from jet_resample_ref import decode_occlusion_scaled, resample_flow
from value_ranges import H, SMALL, W

gpu = pytest.mark.gpu
F32 = np.float32
SHAPES = [(W, H), SMALL]
SHAPE_IDS = ["136x24", "5x4"]


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


def same(ref, got, what=None):
    """got == ref bit for bit with NaN == NaN (a NaN's sign and payload are not compared), and the same positions of NaN, +Inf, -Inf and, for fp32, subnormals"""
    ref, got = np.asarray(ref), np.asarray(got)
    assert ref.shape == got.shape and ref.dtype == got.dtype, (what, ref.shape, got.shape, ref.dtype, got.dtype)
    if ref.dtype.kind != "f":
        bad = ref != got
        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), ref[bad][:4], got[bad][:4])
        return
    sets = [("nan", np.isnan), ("+inf", lambda a: a == np.inf), ("-inf", lambda a: a == -np.inf)]
    if ref.dtype == np.float32:
        sets.append(("subnormal", vr.is_subnormal))
    for name, fn in sets:
        so, sg = fn(ref), fn(got)
        assert np.array_equal(so, sg), (what, name, int(so.sum()), int(sg.sum()), np.argwhere(so != sg)[:4].tolist())
    nan = np.isnan(ref)
    bad = ~nan & ((ref != got) | (np.signbit(ref) != np.signbit(got)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), ref[bad][:4], got[bad][:4])


def differs(a, b):
    """whether two results of one restatement differ anywhere (NaN == NaN)"""
    try:
        for x, y in zip(a, b):
            same(x, y)
    except AssertionError:
        return True
    return False


def mixes(a):
    """a result that holds NaN, an infinity and finite values: the comparison is not of one kind alone"""
    a = np.asarray(a, np.float64)
    return bool(np.isnan(a).any() and np.isinf(a).any() and np.isfinite(a).any())


def bands(w):
    return (8, 3) if w >= 64 else (1, 1)


def strided(a, w, pad=0.0, dtype=F32):
    """(..., h, w) -> (..., h, stride_of(w)) with the padding filled with `pad`"""
    out = np.full(a.shape[:-1] + (sfa.stride_of(w),), pad, dtype)
    out[..., :w] = a
    return out


# ======================================================================================================
# accumulate
# ======================================================================================================
ACC_INPUTS = ("ladder", "edge", "sprinkle")
ACC_FF = 6
# with and without masks, discard 0 / 1, epsilon 0 / 1 / 1e30; all_steps = False is the last plane of the same restatement
ACC_GRID = [(masks, discard, eps) for masks in (False, True) for discard in (False, True) for eps in (0.0, 1.0, 1e30)]
# what the three inputs together must reach (prefixes: value_ranges.accumulate_classes)
ACC_CLASSES = ("pos_fail_nan", "pos_fail_magnitude", "pos_fail_ulp", "pos_pass_ulp", "pos_pass_zero", "pos_pass_last", "pos_pass_integer",
               "tgt_fail_nan", "tgt_fail_magnitude", "tgt_fail_ulp", "tgt_pass_ulp", "tgt_pass_zero", "tgt_pass_last",
               "fwd_edge_zero_tap", "bwd_edge_zero_tap", "fwd_zero_tap", "bwd_zero_tap")


def acc_input(name, w, h, FF=ACC_FF):
    """(fu, fv, bu, bv) fp32 (FF, h, w) and masks uint8 (FF, h, w)"""
    bx, by = bands(w)
    if name == "ladder":
        flows = vr.traj_flows(FF, h, w, 1, band=bx)
    elif name == "edge":
        flows = vr.edge_landing(FF, h, w, bx, by)
    else:                                                                       # flows of a pixel or two, so that trajectories stay and meet the special values
        flows = vr.traj_flows(FF, h, w, 2, band=bx, sprinkle_seed=40, mags=np.ones(1, F32))
    masks = np.where(np.random.default_rng(7).random((FF, h, w)) < 0.1, 0, 255).astype(np.uint8)
    return flows, masks


@pytest.fixture(scope="module")
def acc_refs():
    """the restatement's result, trace and classes of every (shape, input, masks, discard, epsilon): computed once, shared by the CPU and the GPU tests"""
    cache = {}

    def get(shape, name, use_masks, discard, eps):
        key = (shape, name, use_masks, discard, eps)
        if key not in cache:
            w, h = shape
            flows, masks = acc_input(name, w, h)
            trace = []
            with np.errstate(all="ignore"):
                ref = accumulate(*flows, masks if use_masks else None, eps, 0, discard, trace=trace)
            gw, gh, incr, start = grid(w, h, 0)
            cache[key] = (ref, vr.accumulate_classes(trace, flows, h, w, gw, incr, start))
        return cache[key]
    return get


@pytest.mark.parametrize("name", ACC_INPUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_accumulate_restatements_agree(acc_refs, shape, name):
    """vectorised == scalar on every output; on the small shape for the whole parameter grid, on the ladder shape for one setting per epsilon"""
    w, h = shape
    flows, masks = acc_input(name, w, h)
    settings = ACC_GRID if shape == SMALL else [ACC_GRID[0], ACC_GRID[7], ACC_GRID[11]]
    assert {s[2] for s in settings} == {0.0, 1.0, 1e30}
    for use_masks, discard, eps in settings:
        ref, _ = acc_refs(shape, name, use_masks, discard, eps)
        with np.errstate(all="ignore"):
            b = accumulate_scalar(*flows, masks if use_masks else None, eps, 0, discard)
        for k, (x, y) in enumerate(zip(ref, b)):
            same(x, y, (name, use_masks, discard, eps, k))


def test_accumulate_inputs_reach_every_class(acc_refs):
    """on the ladder shape every class is reached in more than one 64-column segment, by the input built for it; the results mix NaN, Inf and finite values"""
    reached = {}
    for name in ACC_INPUTS:
        for use_masks, discard, eps in ACC_GRID:
            ref, classes = acc_refs((W, H), name, use_masks, discard, eps)
            for k, segs in classes.items():
                reached.setdefault((name, k), set()).update(segs)
            if name == "sprinkle":
                assert mixes(ref[0]) and mixes(ref[1]), (name, use_masks, discard, eps)
            if name == "ladder":
                m = np.abs(ref[0][np.isfinite(ref[0]) & (ref[0] != 0)])
                assert m.min() * 2.0 ** 150 < m.max(), (m.min(), m.max())      # subnormal flows and FLT_MAX ones, accumulated
    for k in ACC_CLASSES:
        segs = set().union(*[reached.get((name, k), set()) for name in ACC_INPUTS])
        assert len(segs) > 1, (k, sorted(segs))
    for k in ("pos_fail_ulp", "pos_pass_ulp", "pos_pass_zero", "pos_pass_last", "tgt_fail_ulp", "tgt_pass_ulp"):
        assert len(reached["edge", k]) > 1, k                                   # the edge-landing field lands where it says
    for k in ("pos_fail_magnitude", "tgt_fail_magnitude"):
        assert len(reached["ladder", k]) > 1, k
    for k in ("pos_fail_nan", "tgt_fail_nan", "fwd_edge_zero_tap", "bwd_edge_zero_tap"):
        assert len(reached["sprinkle", k]) > 1, k


def test_edge_landing_positions_are_exact():
    """the positions after step 0 that the field is named for, as doubles: no rounding in x + (double)u"""
    w, h = W, H
    fu, fv, _, _ = vr.edge_landing(3, h, w)
    x = np.arange(w, dtype=np.float64) + fu[0][0].astype(np.float64)
    y = np.arange(h, dtype=np.float64) + fv[0][:, 0].astype(np.float64)
    for c, n in ((x, w), (y, h)):
        assert c[0] == -2.0 ** -149 and (c == n - 1).sum() >= 2 and (c == n).sum() >= 2 and (c == n - 1.5).sum() >= 2 and (c == -1).sum() >= 2
        zero = c == 0
        assert zero.sum() >= 2 and not np.signbit(c[zero]).any()                # +0.0; -0.0 is no sum of a pixel and a flow
    assert np.signbit(fu[0][0]).any() and (fu[0][0][np.signbit(fu[0][0])] == 0).any()    # the -0.0 flows are there
    assert 1.5 - vr.ulp_below(w) == 0.5 * 3.0 + 0.5 * float(fu[1][0, w - 1]) and (w - 1.5) + (1.5 - vr.ulp_below(w)) == np.nextafter(np.float64(w), 0)


@pytest.mark.parametrize("rule", ["zero_weight_tap", "nan_outside"])
def test_accumulate_value_rules_are_pinned(acc_refs, rule):
    """with the rule switched off in the restatement, its result on at least one of the GPU tests' inputs changes: the GPU comparison pins the rule"""
    changed = []
    for name in ACC_INPUTS:
        flows, _ = acc_input(name, W, H)
        ref, _ = acc_refs((W, H), name, False, False, 1.0)
        with np.errstate(all="ignore"):
            changed.append(differs(ref, accumulate(*flows, None, 1.0, 0, False, off=(rule,))))
    assert any(changed), rule


def acc_gpu(ctx, flows, masks, w, eps, discard, all_steps, source=None):
    sw = w if source is None else source.sw
    arrs = [strided(a, sw, pad=np.nan)[None] if source is None else np.ascontiguousarray(a[None]) for a in flows]
    m = None
    if masks is not None:
        m = strided(masks, sw, pad=0, dtype=np.uint8)[None] if source is None else np.ascontiguousarray(masks[None])
    au, av, tr = ctx.accumulate_consistent(*arrs, w, eps, 0, discard, all_steps, m, source=source)
    return au[0], av[0], tr[0]


@gpu
@pytest.mark.parametrize("name", ACC_INPUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_accumulate(ctx, acc_refs, shape, name):
    w, h = shape
    flows, masks = acc_input(name, w, h)
    for use_masks, discard, eps in ACC_GRID:
        ref, _ = acc_refs(shape, name, use_masks, discard, eps)
        for all_steps in (True, False):
            got = acc_gpu(ctx, flows, masks if use_masks else None, w, eps, discard, all_steps)
            want = ref if all_steps else (ref[0][-1:], ref[1][-1:], ref[2])
            for k, (x, y) in enumerate(zip(want, got)):
                same(x, y, (name, use_masks, discard, eps, all_steps, k))


def half_size_case(name):
    """the flows and raw occlusion images of a (68, 12) source of the ladder shape, and the restatement's planes at (136, 24): the double2 path"""
    sw, sh = W // 2, H // 2
    flows, _ = acc_input(name, sw, sh, 4)
    occ = np.where(np.random.default_rng(9).random((4, sh, sw)) < 0.1, 255, 0).astype(np.uint8)
    with np.errstate(all="ignore"):
        f = [resample_flow(flows[0][k], flows[1][k], F32(2)) for k in range(4)]
        b = [resample_flow(flows[2][k], flows[3][k], F32(2)) for k in range(4)]
    at_size = tuple(np.stack([q[i] for q in src]) for src in (f, b) for i in (0, 1))
    masks = np.stack([decode_occlusion_scaled(g, F32(2)) for g in occ])
    return flows, occ, at_size, masks


@pytest.fixture(scope="module")
def half_size():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = half_size_case(name)
        return cache[name]
    return get


@pytest.mark.parametrize("name", ACC_INPUTS)
def test_accumulate_half_size_restatements_agree(half_size, name):
    """the resampled planes are doubles; vectorised == scalar on them, and the result still mixes NaN, Inf and finite values"""
    _, _, at_size, masks = half_size(name)
    assert at_size[0].dtype == np.float64 and at_size[0].shape == (4, H, W)
    with np.errstate(all="ignore"):
        a = accumulate(*at_size, masks, 1.0, 0, False)
        b = accumulate_scalar(*at_size, masks, 1.0, 0, False)
    for k, (x, y) in enumerate(zip(a, b)):
        same(x, y, (name, k))
    if name == "sprinkle":
        assert mixes(a[0])


@gpu
@pytest.mark.parametrize("name", ACC_INPUTS)
def test_accumulate_half_size_source(ctx, half_size, name):
    """only the ladder shape has a half-size source (5 x 4 has none): flows resampled to double2 on the GPU, occlusion images decoded there"""
    flows, occ, at_size, masks = half_size(name)
    src = sfa.jet_source(W // 2, H // 2, rescale=2.0)
    assert src.target() == (W, H)
    for use_masks, discard, eps in ACC_GRID:
        with np.errstate(all="ignore"):
            ref = accumulate(*at_size, masks if use_masks else None, eps, 0, discard)
        for all_steps in (True, False):
            got = acc_gpu(ctx, flows, occ if use_masks else None, W, eps, discard, all_steps, source=src)
            want = ref if all_steps else (ref[0][-1:], ref[1][-1:], ref[2])
            for k, (x, y) in enumerate(zip(want, got)):
                same(x, y, (name, use_masks, discard, eps, all_steps, k))


# ======================================================================================================
# flow resample
# ======================================================================================================
def resample_case(sw, sh):
    """ladder plus sprinkle, with +Inf on the last source row and column (zero weight there: 0 * Inf = NaN) and -Inf / NaN next to them"""
    fu, fv, _, _ = vr.traj_flows(2, sh, sw, 3, band=bands(2 * sw)[0], sprinkle_seed=60)
    fu[:, sh - 1, 1], fu[:, 1, sw - 1], fv[:, sh - 1, sw - 1] = np.inf, np.inf, np.inf
    fv[:, sh - 1, 0], fu[:, 0, sw - 1] = -np.inf, np.nan
    return fu, fv


RESAMPLE_SHAPES = [(W // 2, H // 2), SMALL]            # -> (136, 24) and (10, 8)


@pytest.fixture(scope="module")
def resample_refs():
    out = {}
    for sw, sh in RESAMPLE_SHAPES:
        fu, fv = resample_case(sw, sh)
        with np.errstate(all="ignore"):
            out[sw, sh] = (fu, fv, [resample_flow(fu[k], fv[k], F32(2)) for k in range(2)])
    return out


@pytest.mark.parametrize("shape", RESAMPLE_SHAPES, ids=["68x12", "5x4"])
def test_resample_input_reaches_the_zero_weight_taps(resample_refs, shape):
    """an Inf on the clamped last row / column becomes NaN through its zero-weight product; leaving that product out changes the result"""
    sw, sh = shape
    fu, fv, ref = resample_refs[shape]
    assert np.isnan(ref[0][0][-1, 2]) and np.isnan(ref[0][0][2, -1]) and np.isnan(ref[0][1][-1, -1])     # +Inf under weight zero
    assert mixes(ref[0][0]) and mixes(ref[0][1])
    with np.errstate(all="ignore"):
        off = resample_flow(fu[0], fv[0], F32(2), zero_taps=False)
    assert differs(ref[0], off) and off[0][-1, 2] == np.inf
    if sw > 64:
        nan_cols = np.nonzero(np.isnan(ref[0][0]).any(0))[0]
        assert len(set((nan_cols // 64).tolist())) > 1


@gpu
@pytest.mark.parametrize("shape", RESAMPLE_SHAPES, ids=["68x12", "5x4"])
def test_flow_resample(ctx, resample_refs, shape):
    sw, sh = shape
    fu, fv, ref = resample_refs[shape]
    u, v = ctx.jet_flow_resample(fu, fv, sfa.jet_source(sw, sh, rescale=2.0))
    for k in range(2):
        same(ref[k][0], u[k], ("u", k))
        same(ref[k][1], v[k], ("v", k))


# ======================================================================================================
# hypothesis energies
# ======================================================================================================
EN_JETS = 4
REGIMES = {"equal": 4, "up": 8, "down": 2}            # r_Jets against Jets = 4: adaptFPS copies, subsamples, interpolates (through a float)
PENALTIES = {"quadratic": 0, "modified_l1": 1, "lorentzian": 2}
EN_CLASSES = ("unknown_break", "pos_fail_nan", "pos_fail_magnitude", "tgt_fail_nan", "tgt_fail_magnitude", "frame_zero_tap")
EN_FLOW_CLASSES = ("flow_zero_tap",)


def energy_skip(shape):
    return 1 if shape == (W, H) else 0


def energy_case(oracle, shape, rJ, with_flows):
    """frames and flows with ladder and sprinkle; smooth accumulated flows of a few pixels with the fp64 specials sprinkled in, at tracked == r_Jets pixels
    and elsewhere"""
    w, h = shape
    J, skip = EN_JETS, energy_skip(shape)
    gw, gh, _, _ = grid(w, h, skip)
    rng = np.random.default_rng(100 + rJ)
    tex = rng.standard_normal((J + 1, 3, h, w)).astype(F32)
    with np.errstate(all="ignore"):
        frames = tex * vr.ladder_scale(w, h, vr.FULL["exps"], band=bands(w)[0])
    vr.sprinkle(frames, 70)
    base_u, base_v = rng.uniform(-2, 2, (gh, gw)), rng.uniform(-2, 2, (gh, gw))
    au = np.stack([(f + 1) * base_u * J / rJ + rng.standard_normal((gh, gw)) * 0.3 for f in range(rJ)])
    av = np.stack([(f + 1) * base_v * J / rJ + rng.standard_normal((gh, gw)) * 0.3 for f in range(rJ)])
    vr.specials64(au, 71)
    vr.specials64(av, 72)
    tracked = np.where(rng.random((gh, gw)) < 0.8, rJ, rng.integers(0, rJ, (gh, gw))).astype(np.int32)
    flows = vr.traj_flows(J, h, w, 4, band=bands(w)[0], sprinkle_seed=73) if with_flows else None
    incr, start = skip + 1, int(F32(0.5) * F32(skip))
    for gx in (3, 35, 66):                                                      # a hypothesis that stays on its integer pixel, +Inf on the pixel to its right:
        if gx < gw and gx * incr + start + 1 < w:                               # the tap of weight zero of every frame and flow lookup, in three segments
            au[:, 2, gx], av[:, 2, gx], tracked[2, gx] = 0.0, 0.0, rJ
            frames[1:, :, 2 * incr + start, gx * incr + start + 1] = np.inf
            if with_flows:
                flows[0][:, 2 * incr + start, gx * incr + start + 1] = np.inf
    with np.errstate(all="ignore"):
        dx, dy = derivatives(oracle, np.ascontiguousarray(frames), w)
    return frames, dx, dy, au, av, tracked, flows


@pytest.fixture(scope="module")
def energy_refs(oracle):
    """restatement results shared by the CPU and the GPU tests: (case, energy, bits, terms)"""
    cache = {}

    def get(shape, regime, penalty, with_flows):
        key = (shape, regime, penalty, with_flows)
        if key not in cache:
            case = energy_case(oracle, shape, REGIMES[regime], with_flows)
            frames, dx, dy, au, av, tracked, flows = case
            p = EnergyParams(skip=energy_skip(shape), penalty=PENALTIES[penalty], acc_cv=0.25, weight=0.3)
            with np.errstate(all="ignore"):
                e, b, terms = energies(p, REGIMES[regime], au, av, tracked, frames, dx, dy, flows)
            cache[key] = (case, p, e, b, terms)
        return cache[key]
    return get


@pytest.mark.parametrize("with_flows", [True, False], ids=["flows", "no_flows"])
@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_energy_restatements_agree(energy_refs, shape, regime, with_flows):
    """vectorised == scalar; the penalties differ in one scalar function, so the ladder shape takes one penalty per regime and the small shape all three.
    A hypothesis' energy depends on no other hypothesis, so on the ladder shape the scalar form (seconds per thousand hypotheses) runs on every hypothesis
    that holds a special value and on every sixth of the others"""
    rJ = REGIMES[regime]
    for penalty in (sorted(PENALTIES) if shape == SMALL else [sorted(PENALTIES)[sorted(REGIMES).index(regime)]]):
        (frames, dx, dy, au, av, tracked, flows), p, e, b, _ = energy_refs(shape, regime, penalty, with_flows)
        gy, gx = np.indices(tracked.shape)
        special = ~(np.isfinite(au).all(0) & np.isfinite(av).all(0)) | (np.abs(au) >= 1e9).any(0) | (np.abs(av) >= 1e9).any(0) | ((au == 0).all(0) & (av == 0).all(0))
        subset = (tracked == rJ) & (special | ((gx + 5 * gy) % 6 == 0) | (shape == SMALL))
        assert (special & subset).sum() >= 3 and ((~special & subset).any() or shape == SMALL)      # 5 x 4: the sprinkle leaves no pixel plain
        with np.errstate(all="ignore"):
            e2, b2 = energies_scalar(p, rJ, au, av, np.where(subset, rJ, rJ + 1).astype(np.int32), frames, dx, dy, flows)
        same(e[subset], e2[subset], (regime, penalty, "energy"))
        same(b[subset], b2[subset], (regime, penalty, "bits"))


@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_energy_inputs_reach_every_class(energy_refs, regime):
    """the `> 1e9` break, NaN and magnitude failures of the position tests and zero-weight taps of non-finite values, each in more than one segment; the
    specials sit at hypotheses and elsewhere; the energies hold NaN, Inf (no hypothesis) and finite values of which some differ from the unsprinkled input's"""
    for with_flows in (True, False):
        (frames, dx, dy, au, av, tracked, flows), p, e, b, terms = energy_refs((W, H), regime, "modified_l1", with_flows)
        rJ = REGIMES[regime]
        skip = energy_skip((W, H))
        classes = vr.energy_classes(terms, flows, frames, H, W, skip + 1, int(F32(0.5) * F32(skip)))
        for k in EN_CLASSES + (EN_FLOW_CLASSES if with_flows else ()):
            assert len(classes.get(k, ())) > 1, (k, classes.get(k))
        special = ~np.isfinite(au).all(0) | (np.abs(au) >= 1e9).any(0)
        assert (special & (tracked == rJ)).any() and (special & (tracked != rJ)).any()
        assert np.isnan(e).any() and (e == np.inf).any() and np.isfinite(e).any()
        assert np.array_equal(e == np.inf, tracked != rJ) or np.isinf(e[tracked == rJ]).any()


@pytest.mark.parametrize("rule", ["zero_weight_tap", "unknown_break", "nan_outside"])
def test_energy_value_rules_are_pinned(energy_refs, rule):
    changed = []
    for regime in sorted(REGIMES):
        (frames, dx, dy, au, av, tracked, flows), p, e, b, _ = energy_refs((W, H), regime, "modified_l1", True)
        with np.errstate(all="ignore"):
            e2, b2, _ = energies(p, REGIMES[regime], au, av, tracked, frames, dx, dy, flows, off=(rule,))
        changed.append(differs((e, b), (e2, b2)))
    assert any(changed), rule


@gpu
@pytest.mark.parametrize("with_flows", [True, False], ids=["flows", "no_flows"])
@pytest.mark.parametrize("penalty", sorted(PENALTIES))
@pytest.mark.parametrize("regime", sorted(REGIMES))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_hypothesis_energies(ctx, energy_refs, shape, regime, penalty, with_flows):
    """every penalty exact, the Lorentzian's device log included; the adapted flows as well"""
    w, h = shape
    (frames, dx, dy, au, av, tracked, flows), p, e, b, terms = energy_refs(shape, regime, penalty, with_flows)
    fl = [strided(a, w, pad=np.nan)[None] for a in flows] if flows is not None else None
    ge, gb, gu, gv = ctx.hypothesis_energies(p.to_c(sfa), REGIMES[regime], au[None], av[None], tracked[None], strided(frames, w, pad=np.nan)[None], w, fl, adapted=True)
    same(b, gb[0], "occ_bits")
    same(e, ge[0], "energy")
    for name, got, ref in (("U", gu[0], terms["U"]), ("V", gv[0], terms["V"])):
        full = np.zeros(got.shape)                                              # 0 where there is no hypothesis
        full[:, terms["hy"], terms["hx"]] = ref
        same(full, got, name)


# ======================================================================================================
# fill
# ======================================================================================================
def fill_case(shape):
    w, h = shape
    rng = np.random.default_rng(5)
    J = 3
    au, av = rng.uniform(-3, 3, (J, h, w)), rng.uniform(-3, 3, (J, h, w))
    vr.specials64(au, 80)
    vr.specials64(av, 81)
    au[0, 0, 0], av[0, 0, 0], au[1, -1, -1] = 1e39, -1e39, 1.7e308              # beyond FLT_MAX: the float conversion of the sum
    mask = (rng.random((h, w)) < 0.8).astype(np.uint8)
    mask[0, 0] = mask[-1, -1] = 1
    with np.errstate(all="ignore"):
        planes = [rng.uniform(-3, 3, (J, h, w)).astype(F32) * vr.ladder_scale(w, h, [-140, -20, 0, 60, 126, 127], band=bands(w)[0]) for _ in range(2)]
    for k, pl in enumerate(planes):
        vr.sprinkle(pl, 82 + k)
    return au, av, mask, planes


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fill_inputs_reach_overflow_and_specials(shape):
    w, h = shape
    au, av, mask, planes = fill_case(shape)
    xs, ys = np.arange(w, dtype=np.int32), np.arange(h, dtype=np.int32)
    with np.errstate(all="ignore"):
        m = fill_ref.fill_matches(au, av, mask, xs, ys, 3)
        tu, tv, _ = fill_ref.fill_trajectories(planes[0], planes[1], w, 3)
    assert mixes(m[0][:, 2:]) and vr.float_overflow(au[:, mask == 1] / 3).any()
    assert mixes(tu) and vr.is_subnormal(planes[0]).any()
    big = np.isfinite(planes[0]) & np.isinf(tu)                                 # float * int overflow: finite plane, infinite product
    assert big.any() and (len(set((np.nonzero(big.any((0, 1)))[0] // 64).tolist())) > 1 or w < 64)


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fill(ctx, shape):
    w, h = shape
    au, av, mask, planes = fill_case(shape)
    xs, ys = np.arange(w, dtype=np.int32), np.arange(h, dtype=np.int32)
    for divisor in (2, 3):
        with np.errstate(all="ignore"):
            ref = fill_ref.fill_matches(au, av, mask, xs, ys, divisor)
        got, count = ctx.fill_matches(au[None], av[None], mask[None], xs, ys, divisor)
        assert count[0] == len(ref[0])
        for j in range(au.shape[0]):
            same(ref[j], got[0, j, :count[0]], ("matches", divisor, j))
            assert np.isnan(got[0, j, count[0]:]).all()
    for scale in (2, 3):
        with np.errstate(all="ignore"):
            ru, rv, rt = fill_ref.fill_trajectories(planes[0], planes[1], w, scale)
        gu, gv, gt = ctx.fill_trajectories(strided(planes[0], w, pad=np.nan)[None], strided(planes[1], w, pad=np.nan)[None], w, scale)
        same(ru, gu[0], ("u", scale))
        same(rv, gv[0], ("v", scale))
        same(rt, gt[0], ("tracked", scale))


# ======================================================================================================
# fusion
# ======================================================================================================
FUSE_J = 4
FUSE_ITERS = 3
FUSE_KEYS = ("slot", "u", "v", "occ", "energy", "bound", "iters")


def fuse_skip(shape):
    return 1 if shape == (W, H) else 0


def fuse_case(shape, K, kind, seed=0):
    """one segment's (U, V, energy, occ_bits, weight).
    finite: energies are fp32 values from subnormal to FLT_MAX and +-0 (+Inf: no hypothesis), with exact ties of the float score; |U|, |V| from 2^-20 to
    exactly 1e10 (UNKNOWN_FLOW, the fill-in's trajectories), near-duplicates for the NMS; weights from 1 down to subnormal and 0.
    overflow: the same plus energies and flows beyond FLT_MAX: the float score and the float distance are infinite.
    poisoned: the same plus NaN / -Inf energies and NaN / Inf flows (value_ranges.F64_SPECIALS)"""
    w, h = shape
    J, skip = FUSE_J, fuse_skip(shape)
    gw, gh, incr, start = grid(w, h, skip)
    rng = np.random.default_rng(1000 * K + seed)
    band = bands(w)[0] if skip == 0 else max(bands(w)[0] // 2, 1)               # bands of eight image columns
    col = (np.arange(gw) // band)
    with np.errstate(all="ignore"):
        emag = np.exp2(np.array([-149.0, -126, -20, 0, 20, 100, 127]))[(col + np.arange(K)[:, None, None]) % 7]
        energy = (rng.uniform(0.5, 1.9, (K, gh, gw)) * rng.choice([-1.0, 1.0], (K, gh, gw)) * emag).astype(F32).astype(np.float64)
    vr.sprinkle(energy, seed + 1, values=vr.FINITE_SPECIALS.astype(np.float64))
    energy[rng.random((K, gh, gw)) < 0.2] = np.inf
    energy[:, rng.random((gh, gw)) < 0.05] = np.inf                             # pixels without any hypothesis
    tie = rng.random((gh, gw)) < 0.25
    energy[K - 1][tie] = energy[0][tie]                                         # exact ties: the lower slot first
    base_u, base_v = rng.uniform(-2, 2, (gh, gw)), rng.uniform(-2, 2, (gh, gw))
    U, V = np.zeros((K, J, gh, gw)), np.zeros((K, J, gh, gw))
    fmag = np.array([2.0 ** -20, 1.0, 1.0, 2.0 ** 10, 1.0, 2.0 ** 30])[(col + np.arange(K)[:, None, None]) % 6]
    for k in range(K):
        du, dv = rng.uniform(-1, 1, (gh, gw)), rng.uniform(-1, 1, (gh, gw))
        dup = (rng.random((gh, gw)) < 0.3) & (k > 0)                            # within traj_sim_thres of slot 0: the NMS meets it
        for j in range(J):
            U[k, j] = np.where(dup, U[0, j] + 1e-3, (j + 1) * (base_u + du) * fmag[k])
            V[k, j] = np.where(dup, V[0, j], (j + 1) * (base_v + dv) * fmag[k])
    unknown = rng.random((K, gh, gw)) < 0.1
    U[np.broadcast_to(unknown[:, None], U.shape)] = fr.UNKNOWN_FLOW
    V[np.broadcast_to(unknown[:, None], V.shape)] = fr.UNKNOWN_FLOW
    occ = rng.integers(0, 1 << (J + 2), (K, gh, gw)).astype(np.uint64)
    wmag = np.array([1.0, 2.0 ** -20, 2.0 ** -140, 0.0], F32)[(np.arange(w) // bands(w)[0]) % 4]
    weight = (rng.uniform(0.1, 0.5, (h, w)).astype(F32) * wmag).astype(F32)
    if kind in ("overflow", "poisoned"):
        vr.sprinkle(energy, seed + 2, values=np.array([1e39, -1e39, 2e39, 1.7e308]))
        vr.sprinkle(U.reshape(K * J, gh, gw), seed + 3, values=np.array([1e39, -1e200, 1.7e308]))
    if kind == "poisoned":
        vr.specials64(energy, seed + 4)
        energy[:, 1, 2], energy[K - 1, 1, 2] = np.inf, np.nan                   # NaN the only energy that is not +Inf: no hypothesis at all
        energy[0, 1, 3], energy[1, 1, 3] = np.nan, 1.0                          # NaN in the first slot, a finite one behind it
        vr.specials64(U.reshape(K * J, gh, gw), seed + 5)
        vr.specials64(V.reshape(K * J, gh, gw), seed + 6)
    return U, V, energy, occ, weight


def fuse_params(shape, method):
    return fr.Params(skip=fuse_skip(shape), traj_sim_method=method, trws_max_iter=FUSE_ITERS)


@pytest.fixture(scope="module")
def fuse_refs():
    cache = {}

    def get(shape, K, kind, method, seed=0):
        key = (shape, K, kind, method, seed)
        if key not in cache:
            case = fuse_case(shape, K, kind, seed)
            trace = []
            with np.errstate(all="ignore"):
                ref = fr.fuse(*case, fuse_params(shape, method), shape[0], trace=trace)
            cache[key] = (case, ref, trace)
        return cache[key]
    return get


FUSE_KINDS = ("finite", "overflow", "poisoned")


@pytest.mark.parametrize("kind", FUSE_KINDS)
@pytest.mark.parametrize("method", [0, 1], ids=["adj", "acc"])
@pytest.mark.parametrize("K", [4, 16])
def test_fuse_restatements_agree(fuse_refs, K, method, kind):
    """TRW-S node by node == TRW-S by anti-diagonals on every output; K = 16 on the small shape (the scalar form's time), K = 4 on both"""
    for shape in (SHAPES if K == 4 else [SMALL]):
        case, ref, _ = fuse_refs(shape, K, kind, method)
        with np.errstate(all="ignore"):
            b = fr.fuse(*case, fuse_params(shape, method), shape[0], solver=fr.trws_scalar)
        for k in FUSE_KEYS:
            same(np.asarray(ref[k]), np.asarray(b[k]), (shape, k))


@pytest.mark.parametrize("method", [0, 1], ids=["adj", "acc"])
@pytest.mark.parametrize("K", [4, 16])
def test_fuse_inputs_reach_every_class(fuse_refs, K, method):
    """finite: every magnitude of energy, ties of the float score, zero weights, UNKNOWN_FLOW, NMS discards, finite outputs.  overflow: infinite float scores and
    distances in more than one segment.  poisoned: NaN energies at present slots and NaN flows, and the fusion's outputs hold NaN"""
    skip = fuse_skip((W, H))
    (U, V, energy, occ, weight), ref, trace = fuse_refs((W, H), K, "finite", method)
    present = energy < np.inf
    e = energy[present]
    assert vr.is_subnormal(e).any() and (np.abs(e) == vr.FLT_MAX).any() and (e == 0).any() and np.signbit(e[e == 0]).any() and not vr.float_overflow(e).any()
    assert np.array_equal(e.astype(F32).astype(np.float64), e)                  # fp32 values
    assert ((energy[0] == energy[K - 1]) & present[0]).sum() > 10 and (weight == 0).any() and (U == fr.UNKNOWN_FLOW).any()
    assert any(len(l) < int(present[:, i // U.shape[3], i % U.shape[3]].sum()) for i, l in enumerate(ref["lab"]))        # the NMS discarded something
    assert np.isfinite(ref["energy"]) and np.isfinite(ref["bound"]) and (ref["slot"] >= 0).any() and (ref["slot"] < 0).any()
    assert not any(vr.float_overflow(d).any() for d in trace)
    (U, V, energy, occ, weight), ref, trace = fuse_refs((W, H), K, "overflow", method)
    col = (np.arange(U.shape[3]) * (skip + 1))[None, None, :]
    assert len(vr.segments_reached(vr.float_overflow(energy), col)) > 1
    assert sum(int(vr.float_overflow(d).sum()) for d in trace) > 1
    (U, V, energy, occ, weight), ref, trace = fuse_refs((W, H), K, "poisoned", method)
    assert len(vr.segments_reached(np.isnan(energy), col)) > 1 and np.isnan(U).any() and np.isnan(V).any() and (energy == -np.inf).any()
    lab_slots = [(k, i) for i, l in enumerate(ref["lab"]) for k in l]
    assert not any(np.isnan(energy[k].reshape(-1)[i]) for k, i in lab_slots)    # the rule: a NaN energy is absent
    assert np.isnan(ref["u"]).any() or np.isnan(ref["energy"])


def test_nan_energy_rule_is_pinned(fuse_refs):
    """with NaN energies present again (the rule before), the restatement's result on the poisoned segment changes: the GPU comparison pins present() of fuse.hip"""
    changed = []
    for K in (4, 16):
        case, ref, _ = fuse_refs(SMALL, K, "poisoned", 1)
        assert ref["slot"][1, 2] == -1 and ref["slot"][1, 3] != 0
        with np.errstate(all="ignore"):
            old = fr.fuse(*case, fuse_params(SMALL, 1), SMALL[0], off=("nan_energy_absent",))
        changed.append(differs([np.asarray(ref[k]) for k in FUSE_KEYS], [np.asarray(old[k]) for k in FUSE_KEYS]))
    assert any(changed)


def fuse_gpu(ctx, shape, method, cases):
    w, h = shape
    p = sfa.fuse_params(skip=fuse_skip(shape), traj_sim_method=method, trws_max_iter=FUSE_ITERS)
    return ctx.fuse_hypotheses(p, *[np.stack([c[i] for c in cases]) for i in range(5)], w, h)


def fuse_same(ref, got, s, what):
    for k in FUSE_KEYS:
        r = np.asarray(ref[k])
        same(r.astype(got[k].dtype) if r.dtype.kind in "iu" else r, got[k][s], (what, k))


@gpu
@pytest.mark.parametrize("kind", ["finite", "overflow"])
@pytest.mark.parametrize("method", [0, 1], ids=["adj", "acc"])
@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fuse(ctx, fuse_refs, shape, K, method, kind):
    """slot, flow, occlusion, segment energy, bound and iterations are exactly the restatement's"""
    case, ref, _ = fuse_refs(shape, K, kind, method)
    got = fuse_gpu(ctx, shape, method, [case])
    assert got["iters"][0] <= FUSE_ITERS
    fuse_same(ref, got, 0, kind)


@gpu
@pytest.mark.parametrize("method", [0, 1], ids=["adj", "acc"])
@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_fuse_contains_a_poisoned_segment(ctx, fuse_refs, shape, K, method):
    """three segments, the middle one with NaN energies and flows: the outer two equal their single-segment calls and the restatement; the poisoned one holds
    only -1 or present hypotheses, and with the NaN-energy rule equals the restatement exactly"""
    cases = [fuse_refs(shape, K, "finite", method, seed=10), fuse_refs(shape, K, "poisoned", method), fuse_refs(shape, K, "finite", method, seed=20)]
    got = fuse_gpu(ctx, shape, method, [c[0] for c in cases])
    for s in (0, 2):
        one = fuse_gpu(ctx, shape, method, [cases[s][0]])
        for k in FUSE_KEYS:
            same(one[k][0], got[k][s], ("single", s, k))
        fuse_same(cases[s][1], got, s, ("clean", s))
    energy = cases[1][0][2]
    slot = got["slot"][1]
    assert ((slot >= -1) & (slot < K)).all()
    chosen = np.take_along_axis(energy, np.maximum(slot, 0)[None], 0)[0]
    assert (chosen[slot >= 0] < np.inf).all()                                   # present: neither +Inf nor NaN
    assert np.array_equal(slot < 0, ~(energy < np.inf).any(0))
    fuse_same(cases[1][1], got, 1, "poisoned")


# ======================================================================================================
# the resident job
# ======================================================================================================
JOB_RATE, JOB_SEGMENT = 1, 1


def job_segments():
    """T1's first three segments, and segment 1 with the sprinkle in the flows of rate 1 (rate acc_min_fps: accumulated, and read by the energies of rates 1 and 2)"""
    case = ti.T1
    clean = [ti.segment(case, seed) for seed in case.seeds[:3]]
    dirty = dict(clean[JOB_SEGMENT])
    sw = case.source(JOB_RATE)[0]
    flows = [a.copy() for a in dirty["flows"][JOB_RATE]]
    for k, a in enumerate(flows):
        vr.sprinkle(a, 90 + k, sw)
    dirty["flows"] = list(dirty["flows"])
    dirty["flows"][JOB_RATE] = tuple(flows)
    return case, clean, dirty


@pytest.fixture(scope="module")
def job_refs(oracle):
    case, clean, dirty = job_segments()
    with np.errstate(all="ignore"):
        want = [ti.restate(oracle, case, seg) for seg in (clean[0], dirty, clean[2])]
    return case, clean, dirty, want


def test_job_sprinkle_reaches_the_rates_and_the_fusion(job_refs):
    case, clean, dirty, want = job_refs
    assert np.isnan(dirty["flows"][JOB_RATE][0][..., :case.w]).any() and not np.isnan(clean[JOB_SEGMENT]["flows"][JOB_RATE][0][..., :case.w]).any()
    w1 = want[1]
    assert np.isnan(w1["rate"][JOB_RATE]["u"]).any() or np.isinf(w1["rate"][JOB_RATE]["u"]).any()
    assert any(np.isnan(w1["rate"][r]["energy"]).any() for r in range(case.K))
    assert (w1["fused"]["slot"] >= 0).any()


def job_download(job, case, s):
    out = {}
    for r in range(case.K):
        for k, v in job.download_rate(s, r).items():
            out["rate%d_%s" % (r, k)] = np.asarray(v)
    for k, v in job.download_fused(s).items():
        out["fused_" + k] = np.asarray(v)
    return out


@gpu
def test_track_job_with_the_sprinkle_in_one_segment(ctx, job_refs):
    case, clean, dirty, want = job_refs
    job = sfa.TrackJob(ctx, case.params())
    runs = []
    for group in ((clean[0], dirty, clean[2]), clean):
        for s, seg in enumerate(group):
            for r in range(case.K):
                job.upload_flows(s, r, *seg["flows"][r])
            job.upload_frames(s, seg["frames"])
        job.run(3)
        runs.append([job_download(job, case, s) for s in range(3)])
    job.close()
    for s in range(3):
        got, ref = runs[0][s], want[s]
        best, occluded = ti.best_and_occluded(ref["E"], np.stack([q["occ_bits"] for q in ref["rate"]]))
        for r in range(case.K):
            for k in ("u", "v", "tracked", "energy", "occ_bits"):
                same(ref["rate"][r][k], got["rate%d_%s" % (r, k)], (s, r, k))
            same(occluded[r], got["rate%d_occluded" % r], (s, r, "occluded"))
        for k in ("slot", "u", "v", "occ"):
            same(ref["fused"][k], got["fused_" + k], (s, k))
        same(best, got["fused_best"], (s, "best"))
        same(np.float64(ref["fused"]["energy"]), np.float64(got["fused_energy"]), (s, "energy"))
        same(np.float64(ref["fused"]["bound"]), np.float64(got["fused_bound"]), (s, "bound"))
        assert int(got["fused_iters"]) == int(ref["fused"]["iters"]), s
    for s in (0, 2):                                                            # untouched by the neighbour's NaN
        for k in runs[0][s]:
            same(runs[1][s][k], runs[0][s][k], ("untouched", s, k))
    assert differs([runs[0][1][k] for k in sorted(runs[0][1])], [runs[1][1][k] for k in sorted(runs[1][1])])
