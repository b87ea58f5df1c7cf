"""dense_tracking's unary hypothesis energies: sfa_hypothesis_energies (slowflow_amd/csrc/energy.hip) against tests/energy_ref.py, a float64 restatement
of adaptFPS, setOcclusions, addJC, addBCGC, addOC and their fp32 sum (reference utils/hypothesis.h:136-175, utils/hypothesis.cpp:172-215,
dense_tracking.cpp:176-365, 1219-1257).

CPU: the vectorised restatement against the scalar one, hand-worked cases, every quirk pinned by at least one case.  GPU: the kernel == the restatement
(IEEE equality on energies and occlusion bits, for all three penalties), NaN padding, batching, bad arguments."""
import ctypes as C

import numpy as np
import pytest

import slowflow_amd as sfa
from accum_ref import grid
from energy_ref import QUIRKS, Params, derivatives, energies, energies_scalar, flows_for_rate

F32 = np.float32


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
def random_case(rng, J, rJ, h, w, skip, with_flows=True, scale=2.0):
    """normalised-looking frames, trajectories that drift and partly leave the image, flows near the trajectories' steps with noise"""
    gw, gh, incr, start = grid(w, h, skip)
    frames = rng.standard_normal((J + 1, 3, h, w)).astype(F32)
    base_u = rng.uniform(-scale, scale, (gh, gw))
    base_v = rng.uniform(-scale, scale, (gh, gw))
    acc_u = np.stack([(f + 1) * base_u + rng.standard_normal((gh, gw)) * 0.3 for f in range(rJ)])
    acc_v = np.stack([(f + 1) * base_v + rng.standard_normal((gh, gw)) * 0.3 for f in range(rJ)])
    tracked = np.where(rng.random((gh, gw)) < 0.8, rJ, rng.integers(0, max(rJ, 1), (gh, gw))).astype(np.int32)
    flows = None
    if with_flows:
        su, sv = np.float32(rng.uniform(-scale, scale)), np.float32(rng.uniform(-scale, scale))
        fu = (su + rng.standard_normal((J, h, w)) * 0.5).astype(F32)
        fv = (sv + rng.standard_normal((J, h, w)) * 0.5).astype(F32)
        bu = (-fu + rng.standard_normal((J, h, w)) * rng.choice([0.1, 3.0])).astype(F32)
        bv = (-fv + rng.standard_normal((J, h, w)) * rng.choice([0.1, 3.0])).astype(F32)
        flows = (fu, fv, bu, bv)
    return frames, acc_u, acc_v, tracked, flows


def random_params(rng, skip, penalty=None):
    return Params(acc_jc=float(rng.choice([1.0, 0.7])), acc_bc=float(rng.choice([0.1, 2.5])), acc_gc=float(rng.choice([1.0, 0.3])),
                  acc_occ=float(rng.choice([500.0, 3.0])), acc_cv=float(rng.choice([0.0, 0.25])), acc_temporal_occ=float(rng.choice([10.0, 1.5])),
                  occlusion_threshold=float(rng.choice([5.0, 1.0])), occlusion_fb_threshold=float(rng.choice([5.0, 0.8])),
                  penalty=int(rng.integers(0, 3)) if penalty is None else penalty, penalty_eps=float(rng.choice([0.001, 0.05])),
                  weight=float(rng.choice([0.0, 1.0, 0.3])), skip=skip)


# ---- CPU: the two restatements agree --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(10))
def test_vectorised_restatement_equals_scalar(oracle, seed):
    rng = np.random.default_rng(seed)
    J = int(rng.integers(1, 5))
    rJ = int(rng.choice([J, 2 * J, max(J // 2, 1), J + 1]))
    h, w = int(rng.integers(4, 11)), int(rng.integers(1, 12))
    skip = int(rng.integers(0, min(3, h, w)))
    frames, au, av, tr, flows = random_case(rng, J, rJ, h, w, skip, with_flows=bool(seed % 3))
    dx, dy = derivatives(oracle, frames, w)
    p = random_params(rng, skip)
    e, b, _ = energies(p, rJ, au, av, tr, frames, dx, dy, flows)
    e2, b2 = energies_scalar(p, rJ, au, av, tr, frames, dx, dy, flows)
    assert np.array_equal(e, e2) and np.array_equal(b, b2)


# ---- CPU: hand-worked cases.  Each takes `off` (quirks switched off in the restatement) and asserts the reference's behaviour. --------------------
def zero_derivs(frames):
    return np.zeros_like(frames), np.zeros_like(frames)


def still(J, h, w):
    """zero trajectories on every pixel and zero forward / backward flows: nothing occluded"""
    z = np.zeros((J, h, w), F32)
    return (z, z, z, z)


def case_empty_flows_no_hypothesis_elsewhere(off=()):
    """J = 2, one still pixel, no flows: frames 1 and 2 occluded (occ = 0b110), OC = 2 * acc_occ + 1 change * acc_temporal_occ = 2 * 3 + 1.5, no pairs,
    JC = acc_cv * 0 = 0; the other pixel has no hypothesis and gets +Inf"""
    p = Params(acc_occ=3.0, acc_temporal_occ=1.5, skip=0, weight=0.5)
    frames = np.zeros((3, 3, 4, 2), F32)
    tr = np.array([[2, 2], [2, 2], [2, 2], [2, 1]], np.int32)
    acc = np.zeros((2, 4, 2))
    e, b, t = energies(p, 2, acc, acc, tr, frames, *zero_derivs(frames), None, off)
    assert e[3, 1] == np.inf and b[3, 1] == 0
    assert b[0, 0] == 0b110 and e[0, 0] == 7.5 + 0.5


def case_jet_consistency(off=()):
    """J = 1, flows of 1 px right, the trajectory 1.5 px right: JC = acc_jc * 0.5 * phi((1.5 - 0 - 1)^2) with the quadratic penalty = 0.125,
    CV = sqrt((2 * 1.5)^2) = 3 times acc_cv 0.5"""
    h = w = 6
    p = Params(penalty=0, acc_cv=0.5, occlusion_threshold=1.0, skip=0, acc_bc=0.0, acc_gc=0.0, acc_occ=0.0, acc_temporal_occ=0.0)
    fu = np.ones((1, h, w), F32)
    z = np.zeros((1, h, w), F32)
    frames = np.zeros((2, 3, h, w), F32)
    acc_u, acc_v = np.full((1, h, w), 1.5), np.zeros((1, h, w))
    e, b, t = energies(p, 1, acc_u, acc_v, np.ones((h, w), np.int32), frames, *zero_derivs(frames), (fu, z, -fu, z), off)
    assert b[1, 1] == 0 and t["jc"][np.flatnonzero((t["hy"] == 1) & (t["hx"] == 1))[0]] == F32(0.125 + 1.5)


def case_cv_skipped_by_continue(off=()):
    """J = 2, the pixel at x = 1 of a 3-wide image: its step 1 target (x = 3) leaves the image, so occ = 0b100.  Step 0 adds sqrt((2 u0 - u1)^2) =
    |2 - 2| = 0; step 1 is occluded and its `continue` skips the constant-velocity term |2 u1 - u0| = 3 as well: CV = 0"""
    h, w = 4, 3
    p = Params(penalty=0, acc_cv=1.0, acc_jc=0.0, skip=0, acc_bc=0.0, acc_gc=0.0, acc_occ=0.0, acc_temporal_occ=0.0)
    fu = np.ones((2, h, w), F32)
    z = np.zeros((2, h, w), F32)
    frames = np.zeros((3, 3, h, w), F32)
    acc_u, acc_v = np.stack([np.full((h, w), 1.0), np.full((h, w), 2.0)]), np.zeros((2, h, w))
    e, b, t = energies(p, 2, acc_u, acc_v, np.full((h, w), 2, np.int32), frames, *zero_derivs(frames), (fu, z, -fu, z), off)
    k = np.flatnonzero((t["hy"] == 0) & (t["hx"] == 1))[0]          # x = 1: frame 1 at 2, frame 2 at 3 (outside): occ = 0b100
    assert b[0, 1] == 0b100 and t["cv"][k] == 0.0


def case_float_skip(off=()):
    """r_Jets = 3, Jets = 4: skip = 0.75f; step 2 = last_x + 0.75 (flow[1] - last_x) with last_x = (float) flow[0] = 1/3 rounded to fp32"""
    h = w = 4
    p = Params(skip=0)
    third = 1.0 / 3.0
    acc_u = np.stack([np.full((h, w), third), np.full((h, w), 2 * third), np.full((h, w), 1.0)])
    frames = np.zeros((5, 3, h, w), F32)
    e, b, t = energies(p, 3, acc_u, np.zeros_like(acc_u), np.full((h, w), 3, np.int32), frames, *zero_derivs(frames), None, off)
    lx = np.float64(F32(third))
    assert t["U"][2][0] == lx + np.float64(F32(0.75)) * (2 * third - lx)


def case_fp32_sum(off=()):
    """JC + BCGC + OC + weight in fp32: no flows, so occ = 0b10 and OC = 1; 1 + 2^-24 (a tie) rounds to 1 in fp32, in double it would survive"""
    h = w = 4
    p = Params(skip=0, acc_occ=1.0, acc_temporal_occ=0.0, weight=2.0 ** -24)
    frames = np.zeros((2, 3, h, w), F32)
    acc = np.zeros((1, h, w))
    e, b, t = energies(p, 1, acc, acc, np.ones((h, w), np.int32), frames, *zero_derivs(frames), None, off)
    assert e[0, 0] == 1.0


def case_hole(off=()):
    """w = 2, skip 1, r = 1: the grid pixel at image (0, 0) moves 0, +1, -1 px (frames at x = 0, 0, 1, 0: all inside, nothing occluded).  Its
    neighbour off_x = 1 puts frame 2 at x = 2, outside the image: visible = 3, and the pair loop runs over i < j < 3, so frame 3 (the only frame that
    differs) is never compared: e_p = 0 for that neighbour, where comparing every visible frame would give (0, 3) and (1, 3)."""
    h, w = 4, 2
    p = Params(skip=1, acc_gc=0.0, acc_occ=0.0, acc_temporal_occ=0.0)
    frames = np.zeros((4, 3, h, w), F32)
    frames[3, 2] = 1.0
    steps = np.array([0.0, 1.0, -1.0], F32)
    fu = np.stack([np.full((h, w), s, F32) for s in steps])
    z = np.zeros((3, h, w), F32)
    gw, gh, incr, start = grid(w, h, 1)
    acc_u = np.stack([np.full((gh, gw), a) for a in np.cumsum(steps.astype(np.float64))])
    e, b, t = energies(p, 3, acc_u, np.zeros_like(acc_u), np.full((gh, gw), 3, np.int32), frames, *zero_derivs(frames), (fu, z, -fu, z), off)
    k = np.flatnonzero((t["hy"] == 0) & (t["hx"] == 0))[0]
    assert b[0, 0] == 0
    ep = t["ep"][k]                                                 # neighbour k = (off_x + 1) * 3 + (off_y + 1)
    assert ep[4] > 0                                                # off_x = 0: all four frames inside, frame 3 compared
    assert ep[7] == 0.0                                             # off_x = 1, off_y = 0: the hole


def case_offx_outer(off=()):
    """skip 1 at the grid pixel on image (0, 0): four neighbours in image, summed (0,0), (0,1), (1,0), (1,1) as (off_x, off_y).  e_p(0, 0) = e_p(1, 0)
    = small and e_p(0, 1) = big, small < half an ulp of big < 2 small: off_x outer adds each small to big on its own (both lost), off_y outer adds
    the two smalls first (kept).  Frame 1 = 0, frame 0's c3 holds the per-pixel difference; acc_bc = 3 gives bcw = 1.0002 (mantissa < 4/3)."""
    h = w = 4
    p = Params(skip=1, acc_bc=3.0, acc_gc=0.0, acc_occ=0.0, acc_temporal_occ=0.0)
    frames = np.zeros((2, 3, h, w), F32)
    small = F32(0.75 * 2.0 ** -53)
    frames[0, 2, 0, 0] = small                                      # (x 0, y 0)
    frames[0, 2, 0, 1] = small                                      # (x 1, y 0)
    frames[0, 2, 1, 0] = 1.0                                        # (x 0, y 1)
    gw, gh, _, _ = grid(w, h, 1)
    acc = np.zeros((1, gh, gw))
    e, b, t = energies(p, 1, acc, acc, np.ones((gh, gw), np.int32), frames, *zero_derivs(frames), still(1, h, w), off)
    k = np.flatnonzero((t["hy"] == 0) & (t["hx"] == 0))[0]
    bcw = np.float64(p.acc_bc) * 0.3334
    assert t["bcgc_double"][k] == bcw / 4


def case_channel_order(off=()):
    """|dI c3| + |dI c2| + |dI c1| = (1 + 2^-53) + 2^-53 = 1 (each a tie to even); summed c1 first it would be 1 + 2^-52.  skip 0: one neighbour."""
    h = w = 4
    p = Params(skip=0, acc_bc=3.0, acc_gc=0.0, acc_occ=0.0, acc_temporal_occ=0.0)
    frames = np.zeros((2, 3, h, w), F32)
    frames[0, 2] = 1.0
    frames[0, 1] = F32(2.0 ** -53)
    frames[0, 0] = F32(2.0 ** -53)
    acc = np.zeros((1, h, w))
    e, b, t = energies(p, 1, acc, acc, np.ones((h, w), np.int32), frames, *zero_derivs(frames), still(1, h, w), off)
    assert t["bcgc_double"][0] == np.float64(p.acc_bc) * 0.3334 * 1.0


def case_edge_weight(off=()):
    """a trajectory ending at x = 2.5 on a 3-wide image: the weight on the last column is 0, frame 1's value is that of x = 2, not a blend with x = 0"""
    h, w = 4, 3
    p = Params(skip=0, acc_bc=3.0, acc_gc=0.0, acc_occ=0.0, acc_temporal_occ=0.0)
    frames = np.zeros((2, 3, h, w), F32)
    frames[1, 2, :, 0] = 4.0
    acc_u, acc_v = np.full((1, h, w), 0.5), np.zeros((1, h, w))
    e, b, t = energies(p, 1, acc_u, acc_v, np.ones((h, w), np.int32), frames, *zero_derivs(frames), still(1, h, w), off)
    k = np.flatnonzero((t["hy"] == 0) & (t["hx"] == 2))[0]
    # the 0.5 px step disagrees with the zero flows by 0.5 < 5: nothing occluded; frame 1 at x = 2.5 takes the value of x = 2 (0): e_p = 0
    assert b[0, 2] == 0 and t["ep"][k][0] == 0.0


def case_empty_flows_before_min_fps(off=()):
    """rate 0 comes before acc_min_fps = 1: it sees empty flows, every step t >= 1 is occluded (occ = 0b10), though the flows agree with it"""
    h = w = 4
    p = Params(skip=0)
    frames = np.zeros((2, 3, h, w), F32)
    acc = np.zeros((1, h, w))
    fl = flows_for_rate(0, 1, still(1, h, w), off)
    e, b, t = energies(p, 1, acc, acc, np.ones((h, w), np.int32), frames, *zero_derivs(frames), fl, off)
    assert b[0, 0] == 0b10
    fl = flows_for_rate(1, 1, still(1, h, w), off)
    e, b, t = energies(p, 1, acc, acc, np.ones((h, w), np.int32), frames, *zero_derivs(frames), fl, off)
    assert b[0, 0] == 0


CASES = [case_empty_flows_no_hypothesis_elsewhere, case_jet_consistency, case_cv_skipped_by_continue, case_float_skip, case_fp32_sum, case_hole,
         case_offx_outer, case_channel_order, case_edge_weight, case_empty_flows_before_min_fps]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_hand_worked_case(case):
    case()


@pytest.mark.parametrize("quirk", QUIRKS)
def test_each_quirk_is_pinned(quirk):
    """switching the quirk off makes at least one hand-worked case fail"""
    failed = []
    for case in CASES:
        try:
            case(off=(quirk,))
        except AssertionError:
            failed.append(case.__name__)
    assert failed, "no case pins the quirk %r" % quirk


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


def to_gpu_layout(frames, flows, n=1, pad=0.0):
    """(J + 1, 3, h, w) -> (n, J + 1, 3, h, stride) with the padding filled with `pad`; flows likewise (n, J, h, stride)"""
    J1, _, h, w = frames.shape
    st = sfa.stride_of(w) + (4 if pad != 0 else 0)
    fr = np.full((n, J1, 3, h, st), pad, F32)
    fr[..., :w] = frames
    fl = None
    if flows is not None:
        fl = []
        for a in flows:
            q = np.full((n, a.shape[0], h, st), pad, F32)
            q[..., :w] = a
            fl.append(q)
    return fr, fl


def gpu_energies(ctx, p, rJ, au, av, tr, frames, flows, pad=0.0):
    w = frames.shape[3]
    fr, fl = to_gpu_layout(frames, flows, pad=pad)
    e, b = ctx.hypothesis_energies(p.to_c(sfa), rJ, au[None], av[None], tr[None], fr, w, fl)
    return e[0], b[0]


def check(ctx, oracle, rng, J, rJ, h, w, skip, with_flows=True, penalty=None, scale=2.0):
    frames, au, av, tr, flows = random_case(rng, J, rJ, h, w, skip, with_flows, scale)
    dx, dy = derivatives(oracle, frames, w)
    p = random_params(rng, skip, penalty)
    e_ref, b_ref, _ = energies(p, rJ, au, av, tr, frames, dx, dy, flows)
    e, b = gpu_energies(ctx, p, rJ, au, av, tr, frames, flows)
    assert np.array_equal(b, b_ref)
    # every penalty exact, the Lorentzian included: its fp64 log on the device gave the bits of glibc's after the rounding to fp32 in every case here
    assert np.array_equal(e, e_ref)
    return e, b


SIZES = [(4, 1), (4, 3), (5, 7), (9, 13), (33, 17), (67, 130)]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,skip", [(h, w, skip) for h, w in SIZES for skip in (0, 1, 2) if skip < min(h, w)])   # skip < min(h, w): a grid exists
def test_kernel_equals_restatement(ctx, oracle, h, w, skip):
    rng = np.random.default_rng(h * 1000 + w * 10 + skip)
    for J, rJ in [(1, 1), (3, 3), (4, 8), (4, 2), (3, 5)]:
        for penalty in (0, 1, 2):
            check(ctx, oracle, rng, J, rJ, h, w, skip, with_flows=True, penalty=penalty)
        check(ctx, oracle, rng, J, rJ, h, w, skip, with_flows=False, penalty=1)


@pytest.mark.gpu
@pytest.mark.parametrize("J", [8, 16, 32])
def test_kernel_long_jets(ctx, oracle, J):
    rng = np.random.default_rng(J)
    check(ctx, oracle, rng, J, J, 24, 40, 1, with_flows=True, penalty=1, scale=0.7)
    check(ctx, oracle, rng, J, 2 * J, 24, 40, 1, with_flows=True, penalty=0, scale=0.7)
    check(ctx, oracle, rng, J, max(J // 4, 1), 24, 40, 0, with_flows=False, penalty=1, scale=0.7)


@pytest.mark.gpu
def test_kernel_lorentzian_exact(ctx, oracle):
    rng = np.random.default_rng(7)
    for J in (4, 16):
        check(ctx, oracle, rng, J, J, 20, 30, 1, with_flows=True, penalty=2)
        check(ctx, oracle, rng, J, 2 * J, 33, 17, 0, with_flows=True, penalty=2)


@pytest.mark.gpu
def test_kernel_full_size(ctx, oracle):
    """1024 x 436, skip 1, Jets 4 (the vectorised restatement over 1.1e5 hypotheses)"""
    rng = np.random.default_rng(11)
    check(ctx, oracle, rng, 4, 4, 436, 1024, 1, with_flows=True, penalty=1, scale=4.0)


@pytest.mark.gpu
def test_nan_in_the_stride_padding_changes_nothing(ctx, oracle):
    rng = np.random.default_rng(5)
    frames, au, av, tr, flows = random_case(rng, 3, 3, 13, 21, 1)
    p = random_params(rng, 1, 1)
    a = gpu_energies(ctx, p, 3, au, av, tr, frames, flows)
    b = gpu_energies(ctx, p, 3, au, av, tr, frames, flows, pad=np.nan)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 5])
def test_segments_in_one_call_equal_single_calls(ctx, n):
    rng = np.random.default_rng(n)
    J, rJ, h, w, skip = 4, 4, 11, 17, 1
    cases = [random_case(rng, J, rJ, h, w, skip) for _ in range(n)]
    p = random_params(rng, skip, 1)
    st = sfa.stride_of(w)
    fr = np.zeros((n, J + 1, 3, h, st), F32)
    fl = [np.zeros((n, J, h, st), F32) for _ in range(4)]
    for s, (frames, au, av, tr, flows) in enumerate(cases):
        fr[s, ..., :w] = frames
        for q in range(4):
            fl[q][s, ..., :w] = flows[q]
    AU = np.stack([c[1] for c in cases])
    AV = np.stack([c[2] for c in cases])
    TR = np.stack([c[3] for c in cases])
    e, b = ctx.hypothesis_energies(p.to_c(sfa), rJ, AU, AV, TR, fr, w, fl)
    for s, (frames, au, av, tr, flows) in enumerate(cases):
        e1, b1 = gpu_energies(ctx, p, rJ, au, av, tr, frames, flows)
        assert np.array_equal(e[s], e1) and np.array_equal(b[s], b1)


@pytest.mark.gpu
def test_bad_arguments_return_error_codes(ctx):
    L = sfa.lib()
    _f = C.POINTER(C.c_float)
    L.sfa_hypothesis_energies.argtypes = [C.c_void_p, C.POINTER(sfa.EnergyParams)] + [C.c_int] * 6 + [C.c_void_p] * 3 + [C.POINTER(_f)] * 5 + [
        C.c_void_p, C.c_void_p]
    p = sfa.energy_params(skip=0)
    h, w, J = 8, 8, 2
    fr = np.zeros((J + 1, 3, h, w), F32)
    fp = (_f * (J + 1))(*[sfa.fptr(fr[f]) for f in range(J + 1)])
    pl = np.zeros((J, h, w), F32)
    fl = (_f * J)(*[sfa.fptr(pl[t]) for t in range(J)])
    au = np.zeros(J * h * w)
    tr = np.zeros(h * w, np.int32)
    out = np.zeros(h * w)
    bits = np.zeros(h * w, np.uint64)

    def call(n=1, rJ=J, Jets=J, ww=w, hh=h, stride=w, frames=fp, fwd=fl, bwd=fl, params=p, outp=True):
        return L.sfa_hypothesis_energies(ctx.h, C.byref(params) if params is not None else None, n, rJ, Jets, ww, hh, stride, au.ctypes.data,
                                         au.ctypes.data, tr.ctypes.data, frames, fwd, fwd, bwd, bwd, out.ctypes.data if outp else None, bits.ctypes.data)

    assert call() == 0
    assert call(fwd=None, bwd=None) == 0
    assert call(fwd=None) == -1                                  # SFA_ERR_ARG: the four flow arrays all given or all null
    assert call(params=None) == -1
    assert call(outp=False) == -1
    assert call(frames=None) == -1
    assert call(Jets=33) == -1 and call(Jets=0) == -1 and call(rJ=0) == -1 and call(n=0) == -1
    assert call(hh=3) == -1                                      # the reference's vertical 5-tap is undefined below 4 rows
    assert call(stride=w - 1) == -1
    q = sfa.energy_params(skip=8)
    assert call(params=q) == -1                                  # an empty grid
