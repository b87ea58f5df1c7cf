"""sfa_fill_samples, sfa_fill_matches and sfa_fill_trajectories (slowflow_amd/csrc/fill.hip): the sample loop, the matches and the trajectory scaling of
dense_tracking's EpicFlow fill-in (dense_tracking.cpp:1274-1310) against their plain restatements (tests/fill_ref.py).  Floats and doubles are compared by
their bit patterns; nothing here is approximate."""
import ctypes as C
import re

import numpy as np
import pytest

import fill_ref

SFA_ERR_ARG = -1
W, H = 70, 45                                    # with epic_skip 2: 35 x 22 = 770 samples, four blocks of the compaction


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- CPU: the sample loop (host only) ------------------------------------------------------------------------------------------------------------
def test_fill_samples_is_the_references_loop_with_its_float_step():
    import slowflow_amd as sfa
    literal = {(1, 5): [0, 1, 2, 3, 4],
               (2, 8): [1, 3, 5, 7], (2, 9): [1, 3, 5, 7],                 # the last sample is the last column, and is not
               (2.5, 8): [1, 3, 5, 7], (2.5, 9): [1, 3, 5, 7],              # 1 + 2.5 = 3.5 -> 3: the int truncates after every addition, the step is 2
               (3, 8): [1, 4, 7], (3, 9): [1, 4, 7], (3, 1): [], (3, 2): [1]}
    for (skip, extent), want in literal.items():
        got = sfa.fill_samples(extent, skip)
        assert got.dtype == np.int32 and got.tolist() == want, (skip, extent, got)
    for skip in (1, 2, 2.5, 3, 3.75, 7.5):
        for extent in (1, 2, 7, 8, 9, 70, 131, 1024):
            assert np.array_equal(sfa.fill_samples(extent, skip), fill_ref.fill_samples(extent, skip)), (skip, extent)


def test_fill_samples_refusals():
    import slowflow_amd as sfa
    # beyond 2^24 the fp32 sum x + epic_skip no longer advances x: such an extent is refused, not looped over
    for extent, skip, word in ((0, 2, "extent"), (-3, 2, "extent"), (2 ** 23 + 1, 1, "extent"), (2 ** 29, 1, "extent"), (8, 0.5, "epic_skip"), (8, 0, "epic_skip"), (8, float("nan"), "epic_skip"),
                               (8, -2, "epic_skip")):
        with pytest.raises(sfa.SlowflowError) as e:
            sfa.fill_samples(extent, skip)
        assert word in str(e.value), (extent, skip, str(e.value))
    L = sfa.lib()
    L.sfa_fill_samples.argtypes = [C.c_int, C.c_float, C.c_void_p, C.POINTER(C.c_int)]
    assert L.sfa_fill_samples(8, 2.0, None, None) == SFA_ERR_ARG and "count" in L.sfa_last_error(None).decode()
    c = C.c_int()
    assert L.sfa_fill_samples(9, 2.0, None, C.byref(c)) == 0 and c.value == 4                   # out NULL: the count alone
    assert L.sfa_fill_samples(2 ** 23, 1.0, None, C.byref(c)) == 0 and c.value == 2 ** 23       # the largest extent, the smallest step: every column


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene():
    """three maps: a random mask, a mask with no 1 on any sample, all ones; five steps of trajectories"""
    rng = np.random.default_rng(5)
    xs, ys = fill_ref.fill_samples(W, 2), fill_ref.fill_samples(H, 2)
    mask = np.zeros((3, H, W), np.uint8)
    mask[0] = rng.random((H, W)) < 0.4
    mask[1, ::2, ::2] = 1                        # even rows and columns: the samples of epic_skip 2 are the odd ones
    mask[2] = 1
    acc_u, acc_v = rng.normal(0, 9, (3, 5, H, W)), rng.normal(0, 9, (3, 5, H, W))
    for a in (mask, acc_u, acc_v):
        a.setflags(write=False)
    return dict(xs=xs, ys=ys, mask=mask, acc_u=acc_u, acc_v=acc_v)


@pytest.mark.gpu
@pytest.mark.parametrize("J", (1, 5))
@pytest.mark.parametrize("divisor", (1, 3))
def test_matches_equal_the_match_loop(ctx, scene, J, divisor):
    xs, ys, mask = scene["xs"], scene["ys"], scene["mask"]
    au, av = scene["acc_u"][:, :J], scene["acc_v"][:, :J]
    got, count = ctx.fill_matches(au, av, mask, xs, ys, divisor)
    assert got.shape == (3, J, len(xs) * len(ys), 4) and got.dtype == np.float32
    for i in range(3):
        want = fill_ref.fill_matches(au[i], av[i], mask[i], xs, ys, divisor)
        assert int(count[i]) == len(want[0])
        for j in range(J):
            assert np.array_equal(bits(got[i, j, :count[i]]), bits(want[j])), (i, j)
            assert np.isnan(got[i, j, count[i]:]).all(), (i, j)                                  # nothing is written behind the count
    assert 0 < count[0] < len(xs) * len(ys) and count[1] == 0 and count[2] == len(xs) * len(ys)


@pytest.mark.gpu
def test_the_sum_and_the_division_are_fp64(ctx):
    """x = 1, u = 2^-24 + 2^-50: in fp64 1 + u lies above the middle of two floats and rounds up to 1 + 2^-23; with u rounded to a float first (2^-24) the
    fp32 sum is a tie and rounds to 1.  With divisor 3 the same u times 3: the fp64 quotient is exact again"""
    u = 2.0 ** -24 + 2.0 ** -50
    as_fp64 = np.float32(np.float64(1) + np.float64(u))
    as_fp32 = np.float32(1) + np.float32(u)
    assert as_fp64 == np.float32(1 + 2.0 ** -23) and as_fp32 == np.float32(1) and as_fp64 != as_fp32      # the case tells the two forms apart
    xs, ys = np.array([1], np.int32), np.array([1], np.int32)
    mask = np.ones((1, 3, 3), np.uint8)
    for divisor in (1, 3):
        acc = np.full((1, 1, 3, 3), u * divisor, np.float64)
        assert acc[0, 0, 1, 1] / divisor == u
        got, count = ctx.fill_matches(acc, acc, mask, xs, ys, divisor)
        assert count[0] == 1
        assert np.array_equal(bits(got[0, 0, 0]), bits(np.array([1, 1, as_fp64, as_fp64], np.float32))), (divisor, got[0, 0, 0])
        assert got[0, 0, 0, 2] != as_fp32


@pytest.mark.gpu
@pytest.mark.parametrize("scale", (1, 3))
def test_trajectories_are_the_scaled_planes(ctx, scale):
    rng = np.random.default_rng(11)
    n, J, stride = 2, 3, W + 2
    fx, fy = (rng.normal(0, 20, (n, J, H, stride)).astype(np.float32) for _ in range(2))
    fx[0, 1, 3, 4], fx[0, 1, 3, 5], fx[1, 2, 0, 0], fy[1, 0, H - 1, W - 1] = np.nan, np.inf, -np.inf, np.nan
    fx[0, 0, 7, 7], fy[0, 0, 7, 7] = np.float32(3e38), np.float32(1e-45)                          # overflows with scale 3; a subnormal
    fx[:, :, :, W:], fy[:, :, :, W:] = 12345.0, -54321.0                                           # the padding columns are not read
    au, av, tr = ctx.fill_trajectories(fx, fy, W, scale)
    assert au.shape == (n, J, H, W) and au.dtype == np.float64 and tr.shape == (n, H, W) and tr.dtype == np.int32
    for i in range(n):
        wu, wv, wt = fill_ref.fill_trajectories(fx[i], fy[i], W, scale)
        assert np.array_equal(bits(au[i]), bits(wu)) and np.array_equal(bits(av[i]), bits(wv)), i
        assert np.array_equal(tr[i], wt) and (tr[i] == J).all()
    assert np.isnan(au[0, 1, 3, 4]) and au[0, 1, 3, 5] == np.inf and au[1, 2, 0, 0] == -np.inf and np.isnan(av[1, 0, H - 1, W - 1])
    assert (au[0, 0, 7, 7] == np.inf) == (scale == 3)


@pytest.mark.gpu
def test_refusals_name_the_argument_and_write_nothing(ctx):
    import slowflow_amd as sfa
    L = sfa.lib()
    ptr = lambda a: a.ctypes.data
    # sfa_fill_matches
    L.sfa_fill_matches.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    w, h = 8, 4
    acc, mask = np.zeros((1, 1, h, w), np.float64), np.ones((1, h, w), np.uint8)
    xs, ys, off = np.array([1, 3], np.int32), np.array([1], np.int32), np.array([1, 8], np.int32)
    matches, count = np.full((1, 1, 2, 4), 7, np.float32), np.full(1, -5, np.int32)
    order = ("n", "J", "w", "h", "acc_u", "acc_v", "mask", "xs", "nx", "ys", "ny", "divisor", "matches", "count")
    good = dict(n=1, J=1, w=w, h=h, acc_u=ptr(acc), acc_v=ptr(acc), mask=ptr(mask), xs=ptr(xs), nx=2, ys=ptr(ys), ny=1, divisor=1, matches=ptr(matches),
                count=ptr(count))
    bad = [("n", 0), ("J", 0), ("w", 0), ("h", 0), ("nx", 0), ("ny", 0), ("nx", w + 1), ("divisor", 0), ("acc_u", None), ("acc_v", None), ("mask", None),
           ("xs", None), ("ys", None), ("matches", None), ("count", None), ("xs", ptr(off))]
    for name, value in bad:
        a = dict(good)
        a[name] = value
        rc = L.sfa_fill_matches(ctx.h, *[a[k] for k in order])
        msg = L.sfa_last_error(ctx.h).decode()
        assert rc == SFA_ERR_ARG and "sfa_fill_matches" in msg and re.search(r"\b%s\b" % name, msg), (name, value, rc, msg)
    assert (matches == 7).all() and count[0] == -5
    assert L.sfa_fill_matches(ctx.h, *[good[k] for k in order]) == 0 and count[0] == 2
    # sfa_fill_trajectories
    _f = C.POINTER(C.c_float)
    L.sfa_fill_trajectories.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.POINTER(_f), C.POINTER(_f), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    plane = np.ones((h, w), np.float32)
    planes, holes = (_f * 1)(plane.ctypes.data_as(_f)), (_f * 1)()
    au, av, tr = np.full((1, 1, h, w), 7.0), np.full((1, 1, h, w), 7.0), np.full((1, h, w), -5, np.int32)
    order = ("n", "J", "w", "h", "stride", "flow_x", "flow_y", "scale", "acc_u", "acc_v", "tracked")
    good = dict(n=1, J=1, w=w, h=h, stride=w, flow_x=planes, flow_y=planes, scale=1, acc_u=ptr(au), acc_v=ptr(av), tracked=ptr(tr))
    bad = [("n", 0), ("J", 0), ("w", 0), ("h", 0), ("stride", w - 1), ("scale", 0), ("flow_x", None), ("flow_y", None), ("acc_u", None), ("acc_v", None),
           ("tracked", None), ("flow_x", holes), ("flow_y", holes)]
    for name, value in bad:
        a = dict(good)
        a[name] = value
        rc = L.sfa_fill_trajectories(ctx.h, *[a[k] for k in order])
        msg = L.sfa_last_error(ctx.h).decode()
        assert rc == SFA_ERR_ARG and "sfa_fill_trajectories" in msg and re.search(r"\b%s\b" % name, msg), (name, value, rc, msg)
    assert (au == 7).all() and (av == 7).all() and (tr == -5).all()
    assert L.sfa_fill_trajectories(ctx.h, *[good[k] for k in order]) == 0 and (au == 1).all() and (tr == 1).all()
