"""The two-label cut on every window of a batch (sfa_grid_cut_batch: the launches optimize_occlusions of job.hip shares among the windows of a lockstep
batch) against the exact fp64 minimum cut of each window alone (oracle.grid_cut, which test_grid_cut_is_the_exact_minimum ties to exhaustive search), and
the resident job with occlusion reasoning on and more than one window against the oracle run of each window.

What the windows of a batch share -- the per-window orientation read from counts[2b], the tile flags [nb][tiles_y][tiles_x] and their hand-over to the
neighbour tile, the flags summed over all windows, the tail-batch bound on the total of active tiles, the label planes at a stride that is not the plane
stride -- is reached only here: the other cut tests stage one window.  The inputs are tests/cut_inputs.py; one test below (not marked gpu) checks on the
oracle alone that every window's minimum is unique, which the label comparisons rest on."""
import ctypes as C

import numpy as np
import pytest

import cut_inputs as ci
import oracle as orc
import slowflow_amd as sfa
from test_gpu_parity import TOL_LEVEL, c_, mk_params, normalized_frames, oracle_sensitivity, valid

gpu = pytest.mark.gpu

E_TOL = 1e-5            # |E(gpu labels) - E_min| <= E_TOL * max(1, |E_min|): test_grid_cut_reaches_the_minimum_energy's
SHARE_CAP = 0.01        # share of valid pixels labelled unlike the oracle: the same test's
SFA_ERR_ARG = -1        # include/slowflow_amd.h


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


def _aligned(a):
    o = orc.plane(*a.shape); o[...] = a
    return o


@pytest.fixture(scope="module")
def exact(oracle):
    """(w, h, alpha, kind, seed) -> (d0, d1, oracle labels, minimum energy), each window cut once by the oracle, alone"""
    memo = {}

    def get(w, h, alpha, kind, seed):
        key = (w, h, alpha, kind, seed)
        if key not in memo:
            d0, d1 = ci.window(w, h, kind, seed)
            a0, a1 = _aligned(d0), _aligned(d1)
            occ, e = oracle.grid_cut(a0, a1, alpha, w)
            for a in (a0, a1, occ):
                a.flags.writeable = False
            memo[key] = (a0, a1, occ, e)
        return memo[key]
    return get


@pytest.fixture(scope="module")
def alone(ctx, exact):
    """the same window through sfa_grid_cut, once"""
    memo = {}

    def get(w, h, alpha, kind, seed):
        key = (w, h, alpha, kind, seed)
        if key not in memo:
            d0, d1, _, _ = exact(*key)
            memo[key] = ctx.grid_cut(c_(d0), c_(d1), alpha, w)
            memo[key].flags.writeable = False
        return memo[key]
    return get


def stack(exact, w, h, alpha, wins):
    d0 = np.stack([exact(w, h, alpha, k, s)[0] for (k, s) in wins])
    d1 = np.stack([exact(w, h, alpha, k, s)[1] for (k, s) in wins])
    return c_(d0), c_(d1)


def check_energy(oracle, exact, w, h, alpha, win, occ_b, tag):
    """labels are labels, and they have the oracle's minimum energy; returns the share of pixels labelled unlike the oracle"""
    d0, d1, occ_o, e_o = exact(w, h, alpha, *win)
    assert set(np.unique(valid(occ_b, w))) <= {-1.0, 1.0}, tag
    e_g = oracle.grid_cut_energy(_aligned(occ_b), d0, d1, alpha, w)
    gap = abs(e_g - e_o) / max(1.0, abs(e_o))
    share = float((valid(occ_o, w) != valid(occ_b, w)).mean())
    print("cut_batch_stat %s kind=%s gap=%.3e share=%.5f" % (tag, win[0], gap, 0.0 if win[0] == "equal" else share))
    assert gap <= E_TOL, (tag, e_g, e_o)
    return share


def check_batch(ctx, oracle, exact, alone, w, h, alpha, wins):
    """every assertion of one batch, window by window; returns the batch's labels"""
    d0, d1 = stack(exact, w, h, alpha, wins)
    occ = ctx.grid_cut_batch(d0, d1, alpha, w)
    assert occ.shape == d0.shape
    for b, win in enumerate(wins):
        tag = "%dx%d nb=%d alpha=%g b=%d" % (w, h, len(wins), alpha, b)
        share = check_energy(oracle, exact, w, h, alpha, win, occ[b], tag)
        if win[0] != "equal":                                                    # any uniform labelling is a minimum of `equal`
            assert share < SHARE_CAP, (tag, win, share)
        assert np.array_equal(occ[b], alone(w, h, alpha, *win)), (tag, win)       # the window's schedule depends on the batch, its cut does not
    assert np.array_equal(occ, ctx.grid_cut_batch(d0, d1, alpha, w))             # deterministic
    return occ


def twins(wins):
    return [(i, j) for i, (k, s) in enumerate(wins) for j, (k2, s2) in enumerate(wins) if k2 == ci.swapped(k) and s2 == s]


# ---- the inputs can carry the assertions (CPU) -------------------------------------------------------------------------------------------------------------
def test_every_window_has_one_minimum_and_the_batches_both_orientations(oracle, exact):
    """oracle.grid_cut labels the source side -1, so on a window whose minimum is not unique the cut of (d0, d1) and the negated cut of (d1, d0) are its
    two extreme minima and differ; where they are equal the minimum is unique, and the share cap and `alone == in the batch` rest on nothing else.  Also:
    every mixed batch holds both orientations of the push-relabel, and `equal` has no node at either terminal."""
    for (w, h, alpha, kind, seed) in ci.all_windows():
        d0, d1, occ, e = exact(w, h, alpha, kind, seed)
        if kind == "equal":
            assert (valid(d0, w) == valid(d1, w)).all()
            continue
        occ_s, e_s = oracle.grid_cut(d1, d0, alpha, w)
        assert np.array_equal(valid(occ_s, w), -valid(occ, w)), (w, h, alpha, kind, seed, float((valid(occ_s, w) != -valid(occ, w)).mean()))
        assert e_s == e, (w, h, alpha, kind, seed)
    for (w, h, nb, alpha) in ci.MIXED:
        wins = ci.mixed_of(w, h, nb, alpha)
        assert all(a != b for a, b in zip(wins, wins[1:])) and twins(wins)
        flips = {ci.flip_of(*ci.window(w, h, k, s), w) for (k, s) in wins}
        assert flips == {0, 1}, (w, h, nb, alpha, flips)
        for i, j in twins(wins):
            assert abs(i - j) == 1
            assert ci.flip_of(*ci.window(w, h, *wins[i]), w) != ci.flip_of(*ci.window(w, h, *wins[j]), w)
    for (w, h, nb, alpha) in ci.MANY:
        wins = ci.many_batch(w, h, nb)
        assert {k for k, _ in wins} == set(ci.CYCLE) and all(a[0] != b[0] for a, b in zip(wins, wins[1:]))
        assert {ci.flip_of(*ci.window(w, h, k, s), w) for (k, s) in wins} == {0, 1}
    d0, d1 = ci.window(130, 35, "noise", 130 * 35)
    assert ((valid(d1, 130) > valid(d0, 130)).sum(), (valid(d1, 130) < valid(d0, 130)).sum()) == (2272, 2278)     # noise: flip = 0; blobs, stripes: 1


# ---- the cut of a batch (GPU) ------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("w,h,nb,alpha", ci.MIXED)
def test_mixed_batch_gives_every_window_its_exact_cut(ctx, oracle, exact, alone, w, h, nb, alpha):
    """(a), (b): windows of different kinds and of both orientations in one call; each has the oracle's minimum energy, the oracle's labels, and the bits
    it gets alone; a swapped window's labels are the negation of its twin's"""
    wins = ci.mixed_of(w, h, nb, alpha)
    flips = [ci.flip_of(*ci.window(w, h, k, s), w) for (k, s) in wins]
    assert set(flips) == {0, 1}, flips
    occ = check_batch(ctx, oracle, exact, alone, w, h, alpha, wins)
    assert twins(wins)
    for i, j in twins(wins):
        assert np.array_equal(valid(occ[j], w), -valid(occ[i], w)), (i, j)


@gpu
@pytest.mark.parametrize("w,h,nb,alpha", ci.MANY)
def test_many_windows_give_every_window_its_exact_cut(ctx, oracle, exact, alone, w, h, nb, alpha):
    """(c): 64 windows of 9 tiles (the tail-batch bound leaves its floor of 8 tiles), 128 windows (every word of the per-window counts), and 100"""
    check_batch(ctx, oracle, exact, alone, w, h, alpha, ci.many_batch(w, h, nb))


@gpu
def test_the_order_of_the_windows_does_not_matter(ctx, oracle, exact, alone):
    """(d): the same seven windows, reversed: each keeps its bits"""
    w, h, alpha = 130, 35, 0.5
    wins = ci.mixed_of(w, h, 7, alpha)
    fwd = ctx.grid_cut_batch(*stack(exact, w, h, alpha, wins), alpha, w)
    rev = check_batch(ctx, oracle, exact, alone, w, h, alpha, wins[::-1])
    assert np.array_equal(rev[::-1], fwd)


@gpu
def test_cross_check_schedules_in_a_batch(ctx, oracle, exact, switches):
    """(e): the grid rounds with the one-workgroup-per-window kernel of the sparse phase (blockIdx.x = window) and without it, five windows: the minimum
    energy per window either way, and the same labels (as test_grid_cut_sparse_phase_runs_the_same_rounds asserts for one window)"""
    w, h, alpha, wins = ci.SCHEDULES
    d0, d1 = stack(exact, w, h, alpha, wins)
    switches.set("SFA_CUT_DISCHARGE", "0")
    switches.set("SFA_CUT_TAIL", "1")
    occ_tail = ctx.grid_cut_batch(d0, d1, alpha, w)
    switches.unset("SFA_CUT_TAIL")
    switches.set("SFA_CUT_NO_TAIL", "1")
    occ_grid = ctx.grid_cut_batch(d0, d1, alpha, w)
    for b, win in enumerate(wins):
        check_energy(oracle, exact, w, h, alpha, win, occ_tail[b], "tail b=%d" % b)
        check_energy(oracle, exact, w, h, alpha, win, occ_grid[b], "grid b=%d" % b)
    assert np.array_equal(occ_tail, occ_grid)


@gpu
@pytest.mark.parametrize("w,h", [(130, 35), (65, 17), (5, 4)])
def test_stride_padding_is_not_read(ctx, exact, w, h):
    """(f): NaN in the columns w .. stride of every input plane"""
    alpha = 0.5
    wins = ci.mixed_of(w, h, 7, alpha)
    d0, d1 = stack(exact, w, h, alpha, wins)
    assert d0.shape[2] > w
    occ = ctx.grid_cut_batch(d0, d1, alpha, w)
    p0, p1 = d0.copy(), d1.copy()
    p0[:, :, w:] = np.nan; p1[:, :, w:] = np.nan
    assert np.array_equal(valid(ctx.grid_cut_batch(p0, p1, alpha, w), w), valid(occ, w))


@gpu
def test_refusals_name_the_argument_and_leave_the_context_working(ctx, exact, alone):
    """(g): nb outside 1 .. 128, a null plane, a negative alpha and a stride below w are refused with SFA_ERR_ARG and the argument's name, nothing is written, and
    the next valid call gives every window its lone cut"""
    w, h, alpha = 65, 17, 0.5
    wins = ci.mixed_of(w, h, 3, alpha)
    d0, d1 = stack(exact, w, h, alpha, wins)
    st = d0.shape[2]
    L = sfa.lib()
    L.sfa_grid_cut_batch.restype = C.c_int
    big = np.full((129, h, st), 7.0, np.float32)                                    # large enough for whatever a call that is not refused would touch
    occ = np.full((3, h, st), 7.0, np.float32)
    f, al = sfa.fptr, C.c_float(alpha)
    for args, name in (((f(big), f(big), f(big), 0, w, h, st, al), "nb"), ((f(big), f(big), f(big), 129, w, h, st, al), "nb"),
                       ((f(big), f(big), f(big), -1, w, h, st, al), "nb"),
                       ((None, f(d0), f(d1), 3, w, h, st, al), "occ"), ((f(occ), None, f(d1), 3, w, h, st, al), "d0"), ((f(occ), f(d0), None, 3, w, h, st, al), "d1"),
                       ((f(occ), f(d0), f(d1), 3, w, h, st, C.c_float(-0.5)), "alpha"), ((f(occ), f(d0), f(d1), 3, w, h, w - 1, al), "stride")):
        rc = L.sfa_grid_cut_batch(ctx.h, *args)
        msg = L.sfa_last_error(ctx.h).decode()
        assert rc == SFA_ERR_ARG and "sfa_grid_cut_batch" in msg and name in msg, (name, rc, msg)
        assert (occ == 7.0).all() and (big == 7.0).all()                            # nothing was written
    with pytest.raises(sfa.SlowflowError, match="alpha"):
        ctx.grid_cut(d0[0], d1[0], -1.0, w)                                         # the single-window entry point is the same body
    occ = ctx.grid_cut_batch(d0, d1, alpha, w)
    for b, win in enumerate(wins):
        assert np.array_equal(occ[b], alone(w, h, alpha, *win))


# ---- the job with occlusion reasoning on, more than one window ------------------------------------------------------------------------------------------
@gpu
def test_three_different_windows_with_occlusion_reasoning(ctx, oracle):
    """(h): as test_level_with_occlusion_reasoning, for each of three windows of one job: the labels the GPU found at every alternation are minimum-energy
    labellings of the ORACLE's costs for that window's frames (forced_gap), and the oracle under these labels ends with the GPU's labels and flow.  Window 2
    is window 0 played backwards: the other side of the reference frame is occluded.  Reaches k_occ_costs, the mask weights and the label planes of b > 0."""
    w, h, S, A = 130, 50, 3, 3
    stride = orc.stride_of(w)
    f0, af, sf = normalized_frames(oracle, w, h, 2 * S - 1, seed=4)
    f1 = normalized_frames(oracle, w, h, 2 * S - 1, seed=9)[0]
    wins = [f0, f1, f0[::-1]]
    po, ps = mk_params(oracle, S=S, rho=[1, 1], omega=[0, 2], norm_avg=af, norm_std=sf, niter_outer=2, niter_alter=A, occlusion_reasoning=1, layers=1)
    job = sfa.Job(ctx, ps, w, h, len(wins))
    job.keep_alternation_occlusions(True)
    for b, fr in enumerate(wins):
        job.upload(b, [c_(f) for f in fr])
    job.run()
    got = []
    for b in range(len(wins)):
        wxg, wyg, _ = job.download(b)
        labels = orc.aligned_zeros((A, h, stride))
        for a in range(1, A):
            labels[a] = job.download_alternation_occlusions(b, a)
            assert set(np.unique(valid(labels[a], w))) <= {-1.0, 1.0}, (b, a)
        got.append((wxg, wyg, job.download_occlusions(b), labels))
    job.close()
    for b, (fr, (wxg, wyg, occ_g, labels)) in enumerate(zip(wins, got)):
        assert np.array_equal(occ_g, labels[A - 1]), b
        oracle.force_labels(labels)
        try:
            wxf, wyf = orc.plane(h, stride), orc.plane(h, stride)
            rc, _, occ_f = oracle.compute_one_level(po, wxf, wyf, fr, w, None, want_occ=True)
            gaps = [oracle.forced_gap(a) for a in range(1, A)]
        finally:
            oracle.force_labels(None)
        assert rc == 0 and np.array_equal(valid(occ_f, w), valid(occ_g, w)), b
        assert max(abs(g) for g in gaps) <= 1e-5, (b, gaps)
        d = max(np.abs(valid(wxf, w) - valid(wxg, w)).max(), np.abs(valid(wyf, w) - valid(wyg, w)).max())
        sens = oracle_sensitivity(oracle, po, fr, w, h)
        print("cut_batch_job window %d: max|d(u,v)| %.3g, sensitivity %.3g, gaps %s, label +1 share %.4f" % (b, d, sens, gaps, (valid(occ_g, w) > 0).mean()))
        assert d <= max(TOL_LEVEL, 3 * sens), (b, d)
    differing = [(i, j) for i in range(3) for j in range(i + 1, 3) if not np.array_equal(valid(got[i][2], w), valid(got[j][2], w))]
    assert differing                                                                         # otherwise nothing is proven about which window is which


@gpu
def test_batch_with_thresholds_and_occlusions_keeps_every_window_exact(ctx, oracle):
    """(i): the nine windows of test_batch_with_thresholds_keeps_every_window_exact with the occlusion step on: the still windows stop at once and ride along
    while the others need their cut at the next alternation; flow, changes and labels of every window are those of a lone job"""
    w, h = 130, 98
    sets = [normalized_frames(oracle, w, h, 3, seed=s)[0] for s in (1, 2)]
    frames, af, sf = normalized_frames(oracle, w, h, 3, seed=3)
    still = [frames[1], frames[1], frames[1]]
    wins = [still, sets[0], sets[1], still, frames, sets[0], still, frames, sets[1]]
    which = [0, 1, 2, 0, 4, 1, 0, 4, 2]
    _, ps = mk_params(oracle, S=2, rho=[1], omega=[0], norm_avg=af, norm_std=sf, niter_alter=3, niter_outer=8, niter_inner=2, layers=2, thres_outer=2e-3,
                      thres_inner=1e-3, occlusion_reasoning=1)
    lone = {}
    for i in sorted(set(which)):
        j1 = sfa.Job(ctx, ps, w, h, 1)
        j1.upload(0, [c_(x) for x in wins[i]]); j1.run()
        lone[i] = j1.download(0) + (j1.download_occlusions(0),)
        j1.close()
    job = sfa.Job(ctx, ps, w, h, len(wins))
    for b, f in enumerate(wins):
        job.upload(b, [c_(x) for x in f])
    job.run()
    for b in range(len(wins)):
        gx, gy, chg = job.download(b)
        occ = job.download_occlusions(b)
        rx, ry, rchg, rocc = lone[which[b]]
        assert np.array_equal(gx, rx) and np.array_equal(gy, ry) and chg == rchg, b
        assert np.array_equal(occ, rocc), b
    job.close()
    assert np.abs(lone[0][0]).max() < 1e-3                                                   # the still window did stop early (and stayed put)
    assert any(set(np.unique(valid(lone[i][3], w))) == {-1.0, 1.0} for i in (1, 2, 4))       # a moving window's cut did label both sides
