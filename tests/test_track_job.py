"""The resident track job (sfa_track_job, csrc/track.hip): every segment of a batched run equals, bit for bit, the staged calls on that segment alone
(accumulate_consistent(all_steps) -> hypothesis_energies(adapted=True) -> smoothness_weight -> fuse_hypotheses), a job is reusable for a second group,
and one parametrisation also equals the Python restatements directly.  The inputs are tests/track_inputs.py's; tests/test_track_inputs.py shows on the
restatements that they exercise every stage."""
import numpy as np
import pytest

import slowflow_amd as sfa
import track_inputs as ti
from energy_ref import Params as EnergyRefParams
from fuse_ref import popcount

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    """IEEE == on every element, bit patterns for the doubles"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64 or b.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return a.shape == b.shape and np.array_equal(a, b)


def staged(ctx, case, seg, use_occlusions, discard):
    """today's call sequence on one segment: {"rate": [...], "fused": Context.fuse_hypotheses' dict without the leading axis, "E", "O"}"""
    K, J, w, h = case.K, case.Jets, case.w, case.h
    U, V = np.zeros((1, K, J, case.gh, case.gw)), np.zeros((1, K, J, case.gh, case.gw))
    E, O = np.zeros((1, K, case.gh, case.gw)), np.zeros((1, K, case.gh, case.gw), np.uint64)
    rates = []
    mf = case.min_fps_idx
    assert mf not in case.scaled                                            # hypothesis_energies below passes rate mf's planes as they are
    for r in range(K):
        fu, fv, bu, bv = (a[None] for a in seg["flows"][r])
        au, av, tr = ctx.accumulate_consistent(fu, fv, bu, bv, w, ti.EPSILON, case.skip, discard, True, masks=seg["occ"][r][None] if use_occlusions else None,
                                               source=case.jet_source(r))
        ep = EnergyRefParams(skip=case.skip, weight=ti.WEIGHTS[r]).to_c(sfa)
        flows = tuple(a[None] for a in seg["flows"][mf]) if r >= mf else None
        e, o, au2, av2 = ctx.hypothesis_energies(ep, case.r_Jets[r], au, av, tr, seg["frames"][None], w, flows=flows, adapted=True)
        E[0, r], O[0, r], U[0, r], V[0, r] = e[0], o[0], au2[0], av2[0]
        rates.append(dict(u=au[0, -1], v=av[0, -1], tracked=tr[0], energy=e[0], occ_bits=o[0]))
    frame0 = np.ascontiguousarray(seg["frames"][0])
    weight = ctx.smoothness_weight(frame0, w)
    fp = sfa.fuse_params(trws_max_iter=case.trws_max_iter, trws_eps=case.trws_eps, skip=case.skip)
    f = ctx.fuse_hypotheses(fp, U, V, E, O, weight[None], w, h)
    fused = {k: f[k][0] for k in ("slot", "u", "v", "occ", "energy", "bound", "iters")}
    return dict(rate=rates, fused=fused, E=E[0], O=O[0])


def upload(job, case, s, seg, use_occlusions):
    for r in range(case.K):
        job.upload_flows(s, r, *seg["flows"][r], occ=seg["occ"][r] if use_occlusions else None)
    job.upload_frames(s, seg["frames"])


def check_segment(job, case, s, want, fused=True):
    """the job's downloads of segment s against `want` (staged()'s or restate()'s dict)"""
    best, occluded = ti.best_and_occluded(want["E"], np.stack([q["occ_bits"] for q in want["rate"]]))
    for r in range(case.K):
        got = job.download_rate(s, r)
        for k in ("u", "v", "tracked", "energy", "occ_bits"):
            assert same(got[k], want["rate"][r][k]), (s, r, k)
        assert same(got["occluded"], occluded[r]), (s, r)
        assert same(got["occluded"], popcount(got["occ_bits"]).astype(np.uint8))
    if not fused:
        return
    got = job.download_fused(s)
    for k in ("slot", "u", "v", "occ"):
        assert same(got[k], want["fused"][k]), (s, k)
    assert same(got["best"], best), s
    assert same(np.float64(got["energy"]), np.float64(want["fused"]["energy"])) and same(np.float64(got["bound"]), np.float64(want["fused"]["bound"]))
    assert got["iters"] == int(want["fused"]["iters"]), (s, got["iters"], want["fused"]["iters"])


@pytest.fixture(scope="module")
def segments():
    return {(c.name, seed): ti.segment(c, seed) for c in (ti.T1, ti.T2) for seed in c.seeds}


@pytest.mark.parametrize("use_occlusions,discard", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_t1_every_segment_of_two_runs_equals_the_staged_calls(ctx, oracle, segments, use_occlusions, discard):
    case = ti.T1
    job = sfa.TrackJob(ctx, case.params(use_occlusions=use_occlusions, discard=discard))
    iters = []
    for group in (case.seeds[:3], case.seeds[3:]):                          # run 1: ns = 3; run 2 on the same job: ns = 2 with new segments
        for s, seed in enumerate(group):
            upload(job, case, s, segments[case.name, seed], use_occlusions)
        job.run(len(group))
        for s, seed in enumerate(group):
            want = staged(ctx, case, segments[case.name, seed], use_occlusions, discard)
            check_segment(job, case, s, want)
            iters.append(int(want["fused"]["iters"]))
            if (use_occlusions, discard) == (1, 0):                         # not library code alone: both runs against the restatements directly
                check_segment(job, case, s, ti.restate(oracle, case, segments[case.name, seed], True, False))
    if (use_occlusions, discard) == (0, 1):
        assert len(set(iters)) > 1, iters                                   # what tests/test_track_inputs.py shows on the restatement
    ms = job.stage_ms()
    assert len(ms) == 8 and all(m >= 0 for m in ms) and ms[6] > 0
    job.close()


def test_t2_pitch_and_offset_with_and_without_the_fusion(ctx, oracle, segments):
    case = ti.T2
    job = sfa.TrackJob(ctx, case.params())
    plain = sfa.TrackJob(ctx, case.params(do_fuse=0))
    for s, seed in enumerate(case.seeds):
        upload(job, case, s, segments[case.name, seed], 0)
        upload(plain, case, s, segments[case.name, seed], 0)
    job.run()
    plain.run()
    for s, seed in enumerate(case.seeds):
        want = staged(ctx, case, segments[case.name, seed], 0, 1)
        check_segment(job, case, s, want)
        check_segment(plain, case, s, want, fused=False)
        check_segment(job, case, s, ti.restate(oracle, case, segments[case.name, seed]))
    with pytest.raises(sfa.SlowflowError, match="do_fuse = 0"):
        plain.download_fused(0)
    assert plain.stage_ms()[4:] == [0, 0, 0, 0]
    job.close()
    plain.close()


def refused(ctx, match, **kw):
    p = ti.T1.params()
    for k, v in kw.items():
        setattr(p, k, v)
    with pytest.raises(sfa.SlowflowError, match=match):
        sfa.TrackJob(ctx, p)


def test_refusals_name_their_argument(ctx, segments):
    refused(ctx, "n = 0", n=0)
    refused(ctx, "n = 65", n=65)
    refused(ctx, "K = 17", K=17)
    refused(ctx, "Jets = 33", Jets=33)
    refused(ctx, "h = 3", h=3)
    p = ti.T1.params()
    p.fuse.traj_sim_method = 2
    with pytest.raises(sfa.SlowflowError, match="traj_sim_method 2"):
        sfa.TrackJob(ctx, p)
    p = ti.T1.params()
    p.source[2] = sfa.jet_source(20, 12, rescale=1.5)                       # 30 x 18, not 40 x 24
    with pytest.raises(sfa.SlowflowError, match=r"source\[2\].*30 x 18.*40 x 24"):
        sfa.TrackJob(ctx, p)
    p = ti.T1.params(use_occlusions=1)
    p.source[2] = sfa.jet_source(24, 12, crop=(2, 0, 20, 12), rescale=2.0)
    with pytest.raises(sfa.SlowflowError, match=r"source\[2\].*cropped occlusions"):
        sfa.TrackJob(ctx, p)
    assert sfa.track_job_bytes(ti.T1.params()) > 0
    job = sfa.TrackJob(ctx, ti.T1.params())                                 # T1's parameters themselves are accepted
    with pytest.raises(sfa.SlowflowError, match="ns = 4"):
        job.run(4)
    seg = segments["T1", 11]
    with pytest.raises(sfa.SlowflowError, match="s = 3"):
        job.upload_frames(3, seg["frames"])
    with pytest.raises(sfa.SlowflowError, match="s = 3"):
        job.upload_flows(3, 0, *seg["flows"][0])
    job.close()


def test_nan_in_the_stride_padding_changes_nothing(ctx):
    """the host uploads at a row stride of w + 3: a plain job (K = 1, fused) fed zero padding and NaN padding gives the same rate and fused results.
    The smallest shape the kernels take (h >= 4), odd width and stride so that no alignment hides a wrong pitch"""
    J, w, h = 2, 13, 9
    stride = w + 3
    rng = np.random.default_rng(3)
    valid_frames = rng.normal(0, 1, (J + 1, 3, h, w))
    drift = np.array([0.5, 0.25]).reshape(2, 1, 1, 1) + rng.normal(0, 0.01, (2, J, h, w))   # forward; backward = -forward: consistent within epsilon
    p = sfa.track_params(w, h, J, [J], sources=[sfa.jet_source(w, h, stride)], fuse=sfa.fuse_params(trws_max_iter=4), skip=1, epsilon=ti.EPSILON)
    job = sfa.TrackJob(ctx, p)
    out = []
    for pad in (0.0, np.nan):
        frames = np.full((J + 1, 3, h, stride), pad, np.float32)
        frames[..., :w] = valid_frames
        flows = [np.full((J, h, stride), pad, np.float32) for _ in range(4)]
        for a, v in zip(flows, (drift[0], drift[1], -drift[0], -drift[1])):
            a[..., :w] = v
        job.upload_flows(0, 0, *flows)
        job.upload_frames(0, frames)
        job.run(1)
        out.append((job.download_rate(0, 0), job.download_fused(0)))
    job.close()
    (rate0, fused0), (rate1, fused1) = out
    assert (rate0["tracked"] == J).any() and np.isfinite(rate0["energy"][rate0["tracked"] == J]).all()   # there are hypotheses, and they were scored
    for got, want in ((rate1, rate0), (fused1, fused0)):
        assert got.keys() == want.keys()
        for k in want:
            assert same(got[k], want[k]), k
