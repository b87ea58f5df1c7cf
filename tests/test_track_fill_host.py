"""The host side of the track job that fills in (sfa_track_job_create_fill, csrc/track_fill.hip on csrc/track_job.h): its fixed allocation against the plain job's, the refusals
by name, and -- on the restatements tests/accum_ref.py and tests/fill_ref.py -- that the scenes of tests/fill_inputs.py are what tests/test_track_fill.py
takes them for: at least 100 kept pixels and 160 matches per step (the interpolation's nn: no other path of epic() is taken) where a rate is claimed to
be filled, none where it is not."""
import os

import numpy as np
import pytest

import fill_inputs as fi
import fill_ref
import slowflow_amd as sfa
from accum_ref import accumulate


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()


def test_entry_points_are_declared_and_bound():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slowflow_amd.h")).read()
    for name in ("sfa_track_fill_params_default", "sfa_track_job_bytes_fill", "sfa_track_job_create_fill", "sfa_track_job_upload_fill",
                 "sfa_track_job_upload_fill_device", "sfa_track_job_download_fill", "sfa_track_job_fill_ms", "sfa_track_job_fill_info"):
        assert name + "(" in text and name in sfa.EXPORTS and hasattr(sfa.lib(), name), name
    f = sfa.track_fill_params()
    assert (f.epic_skip, f.min_size, f.workspace_bytes) == (2.0, 100, 0)
    e, d = f.epic, sfa.epic_params(pref_nn=25, nn=160, coef_kernel=1.1)                      # epic_fill_params: the defaults, then the three
    assert [getattr(e, k) for k, _ in sfa.EpicParams._fields_] == [getattr(d, k) for k, _ in sfa.EpicParams._fields_] and e.method == 0


# the fill jobs' bytes of the three scenes, pinned like the plain total below: a change of the plane table (csrc/track_job.h) must not move them unseen
FILL_BYTES = {"base": 40651264, "skip1": 6154496, "tail": 28627968}


def test_bytes_count_the_fill_planes_and_leave_the_plain_job_alone():
    for case in (fi.BASE, fi.SKIP1, fi.TAIL):
        p = case.params()
        plain, fill = sfa.track_job_bytes(p), sfa.track_job_bytes(p, case.fill())
        assert fill > plain > 0
        assert fill == FILL_BYTES[case.name], (case.name, fill)
        gpl = case.gw * case.gh
        # at least: the slots' energies, occlusion words and adapted flows twice, the fill-in's trajectories, the cost planes of the longest rate
        extra = case.n * gpl * (case.K * 16 + case.K * fi.JETS * 16 + sum(fi.RATES) * 16 + max(fi.RATES) * 4)
        assert fill - plain >= extra, (case.name, fill - plain, extra)
        assert sfa.track_job_bytes(p, case.fill(workspace_bytes=1 << 20)) == fill               # the interpolation's workspace is not part of it
    p = fi.BASE.params()
    before = sfa.track_job_bytes(p)
    sfa.track_job_bytes(p, fi.BASE.fill())
    assert sfa.track_job_bytes(p) == before == 30038784                                        # the plain job's bytes, as they were before there was a fill job


def refused(match, case=fi.BASE, params=None, **kw):
    epic = kw.pop("epic", None)
    f = case.fill(**kw)
    for k, v in (epic or {}).items():
        setattr(f.epic, k, v)
    with pytest.raises(sfa.SlowflowError, match=match):
        sfa.track_job_bytes(params if params is not None else case.params(), f)


def test_refusals_name_their_argument():
    refused(r"epic\.nn = 0", epic=dict(nn=0))
    refused(r"epic\.pref_nn = -1", epic=dict(pref_nn=-1))
    refused(r"epic\.method = 2", epic=dict(method=2))
    refused(r"epic_skip = 0\.5", epic_skip=0.5)
    refused(r"epic_skip = nan", epic_skip=float("nan"))
    refused(r"epic_skip = inf", epic_skip=float("inf"))
    refused(r"min_size = 0", min_size=0)
    nine = sfa.track_params(96, 64, 1, (1,) * 9, n=1, skip=0)
    refused(r"K = 9", params=nine)
    sfa.track_job_bytes(sfa.track_params(96, 64, 1, (1,) * 8, n=1, skip=0), fi.BASE.fill())  # 16 slots are taken
    small = sfa.track_params(16, 64, fi.JETS, fi.RATES, n=1, min_fps_idx=fi.MIN_FPS, skip=1)  # a grid of 8 columns
    refused(r"gw x gh = 8 x 32.*saliency_th", params=small)
    sfa.track_job_bytes(small, fi.BASE.fill(epic=sfa.epic_params(saliency_th=0.0, nn=160)))   # without the saliency filter the grid is taken
    with pytest.raises(sfa.SlowflowError, match="sfa_track_job_bytes_fill: n = 0"):           # what the plain job refuses, under the fill call's name
        sfa.track_job_bytes(_with(fi.BASE.params(), n=0), fi.BASE.fill())


def _with(p, **kw):
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("case", (fi.BASE, fi.SKIP1, fi.TAIL), ids=lambda c: c.name)
def test_the_scenes_are_filled_where_claimed_and_nowhere_else(case):
    xs, ys = fill_ref.fill_samples(case.gw, fi.EPIC_SKIP), fill_ref.fill_samples(case.gh, fi.EPIC_SKIP)
    assert np.array_equal(xs, sfa.fill_samples(case.gw, fi.EPIC_SKIP)) and np.array_equal(ys, sfa.fill_samples(case.gh, fi.EPIC_SKIP))
    claims = set()
    for seed in (s for run in case.runs for s in run):
        seg = fi.segment(case, seed)
        for r, rJ in enumerate(fi.RATES):
            fu, fv, bu, bv = (a[:, :, :case.w] for a in seg["flows"][r])
            _, _, tracked = accumulate(fu, fv, bu, bv, None, fi.EPSILON, case.skip, True)
            mask = fill_ref.consistent_regions(tracked, rJ)
            kept, matches = int(mask.sum()), int(mask[np.ix_(ys, xs)].sum())
            claims.add(case.filled(seed, r))
            if case.filled(seed, r):
                assert kept >= 100 and matches >= 160, (seed, r, kept, matches)
                assert (tracked == rJ).sum() > kept                                              # removeSmallSegments does remove something
            else:
                assert (tracked == rJ).sum() >= 3 * 16 and kept == 0 and matches == 0, (seed, r, kept, matches)
    assert 1 in claims and (case is not fi.BASE or 0 in claims)
    if case is fi.BASE:                                                                       # the second run empties a position the first one filled
        assert case.filled(case.runs[0][0], 0) == 1 and case.filled(case.runs[1][0], 0) == 0
