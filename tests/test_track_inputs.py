"""The track-job tests' seeded inputs (tests/track_inputs.py) on the restatements alone, so that the GPU comparisons of tests/test_track_job.py cannot
go vacuous: every slot has hypotheses, the NMS leaves a choice, some pixels have none, the fusion uses more than one slot, TRW-S stops at different
iterations and no two segments fuse to the same flow.  Also the layout of sfa_track_params against the header."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import slowflow_amd as sfa
import track_inputs as ti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def restated(oracle):
    return {(c.name, seed): ti.restate(oracle, c, ti.segment(c, seed)) for c in (ti.T1, ti.T2) for seed in c.seeds}


@pytest.mark.parametrize("case", [ti.T1, ti.T2], ids=lambda c: c.name)
def test_every_segment_exercises_the_stages(restated, case):
    npix = case.gw * case.gh
    for seed in case.seeds:
        r = restated[case.name, seed]
        present = np.isfinite(r["E"])
        for k in range(case.K):
            assert present[k].sum() >= 0.25 * npix, (seed, k, int(present[k].sum()))
        assert (present.sum(0) == 0).any(), seed                            # a pixel without any hypothesis: no node, its edges dropped
        kept = np.array([len(l) for l in r["fused"]["lab"]])
        assert (kept >= 2).sum() >= 0.5 * npix, (seed, int((kept >= 2).sum()))
        slot = r["fused"]["slot"]
        nodes = (slot >= 0).sum()
        used = [k for k in range(case.K) if (slot == k).sum() >= 0.05 * nodes]
        assert len(used) >= 2, (seed, [int((slot == k).sum()) for k in range(case.K)])
        assert len(set(r["best"][r["best"] != 255].tolist())) >= 2, seed


def test_iteration_counts_and_flows_differ_between_segments(restated):
    its = [restated["T1", seed]["fused"]["iters"] for seed in ti.T1.seeds]
    assert len(set(its)) > 1, its
    for case in (ti.T1, ti.T2):
        for a, b in itertools.combinations(case.seeds, 2):
            fa, fb = restated[case.name, a]["fused"], restated[case.name, b]["fused"]
            assert not (np.array_equal(fa["u"], fb["u"]) and np.array_equal(fa["v"], fb["v"])), (case.name, a, b)


def test_track_params_layout_matches_the_header():
    """sfa_track_params field by field in the header's order; csrc/track.hip asserts the same size at build time"""
    src = open(os.path.join(ROOT, "include", "slowflow_amd.h")).read()
    body = re.search(r"typedef struct sfa_track_params \{(.*?)\} sfa_track_params;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[.*", "", n.strip().split()[-1]) for n in decl.split(",")]
    assert names == [f[0] for f in sfa.TrackParams._fields_]
    assert C.sizeof(sfa.JetSource) == 32 and C.sizeof(sfa.EnergyParams) == 64 and C.sizeof(sfa.FuseParams) == 48
    assert sfa.TrackParams.source.offset == 96 and sfa.TrackParams.epsilon.offset == 672 and sfa.TrackParams.energy.offset == 688
    assert sfa.TrackParams.fuse.offset == 752 and sfa.TrackParams.coef.offset == 800 and C.sizeof(sfa.TrackParams) == 832


def test_track_job_bytes_is_host_only_and_grows():
    base = sfa.track_job_bytes(ti.T1.params(n=1))
    assert sfa.track_job_bytes(ti.T1.params(n=2)) > base > 0
    more_rates = sfa.track_params(40, 24, 2, (1, 2, 4, 2), n=1, min_fps_idx=1)
    fewer = sfa.track_params(40, 24, 2, (1, 2, 4), n=1, min_fps_idx=1)
    assert sfa.track_job_bytes(more_rates) > sfa.track_job_bytes(fewer)
    assert sfa.track_job_bytes(sfa.track_params(40, 24, 4, (4,), n=1)) > sfa.track_job_bytes(sfa.track_params(40, 24, 2, (2,), n=1))
    with pytest.raises(sfa.SlowflowError, match="n = 65"):
        sfa.track_job_bytes(ti.T1.params(n=65))
