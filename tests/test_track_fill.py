"""The track job that fills in (sfa_track_job_create_fill, csrc/track_fill.hip beside csrc/track.hip): every segment of a run equals, bit for bit, the library's stage calls on that
segment alone -- accumulate_consistent(all_steps) -> consistent_regions -> fill_matches -> the fp32 additions of euc in numpy -> epic_batch ->
fill_trajectories -> hypothesis_energies(adapted=True) of both kinds -> smoothness_weight -> fuse_hypotheses with 2 K slots -- and one segment also equals
tests/host/epic_fill_tool.cpp's chain of single host epic() calls on one shared edge map, so that the comparison is not library against library only.
The inputs are tests/fill_inputs.py's; tests/test_track_fill_host.py shows on the restatements which of their rates are filled."""
import os
import subprocess

import numpy as np
import pytest

try:                                    # before the library: the two then share one HIP runtime (tests/test_track_device.py imports it first as well)
    import torch
except ImportError:
    torch = None

import fill_inputs as fi
import slowflow_amd as sfa
from fuse_ref import popcount
from test_epic_fill import run_tool, tool  # noqa: F401  (tool: the fixture that builds tests/host/epic_fill_tool.cpp)
from track_inputs import best_and_occluded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
INF = np.float64(np.inf)


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def labtool(tmp_path_factory):
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path_factory.mktemp("lab") / "lab_tool")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-pthread", "-I", HOST, os.path.join(ROOT, "tests", "host", "lab_tool.cpp"), os.path.join(HOST, "libslowflow_host.a"),
                        "-L", os.path.join(ROOT, "slowflow_amd"), "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "slowflow_amd"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def segs(labtool, tmp_path_factory):
    """(case name, seed) -> fill_inputs.segment with "lab": the host's rgb_to_lab of its image"""
    d = tmp_path_factory.mktemp("segs")
    out = {}
    for case in (fi.BASE, fi.SKIP1, fi.TAIL):
        for seed in (s for run in case.runs for s in run):
            seg = fi.segment(case, seed)
            a, b = str(d / ("rgb_%s_%d.bin" % (case.name, seed))), str(d / ("lab_%s_%d.bin" % (case.name, seed)))
            seg["rgb"].tofile(a)
            r = subprocess.run([labtool, a, str(case.gw), str(case.gh), b], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            seg["lab"] = np.fromfile(b, np.float32).reshape(seg["rgb"].shape)
            out[case.name, seed] = seg
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    """IEEE == on every element, bit patterns for the doubles"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64 or b.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return a.shape == b.shape and np.array_equal(a, b)


def staged_fill(ctx, case, seg, rates=(0, 1), euc=fi.EUC):
    """the library's stage calls on one segment.  rates: the indices into fi.RATES the job has, in its order.  -> {"rate": [...], "fill": [...], "fused":
    fuse_hypotheses' dict without the leading axis, "E", "O" (2 K slots)}"""
    K, J, w, h, skip, gw, gh = len(rates), fi.JETS, case.w, case.h, case.skip, case.gw, case.gh
    mf = rates.index(fi.MIN_FPS)
    U, V = np.zeros((1, 2 * K, J, gh, gw)), np.zeros((1, 2 * K, J, gh, gw))
    E, O = np.full((1, 2 * K, gh, gw), INF), np.zeros((1, 2 * K, gh, gw), np.uint64)
    xs, ys = sfa.fill_samples(gw, fi.EPIC_SKIP), sfa.fill_samples(gh, fi.EPIC_SKIP)
    ep = sfa.epic_params(pref_nn=25, nn=160, coef_kernel=1.1, euc=euc)
    rate, fill, calls = [], [], 0
    for k, r in enumerate(rates):
        rJ = fi.RATES[r]
        fu, fv, bu, bv = (a[None] for a in seg["flows"][r])
        au, av, tr = ctx.accumulate_consistent(fu, fv, bu, bv, w, fi.EPSILON, skip, True, True)
        mask, kept = ctx.consistent_regions(tr, [rJ], 100)
        m, count = ctx.fill_matches(au, av, mask, xs, ys, divisor=skip + 1)
        nm = int(count[0])
        # step j's map: the file's after calls + j additions, and then the one epic() makes on entry
        costs = [fi.advanced(seg["edges"], calls + j + 1, euc) for j in range(rJ)]
        calls += rJ
        filled, hu, hv, htr = 0, np.zeros((1, rJ, gh, gw)), np.zeros((1, rJ, gh, gw)), None
        if nm > 0:
            fx, fy, rc, _, _ = ctx.epic_batch([seg["lab"]] * rJ, costs, [m[0, j, :nm] for j in range(rJ)], ep)
            if all(c == 0 for c in rc):
                hu, hv, htr = ctx.fill_trajectories(np.stack(fx)[None], np.stack(fy)[None], gw, scale=skip + 1)
                filled = 1
        p = sfa.energy_params(skip=skip, weight=fi.WEIGHTS[r])
        flows = tuple(a[None] for a in seg["flows"][fi.MIN_FPS]) if k >= mf else None
        for kind, (a_u, a_v, a_t) in enumerate(((au, av, tr), (hu, hv, htr))):
            if kind and not filled:
                continue                                                    # the slot stays empty: +Inf, 0, 0
            slot = 2 * k + kind
            E[0, slot], O[0, slot], U[0, slot], V[0, slot] = (a[0] for a in ctx.hypothesis_energies(p, rJ, a_u, a_v, a_t, seg["frames"][None], w, flows=flows, adapted=True))
        rate.append(dict(u=au[0, -1], v=av[0, -1], tracked=tr[0], energy=E[0, 2 * k].copy(), occ_bits=O[0, 2 * k].copy()))
        fill.append(dict(u=hu[0], v=hv[0], energy=E[0, 2 * k + 1].copy(), occ_bits=O[0, 2 * k + 1].copy(), kept_pixels=int(kept[0]), matches=nm, filled=filled))
    weight = ctx.smoothness_weight(np.ascontiguousarray(seg["frames"][0]), w)
    f = ctx.fuse_hypotheses(sfa.fuse_params(trws_max_iter=8, skip=skip), U, V, E, O, weight[None], w, h)
    return dict(rate=rate, fill=fill, fused={k: f[k][0] for k in ("slot", "u", "v", "occ", "energy", "bound", "iters")}, E=E[0], O=O[0])


@pytest.fixture(scope="module")
def want(ctx, segs):
    """staged_fill of every segment of the three cases, computed once"""
    return {key: staged_fill(ctx, next(c for c in (fi.BASE, fi.SKIP1, fi.TAIL) if c.name == key[0]), seg) for key, seg in segs.items()}


def upload(job, case, s, seg):
    for r in range(case.K):
        job.upload_flows(s, r, *seg["flows"][r])
    job.upload_frames(s, seg["frames"])
    job.upload_fill(s, seg["lab"], seg["edges"])


def check_segment(job, K, s, w):
    """the job's downloads of segment s against staged_fill's dict"""
    best, occluded = best_and_occluded(w["E"][0::2], w["O"][0::2])            # the accumulated hypotheses only
    for r in range(K):
        got = job.download_rate(s, r)
        for k in ("u", "v", "tracked", "energy", "occ_bits"):
            assert same(got[k], w["rate"][r][k]), (s, r, k)
        assert same(got["occluded"], occluded[r]) and same(got["occluded"], popcount(got["occ_bits"]).astype(np.uint8)), (s, r)
        got = job.download_fill(s, r)
        for k in ("kept_pixels", "matches", "filled"):
            assert got[k] == w["fill"][r][k], (s, r, k, got[k], w["fill"][r][k])
        for k in ("u", "v", "energy", "occ_bits"):
            assert same(got[k], w["fill"][r][k]), (s, r, k)
    got = job.download_fused(s)
    for k in ("slot", "u", "v", "occ"):
        assert same(got[k], w["fused"][k]), (s, k)
    assert same(got["best"], best), s
    assert same(np.float64(got["energy"]), np.float64(w["fused"]["energy"])) and same(np.float64(got["bound"]), np.float64(w["fused"]["bound"]))
    assert got["iters"] == int(w["fused"]["iters"]), (s, got["iters"], w["fused"]["iters"])
    return got["slot"]


def run_case(ctx, case, segs, want, **fill_kw):
    """every run of the case on one job, every segment checked; -> the slots of all segments, the job's (completed, re-run) sub-batches per run"""
    job = sfa.TrackJob(ctx, case.params(), case.fill(**fill_kw))
    slots, info = [], []
    for run in case.runs:
        for s, seed in enumerate(run):
            upload(job, case, s, segs[case.name, seed])
        job.run(len(run))
        for s, seed in enumerate(run):
            w = want[case.name, seed]
            for r in range(case.K):
                assert w["fill"][r]["filled"] == case.filled(seed, r), (seed, r)        # what tests/test_track_fill_host.py shows on the restatements
            slots.append(check_segment(job, case.K, s, w))
        info.append(job.fill_info())
    ms, fms = job.stage_ms(), job.fill_ms()
    assert len(ms) == 8 and all(m >= 0 for m in ms) and len(fms) == 4 and all(m >= 0 for m in fms) and fms[2] > 0
    job.close()
    return slots, info


def test_base_two_runs_equal_the_staged_calls(ctx, segs, want):
    """96 x 64, rates (2, 4), three segments of which one keeps only islands on rate 0, then two new segments on the same job: the position that was
    filled in the first run is not in the second and comes out +Inf"""
    case = fi.BASE
    slots, info = run_case(ctx, case, segs, want)
    assert all(i[0] >= case.K for i in info)
    first, again = want[case.name, case.runs[0][0]]["fill"][0], want[case.name, case.runs[1][0]]["fill"][0]
    assert first["filled"] == 1 and np.isfinite(first["energy"]).all()
    assert again["filled"] == 0 and (again["energy"] == INF).all() and (again["occ_bits"] == 0).all() and (again["u"] == 0).all()
    slots = np.stack(slots)
    assert (slots % 2 == 1).any() and ((slots >= 0) & (slots % 2 == 0)).any()  # fill-in and accumulated hypotheses both win somewhere


def test_skip_1_lab_and_edges_at_the_grids_size(ctx, segs, want):
    assert (fi.SKIP1.gw, fi.SKIP1.gh) == (48, 32)
    run_case(ctx, fi.SKIP1, segs, want)


def test_a_plane_that_is_no_multiple_of_four_pixels(ctx, segs, want):
    """99 x 65 = 6435 pixels: six full blocks of the advance kernel, 291 pixels in quads and a tail of three"""
    assert (fi.TAIL.gw * fi.TAIL.gh) % 4 == 3 and (fi.TAIL.gw * fi.TAIL.gh) % 1024 != 0
    run_case(ctx, fi.TAIL, segs, want)


def test_the_call_index_is_live_and_euc_0_adds_nothing(ctx, segs, want):
    """rate 1 alone is the first rate of its job: without the two additions of rate 0's calls its fill-in differs beyond its last bits"""
    case, seed = fi.BASE, fi.BASE.runs[0][0]
    seg = segs[case.name, seed]
    for euc in (fi.EUC, 0.0):
        p = sfa.track_params(case.w, case.h, fi.JETS, fi.RATES[1:], n=1, weights=fi.WEIGHTS[1:], fuse=sfa.fuse_params(trws_max_iter=8), min_fps_idx=0, skip=0,
                             epsilon=fi.EPSILON, discard=1)
        job = sfa.TrackJob(ctx, p, case.fill(euc=euc))
        job.upload_flows(0, 0, *seg["flows"][1])
        job.upload_frames(0, seg["frames"])
        job.upload_fill(0, seg["lab"], seg["edges"])
        job.run(1)
        alone = staged_fill(ctx, case, seg, rates=(1,), euc=euc)
        assert alone["fill"][0]["filled"] == 1
        check_segment(job, 1, 0, alone)
        job.close()
        if euc:
            diff = np.abs(alone["fill"][0]["u"] - want[case.name, seed]["fill"][1]["u"])
            assert (diff > 1e-3).any(), "the call index does not change the second rate's fill-in beyond its last bits"


# The interpolation's workspace of the forced cases.  The base case's first run has 2 x 2 images of rate 0 and 3 x 4 of rate 1, each with about 1000 matches.
# With nn 160 an image owns about 2 MB for the whole chain (two lists of 1000 x 160 entries, four planes of 24.5 KB), and its dense search allocates 16.5 MB
# (sfa_epic_nn_search_info's workspace: `done` = ns x ns floats and the heaps) of which the chain knows the smaller part beforehand.  48 MB therefore hold
# two images and never three, and the chain plans more than fit: measured 8 sub-batches of two with 3 cut short and run again.  The compact search shares
# one workspace among its slices, so the same 16 images need 24 MB before they split: measured 4 sub-batches, 1 run again, 26 slices.
FORCED = {"dense": 48 << 20, "compact": 24 << 20}


@pytest.mark.parametrize("search", ("dense", "compact"))
def test_forced_sub_batches_and_a_rerun_leave_the_bits(ctx, segs, want, search):
    case = fi.BASE
    ctx.set_epic_search(search)
    try:
        job = sfa.TrackJob(ctx, case.params(), case.fill(workspace_bytes=FORCED[search]))
        run = case.runs[0]
        for s, seed in enumerate(run):
            upload(job, case, s, segs[case.name, seed])
        job.run(len(run))
        done, again = job.fill_info()
        info = ctx.epic_nn_search_info()
        print("sub-batches: %d completed, %d run again (%s, %s)" % (done, again, search, info))
        for s, seed in enumerate(run):
            check_segment(job, case.K, s, want[case.name, seed])
        images = sum(fi.RATES[r] * sum(case.filled(seed, r) for seed in run) for r in range(case.K))
        assert images == 16 and done >= 2 * case.K and again >= 1                # every rate's images take at least two sub-batches, one was run again
        job.close()
    finally:
        ctx.set_epic_search("dense")


def test_one_segment_equals_the_hosts_chain_of_single_epic_calls(ctx, tool, segs, want, tmp_path):  # noqa: F811
    case, seed = fi.BASE, fi.BASE.runs[0][0]
    seg, w = segs[case.name, seed], want[case.name, seed]
    inputs = []
    for r in range(case.K):
        fu, fv, bu, bv = (a[None] for a in seg["flows"][r])
        au, av, tr = ctx.accumulate_consistent(fu, fv, bu, bv, case.w, fi.EPSILON, case.skip, True, True)
        inputs.append((au[0], av[0], tr[0]))
    # test_epic_fill.run_tool writes its own scene's image and edge map for `seed`: fill_inputs.segment takes the same ones
    res = run_tool(tool, str(tmp_path), fi.RATES, inputs, fi.EUC, seed=seed, epic_skip=2)
    job = sfa.TrackJob(ctx, case.params(), case.fill())
    upload(job, case, 0, seg)
    job.run(1)
    for r, rJ in enumerate(fi.RATES):
        k, cf, ck, cm, ff, fk, fm, idx = res[r]["line"]
        got = job.download_fill(0, r)
        assert (cf, ck, cm) == (got["filled"], got["kept_pixels"], got["matches"]) == (1, w["fill"][r]["kept_pixels"], w["fill"][r]["matches"])
        assert same(got["u"], res[r]["chain"][0]) and same(got["v"], res[r]["chain"][1]), r
    job.close()


def test_upload_fill_device_from_strided_tensors_equals_the_host_upload(ctx, segs, want):
    if torch is None:
        pytest.skip("torch is not installed")
    from test_track_device import padded
    case, run = fi.BASE, fi.BASE.runs[0]
    dev = torch.device("cuda", 0)
    job = sfa.TrackJob(ctx, case.params(), case.fill())
    for s, seed in enumerate(run):
        seg = segs[case.name, seed]
        for r in range(case.K):
            job.upload_flows(s, r, *seg["flows"][r])
        job.upload_frames(s, seg["frames"])
    lab = padded(np.stack([segs[case.name, seed]["lab"][:, :, :case.gw] for seed in run]), dev)
    edges = padded(np.stack([segs[case.name, seed]["edges"] for seed in run]), dev, pad=(2, 3))
    # channels last for the second and third segment: another set of strides through the same entry point
    last = torch.from_numpy(np.ascontiguousarray(np.stack([segs[case.name, seed]["lab"][:, :, :case.gw] for seed in run[1:]]).transpose(0, 2, 3, 1))).to(dev).permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    ctx.wait_stream(torch.cuda.current_stream(dev))
    job.upload_fill_device(lab[:1], edges[:1], s0=0)
    job.upload_fill_device(last, edges[1:], s0=1)
    job.run(len(run))
    for s, seed in enumerate(run):
        check_segment(job, case.K, s, want[case.name, seed])
    with pytest.raises(sfa.SlowflowError, match="s0 = 2, ns = 2"):
        job.upload_fill_device(last, edges[1:], s0=2)
    job.close()
    plain = sfa.TrackJob(ctx, case.params())
    with pytest.raises(sfa.SlowflowError, match="sfa_track_job_create_fill"):
        plain.upload_fill(0, segs[case.name, run[0]]["lab"], segs[case.name, run[0]]["edges"])
    plain.close()
