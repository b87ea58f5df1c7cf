"""The track job's occlusion images from GPU memory (sfa_track_job_upload_occlusions_device; TrackJob.upload_occlusions_device, device.track(occlusions=)):
a job whose flows and occlusion images come from device tensors equals, on every element of every download, the job that takes them from host planes
through upload_flows(occ=), and both equal the restatement (track_inputs.restate) on the same images.  All comparisons are ==.

track_inputs' own occlusion images are the same for every segment and non-zero only in a rate's last step: they cannot catch a segment or step mix-up.
occlusion_images() below draws, per (seed, rate, step), one or two seeded rectangles of 255 on 0; test_the_images_tell_steps_and_segments_apart shows on
the restatement's accumulation (discard 1) that exchanging the images of any two steps of a rate, or of any two segments, or leaving them out, changes
that rate's `tracked`.  Shape: T1 (40 x 24 frames, r_Jets (1, 2, 4), rate 2 stored at 20 x 12 so that the cubic resize runs, n = 3, five seeds)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import slowflow_amd as sfa
import track_inputs as ti
from accum_ref import accumulate
from jet_resample_ref import decode_occlusion_scaled, resample_flow

torch = pytest.importorskip("torch")
CASE = ti.T1
F32 = np.float32
gpu = pytest.mark.gpu


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def occlusion_images(case, seed):
    """occ[r]: raw uint8 images (r_Jets[r], sh, stride), per step one or two rectangles of 255 on 0, seeded by (seed, rate, step); the padding stays 0"""
    out = []
    for r in range(case.K):
        sw, sh, stride, _ = case.source(r)
        o = np.zeros((case.r_Jets[r], sh, stride), np.uint8)
        for k in range(case.r_Jets[r]):
            rng = np.random.default_rng([seed, r, k, 21])
            for _ in range(int(rng.integers(1, 3))):
                ew, eh = int(rng.integers(sw // 5, sw // 2)), int(rng.integers(sh // 4, sh // 2 + 1))
                x0, y0 = int(rng.integers(0, sw - ew + 1)), int(rng.integers(0, sh - eh + 1))
                o[k, y0:y0 + eh, x0:x0 + ew] = 255
        out.append(o)
    return out


LABELS = np.array([-1, 0, 1, 0.5, -0.5, 2, -3, np.nan, np.inf, -np.inf], F32)
GREY_OF_LABELS = (0, 128, 255, 191, 64, 255, 0, 255, 255, 0)                    # (x + 1) / 2 * 255 rounded to even and clipped; NaN -> 255


def label_images(case, seed):
    """lab[r]: fp32 occlusion labels (r_Jets[r], sh, sw) drawn from LABELS in blocks of 3 x 2 pixels, seeded by (seed, rate)"""
    out = []
    for r in range(case.K):
        sw, sh, _, _ = case.source(r)
        rng = np.random.default_rng([seed, r, 3])
        pick = rng.integers(0, len(LABELS), (case.r_Jets[r], (sh + 1) // 2, (sw + 2) // 3))
        pick.reshape(pick.shape[0], -1)[:, :len(LABELS)] = np.arange(len(LABELS))  # every label at least once
        out.append(LABELS[np.repeat(np.repeat(pick, 2, 1), 3, 2)[:, :sh, :sw]])
    return out


def grey_of(labels):
    """the driver's occlusion_image in numpy: (x + 1) * 0.5f * 255.0f in fp32, rint (halves to even), clipped to 0 .. 255, NaN -> 255"""
    with np.errstate(invalid="ignore"):
        v = (labels.astype(F32) + F32(1)) * F32(0.5) * F32(255)
        assert v.dtype == F32
        g = np.clip(np.rint(v), F32(0), F32(255))
    return np.where(np.isnan(g), F32(255), g).astype(np.uint8)


def in_stride(case, r, img):
    """(rJ, sh, sw) -> (rJ, sh, stride) with zero padding: the host planes of upload_flows"""
    sw, sh, stride, _ = case.source(r)
    o = np.zeros(img.shape[:1] + (sh, stride), np.uint8)
    o[..., :sw] = img
    return o


def segment_with(case, seed, occ):
    seg = dict(ti.segment(case, seed))
    seg["occ"] = occ
    return seg


def flows_at_size(case, seg, r):
    """rate r's four flow arrays at the tracking frames' size, as restate() forms them"""
    sw, _, _, rs = case.source(r)
    fu, fv, bu, bv = (a[:, :, :sw] for a in seg["flows"][r])
    if r not in case.scaled:
        return fu, fv, bu, bv
    f = [resample_flow(fu[k], fv[k], rs) for k in range(fu.shape[0])]
    b = [resample_flow(bu[k], bv[k], rs) for k in range(fu.shape[0])]
    return np.stack([q[0] for q in f]), np.stack([q[1] for q in f]), np.stack([q[0] for q in b]), np.stack([q[1] for q in b])


def same_pixels(case, flows, a, b):
    """True where no trajectory that survives without occlusions reads another mask pixel at step b than at step a (the accumulation truncates the
    position origin + acc[f - 1]): no images can then tell the two steps apart, a discarded trajectory being discarded whichever step did it"""
    au, av, tr = accumulate(*flows, None, ti.EPSILON, case.skip, True)
    gy, gx = np.mgrid[0:case.gh, 0:case.gw] * case.incr + case.start

    def pixel(f):
        return ((gx + au[f - 1]).astype(np.int64), (gy + av[f - 1]).astype(np.int64)) if f else (gx, gy)
    (xa, ya), (xb, yb) = pixel(a), pixel(b)
    return not (((xa != xb) | (ya != yb)) & (tr > 0)).any()


def test_the_images_tell_steps_and_segments_apart():
    """on the CPU: with discard 1, a rate's `tracked` in the restatement changes when the images of two of its steps are exchanged, when another
    segment's images take their place, and when there are none.  Seed 11 moves by less than a pixel per step in both directions: its trajectories read
    the same mask pixel at steps 0 and 1 of rates 1 and 2, which no images can tell apart; the other four segments do, for every pair of steps."""
    case = CASE
    segs = {seed: segment_with(case, seed, occlusion_images(case, seed)) for seed in case.seeds}
    exempt = set()
    for r in range(case.K):
        sw, _, _, rs = case.source(r)
        masks = {seed: np.stack([decode_occlusion_scaled(g[:, :sw], rs) for g in segs[seed]["occ"][r]]) for seed in case.seeds}
        for seed in case.seeds:
            flows = flows_at_size(case, segs[seed], r)

            def tracked(m):
                return accumulate(*flows, m, ti.EPSILON, case.skip, True)[2]
            own = tracked(masks[seed])
            assert 0 < np.count_nonzero(own) < own.size, (r, seed)
            assert not np.array_equal(own, tracked(None)), (r, seed)
            for a, b in itertools.combinations(range(case.r_Jets[r]), 2):
                if same_pixels(case, flows, a, b):
                    exempt.add((r, seed, a, b))
                    continue
                order = list(range(case.r_Jets[r]))
                order[a], order[b] = b, a
                assert not np.array_equal(own, tracked(masks[seed][order])), (r, seed, a, b)
            for other in case.seeds:
                if other != seed:
                    assert not np.array_equal(own, tracked(masks[other])), (r, seed, other)
    assert exempt == {(1, 11, 0, 1), (2, 11, 0, 1)}, exempt


def test_grey_of_gives_the_values_the_header_states():
    assert tuple(grey_of(LABELS)) == GREY_OF_LABELS
    assert all(set(GREY_OF_LABELS) <= set(np.unique(grey_of(lab))) for lab in label_images(CASE, CASE.seeds[0]))


# ---- the GPU tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def segs():
    return {seed: segment_with(CASE, seed, occlusion_images(CASE, seed)) for seed in CASE.seeds}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64 or b.dtype == np.float64:
        a, b = np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64)
    return a.shape == b.shape and np.array_equal(a, b)


def collect(job, s):
    return dict(rate=[job.download_rate(s, r) for r in range(CASE.K)], fused=job.download_fused(s))


def assert_same(got, want, what):
    for r in range(CASE.K):
        for k in ("u", "v", "tracked", "energy", "occ_bits", "occluded"):
            assert same(got["rate"][r][k], want["rate"][r][k]), (what, r, k)
    for k in ("slot", "u", "v", "occ", "best", "energy", "bound", "iters"):
        assert same(got["fused"][k], want["fused"][k]), (what, k)


def assert_restated(got, want, what):
    """a job's downloads against track_inputs.restate's dict"""
    for r in range(CASE.K):
        for k in ("u", "v", "tracked", "energy", "occ_bits"):
            assert same(got["rate"][r][k], want["rate"][r][k]), (what, r, k)
        assert same(got["rate"][r]["occluded"], want["occluded"][r]), (what, r)
    for k in ("slot", "u", "v", "occ"):
        assert same(got["fused"][k], want["fused"][k]), (what, k)
    assert same(got["fused"]["best"], want["best"]), what
    assert same(np.float64(got["fused"]["energy"]), np.float64(want["fused"]["energy"])) and same(np.float64(got["fused"]["bound"]), np.float64(want["fused"]["bound"]))
    assert got["fused"]["iters"] == int(want["fused"]["iters"]), what


def host_route(ctx, groups):
    """job A: flows and occ through upload_flows, one run per group of segments -> one collect() per segment"""
    job = sfa.TrackJob(ctx, CASE.params(use_occlusions=1))
    out = []
    for group in groups:
        for s, seg in enumerate(group):
            for r in range(CASE.K):
                job.upload_flows(s, r, *seg["flows"][r], occ=seg["occ"][r])
            job.upload_frames(s, seg["frames"])
        job.run(len(group))
        out.append([collect(job, s) for s in range(len(group))])
    job.close()
    return out


@pytest.fixture(scope="module")
def job_a(ctx, segs):
    """the host route on the five seeds, two runs as test_track_job's test_t1 does them"""
    return host_route(ctx, [[segs[seed] for seed in CASE.seeds[:3]], [segs[seed] for seed in CASE.seeds[3:]]])


@pytest.fixture(scope="module")
def restated(oracle, segs):
    return {seed: ti.restate(oracle, CASE, segs[seed], True, True) for seed in CASE.seeds}


def padded(a, dev, fill):
    """a numpy array as a view into a larger device tensor of its type: one extra plane in front, one row above and below, two and three columns beside
    the last two dimensions (a padded row pitch, an offset, no contiguity)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    big = torch.full((a.shape[0] + 1,) + tuple(a.shape[1:-2]) + (a.shape[-2] + 2, a.shape[-1] + 5), fill, dtype=t.dtype, device=dev)
    view = big[1:, ..., 1:1 + a.shape[-2], 2:2 + a.shape[-1]]
    view.copy_(t.to(dev))
    assert not view.is_contiguous()
    return view


def device_inputs(group, dev, occ=None):
    """flows[r] = (fwd, bwd) fp32 [ns, r_Jets, 2, sh, sw], occ[r] [ns, r_Jets, sh, sw] (uint8 from the segments, or the arrays of `occ`: one list per
    segment) and frames [ns, Jets + 1, 3, h, w], none of them contiguous"""
    flows, occs = [], []
    for r in range(CASE.K):
        sw = CASE.source(r)[0]
        fwd = np.stack([np.stack([seg["flows"][r][0][..., :sw], seg["flows"][r][1][..., :sw]], 1) for seg in group])
        bwd = np.stack([np.stack([seg["flows"][r][2][..., :sw], seg["flows"][r][3][..., :sw]], 1) for seg in group])
        both = padded(np.stack([fwd, bwd]), dev, 7e29)
        flows.append((both[0], both[1]))
        if occ is None:
            occs.append(padded(np.stack([seg["occ"][r][..., :sw] for seg in group]), dev, 77))
        else:
            occs.append(padded(np.stack([o[r] for o in occ]), dev, 0.25 if occ[0][r].dtype == F32 else 77))
    frames = padded(np.stack([seg["frames"][..., :CASE.w] for seg in group]), dev, 7e29)
    torch.cuda.synchronize()
    return flows, occs, frames


def upload_device(job, flows, occs, frames, occlusions_first=False):
    """segments 1 .. in one call with s0 = 1 and segment 0 in another, per rate"""
    ns = frames.shape[0]
    for r in range(CASE.K):
        for what in (("occ", "flows") if occlusions_first else ("flows", "occ")):
            for lo, hi in ((1, ns), (0, 1)):
                if hi <= lo:
                    continue
                if what == "occ":
                    job.upload_occlusions_device(r, occs[r][lo:hi], s0=lo)
                else:
                    job.upload_flows_device(r, flows[r][0][lo:hi], flows[r][1][lo:hi], s0=lo)
    job.upload_frames_device(frames)


@gpu
@pytest.mark.parametrize("occlusions_first", [True, False])
def test_u8_route_equals_the_host_route_and_the_restatement(ctx, dev, segs, job_a, restated, occlusions_first):
    job = sfa.TrackJob(ctx, CASE.params(use_occlusions=1))
    for g, seeds in enumerate((CASE.seeds[:3], CASE.seeds[3:])):
        upload_device(job, *device_inputs([segs[seed] for seed in seeds], dev), occlusions_first=occlusions_first)
        job.run(len(seeds))
        for s, seed in enumerate(seeds):
            got = collect(job, s)
            assert_same(got, job_a[g][s], (seed, "host route"))
            assert_restated(got, restated[seed], (seed, "restatement"))
    job.close()


@gpu
def test_fp32_labels_equal_the_u8_route_on_their_grey_image_and_the_restatement(ctx, dev, oracle, segs):
    seeds = CASE.seeds[:3]
    labels = [label_images(CASE, seed) for seed in seeds]
    grey = [[grey_of(lab) for lab in per_rate] for per_rate in labels]
    group = [segs[seed] for seed in seeds]
    out = []
    for occ in (labels, grey):
        job = sfa.TrackJob(ctx, CASE.params(use_occlusions=1))
        upload_device(job, *device_inputs(group, dev, occ))
        job.run(3)
        out.append([collect(job, s) for s in range(3)])
        job.close()
    for s, seed in enumerate(seeds):
        assert_same(out[0][s], out[1][s], (seed, "u8 route on the grey image"))
        seg = segment_with(CASE, seed, [in_stride(CASE, r, grey[s][r]) for r in range(CASE.K)])
        want = ti.restate(oracle, CASE, seg, True, True)
        assert_restated(out[0][s], want, (seed, "restatement"))
        plain = [np.count_nonzero(q["tracked"]) for q in want["rate"]]
        assert all(0 < c for c in plain), plain                                # the masks leave trajectories alive


@gpu
def test_segment_0_from_the_host_and_the_others_from_the_device(ctx, dev, segs, job_a):
    group = [segs[seed] for seed in CASE.seeds[:3]]
    flows, occs, frames = device_inputs(group, dev)
    job = sfa.TrackJob(ctx, CASE.params(use_occlusions=1))
    for r in range(CASE.K):
        job.upload_flows(0, r, *group[0]["flows"][r], occ=group[0]["occ"][r])
        job.upload_occlusions_device(r, occs[r][1:], s0=1)
        job.upload_flows_device(r, flows[r][0][1:], flows[r][1][1:], s0=1)
    job.upload_frames(0, group[0]["frames"])
    job.upload_frames_device(frames[1:], s0=1)
    job.run(3)
    for s in range(3):
        assert_same(collect(job, s), job_a[0][s], s)
    job.close()


@gpu
def test_track_with_occlusions_and_rates_on_a_side_stream_equals_the_host_route(ctx, dev, segs, job_a):
    from slowflow_amd import device as sfd
    group = [segs[seed] for seed in CASE.seeds[:3]]
    params = CASE.params(use_occlusions=1)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):                                           # the inputs are produced on the side stream that is passed on
        flows, occs, frames = device_inputs(group, dev)
        got = sfd.track(ctx, params, flows, frames, occlusions=occs, rates=True, stream=side)
    side.synchronize()
    assert len(got) == 5
    flow, slot, occ, stats = (t.cpu().numpy() for t in got[:4])
    best = got[4]["best"].cpu().numpy()
    for s, want in enumerate(job_a[0]):
        f = want["fused"]
        assert same(flow[s, 0], f["u"]) and same(flow[s, 1], f["v"]) and same(slot[s], f["slot"]) and same(occ[s], f["occ"]), s
        assert stats[s, 0] == f["energy"] and stats[s, 1] == f["bound"] and stats[s, 2] == f["iters"], s
        assert same(best[s], f["best"]), s
        for r in range(CASE.K):
            d = {k: t.cpu().numpy() for k, t in got[4]["rate"][r].items()}
            w = want["rate"][r]
            assert same(d["acc"][s, 0], w["u"]) and same(d["acc"][s, 1], w["v"]), (s, r)
            assert same(d["tracked"][s], w["tracked"]) and same(d["energy"][s], w["energy"]) and same(d["occluded"][s], w["occluded"]), (s, r)
            assert same(d["occ_bits"][s].view(np.uint64), w["occ_bits"]), (s, r)
    with pytest.raises(sfa.SlowflowError, match="occlusions.*use_occlusions"):
        sfd.track(ctx, params, flows, frames)
    with pytest.raises(sfa.SlowflowError, match="occlusions.*use_occlusions"):
        sfd.track(ctx, CASE.params(), flows, frames, occlusions=occs)
    assert len(sfd.track(ctx, CASE.params(), flows, frames)) == 4           # the defaults: today's four values


def loaded_hip_runtime():
    """the HIP runtime this process already uses (torch's), by the path it was mapped from"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime is loaded")


class Claimed:
    """an object that claims a view of device memory through __cuda_array_interface__"""

    def __init__(self, ptr, shape, strides, typestr, dev):
        self.device = dev
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 3,
                                         "strides": tuple(int(s) for s in strides)}


@gpu
def test_refusals_name_their_argument_and_leave_the_job_as_it_was(ctx, dev, segs, job_a):
    case = CASE
    group = [segs[seed] for seed in case.seeds[:3]]
    flows, occs, frames = device_inputs(group, dev)
    job = sfa.TrackJob(ctx, case.params(use_occlusions=1))
    upload_device(job, flows, occs, frames)
    gpl = case.gh * case.gw

    def refused(call, *words):
        with pytest.raises(sfa.SlowflowError) as e:
            call()
        assert all(w in str(e.value) for w in words), str(e.value)
        job.run(3)                                                          # the job is as it was: job A's bits
        for s in range(3):
            assert_same(collect(job, s), job_a[0][s], (words, s))

    plain = sfa.TrackJob(ctx, case.params())
    refused(lambda: plain.upload_occlusions_device(1, occs[1]), "sfa_track_job_upload_occlusions_device", "use_occlusions")
    plain.close()
    refused(lambda: job.upload_occlusions_device(1, occs[1].to(torch.int16)), "occ", "i2")
    refused(lambda: job.upload_occlusions_device(1, occs[1].to(torch.float64)), "occ", "f8")
    refused(lambda: job.upload_occlusions_device(1, occs[1].cpu()), "occ", "cpu")
    L = sfa.lib()
    st = (C.c_longlong * 4)(*occs[1].stride())
    for dtype in (2, 9):                                                    # u16 and no type at all, at the C call
        assert L.sfa_track_job_upload_occlusions_device(job.h_, 0, 3, 1, C.c_void_p(occs[1].data_ptr()), dtype, st) == -1
        assert "dtype %d" % dtype in L.sfa_last_error(ctx.h).decode()
    # a view one row too long for its allocation: an allocation of the runtime's own (torch's allocator hands out parts of larger ones), the view at its end
    hip = loaded_hip_runtime()
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    sw, sh, rJ, size = case.source(1)[0], case.source(1)[1], case.r_Jets[1], 2 << 20
    mem = C.c_void_p()
    assert hip.hipMalloc(C.byref(mem), size) == 0
    try:
        inside = Claimed(mem.value + size - 3 * rJ * sh * sw, (3, rJ, sh, sw), (rJ * sh * sw, sh * sw, sw, 1), "|u1", dev)
        job.upload_occlusions_device(1, inside)                             # ends on the allocation's last byte: accepted
        job.upload_occlusions_device(1, occs[1])
        longer = Claimed(mem.value + size - 3 * rJ * sh * sw + sw, (3, rJ, sh, sw), (rJ * sh * sw, sh * sw, sw, 1), "|u1", dev)
        refused(lambda: job.upload_occlusions_device(1, longer), "occ_dev", "beyond its allocation")
    finally:
        ctx.sync()
        assert hip.hipFree(mem) == 0
    refused(lambda: job.upload_occlusions_device(case.K, occs[2]), "r = %d" % case.K)
    refused(lambda: job.upload_occlusions_device(1, occs[1][:2], s0=2), "s0 = 2, ns = 2")
    refused(lambda: job.download_rate_device(case.K, tracked=torch.empty((3, case.gh, case.gw), dtype=torch.int32, device=dev)), "r = %d" % case.K)
    one = torch.empty((3, 1, case.gh, case.gw), dtype=torch.float64, device=dev)
    refused(lambda: job.download_rate_device(1, acc=one.expand(3, 2, case.gh, case.gw)), "acc_dev", "share an address")     # a zero u|v stride
    energy = torch.empty((3, case.gh, case.gw), dtype=torch.float64, device=dev)
    tracked = energy.view(-1).view(torch.int32)[gpl:4 * gpl].view(3, case.gh, case.gw)
    refused(lambda: job.download_rate_device(1, tracked=tracked, energy=energy), "tracked_dev and energy_dev overlap")
    refused(lambda: job.download_best_device(torch.empty((4, case.gh, case.gw), dtype=torch.uint8, device=dev)), "s0 = 0, ns = 4")
    job.close()
