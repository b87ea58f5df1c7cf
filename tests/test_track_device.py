"""The track job's device seam (slowflow_amd/device.py: track, track_job_upload_*_device, track_job_download_device): T1's inputs as torch tensors that
are not contiguous, produced on a side stream, give exactly what the host-upload job downloads."""
import numpy as np
import pytest

import slowflow_amd as sfa
import track_inputs as ti
from slowflow_amd import device as sfd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def segs():
    return [ti.segment(ti.T1, seed) for seed in ti.T1.seeds[:3]]


@pytest.fixture(scope="module")
def host_result(ctx, segs):
    """the host-upload job's downloads of the three segments"""
    case = ti.T1
    job = sfa.TrackJob(ctx, case.params())
    for s, seg in enumerate(segs):
        for r in range(case.K):
            job.upload_flows(s, r, *seg["flows"][r])
        job.upload_frames(s, seg["frames"])
    job.run(3)
    out = [job.download_fused(s) for s in range(3)]
    job.close()
    return out


def padded(a, dev, pad=(1, 2)):
    """a numpy array as a view into a larger device tensor: one extra plane in front and pad rows / columns around the last two dimensions"""
    big = torch.full((a.shape[0] + 1,) + tuple(a.shape[1:-2]) + (a.shape[-2] + 2 * pad[0], a.shape[-1] + 2 * pad[1]), 7e29, dtype=torch.float32, device=dev)
    view = big[1:, ..., pad[0]:pad[0] + a.shape[-2], pad[1]:pad[1] + a.shape[-1]]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    assert not view.is_contiguous()
    return view


def device_inputs(segs, dev, permuted_frames):
    """flows[r] = (fwd, bwd) [ns, r_Jets, 2, sh, sw] and frames [ns, Jets + 1, 3, h, w], none of them contiguous"""
    case = ti.T1
    flows = []
    for r in range(case.K):
        sw = case.source(r)[0]
        fwd = np.stack([np.stack([seg["flows"][r][0][..., :sw], seg["flows"][r][1][..., :sw]], 1) for seg in segs])
        bwd = np.stack([np.stack([seg["flows"][r][2][..., :sw], seg["flows"][r][3][..., :sw]], 1) for seg in segs])
        both = padded(np.stack([fwd, bwd]), dev)                            # one layout for the two directions
        flows.append((both[0], both[1]))
    fr = np.stack([seg["frames"][..., :case.w] for seg in segs])
    if permuted_frames:                                                     # stored channels-last, passed as the permuted view
        frames = torch.from_numpy(np.ascontiguousarray(fr.transpose(0, 1, 3, 4, 2))).to(dev).permute(0, 1, 4, 2, 3)
        assert not frames.is_contiguous()
    else:
        frames = padded(fr, dev)
    return flows, frames


def check(got, want):
    flow, slot, occ, stats = (t.cpu().numpy() for t in got)
    for s, w in enumerate(want):
        assert np.array_equal(flow[s, 0].view(np.uint64), w["u"].view(np.uint64)) and np.array_equal(flow[s, 1].view(np.uint64), w["v"].view(np.uint64)), s
        assert np.array_equal(slot[s], w["slot"]) and np.array_equal(occ[s], w["occ"]), s
        assert stats[s, 0] == w["energy"] and stats[s, 1] == w["bound"] and stats[s, 2] == w["iters"], s
    assert len({tuple(w["slot"].ravel()) for w in want}) == len(want)


@pytest.mark.parametrize("permuted_frames", [False, True])
def test_track_on_a_side_stream_equals_the_host_upload_job(ctx, segs, host_result, permuted_frames):
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):                                           # the inputs are produced on the side stream that is passed on
        flows, frames = device_inputs(segs, dev, permuted_frames)
        got = sfd.track(ctx, ti.T1.params(), flows, frames, stream=side)
    side.synchronize()
    check(got, host_result)


def test_half_from_the_host_and_half_from_the_device(ctx, segs, host_result):
    case = ti.T1
    dev = torch.device("cuda", 0)
    flows, frames = device_inputs(segs, dev, False)
    torch.cuda.synchronize()
    job = sfa.TrackJob(ctx, case.params())
    for r in range(case.K):                                                 # segment 0 from the host, 1 and 2 from the device
        job.upload_flows(0, r, *segs[0]["flows"][r])
        job.upload_flows_device(r, flows[r][0][1:], flows[r][1][1:], s0=1)
    job.upload_frames(0, segs[0]["frames"])
    job.upload_frames_device(frames[1:], s0=1)
    job.run(3)
    out = (torch.empty((3, 2, case.gh, case.gw), dtype=torch.float64, device=dev), torch.empty((3, case.gh, case.gw), dtype=torch.int32, device=dev),
           torch.empty((3, case.gh, case.gw), dtype=torch.uint8, device=dev), torch.empty((3, 3), dtype=torch.float64, device=dev))
    ctx.wait_stream(torch.cuda.current_stream(dev))
    job.download_device(*out)
    ctx.signal_stream(torch.cuda.current_stream(dev))
    check(out, host_result)
    job.close()


def test_other_element_types_and_host_tensors_are_refused_by_name(ctx, segs):
    dev = torch.device("cuda", 0)
    flows, frames = device_inputs(segs, dev, False)
    with pytest.raises(sfa.SlowflowError, match="frames.*f2"):
        sfd.track(ctx, ti.T1.params(), flows, frames.half())
    with pytest.raises(sfa.SlowflowError, match="frames.*cpu"):
        sfd.track(ctx, ti.T1.params(), flows, frames.cpu())
    job = sfa.TrackJob(ctx, ti.T1.params())
    with pytest.raises(sfa.SlowflowError, match="fwd.*f2"):
        job.upload_flows_device(1, flows[1][0].half(), flows[1][1])
    with pytest.raises(sfa.SlowflowError, match="bwd.*cpu"):
        job.upload_flows_device(1, flows[1][0], flows[1][1].cpu())
    job.close()


def test_download_destinations_that_share_addresses_are_refused(ctx, segs):
    case = ti.T1
    dev = torch.device("cuda", 0)
    job = sfa.TrackJob(ctx, case.params())
    one = torch.empty((3, 1, case.gh, case.gw), dtype=torch.float64, device=dev)
    with pytest.raises(sfa.SlowflowError, match="share an address"):
        job.download_device(one.expand(3, 2, case.gh, case.gw))              # u and v at one address
    flow = torch.empty((3, 2, case.gh, case.gw), dtype=torch.float64, device=dev)
    with pytest.raises(sfa.SlowflowError, match="flow_dev and stats_dev overlap"):
        job.download_device(flow, stats=flow.view(-1)[:9].view(3, 3))
    job.close()
