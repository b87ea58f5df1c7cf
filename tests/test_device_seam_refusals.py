"""The device entry points' refusals through the C-ABI (ctypes: strides no tensor library would hand over), one table per entry point that goes through
check_view / check_disjoint (slowflow_amd/csrc/api.hip on dev_view.h).  Every case: status -1 and a message that names the function and the argument;
after a sync every destination still holds the sentinel it was filled with; one valid call on the same objects then succeeds and gives what it gave before
any refusal.

Every refused view lies inside one live allocation, element for element as a kernel would address it if the check were broken (a negative stride starts
on the last row or plane of its tensor; zero strides and overlaps stay inside by construction), so a regression shows as a failed assertion.  Views that
leave their allocation or the 64-bit range cannot be built that way: tests/host/test_dev_view.cpp and tests/test_device_io.py hold those.

Shapes: 4 wide, 5 high (the pair job takes h >= 5), two windows / pairs / frames / groups; the multi-frame job 6 x 6, the smallest image its pyramid
rule gives one level; the track job on track_inputs.T1.  sfa_job_set_flow_device's start flow is read by a run only, so its valid call is the start
flow, one short run and a download."""
import ctypes as C

import numpy as np
import pytest

import slowflow_amd as sfa
import track_inputs as ti
from slowflow_amd import device

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H, N = 4, 5, 2
PL = W * H
JOB_W, JOB_H = 6, 6                                 # sfa_job_create: floor(0.9 w) and floor(0.9 h) above the pyramid filter's order + 1
SENTINEL = 7                                        # a value every destination's element type holds


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def ll(*v):
    return (C.c_longlong * len(v))(*v)


def at(t, *index):
    """the address of element `index` of a tensor"""
    return t.data_ptr() + sum(i * s for i, s in zip(index, t.stride())) * t.element_size()


def run_cases(ctx, fn, cases, dests, valid):
    """cases: (what, argument named, () -> status); dests: the tensors a broken check could let a kernel write; valid: () -> the valid call's result"""
    L = device._lib()
    L.sfa_last_error.restype = C.c_char_p
    before = valid()
    for what, arg, call in cases:
        for d in dests:
            d.fill_(SENTINEL)
        torch.cuda.synchronize()
        rc = call()
        msg = L.sfa_last_error(ctx.h).decode()
        assert rc == -1 and fn in msg and arg in msg, (what, rc, msg)
        ctx.sync()
        torch.cuda.synchronize()
        for d in dests:
            assert bool((d == SENTINEL).all()), (what, "a destination was written")
        again = valid()
        assert len(again) == len(before) and all(np.array_equal(a, b) for a, b in zip(again, before)), what


def flow_source_cases(call, flow, host):
    """the refusals of a read view: flow = a contiguous tensor [N,2,h,w], call(pointer, strides) -> status.  A null pointer is no refusal here: it asks for zeros"""
    h, w = flow.shape[2:]
    pl = h * w
    return [("null strides", "flow_dev", lambda: call(flow.data_ptr(), None)),
            ("negative row stride", "flow_dev", lambda: call(at(flow, 0, 0, h - 1, 0), ll(2 * pl, pl, -w, 1))),
            ("negative window stride", "flow_dev", lambda: call(at(flow, N - 1, 0, 0, 0), ll(-2 * pl, pl, w, 1))),
            ("column stride 0", "flow_dev", lambda: call(flow.data_ptr(), ll(2 * pl, pl, w, 0))),
            ("host pointer", "flow_dev", lambda: call(host.ctypes.data, ll(2 * pl, pl, w, 1)))]


def flow_destination_cases(call, flow, host):
    """the refusals of a written view: flow = a contiguous tensor [N,2,h,w], call(pointer, strides) -> status"""
    h, w = flow.shape[2:]
    pl = h * w
    return [("null pointer", "flow_dev", lambda: call(None, ll(2 * pl, pl, w, 1)))] + flow_source_cases(call, flow, host) + [
        ("window stride 0", "flow_dev", lambda: call(flow.data_ptr(), ll(0, pl, w, 1))),
        ("plane stride 0", "flow_dev", lambda: call(flow.data_ptr(), ll(2 * pl, 0, w, 1))),
        ("rows closer than the width", "flow_dev", lambda: call(flow.data_ptr(), ll(2 * pl, pl, w - 1, 1)))]


# ---- the multi-frame job and the pair job -------------------------------------------------------------------------------------------------
def small_job(ctx):
    """one level, two outer iterations of 5 sweeps, no occlusion step: a run of a few launches"""
    p = sfa.default_params()
    p.S, p.layers, p.niter_alter, p.niter_outer, p.niter_inner, p.niter_solver = 2, 1, 1, 2, 1, 5
    p.thres_outer, p.thres_inner, p.occlusion_reasoning, p.hbit = 0, 0, 0, 0
    p.rho[0], p.omega[0] = 1, 0
    return sfa.Job(ctx, p, JOB_W, JOB_H, N)


def test_job_set_flow_device(ctx, dev):
    L, fn = device._lib(), "sfa_job_set_flow_device"
    w, h, pl = JOB_W, JOB_H, JOB_W * JOB_H
    job = small_job(ctx)
    rng = np.random.default_rng(3)
    frames = torch.from_numpy(rng.standard_normal((N, 3, 3, h, w)).astype(np.float32)).to(dev)
    flow = torch.from_numpy(rng.uniform(-1, 1, (N, 2, h, w)).astype(np.float32)).to(dev)
    out = torch.empty((N, 2, h, w), device=dev)
    host = np.zeros((N, 2, h, w), np.float32)
    torch.cuda.synchronize()

    def call(ptr, st):
        return L.sfa_job_set_flow_device(job.h_, 0, N, C.c_void_p(ptr), st)

    def valid():
        """the start flow, a run from it, the result: what a refusal must leave as it was"""
        job.upload_device(frames)
        assert call(flow.data_ptr(), ll(2 * pl, pl, w, 1)) == 0
        job.run()
        job.download_device(out)
        ctx.sync()
        return [out.cpu().numpy()]
    try:
        run_cases(ctx, fn, flow_source_cases(call, flow, host), [out], valid)
        with_start = valid()[0]
        assert L.sfa_job_set_flow_device(job.h_, 0, N, None, None) == 0           # zeros instead: the result depends on the start flow
        job.run()
        job.download_device(out)
        ctx.sync()
        assert np.isfinite(with_start).all() and not np.array_equal(out.cpu().numpy(), with_start)
    finally:
        job.close()


def test_job_download_device(ctx, dev):
    L, fn = device._lib(), "sfa_job_download_device"
    w, h, pl = JOB_W, JOB_H, JOB_W * JOB_H
    job = small_job(ctx)
    flow = torch.empty((N, 2, h, w), device=dev)
    occ = torch.empty((N, h, w), device=dev)
    host = np.zeros((N, 2, h, w), np.float32)
    fst, ost = ll(2 * pl, pl, w, 1), ll(pl, w, 1)

    def call(ptr, st, optr=None, ost_=None):
        return L.sfa_job_download_device(job.h_, 0, N, C.c_void_p(ptr), st, C.c_void_p(optr), ost_)

    def with_occ(optr, ost_):
        return call(flow.data_ptr(), fst, optr, ost_)

    def valid():
        assert call(flow.data_ptr(), fst, occ.data_ptr(), ost) == 0
        ctx.sync()
        return [flow.cpu().numpy(), occ.cpu().numpy()]
    cases = flow_destination_cases(call, flow, host) + [
        ("occ: null strides", "occ_dev", lambda: with_occ(occ.data_ptr(), None)),
        ("occ: negative row stride", "occ_dev", lambda: with_occ(at(occ, 0, h - 1, 0), ll(pl, -w, 1))),
        ("occ: column stride 0", "occ_dev", lambda: with_occ(occ.data_ptr(), ll(pl, w, 0))),
        ("occ: host pointer", "occ_dev", lambda: with_occ(host.ctypes.data, ost)),
        ("occ: window stride 0", "occ_dev", lambda: with_occ(occ.data_ptr(), ll(0, w, 1))),
        ("occ laid over u", "occ_dev", lambda: with_occ(flow.data_ptr(), ll(2 * pl, w, 1)))]
    try:
        run_cases(ctx, fn, cases, [flow, occ], valid)
        assert not valid()[0].any() and bool((flow == 0).all())     # a job that has not run holds zeros: the valid call did write over the sentinel
    finally:
        job.close()


def test_pair_job_set_flow_and_download_device(ctx, dev):
    L = device._lib()
    job = sfa.PairJob(ctx, W, H, N)
    start = torch.arange(N * 2 * PL, dtype=torch.float32, device=dev).reshape(N, 2, H, W)
    out = torch.empty((N, 2, H, W), device=dev)
    host = np.zeros((N, 2, H, W), np.float32)
    dense = ll(2 * PL, PL, W, 1)

    def set_flow(ptr, st):
        return L.sfa_pair_job_set_flow_device(job.h_, 0, N, C.c_void_p(ptr), st)

    def download(ptr, st):
        return L.sfa_pair_job_download_device(job.h_, 0, N, C.c_void_p(ptr), st)

    def valid():
        assert set_flow(start.data_ptr(), dense) == 0 and download(out.data_ptr(), dense) == 0
        ctx.sync()
        return [out.cpu().numpy()]
    try:
        assert np.array_equal(valid()[0], start.cpu().numpy())       # what goes in comes out: the refusals below are watched through this pair of calls
        run_cases(ctx, "sfa_pair_job_set_flow_device", flow_source_cases(set_flow, start, host), [out], valid)
        run_cases(ctx, "sfa_pair_job_download_device", flow_destination_cases(download, out, host), [out], valid)
    finally:
        job.close()


# ---- frames into a sequence ------------------------------------------------------------------------------------------------------------------
def test_sequence_upload_device(ctx, dev):
    L, fn = device._lib(), "sfa_sequence_upload_device"
    seq = sfa.Sequence(ctx, W, H, N)
    frames = torch.arange(N * 3 * PL, dtype=torch.float32, device=dev).reshape(N, 3, H, W)
    host = np.zeros((N, 3, H, W), np.float32)

    def layout(**kw):
        lay = device.DevLayout(0, 0, 3 * PL, PL, W, 1)
        for k, v in kw.items():
            setattr(lay, k, v)
        return lay

    def call(ptr, lay):
        return L.sfa_sequence_upload_device(seq.h_, 0, N, C.c_void_p(ptr), C.byref(lay) if lay is not None else None)

    def valid():
        assert call(frames.data_ptr(), layout()) == 0
        ctx.sync()
        return [seq.download(f)[:, :, :W] for f in range(N)]
    cases = [("null pointer", "frames_dev", lambda: call(None, layout())),
             ("null layout", "layout", lambda: call(frames.data_ptr(), None)),
             ("negative row stride", "layout.row", lambda: call(at(frames, 0, 0, H - 1, 0), layout(row=-W))),
             ("negative frame stride", "layout.frame", lambda: call(at(frames, N - 1, 0, 0, 0), layout(frame=-3 * PL))),
             ("negative channel stride", "layout.channel", lambda: call(at(frames, 0, 2, 0, 0), layout(channel=-PL))),
             ("column stride 0", "layout.column", lambda: call(frames.data_ptr(), layout(column=0))),
             ("host pointer", "frames_dev", lambda: call(host.ctypes.data, layout()))]
    try:
        assert np.array_equal(np.stack(valid()), frames.cpu().numpy())
        run_cases(ctx, fn, cases, [], valid)
    finally:
        seq.close()


# ---- the Bayer ingest -----------------------------------------------------------------------------------------------------------------------
def test_demosaic_device(ctx, dev):
    L, fn = device._lib(), "sfa_demosaic_device"
    both = torch.empty(N * PL + N * 3 * PL, device=dev)              # the mosaics and, behind them, the frames: one allocation for the overlap case
    mosaic, dst = both[:N * PL].view(N, H, W), both[N * PL:].view(N, 3, H, W)
    pattern = (torch.arange(N * PL, dtype=torch.float32, device=dev) * 37 % 251).view(N, H, W)
    host = np.zeros((N, 3, H, W), np.float32)
    dense = ll(3 * PL, PL, W, 1)

    def desc(**kw):
        d = device.MosaicDesc(0, PL, W, 1, W, H, 0, 0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(src, d, to, st, w=W, h=H):
        return L.sfa_demosaic_device(ctx.h, N, C.c_void_p(src), C.byref(d) if d is not None else None, 0, 1, 0, C.c_void_p(to), st, w, h)

    def source(src, d):
        return call(src, d, dst.data_ptr(), dense)

    def dest(to, st, w=W, h=H):
        return call(mosaic.data_ptr(), desc(), to, st, w, h)

    def valid():
        mosaic.copy_(pattern)
        torch.cuda.synchronize()
        assert source(mosaic.data_ptr(), desc()) == 0
        ctx.sync()
        return [dst.cpu().numpy()]
    cases = [("mosaic: null pointer", "mosaic_dev", lambda: source(None, desc())),
             ("mosaic: null descriptor", "desc", lambda: source(mosaic.data_ptr(), None)),
             ("mosaic: negative row stride", "desc.row", lambda: source(at(mosaic, 0, H - 1, 0), desc(row=-W))),
             ("mosaic: negative frame stride", "desc.frame", lambda: source(at(mosaic, N - 1, 0, 0), desc(frame=-PL))),
             ("mosaic: column stride 0", "desc.column", lambda: source(mosaic.data_ptr(), desc(column=0))),
             ("mosaic: host pointer", "mosaic_dev", lambda: source(host.ctypes.data, desc())),
             ("dst: null pointer", "dst_dev", lambda: dest(None, dense)),
             ("dst: null strides", "dst_dev", lambda: dest(dst.data_ptr(), None)),
             ("dst: negative row stride", "dst_dev", lambda: dest(at(dst, 0, 0, H - 1, 0), ll(3 * PL, PL, -W, 1))),
             ("dst: column stride 0", "dst_dev", lambda: dest(dst.data_ptr(), ll(3 * PL, PL, W, 0))),
             ("dst: host pointer", "dst_dev", lambda: dest(host.ctypes.data, dense)),
             ("dst: frame stride 0", "dst_dev", lambda: dest(dst.data_ptr(), ll(0, PL, W, 1))),
             ("dst: channel stride 0", "dst_dev", lambda: dest(dst.data_ptr(), ll(3 * PL, 0, W, 1))),
             ("dst: 3 x 2 at (2, 3)", "dst_dev", lambda: dest(dst.data_ptr(), ll(24, 8, 2, 3), w=2, h=3)),      # six distinct addresses per plane; refused all the same
             ("dst laid over the mosaics", "dst_dev", lambda: dest(both.data_ptr(), dense))]
    run_cases(ctx, fn, cases, [both], valid)


# ---- the track job -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def track(ctx, dev):
    """a T1 job with two segments uploaded from device tensors and run once"""
    case = ti.T1
    segs = [ti.segment(case, seed) for seed in case.seeds[:N]]
    flows = []
    for r in range(case.K):
        sw = case.source(r)[0]
        fwd = np.stack([np.stack([seg["flows"][r][0][..., :sw], seg["flows"][r][1][..., :sw]], 1) for seg in segs])
        bwd = np.stack([np.stack([seg["flows"][r][2][..., :sw], seg["flows"][r][3][..., :sw]], 1) for seg in segs])
        flows.append(torch.from_numpy(np.stack([fwd, bwd])).to(dev))           # [2][ns][rJ][2][sh][sw]: one layout for the two directions
    frames = torch.from_numpy(np.stack([seg["frames"][..., :case.w] for seg in segs])).to(dev)
    torch.cuda.synchronize()
    job = sfa.TrackJob(ctx, case.params())
    for r in range(case.K):
        job.upload_flows_device(r, flows[r][0], flows[r][1])
    job.upload_frames_device(frames)
    job.run(N)
    yield job, flows, frames
    job.close()


def fused(job):
    job.run(N)
    out = [job.download_fused(s) for s in range(N)]
    return [np.asarray(o[k]) for o in out for k in ("slot", "u", "v", "occ", "best", "energy", "bound", "iters")]


def test_track_job_upload_flows_device(ctx, track):
    L, fn = device._lib(), "sfa_track_job_upload_flows_device"
    job, flows, _ = track
    r = 1
    fwd, bwd = flows[r][0], flows[r][1]
    st = ll(*fwd.stride())
    host = np.zeros(tuple(fwd.shape), np.float32)
    rows = fwd.shape[3]

    def call(f, b, strides):
        return L.sfa_track_job_upload_flows_device(job.h_, 0, N, r, C.c_void_p(f), C.c_void_p(b), strides)

    def valid():
        assert call(fwd.data_ptr(), bwd.data_ptr(), st) == 0
        return fused(job)
    s = fwd.stride()
    cases = [("fwd: null pointer", "fwd_dev", lambda: call(None, bwd.data_ptr(), st)),
             ("bwd: null pointer", "bwd_dev", lambda: call(fwd.data_ptr(), None, st)),
             ("null strides", "fwd_dev", lambda: call(fwd.data_ptr(), bwd.data_ptr(), None)),
             ("negative row stride", "fwd_dev", lambda: call(at(fwd, 0, 0, 0, rows - 1, 0), at(bwd, 0, 0, 0, rows - 1, 0), ll(s[0], s[1], s[2], -s[3], 1))),
             ("negative segment stride", "fwd_dev", lambda: call(at(fwd, N - 1, 0, 0, 0, 0), at(bwd, N - 1, 0, 0, 0, 0), ll(-s[0], s[1], s[2], s[3], 1))),
             ("column stride 0", "fwd_dev", lambda: call(fwd.data_ptr(), bwd.data_ptr(), ll(s[0], s[1], s[2], s[3], 0))),
             ("fwd: host pointer", "fwd_dev", lambda: call(host.ctypes.data, bwd.data_ptr(), st)),
             ("bwd: host pointer", "bwd_dev", lambda: call(fwd.data_ptr(), host.ctypes.data, st))]
    run_cases(ctx, fn, cases, [], valid)


def test_track_job_upload_frames_device(ctx, track):
    L, fn = device._lib(), "sfa_track_job_upload_frames_device"
    job, _, frames = track
    s = frames.stride()
    st = ll(*s)
    host = np.zeros(tuple(frames.shape), np.float32)

    def call(ptr, strides):
        return L.sfa_track_job_upload_frames_device(job.h_, 0, N, C.c_void_p(ptr), strides)

    def valid():
        assert call(frames.data_ptr(), st) == 0
        return fused(job)
    cases = [("null pointer", "frames_dev", lambda: call(None, st)),
             ("null strides", "frames_dev", lambda: call(frames.data_ptr(), None)),
             ("negative row stride", "frames_dev", lambda: call(at(frames, 0, 0, 0, frames.shape[3] - 1, 0), ll(s[0], s[1], s[2], -s[3], 1))),
             ("negative channel stride", "frames_dev", lambda: call(at(frames, 0, 0, 2, 0, 0), ll(s[0], s[1], -s[2], s[3], 1))),
             ("column stride 0", "frames_dev", lambda: call(frames.data_ptr(), ll(s[0], s[1], s[2], s[3], 0))),
             ("host pointer", "frames_dev", lambda: call(host.ctypes.data, st))]
    run_cases(ctx, fn, cases, [], valid)


def test_track_job_download_device(ctx, dev, track):
    L, fn = device._lib(), "sfa_track_job_download_device"
    job = track[0]
    gh, gw = job.gh, job.gw
    g = gh * gw
    flow = torch.empty((N, 2, gh, gw), dtype=torch.float64, device=dev)
    slot = torch.empty((N, gh, gw), dtype=torch.int32, device=dev)
    occ = torch.empty((N, gh, gw), dtype=torch.uint8, device=dev)
    stats = torch.empty((N, 3), dtype=torch.float64, device=dev)
    spare = torch.empty(N * g, dtype=torch.int32, device=dev)        # room for N x g int32, N x g bytes or 3 N doubles: the overlap cases' second argument
    host = np.zeros((N, 2, gh, gw), np.float64)
    dense = ll(2 * g, g, gw, 1)

    def call(f, st, sl=None, oc=None, sa=None):
        return L.sfa_track_job_download_device(job.h_, 0, N, C.c_void_p(f), st, C.c_void_p(sl), C.c_void_p(oc), C.c_void_p(sa))

    def valid():
        job.run(N)
        assert call(flow.data_ptr(), dense, slot.data_ptr(), occ.data_ptr(), stats.data_ptr()) == 0
        ctx.sync()
        return [t.cpu().numpy() for t in (flow, slot, occ, stats)]
    cases = [("flow: null pointer", "flow_dev", lambda: call(None, dense)),
             ("flow: null strides", "flow_dev", lambda: call(flow.data_ptr(), None)),
             ("flow: negative row stride", "flow_dev", lambda: call(at(flow, 0, 0, gh - 1, 0), ll(2 * g, g, -gw, 1))),
             ("flow: negative segment stride", "flow_dev", lambda: call(at(flow, N - 1, 0, 0, 0), ll(-2 * g, g, gw, 1))),
             ("flow: column stride 0", "flow_dev", lambda: call(flow.data_ptr(), ll(2 * g, g, gw, 0))),
             ("flow: host pointer", "flow_dev", lambda: call(host.ctypes.data, dense)),
             ("slot: host pointer", "slot_dev", lambda: call(flow.data_ptr(), dense, sl=host.ctypes.data)),
             ("occ: host pointer", "occ_dev", lambda: call(flow.data_ptr(), dense, oc=host.ctypes.data)),
             ("stats: host pointer", "stats_dev", lambda: call(flow.data_ptr(), dense, sa=host.ctypes.data)),
             ("flow: segment stride 0", "flow_dev", lambda: call(flow.data_ptr(), ll(0, g, gw, 1))),
             ("flow: u and v at one address", "flow_dev", lambda: call(flow.data_ptr(), ll(2 * g, 0, gw, 1))),
             ("flow: rows closer than the width", "flow_dev", lambda: call(flow.data_ptr(), ll(2 * g, g, gw - 1, 1))),
             ("slot laid over the flow", "slot_dev", lambda: call(flow.data_ptr(), dense, sl=flow.data_ptr())),
             ("occ laid over slot", "occ_dev", lambda: call(flow.data_ptr(), dense, sl=spare.data_ptr(), oc=spare.data_ptr())),
             ("stats laid over occ", "stats_dev", lambda: call(flow.data_ptr(), dense, oc=spare.data_ptr(), sa=spare.data_ptr()))]
    assert N * g * 4 >= 3 * N * 8
    run_cases(ctx, fn, cases, [flow, slot, occ, stats, spare], valid)


# ---- grouped flow-magnitude quantiles ---------------------------------------------------------------------------------------------------------
def test_flow_magnitude_quantiles_device(ctx, dev):
    L, fn = device._lib(), "sfa_flow_magnitude_quantiles_device"
    n = 2
    flow = torch.empty((N, n, 2, H, W), device=dev)
    values = torch.from_numpy(np.random.default_rng(5).standard_normal((N, n, 2, H, W)).astype(np.float32)).to(dev)
    out = torch.empty((N, 2), dtype=torch.float64, device=dev)
    host = np.zeros((N, n, 2, H, W), np.float32)
    dense = ll(n * 2 * PL, 2 * PL, W, 1)
    u, v = flow.data_ptr(), at(flow, 0, 0, 1, 0, 0)

    def call(up, vp, st, op, w=W, h=H):
        return L.sfa_flow_magnitude_quantiles_device(ctx.h, N, n, None, C.c_void_p(up), C.c_void_p(vp), st, w, h, 1.0, 0.9, C.c_void_p(op))

    def valid():
        flow.copy_(values)
        torch.cuda.synchronize()
        assert call(u, v, dense, out.data_ptr()) == 0
        ctx.sync()
        return [out.cpu().numpy()]
    cases = [("u: null pointer", "u_dev", lambda: call(None, v, dense, out.data_ptr())),
             ("v: null pointer", "v_dev", lambda: call(u, None, dense, out.data_ptr())),
             ("out: null pointer", "out_dev", lambda: call(u, v, dense, None)),
             ("null strides", "strides", lambda: call(u, v, None, out.data_ptr())),
             ("negative field stride", "u_dev", lambda: call(at(flow, 0, n - 1, 0, 0, 0), at(flow, 0, n - 1, 1, 0, 0), ll(n * 2 * PL, -2 * PL, W, 1), out.data_ptr())),
             ("negative group stride", "u_dev", lambda: call(at(flow, N - 1, 0, 0, 0, 0), at(flow, N - 1, 0, 1, 0, 0), ll(-n * 2 * PL, 2 * PL, W, 1), out.data_ptr())),
             ("column stride 0", "strides", lambda: call(u, v, ll(n * 2 * PL, 2 * PL, W, 0), out.data_ptr())),
             ("u: host pointer", "u_dev", lambda: call(host.ctypes.data, v, dense, out.data_ptr())),
             ("out: host pointer", "out_dev", lambda: call(u, v, dense, host.ctypes.data)),
             ("field stride 0", "strides", lambda: call(u, v, ll(n * 2 * PL, 0, W, 1), out.data_ptr())),
             ("3 x 2 at (2, 3)", "strides", lambda: call(u, v, ll(n * 2 * PL, 2 * PL, 2, 3), out.data_ptr(), w=2, h=3)),   # distinct addresses; refused all the same
             ("out laid over u", "out_dev", lambda: call(u, v, dense, flow.data_ptr())),
             ("out laid over v", "v_dev", lambda: call(u, v, dense, at(flow, N - 1, n - 1, 1, 0, 0)))]
    run_cases(ctx, fn, cases, [out], valid)
    got = valid()[0]
    assert np.isfinite(got).all() and (got[:, 0] <= got[:, 1]).all() and (got[:, 1] > 0).all()     # quantile <= maximum: the valid call did write over the sentinel
