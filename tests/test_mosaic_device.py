"""Raw Bayer ingest on the GPU (csrc/mosaic.hip; include/slowflow_amd.h: sfa_demosaic_device, sfa_sequence_upload_mosaic*, sfa_job_set_raw_weights,
sfa_sequence_rescale; cfg key gpu_ingest).  The kernels restate the host routines statement by statement, so the condition throughout is bit identity:
np.array_equal against tests/mosaic_ref.py (held against the pinned host formulations in tests/test_mosaic.py), against the existing bindings, and byte
identity of the driver's output files between gpu_ingest 1 and 0."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import mosaic_ref as mr
import slowflow_amd as sfa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
TX, TY = sfa.MOSAIC_TILE                         # the kernels' tile (csrc/mosaic.hip: MOS_TX x MOS_TY)
SMALL = [(2, 2), (3, 2), (2, 7), (7, 2), (5, 4), (37, 22)]
TILES = [(TX + 1, TY + 1), (TX - 1, TY - 1), (2 * TX + 5, 2 * TY + 3)]       # one past the tile, one short of it, three tiles with a ragged edge
NP_DTYPES = {"f4": np.float32, "u1": np.uint8, "u2": np.uint16}


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def to_dev(a, dev):
    """numpy -> torch on the GPU (torch has no uint16 arithmetic, but it holds and exports the type)"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def mosaic(w, h, kind, method, seed=0, n=1):
    """n mosaics [n,h,w]: fp32 20..4000 (method 0) or -20..300 with exact halves, values below 0 and above 255 (method 2); u8 and u16 over their range
    (from 1 with method 0: a zero green is test 4's)"""
    rng = np.random.default_rng(1000 * seed + 7 * w + h + (3 if method else 0))
    if kind == "f4":
        if method == 0:
            return rng.uniform(20, 4000, (n, h, w)).astype(np.float32)
        m = rng.uniform(-20, 300, (n, h, w)).astype(np.float32)
        halves = np.array([0.5, 1.5, 2.5, 254.5, 255.5, -0.5, 127.5, 128.5], np.float32)
        flat = m.reshape(-1)
        idx = rng.permutation(flat.size)[:min(flat.size // 2, 8)]
        flat[idx] = halves[:idx.size]
        return m
    lo = 1 if method == 0 else 0
    return rng.integers(lo, 256 if kind == "u1" else 65536, (n, h, w)).astype(NP_DTYPES[kind])


@functools.lru_cache(maxsize=None)
def reference(w, h, kind, method, red, seed=0, n=1):
    return np.stack([mr.demosaic(m, red[0], red[1], method) for m in mosaic(w, h, kind, method, seed, n)])


def run_demosaic(ctx, dev, m, red, method, origin=(0, 0), size=None):
    from slowflow_amd import device
    out = device.demosaic(ctx, m if isinstance(m, torch.Tensor) else to_dev(m, dev), red, method, origin, size)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_sizes(ctx, dev, sizes, method):
    for (w, h) in sizes:
        for kind in ("f4", "u1", "u2"):
            m = to_dev(mosaic(w, h, kind, method), dev)
            for red in mr.REDS:
                got = run_demosaic(ctx, dev, m, red, method)
                want = reference(w, h, kind, method, red)
                assert got.shape == want.shape and got.dtype == np.float32
                assert np.array_equal(got, want), (w, h, kind, red, np.argwhere(got != want)[:4])


# ---- 1, 2. demosaic() against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [SMALL, TILES], ids=["small", "tile_edges"])
def test_method_0_equals_the_restatement(ctx, dev, sizes):
    check_sizes(ctx, dev, sizes, 0)


@pytest.mark.parametrize("sizes", [SMALL + [(1, 1), (2, 5), (3, 3)], TILES], ids=["small", "tile_edges"])
def test_method_2_equals_the_restatement(ctx, dev, sizes):
    check_sizes(ctx, dev, sizes, 2)
    if (3, 3) in sizes:
        for red in mr.REDS:                                                      # no interior: zeros; one interior pixel: copied everywhere
            assert not reference(1, 1, "u1", 2, red).any() and not reference(2, 5, "f4", 2, red).any()
            one = reference(3, 3, "u2", 2, red)[0]
            assert np.array_equal(one, np.broadcast_to(one[:, 1:2, 1:2], one.shape))


# ---- 3. crops of a strided view, three frames in one launch --------------------------------------------------------------------------------
W41, H29 = 41, 29
CROPS = [((0, 0), (20, 12)), ((1, 0), (20, 12)), ((0, 1), (20, 12)), ((3, 5), (20, 12)), ((W41 - 20, H29 - 12), (20, 12)), ((0, 0), (W41, H29))]


@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("kind", ["f4", "u1"])
def test_crops_equal_demosaic_then_slice(ctx, dev, method, kind):
    n, red = 3, (1, 0)
    m = mosaic(W41, H29, kind, method, seed=1, n=n)
    big = torch.zeros((n + 1, H29 + 3, W41 + 7), dtype=to_dev(m[:1], dev).dtype, device=dev)
    view = big[:n, 1:1 + H29, 2:2 + W41]                                       # row stride above W, frame stride above a frame
    view.copy_(to_dev(m, dev))
    assert view.stride(1) > W41 and view.stride(0) > view.stride(1) * H29
    full = reference(W41, H29, kind, method, red, seed=1, n=n)
    for origin, size in CROPS:
        got = run_demosaic(ctx, dev, view, red, method, origin, size)
        want = full[:, :, origin[1]:origin[1] + size[1], origin[0]:origin[0] + size[0]]
        assert np.array_equal(want[0], mr.demosaic_crop(m[0], red[0], red[1], method, origin, size))
        assert np.array_equal(got, want), (origin, size, np.argwhere(got != want)[:4])


# ---- 4. a zero green -----------------------------------------------------------------------------------------------------------------------
def test_zero_green_puts_inf_and_nan_where_the_host_does(ctx, dev):
    m = mosaic(14, 12, "f4", 0, seed=2)[0].copy()
    m[4:8, 5:9] = 0
    want = mr.bayer_gr(m, 1, 0)
    got = run_demosaic(ctx, dev, m[None], (1, 0), 0)[0]
    assert np.isnan(want).any()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.array_equal(got, want, equal_nan=True)


# ---- 5. sequence uploads -------------------------------------------------------------------------------------------------------------------
def host_planes(a, w):
    out = np.zeros(a.shape[:-1] + (sfa.stride_of(w),), np.float32)
    out[..., :w] = a
    return out


@pytest.mark.parametrize("method,kind,origin,size", [(0, "u2", (0, 0), (37, 22)), (2, "u1", (3, 5), (30, 16)), (0, "f4", (1, 1), (36, 21))])
def test_sequence_uploads_leave_the_bits_of_the_host_frames(ctx, dev, method, kind, origin, size):
    W, H, N, red = 37, 22, 3, (0, 1)
    w, h = size
    m = mosaic(W, H, kind, method, seed=3, n=N)
    want = np.stack([mr.demosaic_crop(m[f], red[0], red[1], method, origin, size) for f in range(N)])
    a, b, c = (sfa.Sequence(ctx, w, h, N) for _ in range(3))
    try:
        ctx.wait_stream()
        a.upload_mosaic_device(to_dev(m, dev), red, method, origin=origin, size=size)
        for f in range(N):
            b.upload_mosaic(f, m[f], red, method, origin)
            c.upload(f, host_planes(want[f], w))
        for f in range(N):
            ref = c.download(f)
            assert np.array_equal(ref[:, :, :w], want[f])
            assert np.array_equal(a.download(f).view(np.uint32), ref.view(np.uint32)) and np.array_equal(b.download(f).view(np.uint32), ref.view(np.uint32))
        sa, sb, sc = a.normalize(), b.normalize(), c.normalize()
        assert sa == sc and sb == sc
        assert np.array_equal(a.download(1).view(np.uint32), c.download(1).view(np.uint32))
    finally:
        a.close(); b.close(); c.close()


# ---- 6. rescale ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.5, 0.25, 0.3])
def test_rescale_equals_blur_and_resize_per_channel(ctx, dev, scale):
    w, h, N = 64, 48, 2
    rng = np.random.default_rng(5)
    frames = host_planes(rng.uniform(0, 255, (N, 3, h, w)).astype(np.float32), w)
    dw, dh = mr.rescaled_size(w, h, scale)
    fx, sigma = float(np.float32(scale)), mr.rescale_sigma(scale)
    src, dst = sfa.Sequence(ctx, w, h, N), sfa.Sequence(ctx, dw, dh, N)
    try:
        for f in range(N):
            src.upload(f, frames[f])
        dst.rescale_from(src, scale)
        for f in range(N):
            got = dst.download(f)
            for k in range(3):
                want, ww = ctx.resize_linear_fx(ctx.gaussian_blur(frames[f, k], w, sigma), w, fx, fx)
                assert ww == dw and want.shape[0] == dh
                assert np.array_equal(got[k, :, :dw], want[:, :dw]), (scale, f, k)
    finally:
        src.close(); dst.close()


# ---- 7. weights ----------------------------------------------------------------------------------------------------------------------------
def make_weight_job(ctx, w, h, stride):
    """a 2-window, 2-level job on frames of width w in host planes of `stride` floats a row: (run, flow without weights, close)"""
    from synth import texture_frame
    tight = [np.ascontiguousarray(texture_frame(w, h, k)) for k in range(4)]
    avg, std = ctx.normalize(tight, w)
    frames = [np.zeros((3, h, stride), np.float32) for _ in tight]
    for f, t in zip(frames, tight):
        f[:, :, :w] = t[:, :, :w]
    p = sfa.default_params()
    p.S = 2; p.layers = 2; p.niter_alter = 1; p.niter_outer = 3; p.niter_inner = 1; p.niter_solver = 30; p.thres_outer = 0; p.thres_inner = 0
    p.occlusion_reasoning = 0; p.hbit = 0; p.rho[0] = 1; p.omega[0] = 0
    for k in range(3):
        p.norm_avg[k] = avg[k]; p.norm_std[k] = std[k]
    job = sfa.Job(ctx, p, w, h, 2)

    def run(weights):
        """weights: None, ("chw", planes) through upload, or ("gpu", red, weight) through set_raw_weights"""
        for b in range(2):
            job.upload(b, frames[b:b + 3], chw=weights[1] if weights and weights[0] == "chw" else None)
        if weights and weights[0] == "gpu":
            job.set_raw_weights(weights[1], weights[2])
        job.run()
        return np.stack([np.stack(job.download(b)[:2])[:, :, :w] for b in range(2)])
    return run, run(None), job


def weight_planes(w, h, stride, red, weight):
    """rawWeighting's planes in host rows of `stride` floats; the padding columns hold the ones the driver's planes hold there"""
    from test_host import raw_weights_numpy
    planes = np.ones((3, h, stride), np.float32)
    planes[:, :, :w] = raw_weights_numpy(w, h, red[0], red[1], weight)
    return [np.ascontiguousarray(planes[k]) for k in range(3)]


@pytest.fixture(scope="module")
def weight_job(ctx):
    w, h = 48, 40
    run, plain, job = make_weight_job(ctx, w, h, sfa.stride_of(w))
    yield w, h, run, plain
    job.close()


@pytest.mark.parametrize("red", [(1, 0), (0, 1)])
@pytest.mark.parametrize("weight", [0.5, 2.0, 5.0])
def test_raw_weights_on_the_gpu_give_the_flow_of_the_host_planes(weight_job, red, weight):
    w, h, run, plain = weight_job
    host = run(("chw", weight_planes(w, h, sfa.stride_of(w), red, weight)))
    gpu = run(("gpu", red, weight))
    assert np.array_equal(gpu, host)
    assert not np.array_equal(gpu, plain)                                        # the weights do reach the data term
    assert np.array_equal(run(None), plain)                                      # and an upload without them sets them back to ones


def test_raw_weights_take_the_stride_of_the_upload(ctx):
    """a width that is no multiple of 4 (46: stride_of gives 48) uploaded in rows of 52 floats: the weight planes are indexed by y * 52 + x, as chw planes
    given to that upload are; and a job keeps one stride"""
    w, h, stride = 46, 40, 52
    assert stride > sfa.stride_of(w) > w
    run, plain, job = make_weight_job(ctx, w, h, stride)
    try:
        for red, weight in (((1, 0), 2.0), ((0, 1), 0.5)):
            host = run(("chw", weight_planes(w, h, stride, red, weight)))
            gpu = run(("gpu", red, weight))
            assert np.array_equal(gpu, host), (red, weight)
            assert not np.array_equal(gpu, plain)
        assert np.array_equal(run(None), plain)
        tight = [np.zeros((3, h, sfa.stride_of(w)), np.float32)] * 3
        job.upload(0, tight)                                                     # (weights of stride 52 are held; this upload brings stride 48)
        with pytest.raises(sfa.SlowflowError) as e:
            job.set_raw_weights((1, 0), 2.0)
        assert "-> -1" in str(e.value) and "stride 52" in str(e.value) and "stride 48" in str(e.value), str(e.value)
    finally:
        job.close()


# ---- 8. the driver -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_build():
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return HOST


def write_pgm_mosaics(folder, w, h, nframes, first, sixteen):
    """the Bayer samples (red at (1, 0)) of a moving texture as binary PGM, 8 bit or 16 bit big-endian (values up to 1020: above the 8-bit range)"""
    from synth import texture_frame
    Y, X = np.mgrid[0:h, 0:w]
    red_row, red_col = (Y - 0) % 2 == 0, (X - 1) % 2 == 0
    ch = np.where(red_row & red_col, 0, np.where(~red_row & ~red_col, 2, 1))
    for k in range(nframes):
        rgb = np.clip(np.round(texture_frame(w, h, k)[:, :, :w]), 0, 255)
        m = np.take_along_axis(rgb, ch[None], 0)[0]
        with open(os.path.join(folder, "m_%03d.pgm" % (first + k)), "wb") as f:
            if sixteen:
                f.write(b"P5\n%d %d\n65535\n" % (w, h) + (m * 4).astype(">u2").tobytes())
            else:
                f.write(b"P5\n%d %d\n255\n" % (w, h) + m.astype(np.uint8).tobytes())


ODD_CROP = ((32, 24), (38, 30))                 # center, extent: starts at (13, 9); 38 wide (rows of 40 floats), 19 x 15 at scale 0.5 (rows of 20)
DRIVER_CASES = [  # raw_demosaicing, scale, crop (center, extent), raw_weight, 16bit, mosaic size
    (0, 1.0, None, 1, 0, (64, 48)), (2, 0.5, ((33, 25), (40, 32)), 1, 0, (64, 48)), (0, 0.5, ((33, 25), (40, 32)), 1, 1, (64, 48)),
    (2, 1.0, None, 2, 1, (64, 48)), (0, 1.0, ((33, 25), (40, 32)), 2, 0, (64, 48)), (2, 0.5, None, 1, 1, (64, 48)),
    (0, 0.5, ODD_CROP, 1, 1, (64, 48)), (2, 1.0, ODD_CROP, 1, 0, (64, 48)),   # widths that are no multiple of 4, before and after the rescaling
    (2, 0.5, ODD_CROP, 2, 1, (64, 48)),                                        # raw_weight 2 with scale and crop in the cfg (both skipped: no preprocessing)
    (0, 1.0, None, 2, 0, (62, 46)), (2, 0.5, None, 1, 0, (62, 46))]            # a mosaic 62 wide: weight planes with padding columns; 31 x 23 after the rescaling


@pytest.mark.parametrize("dem,scale,crop,rw,hbit,size", DRIVER_CASES)
def test_driver_outputs_are_byte_identical_with_gpu_ingest(host_build, tmp_path, dem, scale, crop, rw, hbit, size):
    import json
    (w, h), jets, first = size, 2, 9
    write_pgm_mosaics(str(tmp_path), w, h, 1 + (jets + 2), first, hbit)
    outs = {}
    for gi in (0, 1):
        cfg = tmp_path / ("run%d.cfg" % gi)
        cfg.write_text(
            "file\t%s/m_%%03i.pgm\noutput\t%s/out%d\nJets\t%d\nstart\t10\nmax_fps\t200\n16bit\t%d\nraw\t1\nraw_demosaicing\t%d\nraw_red_loc\t1,0\nraw_weight\t%d\n"
            "scale\t%g\n%sdeep_matching\t0\nslow_flow_S\t2\nslow_flow_layers\t2\nslow_flow_niter_alter\t2\nslow_flow_niter_outer\t2\nslow_flow_occlusion_reasoning\t1\n"
            "slow_flow_output_occlusions\t1\nslow_flow_thres_outer\t0\nslow_flow_thres_inner\t0\nslow_flow_rho_0\t1\nslow_flow_omega_0\t0\ngpus\t1\ngpu_batch\t4\ngpu_ingest\t%d\n"
            % (tmp_path, tmp_path, gi, jets, hbit, dem, rw, scale, "center\t%d,%d\nextent\t%d,%d\n" % (crop[0] + crop[1]) if crop else "", gi))    # ((33, 25), (40, 32)) starts at (13, 9) too
        r = subprocess.run([os.path.join(HOST, "slow_flow"), str(cfg), "-overwrite"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Done!" in r.stdout, r.stdout + r.stderr
        outs[gi] = tmp_path / ("out%d" % gi)
    names = sorted(str(p.relative_to(outs[0])) for p in outs[0].rglob("*") if p.suffix in (".flo", ".pgm", ".png"))
    assert len([n for n in names if n.endswith(".flo")]) == 2 * jets and len([n for n in names if n.startswith("occlusion")]) == jets
    assert names == sorted(str(p.relative_to(outs[1])) for p in outs[1].rglob("*") if p.suffix in (".flo", ".pgm", ".png"))
    for n in names:
        assert (outs[0] / n).read_bytes() == (outs[1] / n).read_bytes(), n
    preprocess = rw == 1
    want_w, want_h = crop[1] if (crop and preprocess) else (w, h)
    if preprocess and scale != 1:
        want_w, want_h = mr.rescaled_size(want_w, want_h, scale)
    with open(str(outs[1] / "m_010.flo"), "rb") as f:
        assert np.frombuffer(f.read(12), np.int32)[1:].tolist() == [want_w, want_h]
    paths = [{t["ingest"] for t in json.load(open(str(outs[gi] / "timings.json")))} for gi in (0, 1)]
    assert paths == [{"host"}, {"gpu"}]
    assert [json.load(open(str(outs[gi] / "run.json")))["ingest_path"] for gi in (0, 1)] == ["host", "gpu"]


@pytest.mark.parametrize("extra,word", [("raw\t0\ndeep_matching\t0\n", "raw 0"), ("raw\t1\nraw_demosaicing\t0\ndeep_matching\t1\n", "deep_matching 1"),
                                        ("raw\t1\nraw_demosaicing\t2\ndeep_matching\t0\nverbose\t0000100000\n", "sequence/frame_")])
def test_driver_refuses_gpu_ingest_by_name(host_build, tmp_path, extra, word):
    cfg = tmp_path / "a.cfg"
    cfg.write_text("file\t%s/m_%%03i.pgm\noutput\t%s/out\nJets\t1\nstart\t1\ngpu_ingest\t1\n" % (tmp_path, tmp_path) + extra)
    r = subprocess.run([os.path.join(HOST, "slow_flow"), str(cfg), "-overwrite"], capture_output=True, text=True)
    assert r.returncode == 1 and "gpu_ingest" in r.stderr and word in r.stderr, (r.returncode, r.stderr)


# ---- 9. refusals: SFA_ERR_ARG, the argument named, and the context still works ---------------------------------------------------------
class HostArray:
    """a host array that claims to be a device array"""

    def __init__(self, a):
        self.a = a
        self.__cuda_array_interface__ = {"shape": a.shape, "typestr": "<f4", "data": (a.ctypes.data, False), "version": 3, "strides": None}


def refused(ctx, dev, call, *words):
    with pytest.raises(sfa.SlowflowError) as e:
        call()
    assert "-> -1" in str(e.value) and all(word in str(e.value) for word in words), str(e.value)
    got = run_demosaic(ctx, dev, mosaic(37, 22, "u2", 0), (1, 0), 0)           # nothing was launched, and the context runs a valid call
    assert np.array_equal(got, reference(37, 22, "u2", 0, (1, 0)))


def test_refuses_a_host_pointer(ctx, dev):
    from slowflow_amd import device
    host = np.ones((1, 8, 8), np.float32)
    refused(ctx, dev, lambda: device.demosaic(ctx, _Fake(HostArray(host), dev), (1, 0), 0), "sfa_demosaic_device", "mosaic_dev", "not device memory")


class _Fake:
    """an object demosaic() can ask for its device, with another object's array interface"""

    def __init__(self, inner, dev):
        self.__cuda_array_interface__ = inner.__cuda_array_interface__
        self.inner, self.device = inner, dev


def test_refuses_a_view_that_leaves_its_allocation(ctx, dev):
    from slowflow_amd import device
    t = torch.ones((2, 8, 8), device=dev)

    class Far:                                                                   # the second frame 2^40 elements after the first
        device = t.device
        __cuda_array_interface__ = {"shape": (2, 8, 8), "typestr": "<f4", "data": (t.data_ptr(), False), "version": 3, "strides": ((1 << 40) * 4, 32, 4)}
    refused(ctx, dev, lambda: device.demosaic(ctx, Far(), (1, 0), 0), "mosaic_dev", "beyond its allocation")


def test_refuses_method_1(ctx, dev):
    from slowflow_amd import device
    refused(ctx, dev, lambda: device.demosaic(ctx, torch.ones((1, 8, 8), device=dev), (1, 0), 1), "method 1")


def test_refuses_red_location_2(ctx, dev):
    from slowflow_amd import device
    refused(ctx, dev, lambda: device.demosaic(ctx, torch.ones((1, 8, 8), device=dev), (2, 0), 0), "red_x = 2")
    refused(ctx, dev, lambda: device.demosaic(ctx, torch.ones((1, 8, 8), device=dev), (0, 2), 2), "red_y = 2")


def test_refuses_a_one_row_mosaic_with_method_0(ctx, dev):
    from slowflow_amd import device
    refused(ctx, dev, lambda: device.demosaic(ctx, torch.ones((1, 1, 8), device=dev), (1, 0), 0), "desc.H = 1", "method 0")
    assert not run_demosaic(ctx, dev, torch.ones((1, 1, 8), device=dev), (1, 0), 2).any()      # method 2 takes it: no interior, zeros


def test_refuses_a_crop_outside_the_mosaic(ctx, dev):
    from slowflow_amd import device
    refused(ctx, dev, lambda: device.demosaic(ctx, torch.ones((1, 10, 10), device=dev), (1, 0), 0, origin=(5, 5), size=(8, 8)), "crop", "desc.x0 = 5", "leaves the mosaic")


def test_refuses_a_destination_that_overlaps_the_source(ctx, dev):
    from slowflow_amd import device
    w, h = 16, 8
    buf = torch.ones(4 * w * h, device=dev)
    desc = device.MosaicDesc(0, w * h, w, 1, w, h, 0, 0)
    L = device._lib()
    st = (C.c_longlong * 4)(3 * w * h, w * h, w, 1)

    def call():
        ctx._ck(L.sfa_demosaic_device(ctx.h, 1, C.c_void_p(buf.data_ptr()), C.byref(desc), 0, 1, 0, C.c_void_p(buf.data_ptr() + 2 * w * h), st, w, h), "sfa_demosaic_device")
    refused(ctx, dev, call, "dst_dev overlaps mosaic_dev")
    torch.cuda.synchronize()
    assert bool((buf == 1).all())


def test_refuses_a_rescale_into_a_sequence_of_the_wrong_size(ctx, dev):
    src, dst = sfa.Sequence(ctx, 64, 48, 1), sfa.Sequence(ctx, 32, 25, 1)
    try:
        refused(ctx, dev, lambda: dst.rescale_from(src, 0.5), "sfa_sequence_rescale", "dst_seq", "32 x 24")
    finally:
        src.close(); dst.close()
