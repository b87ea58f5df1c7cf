"""EpicFlow's initialisation on resident data (csrc/epic_init.hip, csrc/lab_math.h; include/slowflow_amd.h: sfa_rgb8_to_lab_device, sfa_sequence_lab,
sfa_epic_job_*, sfa_job_set_flow_epic; slowflow_amd/device.py: rgb8_to_lab, epic): the Lab kernel against the host function over its whole domain and through
every layout, the epic job against sfa_epic_batch on the same inputs, the initial flow against sfa_resize_linear and image_mul_scalar, a job end to end
against sfa_job_upload_resident with the host's planes.  The boundary (declared, exported, bound) is tests/test_lab_math_host.py's.  Every comparison is on bit patterns (NaN against NaN where NaN is expected)."""
import os
import subprocess

import numpy as np
import pytest

import slowflow_amd as sfa
from test_epic import scene, stride_of
from test_lab_math_host import build_with_host_epic

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUC = 0.001


# ---- the GPU tests ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def labtool(tmp_path_factory):
    return build_with_host_epic(str(tmp_path_factory.mktemp("lab_math") / "test_lab_math"))


def host_lab(labtool, tmp, rgb, norm):
    """rgb8_to_lab of host/epic.cpp on images [n,3,h,w] -> [n,3,h,w]"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    n, _, h, w = rgb.shape
    src, dst = os.path.join(str(tmp), "rgb.bin"), os.path.join(str(tmp), "lab.bin")
    np.ascontiguousarray(rgb.transpose(1, 0, 2, 3)).tofile(src)
    r = subprocess.run([labtool, "conv", src, str(n * h * w), repr(float(norm)), dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.ascontiguousarray(np.fromfile(dst, np.float32).reshape(3, n, h, w).transpose(1, 0, 2, 3))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """bit patterns; NaN against NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def frames_rgb(n, h, w, seed, lo=-20.0, hi=300.0):
    """frames with samples on both sides of 0 .. 255, exact halves among them"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(lo, hi, (n, 3, h, w)).astype(np.float32)
    flat = a.reshape(-1)
    halves = np.array([0.5, 1.5, 2.5, 253.5, 254.5, 255.5, -0.5, 127.5], np.float32) * np.float32(255.0 if hi > 1000 else 1.0)   # (16-bit frames: ties after the division)
    flat[rng.permutation(flat.size)[:8]] = halves
    return a


# ---- 1. k_rgb8_to_lab ----------------------------------------------------------------------------------------------------------------------------
def test_lab_kernel_on_every_8_bit_triple(ctx, dev, labtool, tmp_path):
    """a 4096 x 4096 image holding every 8-bit triple once: the kernel's whole domain (rgb8_to_lab rounds to 8 bits first) against the host function"""
    from slowflow_amd import device
    t = torch.arange(1 << 24, device=dev, dtype=torch.int32)
    rgb = torch.stack([t >> 16, (t >> 8) & 255, t & 255]).to(torch.float32).reshape(1, 3, 4096, 4096)
    got = device.rgb8_to_lab(ctx, rgb, 1.0)
    torch.cuda.synchronize()
    got = got.cpu().numpy().reshape(3, -1)
    dst = str(tmp_path / "all8.bin")
    r = subprocess.run([labtool, "all8", dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = np.fromfile(dst, np.float32).reshape(3, -1)
    os.remove(dst)
    differ = int((bits(got) != bits(want)).sum())
    print("k_rgb8_to_lab over all 2^24 triples: %d values differ" % differ)
    assert differ == 0


def test_lab_kernel_layouts(ctx, dev, labtool, tmp_path):
    from slowflow_amd import device
    n, h, w = 3, 5, 37
    rgb = frames_rgb(n, h, w, 1)
    want = host_lab(labtool, tmp_path, rgb, 1.0)
    assert len(np.unique(want)) > 100
    # rows of 40 floats on both sides, the destination's padding columns poisoned: columns >= w are untouched
    src = torch.full((n, 3, h, 40), 7.0, device=dev)
    src[..., :w] = to_dev(rgb, dev)
    dst = torch.full((n, 3, h, 40), -777.0, device=dev)
    device.rgb8_to_lab(ctx, src[..., :w], 1.0, out=dst[..., :w])
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    assert same(out[..., :w], want) and (out[..., w:] == -777.0).all()
    # a crop of a larger tensor as source and as destination
    big = torch.full((n + 1, 3, h + 4, w + 9), 3.0, device=dev)
    big[:n, :, 2:2 + h, 5:5 + w] = to_dev(rgb, dev)
    bigout = torch.full((n, 3, h + 3, w + 6), -777.0, device=dev)
    device.rgb8_to_lab(ctx, big[:n, :, 2:2 + h, 5:5 + w], 1.0, out=bigout[:, :, 1:1 + h, 4:4 + w])
    torch.cuda.synchronize()
    out = bigout.cpu().numpy()
    assert same(out[:, :, 1:1 + h, 4:4 + w], want)
    out[:, :, 1:1 + h, 4:4 + w] = -777.0
    assert (out == -777.0).all()
    # a channels-last source
    cl = to_dev(rgb.transpose(0, 2, 3, 1), dev).permute(0, 3, 1, 2)
    assert cl.stride(1) == 1 and cl.stride(3) == 3
    got = device.rgb8_to_lab(ctx, cl, 1.0)
    torch.cuda.synchronize()
    assert same(got.cpu().numpy(), want)
    # 16-bit samples at 1/255, NaN and the infinities among them
    rgb16 = frames_rgb(2, h, w, 2, -500.0, 70000.0)
    rgb16[0, 0, 0, :3] = [np.nan, np.inf, -np.inf]
    want16 = host_lab(labtool, tmp_path, rgb16, np.float32(1.0 / 255))
    got = device.rgb8_to_lab(ctx, to_dev(rgb16, dev), float(np.float32(1.0 / 255)))
    torch.cuda.synchronize()
    assert same(got.cpu().numpy(), want16) and np.isnan(want16[0, :, 0, 0]).all() and np.isfinite(want16[0, :, 0, 1:3]).all()


@pytest.mark.parametrize("norm", [1.0, float(np.float32(1.0 / 255))])
def test_sequence_lab_equals_download_and_the_host_function(ctx, labtool, tmp_path, norm):
    w, h, n = 38, 30, 3                                                         # a width that is no multiple of 4
    rgb = frames_rgb(n, h, w, 3, -20.0, 300.0 if norm == 1.0 else 70000.0)
    src, dst = sfa.Sequence(ctx, w, h, n), sfa.Sequence(ctx, w, h, n + 1)
    try:
        for f in range(n):
            a = np.zeros((3, h, stride_of(w)), np.float32)
            a[:, :, :w] = rgb[f]
            src.upload(f, a)
        dst.lab_from(src, norm, f_dst=1)
        back = np.stack([src.download(f)[:, :, :w] for f in range(n)])
        assert same(back, rgb)                                                 # the source is as it was
        want = host_lab(labtool, tmp_path, back, norm)
        got = np.stack([dst.download(1 + f)[:, :, :w] for f in range(n)])
        assert same(got, want) and not dst.download(0).any()
    finally:
        src.close(); dst.close()


# ---- 2. the epic job against sfa_epic_batch ------------------------------------------------------------------------------------------------------------
def lab_of_scenes(labtool, tmp, scenes, w):
    return host_lab(labtool, tmp, np.stack([s[0][:, :, :w] for s in scenes]), 1.0)


def batch_reference(ctx, lab, scenes, p):
    """sfa_epic_batch (pinned to epic() by tests/test_epic_batch.py) on the same inputs: euc added on the host, one fp32 addition"""
    n, _, h, w = lab.shape
    labs = None
    if p.saliency_th != 0:
        labs = [np.zeros((3, h, stride_of(w)), np.float32) for _ in range(n)]
        for a, l in zip(labs, lab):
            a[:, :, :w] = l
    costs = [s[1] + np.float32(p.euc) if p.euc else s[1] for s in scenes]
    return ctx.epic_batch(labs, costs, [s[2] for s in scenes], p)


def job_from_host(ctx, lab, scenes, p):
    """the driver's way in: match and edge arrays from the host, the Lab frames from a resident sequence"""
    n, _, h, w = lab.shape
    job = ctx.epic_job(p, w, h, n)
    seq = sfa.Sequence(ctx, w, h, n)
    for i, s in enumerate(scenes):
        job.upload(i, s[2], s[1])
        a = np.zeros((3, h, stride_of(w)), np.float32)
        a[:, :, :w] = lab[i]
        seq.upload(i, a)
    job.set_lab(seq, list(range(n)))
    ctx.sync()
    seq.close()
    return job


def check_job(job, ref, w):
    fx, fy, rc, counts, _ = ref
    jrc, jcounts = job.run()
    assert jrc == rc and np.array_equal(jcounts, np.stack(counts))
    for i in range(len(rc)):
        u, v = job.download(i)
        if rc[i] == 0:
            assert same(u, fx[i][:, :w]) and same(v, fy[i][:, :w]), i
            assert len(np.unique(u)) > 20
        else:
            assert not u.any() and not v.any(), i
    return jrc, jcounts


GRID = [(w, h, method, sal, pref_nn) for (w, h) in ((64, 48), (33, 21)) for method in ("LA", "NW") for sal in (0.045, 0.0) for pref_nn in (25, 0)]


@pytest.fixture(scope="module")
def grid_scenes(labtool, tmp_path_factory):
    out = {}
    for (w, h) in ((64, 48), (33, 21)):
        scenes = [scene(w, h, 60 + k, n_matches=300 if w == 64 else 200, outliers=10) for k in range(3)]
        scenes[2][0][:, :h // 2, :w // 2] = 128.0                               # a flat quarter: nothing salient there, its matches go
        out[(w, h)] = (scenes, lab_of_scenes(labtool, tmp_path_factory.mktemp("lab%d" % w), scenes, w))
    return out


@pytest.mark.parametrize("w,h,method,sal,pref_nn", GRID)
def test_epic_job_equals_epic_batch(ctx, grid_scenes, w, h, method, sal, pref_nn):
    scenes, lab = grid_scenes[(w, h)]
    p = sfa.epic_params(method=method, saliency_th=sal, pref_nn=pref_nn, nn=100, euc=EUC)
    ref = batch_reference(ctx, lab, scenes, p)
    assert ref[2] == [0, 0, 0] and all(c[2] > 0 for c in ref[3]), (ref[2], ref[3])    # every scene keeps matches on the host path: the comparison shows something
    if sal:
        assert any(c[1] < c[0] for c in ref[3])                                # and the saliency filter does remove some
    job = job_from_host(ctx, lab, scenes, p)
    try:
        check_job(job, ref, w)
    finally:
        job.close()


def test_epic_job_in_the_compact_search_mode(ctx, grid_scenes):
    scenes, lab = grid_scenes[(64, 48)]
    p = sfa.epic_params(method="LA", saliency_th=0.045, pref_nn=25, nn=100, euc=EUC)
    ref = batch_reference(ctx, lab, scenes, p)
    job = job_from_host(ctx, lab, scenes, p)
    ctx.set_epic_search(1)
    try:
        check_job(job, ref, 64)
        assert ctx.epic_nn_search_info()["slices"] >= 3
    finally:
        ctx.set_epic_search(0)
        job.close()


@pytest.fixture(scope="module")
def dropout_batch(labtool, tmp_path_factory):
    """test_epic_batch.py's dropout scene between two ordinary ones, and an image without a match: [a, none, loses all in the consistency filter, b]"""
    w, h = 96, 64
    a, b = scene(w, h, 51), scene(w, h, 52)
    rgb, edges, m = scene(w, h, 53, n_matches=40, outliers=0)
    rng = np.random.default_rng(53)
    ang = rng.uniform(0, 2 * np.pi, 40)
    m[:, 0] = rng.uniform(20, w - 20, 40); m[:, 1] = rng.uniform(20, h - 20, 40)
    m[:, 2] = m[:, 0] + (np.arange(40) % 2 * 2 - 1) * 19 * np.cos(ang); m[:, 3] = m[:, 1] + 19 * np.sin(ang) * (1 - np.arange(40) % 4 // 2 * 2)
    scenes = [a, (a[0], a[1], np.zeros((0, 4), np.float32)), (rgb, edges, m.astype(np.float32)), b]
    return scenes, lab_of_scenes(labtool, tmp_path_factory.mktemp("lab_dropout"), scenes, w)


def initial_flow_params(S=2, layers=1, niter_outer=0):
    p = sfa.default_params()
    p.S = S; p.niter_alter = 1; p.niter_outer = niter_outer; p.occlusion_reasoning = 0; p.thres_outer = 0; p.thres_inner = 0
    p.hbit = 0; p.layers = layers; p.rho[0] = 1; p.omega[0] = 0
    return p


def read_initial_flow(job, nb):
    """a one-level run without an outer iteration copies the initial flow into the flow planes and changes nothing: download gives the initial flow"""
    job.run()
    return [job.download(b)[:2] for b in range(nb)]


def test_images_without_a_match_left_start_from_zero(ctx, dropout_batch):
    scenes, lab = dropout_batch
    w, h = 96, 64
    p = sfa.epic_params(method="LA", saliency_th=0.0, pref_nn=25, nn=100, euc=EUC)
    ref = batch_reference(ctx, lab, scenes, p)
    assert ref[2] == [0, 1, 1, 0] and list(ref[3][1]) == [0, 0, 0] and list(ref[3][2]) == [40, 40, 0]
    job = job_from_host(ctx, lab, scenes, p)
    vjob = sfa.Job(ctx, initial_flow_params(), w, h, 4)
    try:
        check_job(job, ref, w)                                                 # rc, counts, the neighbours' planes, zeros for the two
        for k in (0, 3):                                                        # the neighbours' fields are their fields alone
            alone = batch_reference(ctx, lab[k:k + 1], scenes[k:k + 1], p)
            assert same(job.download(k)[0], alone[0][0]) and same(job.download(k)[1], alone[1][0])
        vjob.set_flow_device(to_dev(np.full((4, 2, h, w), 5.0, np.float32), torch.device("cuda", 0)))     # (what the windows held before)
        vjob.set_flow_epic(job, 0.5, 0.25)
        flows = read_initial_flow(vjob, 4)
        for k in (1, 2):
            assert not flows[k][0].any() and not flows[k][1].any()
        for k in (0, 3):
            assert same(flows[k][0][:, :w], ref[0][k] * np.float32(0.5)) and same(flows[k][1][:, :w], ref[1][k] * np.float32(0.25))
    finally:
        vjob.close(); job.close()


def test_an_image_the_run_flags_holds_no_field_until_one_is_uploaded(ctx, grid_scenes):
    """a workspace of one byte holds no image: every image comes back with status 1, untouched, as from sfa_epic_batch; the driver then computes epic() on
    the host and hands the field over with sfa_epic_job_upload_flow, after which the image serves sfa_job_set_flow_epic like any other"""
    scenes, lab = grid_scenes[(64, 48)]
    w, h = 64, 48
    p = sfa.epic_params(method="LA", saliency_th=0.045, pref_nn=25, nn=100, euc=EUC)
    ref = batch_reference(ctx, lab, scenes, p)
    job = job_from_host(ctx, lab, scenes, p)
    vjob = sfa.Job(ctx, initial_flow_params(), w, h, 3)
    try:
        with pytest.raises(sfa.SlowflowError) as e:
            job.run(workspace_bytes=1)
        assert "do not fit" in str(e.value)
        rc, counts, status = job.run(workspace_bytes=1, with_status=True)
        assert status == [1, 1, 1]
        for call in (lambda: job.download(1), lambda: vjob.set_flow_epic(job)):
            with pytest.raises(sfa.SlowflowError) as e:
                call()
            assert "-> -1" in str(e.value) and "holds no field" in str(e.value), str(e.value)
        for i in range(3):                                                      # the host's fields (here: sfa_epic_batch's, which is pinned to epic())
            job.upload_flow(i, ref[0][i], ref[1][i])
        vjob.set_flow_epic(job, 0.5, 0.5)
        flows = read_initial_flow(vjob, 3)
        assert all(same(flows[i][0][:, :w], ref[0][i] * np.float32(0.5)) and same(flows[i][1][:, :w], ref[1][i] * np.float32(0.5)) for i in range(3))
        check_job(job, ref, w)                                                 # and the job still runs with room
    finally:
        vjob.close(); job.close()


# ---- 3. device inputs -------------------------------------------------------------------------------------------------------------------------------
def test_device_inputs_give_the_same_planes(ctx, dev, grid_scenes):
    scenes, lab = grid_scenes[(64, 48)]
    w, h, n = 64, 48, 3
    p = sfa.epic_params(method="LA", saliency_th=0.045, pref_nn=25, nn=100, euc=EUC)
    ref = batch_reference(ctx, lab, scenes, p)
    # strided tensors: the Lab images a crop of a larger tensor, the costs with rows of 70 floats, the matches each a tensor of its own
    big = torch.zeros((n, 3, h + 2, w + 8), device=dev)
    big[:, :, 1:1 + h, 3:3 + w] = to_dev(lab, dev)
    cost = torch.zeros((n, h, 70), device=dev)
    cost[:, :, :w] = to_dev(np.stack([s[1] for s in scenes]), dev)
    job = ctx.epic_job(p, w, h, n)
    job2 = ctx.epic_job(p, w, h, n)
    try:
        ctx.wait_stream()
        job.upload_device(big[:, :, 1:1 + h, 3:3 + w], cost[:, :, :w])
        held = [to_dev(s[2], dev) for s in scenes]                           # alive until the run has waited: the copies are only enqueued
        torch.cuda.synchronize()
        for i, m in enumerate(held):
            job.set_matches_device(i, m)
        check_job(job, ref, w)
        out = torch.full((n, 2, h, w + 4), -777.0, device=dev)
        job.download_device(out[..., :w])
        ctx.signal_stream()
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert all(same(out[i, 0, :, :w], ref[0][i]) and same(out[i, 1, :, :w], ref[1][i]) for i in range(n)) and (out[..., w:] == -777.0).all()
        # costs that hold euc already (added on the host) against costs the job adds it to
        with_euc = to_dev(np.stack([s[1] + np.float32(EUC) for s in scenes]), dev)
        ctx.wait_stream()
        job2.upload_device(to_dev(lab, dev), with_euc, cost_has_euc=True)
        for i, m in enumerate(held):
            job2.set_matches_device(i, m)
        check_job(job2, ref, w)
        ctx.signal_stream()
    finally:
        job.close(); job2.close()


# ---- 4. the initial flow ----------------------------------------------------------------------------------------------------------------------------
def field(w, h, seed):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-30, 30, (2, h, w)).astype(np.float32)
    a[0, 0, :4] = [-0.0, 1e-40, -1e-42, 0.0]                                 # minus zero and subnormals
    a[1, 1, :3] = [3e38, -1e-38, -0.0]
    return a


def test_initial_flow_equals_resize_linear_then_mul_scalar(ctx, dev):
    w, h, ew, eh = 64, 48, 32, 24
    p = sfa.epic_params(saliency_th=0.0)
    small, full, odd = ctx.epic_job(p, ew, eh, 2), ctx.epic_job(p, w, h, 2), ctx.epic_job(p, 21, 15, 1)
    vjob = sfa.Job(ctx, initial_flow_params(), w, h, 2)
    try:
        # the reading itself: a known flow comes back as it went in
        known = np.stack([field(w, h, 70), field(w, h, 71)])
        vjob.set_flow_device(to_dev(known, dev))
        back = read_initial_flow(vjob, 2)
        assert all(same(back[b][k][:, :w], known[b][k]) for b in range(2) for k in range(2))
        # 32 x 24 into 64 x 48 with steps 2: sfa_resize_linear per plane, then image_mul_scalar(fx / steps); and with steps 3, where the product rounds
        fs = [field(ew, eh, 72), field(ew, eh, 73)]
        for i, f in enumerate(fs):
            small.upload_flow(i, f[0], f[1])
        for steps in (2, 3):
            mul = np.float32(np.float32(w // ew) / np.float32(steps))
            vjob.set_flow_epic(small, float(mul), float(mul))
            got = read_initial_flow(vjob, 2)
            for i, f in enumerate(fs):
                for k in range(2):
                    plane = np.zeros((eh, stride_of(ew)), np.float32)
                    plane[:, :ew] = f[k]
                    want = ctx.resize_linear(plane, ew, w, h)[:, :w] * mul
                    assert same(got[i][k][:, :w], want), (steps, i, k)
        # 64 x 48 into 64 x 48: the multiplication alone, minus zero and the subnormals as they are
        gs = [field(w, h, 74), field(w, h, 75)]
        for i, f in enumerate(gs):
            full.upload_flow(i, f[0], f[1])
        mu, mv = np.float32(1.0 / 3), np.float32(0.5)
        vjob.set_flow_epic(full, float(mu), float(mv))
        got = read_initial_flow(vjob, 2)
        for i, f in enumerate(gs):
            assert same(got[i][0][:, :w], f[0] * mu) and same(got[i][1][:, :w], f[1] * mv), i
        assert bits(got[0][0])[0, 0] == 0x80000000 and got[0][0][0, 1] != 0    # -0.0 * mu = -0.0; the subnormal is not flushed
        # windows b0 .. from images i0 ..
        vjob.set_flow_epic(full, 1.0, 1.0, b0=1, n=1, i0=0)
        got = read_initial_flow(vjob, 2)
        assert same(got[1][0][:, :w], gs[0][0]) and same(got[0][0][:, :w], gs[0][0] * mu)
        # 21 x 15 into 64 x 48 is refused, and so is an image without a field
        odd.upload_flow(0, np.zeros((15, 21), np.float32), np.zeros((15, 21), np.float32))
        with pytest.raises(sfa.SlowflowError) as e:
            vjob.set_flow_epic(odd, 1.0, 1.0, n=1)
        assert "-> -1" in str(e.value) and "21 x 15" in str(e.value) and "64 x 48" in str(e.value), str(e.value)
        fresh = ctx.epic_job(p, w, h, 1)
        with pytest.raises(sfa.SlowflowError) as e:
            vjob.set_flow_epic(fresh, 1.0, 1.0, n=1)
        assert "holds no field" in str(e.value), str(e.value)
        fresh.close()
    finally:
        vjob.close(); small.close(); full.close(); odd.close()


# ---- 5. a job end to end ------------------------------------------------------------------------------------------------------------------------------
def test_a_job_from_the_resident_fields_equals_a_job_from_the_hosts_planes(ctx, grid_scenes):
    from synth import texture_frame
    scenes, lab = grid_scenes[(64, 48)]
    w, h, S = 64, 48, 2
    steps = S - 1
    p = sfa.epic_params(method="LA", saliency_th=0.045, pref_nn=25, nn=100, euc=EUC)
    ejob = job_from_host(ctx, lab[:2], scenes[:2], p)
    seq = sfa.Sequence(ctx, w, h, 4)
    vp = initial_flow_params(S=S, layers=2, niter_outer=3)
    vjob = sfa.Job(ctx, vp, w, h, 2)
    try:
        for f in range(4):
            seq.upload(f, texture_frame(w, h, f))
        seq.normalize()
        assert ejob.run()[0] == [0, 0]
        mul = np.float32(np.float32(1.0) / np.float32(steps))
        idx = [[0, 1, 2], [1, 2, 3]]
        for b in range(2):
            vjob.upload_resident(b, seq, idx[b])
        vjob.set_flow_epic(ejob, float(mul), float(mul))
        vjob.run()
        resident = [vjob.download(b) for b in range(2)]
        for b in range(2):
            u, v = ejob.download(b, stride_of(w))
            u[:, w:] = 0; v[:, w:] = 0
            vjob.upload_resident(b, seq, idx[b], np.ascontiguousarray(u * mul), np.ascontiguousarray(v * mul))
        vjob.run()
        for b in range(2):
            host = vjob.download(b)
            assert same(resident[b][0][:, :w], host[0][:, :w]) and same(resident[b][1][:, :w], host[1][:, :w]), b
            assert np.abs(resident[b][0][:, :w]).max() > 0.5
        for b in range(2):                                                      # and the initial flow does reach the result
            vjob.upload_resident(b, seq, idx[b])
        vjob.run()
        assert not same(vjob.download(0)[0][:, :w], resident[0][0][:, :w])
    finally:
        vjob.close(); seq.close(); ejob.close()


# ---- 6. refusals: SFA_ERR_ARG, the argument named, and the context still works -----------------------------------------------------------------------
class HostArray:
    """a host array that claims to be a device array"""

    def __init__(self, a, dev):
        self.a, self.device = a, dev
        self.__cuda_array_interface__ = {"shape": a.shape, "typestr": "<f4", "data": (a.ctypes.data, False), "version": 3, "strides": None}


def test_refusals_name_the_argument_and_leave_the_context_working(ctx, dev, labtool, tmp_path):
    from slowflow_amd import device
    rgb = frames_rgb(1, 6, 9, 9)
    want = host_lab(labtool, tmp_path, rgb, 1.0)

    def refused(call, *words):
        with pytest.raises(sfa.SlowflowError) as e:
            call()
        assert "-> -1" in str(e.value) and all(word in str(e.value) for word in words), str(e.value)
        got = device.rgb8_to_lab(ctx, to_dev(rgb, dev), 1.0)                 # nothing was launched, and the context runs a valid call
        torch.cuda.synchronize()
        assert same(got.cpu().numpy(), want)

    refused(lambda: device.rgb8_to_lab(ctx, HostArray(np.ones((1, 3, 8, 8), np.float32), dev), 1.0), "sfa_rgb8_to_lab_device", "rgb_dev", "not device memory")
    t = torch.ones((2, 3, 8, 8), device=dev)

    class Far:                                                                   # the second image 2^40 elements after the first
        device = t.device
        __cuda_array_interface__ = {"shape": (2, 3, 8, 8), "typestr": "<f4", "data": (t.data_ptr(), False), "version": 3, "strides": ((1 << 40) * 4, 256, 32, 4)}
    refused(lambda: device.rgb8_to_lab(ctx, Far(), 1.0), "rgb_dev", "beyond its allocation")
    buf = torch.ones((4, 3, 8, 8), device=dev)
    refused(lambda: device.rgb8_to_lab(ctx, buf[0:2], 1.0, out=buf[1:3]), "lab_dev overlaps rgb_dev")
    torch.cuda.synchronize()
    assert bool((buf == 1).all())
    a, b = sfa.Sequence(ctx, 38, 30, 1), sfa.Sequence(ctx, 40, 30, 1)
    refused(lambda: b.lab_from(a), "sfa_sequence_lab", "dst_seq is 40 x 30", "38 x 30")
    p = sfa.epic_params(saliency_th=0.045)
    ej = ctx.epic_job(p, 64, 48, 1)
    refused(lambda: ej.set_lab(a, [0]), "sfa_epic_job_set_lab", "lab_seq is 38 x 30")
    refused(lambda: ej.run(), "sfa_epic_job_run", "image 0 has no matches yet")
    other = sfa.Context(0)
    ej2 = other.epic_job(p, 64, 48, 1)
    ej2.upload_flow(0, np.zeros((48, 64), np.float32), np.zeros((48, 64), np.float32))
    vjob = sfa.Job(ctx, initial_flow_params(), 64, 48, 1)
    refused(lambda: vjob.set_flow_epic(ej2), "sfa_job_set_flow_epic", "epic_job lives on another context")
    refused(lambda: ej.upload(0, np.array([[1, 1, np.nan, 2]], np.float32), np.zeros((48, 64), np.float32)), "sfa_epic_job_upload", "not finite")
    bad = np.zeros((48, 64), np.float32); bad[3, 5] = -1.0
    refused(lambda: ej.upload(0, np.zeros((0, 4), np.float32), bad), "sfa_epic_job_upload", "edges of image 0")
    for o in (vjob, ej2, ej, a, b):
        o.close()
    other.close()


# ---- 7. Python: tensors in, a tensor out --------------------------------------------------------------------------------------------------------------
def test_device_epic_then_refine_pairs_equals_the_numpy_route(ctx, dev, grid_scenes):
    from slowflow_amd import device
    from synth import texture_frame
    scenes, lab = grid_scenes[(64, 48)]
    w, h, B = 64, 48, 2
    p = sfa.epic_params(method="LA", saliency_th=0.045, pref_nn=25, nn=100, euc=EUC)
    frames = to_dev(np.stack([np.stack([texture_frame(w, h, b + k)[:, :, :w] for k in range(2)]) for b in range(B)]), dev)
    rgb = to_dev(np.stack([s[0][:, :, :w] for s in scenes[:B]]), dev)
    lab_t = device.rgb8_to_lab(ctx, rgb, 1.0)
    cost = to_dev(np.stack([s[1] for s in scenes[:B]]), dev)
    flow, rc = device.epic(ctx, p, lab_t, cost, [to_dev(scenes[0][2], dev), scenes[1][2]])     # one list in GPU memory, one on the host
    assert rc == [0, 0] and flow.shape == (B, 2, h, w) and flow.is_cuda
    with pytest.raises(sfa.SlowflowError) as e:                                # the job is kept between calls: a missing Lab image is not served by the last one's
        device.epic(ctx, p, None, cost, [scenes[0][2], scenes[1][2]])
    assert "lab" in str(e.value) and "saliency_th" in str(e.value)
    out = device.refine_pairs(ctx, frames, flow0=flow)
    torch.cuda.synchronize()
    assert same(lab_t.cpu().numpy(), lab[:B])
    ref = batch_reference(ctx, lab[:B], scenes[:B], p)
    host_flow = np.stack([np.stack([ref[0][i], ref[1][i]]) for i in range(B)])
    assert same(flow.cpu().numpy(), host_flow)
    want = device.refine_pairs(ctx, frames, flow0=to_dev(host_flow, dev))
    torch.cuda.synchronize()
    assert same(out.cpu().numpy(), want.cpu().numpy()) and not same(out.cpu().numpy(), device.refine_pairs(ctx, frames).cpu().numpy())


# ---- 8. the driver: gpu_ingest 1 with deep_matching 1 and gpu_epic 1 ------------------------------------------------------------------------------------
HOST = os.path.join(ROOT, "slowflow_amd", "host")


@pytest.fixture(scope="module")
def host_build():
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return HOST


def write_mosaics(folder, w, h, nframes, first, sixteen):
    """the Bayer samples (red at (1, 0)) of a moving texture as binary PGM, 8 bit or 16 bit big-endian over the whole 16-bit range (so that the 8-bit copy the
    saliency reads, samples / 255, keeps its texture)"""
    from synth import texture_frame
    Y, X = np.mgrid[0:h, 0:w]
    red_row, red_col = (Y - 0) % 2 == 0, (X - 1) % 2 == 0
    ch = np.where(red_row & red_col, 0, np.where(~red_row & ~red_col, 2, 1))
    for k in range(nframes):
        rgb = np.clip(np.round(texture_frame(w, h, k)[:, :, :w]), 0, 255)
        m = np.take_along_axis(rgb, ch[None], 0)[0]
        with open(os.path.join(folder, "m_%03d.pgm" % (first + k)), "wb") as f:
            if sixteen:
                f.write(b"P5\n%d %d\n65535\n" % (w, h) + (m * 257 - (m % 7)).clip(0, 65535).astype(">u2").tobytes())     # (no multiples of 255 only)
            else:
                f.write(b"P5\n%d %d\n255\n" % (w, h) + m.astype(np.uint8).tobytes())


def write_epic_files(out, w, h, dm_scale, jets, start):
    """synthetic match and edge files at the reference's locations, in the coordinates of the interpolation's size"""
    ew, eh = int(round(w * dm_scale)), int(round(h * dm_scale))
    os.makedirs(os.path.join(out, "tmp"))
    rng = np.random.default_rng(5)
    for j in range(jets):
        a, b = start + j, start + j + 1
        for (p, q, sx, sy) in ((a, b, 1.5, -0.75), (b, a, -1.5, 0.75)):
            with open(os.path.join(out, "tmp", "matches_%d_%d.dat" % (p, q)), "w") as f:
                for _ in range(300):
                    x, y = rng.uniform(2, ew - 3), rng.uniform(2, eh - 3)
                    f.write("%.3f %.3f %.3f %.3f 3.1 1\n" % (x, y, x + sx * dm_scale + rng.normal(0, 0.1), y + sy * dm_scale + rng.normal(0, 0.1)))
    for n in range(start, start + jets + 1):
        (0.05 + 0.02 * rng.uniform(0, 1, (eh, ew))).astype(np.float32).tofile(os.path.join(out, "tmp", "edges_%d.dat" % n))


def driver_cfg(tmp_path, name, out, jets, hbit, dem, dm_scale, gpu_ingest, gpu_epic, extra=""):
    cfg = tmp_path / name
    cfg.write_text(
        "file\t%s/m_%%03i.pgm\noutput\t%s/\nJets\t%d\nstart\t10\nmax_fps\t200\n16bit\t%d\nraw\t1\nraw_demosaicing\t%d\nraw_red_loc\t1,0\nraw_weight\t1\nscale\t1.0\n"
        "deep_matching\t1\ndm_scale\t%g\ngpu_epic\t%d\nslow_flow_S\t2\nslow_flow_layers\t2\nslow_flow_niter_alter\t2\nslow_flow_niter_outer\t2\nslow_flow_occlusion_reasoning\t1\n"
        "slow_flow_output_occlusions\t1\nslow_flow_thres_outer\t0\nslow_flow_thres_inner\t0\nslow_flow_rho_0\t1\nslow_flow_omega_0\t0\ngpus\t1\ngpu_batch\t4\ngpu_ingest\t%d\n"
        % (tmp_path, out, jets, hbit, dem, dm_scale, gpu_epic, gpu_ingest) + extra)
    return cfg


# (16-bit mosaics go with raw_demosaicing 0: method 2 is the 8-bit conversion, which saturates them to 0 .. 255, and the 8-bit copy of that frame, samples / 255,
#  is flat -- no match is salient on either route, every window starts from zero and the comparison would show nothing)
@pytest.mark.parametrize("dm_scale,hbit,dem,search", [(1.0, 0, 0, 0), (0.5, 0, 2, 0), (1.0, 0, 2, 0), (1.0, 1, 0, 0), (0.5, 1, 0, 0), (1.0, 0, 0, 1)])
def test_driver_outputs_are_byte_identical_with_the_resident_initialisation(host_build, tmp_path, dm_scale, hbit, dem, search):
    import json
    w, h, jets, first = 64, 48, 2, 9
    write_mosaics(str(tmp_path), w, h, 1 + (jets + 2), first, hbit)
    outs, runs = {}, {}
    for gi in (0, 1):
        outs[gi] = tmp_path / ("out%d" % gi)
        write_epic_files(str(outs[gi]), w, h, dm_scale, jets, 10)
        cfg = driver_cfg(tmp_path, "run%d.cfg" % gi, outs[gi], jets, hbit, dem, dm_scale, gi, 1, "gpu_epic_search\t%d\n" % search)
        r = subprocess.run([os.path.join(HOST, "slow_flow"), str(cfg), "-overwrite"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "Done!" in r.stdout, r.stdout + r.stderr
        runs[gi] = json.load(open(str(outs[gi] / "run.json")))
    names = sorted(str(p.relative_to(outs[0])) for p in outs[0].rglob("*") if p.suffix in (".flo", ".pgm", ".png"))
    assert len([n for n in names if n.endswith(".flo")]) == 2 * jets and len([n for n in names if n.startswith("occlusion")]) == jets
    assert names == sorted(str(p.relative_to(outs[1])) for p in outs[1].rglob("*") if p.suffix in (".flo", ".pgm", ".png"))
    for n in names:
        assert (outs[0] / n).read_bytes() == (outs[1] / n).read_bytes(), n
    assert [runs[gi]["epic_init_path"] for gi in (0, 1)] == ["host", "resident"] and [runs[gi]["ingest_path"] for gi in (0, 1)] == ["host", "gpu"]
    for gi in (0, 1):                                                           # every window starts from its matches: a run from zero would show nothing
        assert (runs[gi]["epic_init_from_matches"], runs[gi]["epic_init_from_zero"]) == (2 * jets, 0), runs[gi]
    # gpu_epic_search reaches the context that ran the epic jobs (the worker's), and the library counted their searches: one image per window
    info = runs[1]["epic_init_search"]
    assert info["mode"] == search and runs[1]["gpu_epic_search"] == search and info["slices"] >= 1 and info["dense"] + info["sparse"] == 2 * jets, info
    assert runs[0]["epic_init_search"]["mode"] == -1                           # (the host route runs no epic job)
    u = np.fromfile(str(outs[1] / "m_010.flo"), np.float32)[3:].reshape(h, w, 2)[..., 0]
    assert abs(np.median(u) - 1.5) < 0.5                                       # the motion of the texture


def test_driver_refuses_gpu_ingest_with_deep_matching_without_gpu_epic(host_build, tmp_path):
    cfg = driver_cfg(tmp_path, "a.cfg", tmp_path / "out", 1, 0, 0, 1.0, 1, 0)
    r = subprocess.run([os.path.join(HOST, "slow_flow"), str(cfg), "-overwrite"], capture_output=True, text=True)
    assert r.returncode == 1 and "gpu_ingest" in r.stderr and "deep_matching 1" in r.stderr and "gpu_epic 1" in r.stderr, (r.returncode, r.stderr)


def test_driver_refuses_a_field_size_that_does_not_divide_the_frames(host_build, tmp_path):
    """dm_scale 0.75 on 64 x 48 frames: a field of 48 x 36, which the resident route cannot bring to the frames' size; refused by name with status 1
    once the size is known, before anything is refined"""
    write_mosaics(str(tmp_path), 64, 48, 4, 9, 0)
    out = tmp_path / "out"
    write_epic_files(str(out), 64, 48, 0.75, 1, 10)
    cfg = driver_cfg(tmp_path, "a.cfg", out, 1, 0, 0, 0.75, 1, 1)
    r = subprocess.run([os.path.join(HOST, "slow_flow"), str(cfg), "-overwrite"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "gpu_ingest 1 is refused" in r.stderr and "dm_scale 0.75" in r.stderr and "48 x 36" in r.stderr, (r.returncode, r.stderr)
    assert not list(out.rglob("*.flo"))
