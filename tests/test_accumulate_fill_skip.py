"""accumulate -fill on the reference's own grid, acc_skip_pixel 1: the two-rate scene of tests/test_accumulate_fill.py with frames and jets at twice its width
and height (104 x 58), so that the grid is that test's 52 x 29.  Edge maps are written at the grid's size.  The program's fused flow, occlusions and labels
equal, byte for byte, the chain assembled here as that test assembles it: rgb.bin = the reduced 8-bit image of frame 0 by tests/ref_image_ref.py (the numpy
restatement of INTEGRATION.md 4c''s definition), the fill-in trajectories of the plain host chain (tests/host/epic_fill_tool.cpp with skip_pixel 1), the
energies of both hypotheses per rate and sfa_fuse_hypotheses with skip 1.  -reference writes that reduced image as the reference's frame_epic_<start>.png;
acc_skip_pixel 2 stays refused by name, and so does acc_skip_pixel 1 without the cfg key acc_gpu_reference_image 1; -alternate at skip 1 equals the track job
driven from Python with the same inputs."""
import json
import struct
import subprocess
import zlib

import numpy as np
import pytest

import oracle as orc
import ref_image_ref as R
import test_accumulate as ta
import test_accumulate_energies as tae
import test_accumulate_fill as taf
from test_accumulate import host_build, read_flo, read_pgm  # noqa: F401  (host_build: the fixture)
from test_accumulate_fill import INNER, STARTS, UNKNOWN, run
from test_accumulate_fill_groups import outputs
from test_epic_fill import tool  # noqa: F401  (the fixture that builds tests/host/epic_fill_tool.cpp)

JETS, MIN_FPS = tae.JETS, tae.MIN_FPS
SKIP = 1
GW, GH = taf.WF, 29                              # the grid: tests/test_accumulate_fill.py's frame
W2, H2 = 2 * GW, 2 * GH
BLOCK2 = (slice(16, 40), slice(60, 88))          # that test's BLOCK on the frames: the grid's rows 8 .. 19, columns 30 .. 43
ALT_KEYS = "acc_alternate\t2\nacc_perturb_keep\t3\nacc_hyp_neigh_tryouts\t6\nseed\t3\n"


@pytest.fixture
def double_size(monkeypatch):
    for mod in (ta, tae):
        monkeypatch.setattr(mod, "W", W2)
        monkeypatch.setattr(mod, "H", H2)
    monkeypatch.setattr(taf, "BLOCK", BLOCK2)


@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


def write_cfg(root, out, extra="", skip_pixel=SKIP, restated=True):
    return taf.write_cfg(root, out, extra=extra + ("acc_gpu_reference_image\t1\n" if restated else ""), skip_pixel=skip_pixel)


def write_edges(out, seed=0):
    """<output>/accumulated/tmp/edges_<start>.dat at the GRID's size"""
    d = out / "accumulated" / "tmp"
    d.mkdir(parents=True)
    maps = {}
    for k, start in enumerate(STARTS):
        maps[start] = np.random.default_rng(seed + k).uniform(0.01, 0.5, (GH, GW)).astype(np.float32)
        maps[start].tofile(d / ("edges_%d.dat" % start))
    return maps


def raw_frames(seq, start):
    """the Jets + 1 frames of a start_jet as read: fp32 (3, H2, stride) each"""
    raw = []
    for f in range(JETS + 1):
        rgb = np.fromfile(seq / ("frame_%d.ppm" % (start + 2 * f)), np.uint8)[-3 * W2 * H2:].reshape(H2, W2, 3)
        im = orc.aligned_zeros((3, H2, orc.stride_of(W2)))
        im[:, :, :W2] = rgb.transpose(2, 0, 1).astype(np.float32)
        raw.append(im)
    return raw


def read_png_rgb8(path):
    """an 8-bit RGB PNG of one IDAT stream with filter 0 rows (what host/png.cpp writes) -> (3, h, w) uint8"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", data[pos + 8:pos + 8 + n])
        if kind == b"IDAT":
            idat += data[pos + 8:pos + 8 + n]
        pos += 12 + n
    w, h, depth, ctype = head[:4]
    assert (depth, ctype) == (8, 2)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3).transpose(2, 0, 1)


def chain(ctx, oracle, tool_exe, work, truth, seq, start, edges, trws_max_iter=6):
    """the fused result of one start_jet, assembled from the stages (tests/test_accumulate_fill.py's chain on the skipped grid)"""
    import slowflow_amd as sfa
    raw = raw_frames(seq, start)
    work.mkdir()
    rgb8 = R.reference_rgb8(raw[0][:, :, :W2], SKIP)                           # the reference's resized 8-bit image of frame 0, by the restatement
    assert rgb8.shape == (3, GH, GW)
    small = orc.aligned_zeros((3, GH, orc.stride_of(GW)))
    small[:, :, :GW] = rgb8.astype(np.float32)
    np.ascontiguousarray(small).tofile(work / "rgb.bin")
    edges.tofile(work / "edges.bin")
    frames = [f.copy() for f in raw]
    oracle.normalize(frames, W2)
    stack = np.ascontiguousarray(np.stack(frames))[None]
    acc = []
    for r in range(2):
        fu, fv, bu, bv, _ = truth[r, start]
        au, av, tr = ctx.accumulate_consistent(fu[None], fv[None], bu[None], bv[None], W2, 0.5, SKIP, False, all_steps=True)
        assert au.shape[2:] == (GH, GW)
        acc.append((au[0], av[0], tr[0]))
        au[0].tofile(work / ("acc_u_%d.bin" % r)); av[0].tofile(work / ("acc_v_%d.bin" % r)); tr[0].tofile(work / ("tracked_%d.bin" % r))
    rates = [a[0].shape[0] for a in acc]
    r = subprocess.run([tool_exe, str(work), str(GW), str(GH), str(SKIP), "2", "0.001"] + [str(J) for J in rates], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    tool_filled = [int(line.split()[3]) for line in r.stdout.splitlines() if line.startswith("rate ")]
    K = 4
    U, V = np.zeros((1, K, JETS, GH, GW)), np.zeros((1, K, JETS, GH, GW))
    E = np.full((1, K, GH, GW), np.inf)
    O = np.zeros((1, K, GH, GW), np.uint64)
    filled = []
    for r in range(2):
        J = rates[r]
        cu = np.fromfile(work / ("chain_u_%d.bin" % r), np.float64).reshape(J, GH, GW)
        cv = np.fromfile(work / ("chain_v_%d.bin" % r), np.float64).reshape(J, GH, GW)
        ct = np.fromfile(work / ("chain_tracked_%d.bin" % r), np.int32).reshape(GH, GW)
        filled.append(bool((ct == J).all()))
        flows = None if r < MIN_FPS else tuple(a[None] for a in truth[MIN_FPS, start][:4])
        p = sfa.energy_params(skip=SKIP, weight=float(r), acc_cv=0.25)
        for kind, (au, av, tr) in enumerate((acc[r], (cu, cv, ct))):
            if kind == 1 and not filled[r]:
                continue
            e, o, u, v = ctx.hypothesis_energies(p, J, au[None], av[None], tr[None], stack, W2, flows=flows, adapted=True)
            E[0, 2 * r + kind], O[0, 2 * r + kind], U[0, 2 * r + kind], V[0, 2 * r + kind] = e[0], o[0], u[0], v[0]
    assert tool_filled == [int(f) for f in filled]
    weight = ctx.smoothness_weight(frames[0], W2)
    out = ctx.fuse_hypotheses(sfa.fuse_params(skip=SKIP, trws_max_iter=trws_max_iter), U, V, E, O, weight[None], W2, H2)
    return out, filled, rgb8


@pytest.mark.gpu
def test_program_fill_at_skip_1_end_to_end(host_build, tool, ctx, oracle, tmp_path, double_size):
    import slowflow_amd as sfa
    truth, seq = taf.make_scene(tmp_path)
    assert sfa.reference_grid(W2, H2, SKIP) == (GW, GH)
    # plain -fuse: the block has no hypothesis of either rate
    r = run([write_cfg(tmp_path, tmp_path / "plain"), "-fuse"])
    assert r.returncode == 0, r.stdout + r.stderr
    plain = tmp_path / "plain" / "accumulated"
    for start in STARTS:
        u, v = read_flo(plain / ("frame_%d.flo" % start))
        assert u.shape == (GH, GW) and (u[INNER] > UNKNOWN).all() and (v[INNER] > UNKNOWN).all()   # the scene does exercise the gap
    # -fill
    out = tmp_path / "result"
    edges = write_edges(out)
    cfg = write_cfg(tmp_path, out)
    r = run([cfg, "-fill", "-resume"])
    assert r.returncode == 0, r.stdout + r.stderr                                # (status 1 and "acc_skip_pixel" before this stage existed)
    acc = out / "accumulated"
    rj = json.load(open(acc / "run.json"))
    assert rj["fused"] is True and rj["epic_fill"] is True and rj["acc_skip_pixel"] == 1 and (rj["width"], rj["height"]) == (W2, H2)
    assert rj["reference_image"] == {"skip": 1, "taps": [1, 14, 62, 102, 62, 14, 1], "size": [GW, GH]}
    assert [f["filled"] for f in rj["fill"]] == [True] * 4                       # both rates of both start_jets
    for start in STARTS:
        want, filled, _ = chain(ctx, oracle, tool, tmp_path / ("chain_%d" % start), truth, seq, start, edges[start])
        assert all(filled)
        u, v = read_flo(acc / ("frame_%d.flo" % start))
        assert (np.abs(u) < UNKNOWN).all() and (np.abs(v) < UNKNOWN).all()      # no hole is left
        assert np.array_equal(u.view(np.uint32), want["u"][0].astype(np.float32).view(np.uint32))
        assert np.array_equal(v.view(np.uint32), want["v"][0].astype(np.float32).view(np.uint32))
        labels = read_pgm(acc / ("labels_%d.pgm" % start))
        assert np.array_equal(labels, want["slot"][0].astype(np.uint8)) and (want["slot"][0] >= 0).all()
        assert (labels[INNER] % 2 == 1).all() and (labels % 2 == 0).any()       # fill-in slots in the block, accumulated ones elsewhere
        assert np.array_equal(read_pgm(acc / "occlusions" / ("frame_%d.pgm" % start)), (want["occ"][0] * 255).astype(np.uint8))
        seg = [s for s in rj["fusion"] if s["sequence_start"] == start][0]
        assert seg["energy"] == want["energy"][0] and seg["lower_bound"] == want["bound"][0] and seg["iterations"] == want["iters"][0]
        assert seg["nodes"] == GH * GW


@pytest.mark.gpu
def test_reference_flag_writes_the_reduced_image(host_build, tmp_path, double_size):
    _, seq = taf.make_scene(tmp_path)
    for skip in (1, 0, 3):
        out = tmp_path / ("ref%d" % skip)
        r = run([write_cfg(tmp_path, out, skip_pixel=skip), "-reference"])
        if skip == 3:                                                            # 58 / 4 = 14.5 rounds to 14 = floor: served; the grid is 26 x 14
            assert R.grid(W2, H2, 3) == (26, 14)
        assert r.returncode == 0, r.stdout + r.stderr
        acc = out / "accumulated"
        assert sorted(p.name for p in acc.iterdir()) == ["tmp"]                 # nothing but the images is written
        for start in STARTS:
            got = read_png_rgb8(acc / "tmp" / ("frame_epic_%d.png" % start))
            assert np.array_equal(got, R.reference_rgb8(raw_frames(seq, start)[0][:, :, :W2], skip))
    out = tmp_path / "sel"
    r = run([write_cfg(tmp_path, out), "-reference", "-select", "1"])
    assert r.returncode == 0 and sorted(p.name for p in (out / "accumulated" / "tmp").iterdir()) == ["frame_epic_18.png"]


@pytest.mark.gpu
def test_other_skips_stay_refused_by_name(host_build, tmp_path, double_size):
    taf.make_scene(tmp_path, seed=1)
    for skip in (2, 7):
        for flag in ("-fill", "-alternate", "-reference"):
            r = run([write_cfg(tmp_path, tmp_path / "refused", skip_pixel=skip), flag])
            named = "-reference" if flag == "-reference" else "-fill"            # -alternate implies -fill, whose limit it is
            assert r.returncode == 1 and named in r.stderr and "acc_skip_pixel" in r.stderr, (skip, flag, r.stdout, r.stderr)
            assert not (tmp_path / "refused").exists()
    for flag in ("-fill", "-alternate"):                                         # the restatement is the cfg's choice: without its key, as before it existed
        r = run([write_cfg(tmp_path, tmp_path / "refused", restated=False), flag])
        assert r.returncode == 1 and "-fill" in r.stderr and "acc_skip_pixel" in r.stderr and "acc_gpu_reference_image" in r.stderr, (flag, r.stdout, r.stderr)
        assert not (tmp_path / "refused").exists()


def python_job(ctx, oracle, truth, seq, starts, edges):
    """the track job that alternates, driven from Python with the program's inputs and keys: frame 0 as read goes to upload_fill_reference"""
    import slowflow_amd as sfa
    p = sfa.track_params(W2, H2, JETS, [2, 4], n=len(starts), weights=[0.0, 1.0], energy=sfa.energy_params(acc_cv=0.25), fuse=sfa.fuse_params(trws_max_iter=6),
                         min_fps_idx=MIN_FPS, do_fuse=1, epsilon=0.5, skip=SKIP, discard=0, coef=5.0)
    job = sfa.TrackJob(ctx, p, fill=sfa.track_fill_params(), alt=sfa.track_alt_params(2, perturb_keep=3, hyp_neigh_tryouts=6, seed=3))
    for s, start in enumerate(starts):
        raw = raw_frames(seq, start)
        frames = [f.copy() for f in raw]
        oracle.normalize(frames, W2)
        for r in range(2):
            job.upload_flows(s, r, *truth[r, start][:4])
        job.upload_frames(s, np.stack(frames))
        job.upload_fill_reference(s, raw[0], edges[start])
    job.set_sequence_starts(list(starts))
    job.run(len(starts))
    got = [(job.download_fused(s), job.download_alternation(s)) for s in range(len(starts))]
    job.close()
    return got


@pytest.mark.gpu
def test_alternate_at_skip_1_equals_the_job_driven_from_python(host_build, ctx, oracle, tmp_path, double_size):
    truth, seq = taf.make_scene(tmp_path)
    got = {}
    for batch in (1, 2):
        out = tmp_path / ("batch%d" % batch)
        edges = write_edges(out)
        r = run([write_cfg(tmp_path, out, extra=ALT_KEYS + "acc_gpu_batch\t%d\n" % batch), "-alternate", "-resume"])
        assert r.returncode == 0, r.stdout + r.stderr
        got[batch] = (outputs(out / "accumulated"), json.load(open(out / "accumulated" / "run.json")))
    assert got[1][0] == got[2][0] and any(n.startswith("proposed_") for n in got[1][0])      # groups of one and of two: the same files
    acc = tmp_path / "batch2" / "accumulated"
    for s, (fused, alt) in enumerate(python_job(ctx, oracle, truth, seq, STARTS, edges)):
        start = STARTS[s]
        u, v = read_flo(acc / ("frame_%d.flo" % start))
        assert (np.abs(u) < UNKNOWN).all()
        assert np.array_equal(u.view(np.uint32), fused["u"].astype(np.float32).view(np.uint32))
        assert np.array_equal(v.view(np.uint32), fused["v"].astype(np.float32).view(np.uint32))
        assert np.array_equal(read_pgm(acc / ("labels_%d.pgm" % start)), np.where(fused["slot"] >= 0, alt["origin"] & 0x7f, 255).astype(np.uint8))
        assert np.array_equal(read_pgm(acc / ("proposed_%d.pgm" % start)), np.where((fused["slot"] >= 0) & (alt["origin"] & 0x80 > 0), 255, 0).astype(np.uint8))
        seg = [f for f in got[2][1]["fusion"] if f["sequence_start"] == start][0]
        assert [q["energy"] for q in seg["rounds"]] == alt["energy"].tolist() and [q["accepted_proposals"] for q in seg["rounds"]] == alt["accepted"].tolist()
