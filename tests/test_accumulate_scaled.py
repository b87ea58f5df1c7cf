"""The accumulate program on jets of another size than the tracking frames (slow_flow.cfg's scale 0.25 against dense_tracking.cfg's scale 1.0):
quarter-size jets through -fuse, rates of mixed sizes in the plain mode, center / extent, and the refusals, against the restated chain
(tests/jet_resample_ref.py -> accum_ref -> energy_ref -> fuse_ref).  Equal-size jets give the bytes the existing entry points give."""
import json
import struct
import subprocess

import numpy as np
import pytest

import fuse_ref as fr
import oracle as orc
import slowflow_amd as sfa
import test_accumulate as ta
import test_accumulate_energies as tae
from accum_ref import accumulate, grid
from energy_ref import Params, derivatives, energies, flows_for_rate
from jet_resample_ref import decode_occlusion_scaled, resample_flow, rescale_of
from test_accumulate import PROGRAM, host_build, read_flo, read_pgm  # noqa: F401  (host_build: the fixture)

SW, SH, TW, TH = 13, 10, 52, 40
JETS, MIN_FPS = tae.JETS, tae.MIN_FPS


def set_size(monkeypatch, w, h):
    """the size tests/test_accumulate.py's make_jets and tests/test_accumulate_energies.py's make_frames write at"""
    for m in (ta, tae):
        monkeypatch.setattr(m, "W", w)
        monkeypatch.setattr(m, "H", h)


def run_program(*args):
    return subprocess.run(["timeout", "-k", "10", "300", PROGRAM] + [str(a) for a in args], capture_output=True, text=True, timeout=330)


def write_cfg(root, out, low, high, extra=""):
    """tests/test_accumulate_energies.py's cfg (acc_min_fps 1: Jets 4, rate 0 adapts 2 steps) with each rate's folder given"""
    lines = ["jet_estimation\t%s/" % low, "jet_estimation\t%s/" % high, "flow_format\tframe_%i", "output\t%s" % out, "start\t10",
             "file\t%s/frame_%%i.ppm" % (root / "seq"), "ref_fps\t25", "ref_fps_F\t2", "max_fps\t200", "acc_min_fps\t%d" % MIN_FPS, "acc_skip_pixel\t1",
             "acc_discard_inconsistent\t0", "acc_consistency_threshold\t0.5", "acc_cv\t0.25"]
    cfg = root / "scaled.cfg"
    cfg.write_text("\n".join(lines) + "\n" + extra)
    return cfg


def raw_occlusions(folder, r, start, FF):
    """the occlusion images make_jets wrote for rate r (names: dense_tracking.cpp:1161)"""
    rate = ta.RATES[r]
    step = (rate["S"] - 1) * (200 // rate["fps"])
    return [read_pgm(folder / "occlusion" / ("frame_%d.pgm" % (start + f * step))) for f in range(FF)]


def resampled(truth, r, start, w, folder=None):
    """rate r's flows of one start as dense_tracking reads them at width w: float64 planes (identity: the floats, which the program does not
    resample) and, with `folder`, the decoded occlusion masks"""
    fu, fv, bu, bv, masks = truth[r, start]
    FF, sw = fu.shape[0], fu.shape[2]
    if sw == w:
        return fu, fv, bu, bv, (masks if folder else None)
    rs = rescale_of(w, sw)
    f = [resample_flow(fu[k], fv[k], rs) for k in range(FF)]
    b = [resample_flow(bu[k], bv[k], rs) for k in range(FF)]
    m = np.stack([decode_occlusion_scaled(g, rs) for g in raw_occlusions(folder, r, start, FF)]) if folder else None
    return np.stack([x[0] for x in f]), np.stack([x[1] for x in f]), np.stack([x[0] for x in b]), np.stack([x[1] for x in b]), m


def expected_fusion(flows, seq_dir, start, oracle, p):
    """tests/test_accumulate_fuse.py's expected() with the flows already at the frames' size: flows[r] = (fu, fv, bu, bv, masks)"""
    frames = []
    for f in range(JETS + 1):
        rgb = np.fromfile(seq_dir / ("frame_%d.ppm" % (start + 2 * f)), np.uint8)[-3 * TW * TH:].reshape(TH, TW, 3)
        im = orc.aligned_zeros((3, TH, orc.stride_of(TW)))
        im[:, :, :TW] = rgb.transpose(2, 0, 1).astype(np.float32)
        frames.append(im)
    oracle.normalize(frames, TW)
    stack = np.ascontiguousarray(np.stack(frames)[..., :TW])
    dx, dy = derivatives(oracle, stack, TW)
    gw, gh, _, _ = grid(TW, TH, 1)
    K = 2
    U, V = np.zeros((K, JETS, gh, gw)), np.zeros((K, JETS, gh, gw))
    E = np.full((K, gh, gw), np.inf)
    O = np.zeros((K, gh, gw), np.uint64)
    last = {}
    for r in range(K):
        fu, fv, bu, bv, masks = flows[r]
        au, av, tr = accumulate(fu, fv, bu, bv, masks, 0.5, 1, False)
        last[r] = (au[-1], av[-1], tr)
        e, b, terms = energies(Params(skip=1, weight=float(r), acc_cv=0.25), fu.shape[0], au, av, tr, stack, dx, dy, flows_for_rate(r, MIN_FPS, flows[MIN_FPS][:4]))
        E[r], O[r] = e, b
        U[r][:, terms["hy"], terms["hx"]] = terms["U"]
        V[r][:, terms["hy"], terms["hx"]] = terms["V"]
    return fr.fuse(U, V, E, O, fr.smoothness_weight(oracle, frames[0], TW), p, TW), last, E


@pytest.mark.gpu
def test_quarter_size_jets_fuse_end_to_end(host_build, oracle, tmp_path, monkeypatch):
    """the reference's shipped pair of configurations: jets estimated at a quarter of the frames' size.  Before jets of another size were
    resampled this exited with status 1 ("rescaling is not implemented")"""
    set_size(monkeypatch, SW, SH)
    truth = ta.make_jets(tmp_path)
    set_size(monkeypatch, TW, TH)
    seq = tae.make_frames(tmp_path)
    cfg = write_cfg(tmp_path, tmp_path / "result", tmp_path / "low", tmp_path / "high", "acc_trws_max_iter\t6\nacc_use_jet_occlusions\t1\n")
    r = run_program(cfg, "-fuse")
    assert r.returncode == 0, r.stdout + r.stderr
    acc = tmp_path / "result" / "accumulated"
    run = json.load(open(acc / "run.json"))
    assert (run["width"], run["height"]) == (TW, TH)
    assert [(q["source_width"], q["source_height"], q["rescale"]) for q in run["rates"]] == [(SW, SH, 4), (SW, SH, 4)]
    p = fr.Params(trws_max_iter=6)
    for start in (10, 18):
        flows = {k: resampled(truth, k, start, TW, tmp_path / ta.RATES[k]["name"]) for k in (0, 1)}
        want, last, E = expected_fusion(flows, seq, start, oracle, p)
        for k in (0, 1):
            au, av, tr = last[k]
            FF = flows[k][0].shape[0]
            u, v = read_flo(acc / str(k) / ("frame_%d.flo" % start))
            assert np.array_equal(u, au.astype(np.float32)) and np.array_equal(v, av.astype(np.float32))
            assert np.array_equal(read_pgm(acc / str(k) / ("tracked_%d.pgm" % start)), np.where(tr == FF, 255, 255 * tr // FF).astype(np.uint8))
            assert np.array_equal(tae.read_pfm(acc / str(k) / ("energy_%d.pfm" % start)), E[k].astype(np.float32))
            assert 0 < (tr == FF).sum() < tr.size
        u, v = read_flo(acc / ("frame_%d.flo" % start))
        assert np.array_equal(u, want["u"].astype(np.float32)) and np.array_equal(v, want["v"].astype(np.float32))
        assert np.array_equal(read_pgm(acc / ("labels_%d.pgm" % start)), np.where(want["slot"] < 0, 255, want["slot"]).astype(np.uint8))
        assert np.array_equal(read_pgm(acc / "occlusions" / ("frame_%d.pgm" % start)), (want["occ"] * 255).astype(np.uint8))
        seg = [s for s in run["fusion"] if s["sequence_start"] == start][0]
        assert seg["energy"] == want["energy"] and seg["lower_bound"] == want["bound"] and seg["iterations"] == want["iters"]
        assert seg["nodes"] == int((want["slot"] >= 0).sum()) > 0


@pytest.mark.gpu
def test_mixed_sizes_in_the_plain_mode(host_build, tmp_path, monkeypatch):
    """one rate at the frames' size, the other at a quarter: the target is the ingested frame at `start`; the full-size rate is not resampled"""
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    set_size(monkeypatch, TW, TH)
    big = ta.make_jets(tmp_path / "a", seed=4)
    seq = tae.make_frames(tmp_path)
    set_size(monkeypatch, SW, SH)
    small = ta.make_jets(tmp_path / "b", seed=5)
    cfg = write_cfg(tmp_path, tmp_path / "result", tmp_path / "a" / "low", tmp_path / "b" / "high", "acc_occlusion\t1\n")
    r = run_program(cfg)
    assert r.returncode == 0, r.stdout + r.stderr
    acc = tmp_path / "result" / "accumulated"
    run = json.load(open(acc / "run.json"))
    assert (run["width"], run["height"]) == (TW, TH) and [q["rescale"] for q in run["rates"]] == [1, 4] and run["calls"] == 2
    for start in (10, 18):
        for k, truth, folder in ((0, big, tmp_path / "a" / "low"), (1, small, tmp_path / "b" / "high")):
            fu, fv, bu, bv, masks = resampled(truth, k, start, TW, folder)
            au, av, tr = accumulate(fu, fv, bu, bv, masks, 0.5, 1, False)
            u, v = read_flo(acc / str(k) / ("frame_%d.flo" % start))
            assert np.array_equal(u, au[-1].astype(np.float32)) and np.array_equal(v, av[-1].astype(np.float32))
            assert np.array_equal(read_pgm(acc / str(k) / ("tracked_%d.pgm" % start)), np.where(tr == fu.shape[0], 255, 255 * tr // fu.shape[0]).astype(np.uint8))
    # the frame that gives the target is named where it is missing: status 2
    (seq / "frame_10.ppm").unlink()
    r = run_program(cfg)
    assert r.returncode == 2 and str(seq / "frame_10.ppm") in r.stderr.replace("//", "/")


def flo_bytes(u, v):
    return struct.pack("<fii", 202021.25, u.shape[1], u.shape[0]) + np.stack([u, v], -1).astype("<f4").tobytes()


def pgm_bytes(g):
    return b"P5\n%d %d\n255\n" % (g.shape[1], g.shape[0]) + np.ascontiguousarray(g, np.uint8).tobytes()


@pytest.mark.gpu
def test_equal_size_jets_give_the_bytes_of_the_existing_entry_points(host_build, tmp_path):
    """the plain mode on jets of one size: what sfa_accumulate_consistent gives on host-decoded masks, byte for byte"""
    truth = ta.make_jets(tmp_path, seed=6)
    cfg = ta.write_cfg(tmp_path, tmp_path / "result")
    r = run_program(cfg)
    assert r.returncode == 0, r.stdout + r.stderr
    acc = tmp_path / "result" / "accumulated"
    run = json.load(open(acc / "run.json"))
    assert run["calls"] == 2 and [(q["source_width"], q["source_height"], q["rescale"]) for q in run["rates"]] == [(ta.W, ta.H, 1)] * 2
    ctx = sfa.Context(0)
    try:
        stride = sfa.stride_of(ta.W)
        for (k, start), (fu, fv, bu, bv, masks) in truth.items():
            def pad(a, dtype):
                out = np.zeros((1,) + a.shape[:-1] + (stride,), dtype)
                out[0, ..., :ta.W] = a
                return out
            au, av, tr = ctx.accumulate_consistent(pad(fu, np.float32), pad(fv, np.float32), pad(bu, np.float32), pad(bv, np.float32), ta.W, 0.5, 1, False,
                                                   all_steps=False, masks=pad(masks, np.uint8))
            FF = fu.shape[0]
            assert (acc / str(k) / ("frame_%d.flo" % start)).read_bytes() == flo_bytes(au[0, 0].astype(np.float32), av[0, 0].astype(np.float32))
            assert (acc / str(k) / ("tracked_%d.pgm" % start)).read_bytes() == pgm_bytes(np.where(tr[0] == FF, 255, 255 * tr[0] // FF))
    finally:
        ctx.close()


def write_rate(folder, r, start, fu, fv, bu, bv):
    """one start of rate r under the names make_jets uses"""
    rate = ta.RATES[r]
    step = (rate["S"] - 1) * (200 // rate["fps"])
    folder.mkdir(parents=True, exist_ok=True)
    (folder / "config.cfg").write_text("# slow flow\nslow_flow_S\t%d\njet_fps\t%d\n" % (rate["S"], rate["fps"]))
    for f in range(fu.shape[0]):
        a = start + f * step
        ta.write_flo(folder / ("frame_%d.flo" % a), fu[f], fv[f])
        ta.write_flo(folder / ("frame_%d_back.flo" % (a + step)), bu[f], bv[f])


@pytest.mark.gpu
def test_center_and_extent_equal_a_run_on_cropped_files(host_build, tmp_path):
    """center 26,14 / extent 20,12 on 53 x 29 jets: columns 16 .. 35, rows 8 .. 19 (utils.cpp:308-318), the common cropped size being the target"""
    truth = ta.make_jets(tmp_path, seed=7)
    for (k, start), (fu, fv, bu, bv, _) in truth.items():
        write_rate(tmp_path / "cropped" / ta.RATES[k]["name"], k, start, *(a[:, 8:20, 16:36] for a in (fu, fv, bu, bv)))
    full = write_cfg(tmp_path, tmp_path / "full", tmp_path / "low", tmp_path / "high", "center\t26,14\nextent\t20,12\n")
    r = run_program(full)
    assert r.returncode == 0, r.stdout + r.stderr
    run = json.load(open(tmp_path / "full" / "accumulated" / "run.json"))
    assert (run["width"], run["height"]) == (20, 12) and [(q["source_width"], q["rescale"]) for q in run["rates"]] == [(ta.W, 1)] * 2
    cropped = write_cfg(tmp_path / "cropped", tmp_path / "pre", tmp_path / "cropped" / "low", tmp_path / "cropped" / "high")
    r = run_program(cropped)
    assert r.returncode == 0, r.stdout + r.stderr
    for k in (0, 1):
        for start in (10, 18):
            for name in ("frame_%d.flo" % start, "tracked_%d.pgm" % start):
                assert (tmp_path / "full" / "accumulated" / str(k) / name).read_bytes() == (tmp_path / "pre" / "accumulated" / str(k) / name).read_bytes()
    u, _ = read_flo(tmp_path / "full" / "accumulated" / "0" / "frame_10.flo")
    assert u.shape == (6, 10)


@pytest.mark.gpu
def test_refusals_by_message_and_status(host_build, tmp_path, monkeypatch):
    set_size(monkeypatch, SW, SH)
    ta.make_jets(tmp_path, seed=8)
    set_size(monkeypatch, TW, TH + 4)
    tae.make_frames(tmp_path)
    # a rate whose rescaled size is not the target: 13 x 10 by 4 is 52 x 40, the frames 52 x 44
    cfg = write_cfg(tmp_path, tmp_path / "mismatch", tmp_path / "low", tmp_path / "high")
    r = run_program(cfg, "-energies")
    assert r.returncode == 1 and "52 x 40, not the target 52 x 44" in r.stderr, r.stdout + r.stderr
    # a crop outside a flow
    cfg = write_cfg(tmp_path, tmp_path / "refused", tmp_path / "low", tmp_path / "high", "center\t10,8\nextent\t8,6\n")
    r = run_program(cfg)
    assert r.returncode == 1 and "the crop leaves the 13 x 10 flows" in r.stderr, r.stdout + r.stderr
    # occlusions together with center
    cfg = write_cfg(tmp_path, tmp_path / "refused", tmp_path / "low", tmp_path / "high", "center\t6,5\nextent\t8,6\nacc_occlusion\t1\n")
    r = run_program(cfg)
    assert r.returncode == 1 and "occlusions" in r.stderr and "center" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "refused").exists()
