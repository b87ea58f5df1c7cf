"""The accumulate program's -energies flag end to end: frames from tests/synth.py, flows written by tests/test_accumulate.py's make_jets, two rates with
acc_min_fps 1 (so rate 0 sees empty flows and adapts 2 steps to Jets = 4), against tests/accum_ref.py and tests/energy_ref.py.  Without the flag the
program writes exactly what it wrote before."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle as orc
import slowflow_amd as sfa
from accum_ref import accumulate
from energy_ref import Params, derivatives, energies, flows_for_rate
from synth import texture_frame
from test_accumulate import H, PROGRAM, W, host_build, make_jets, read_pgm  # noqa: F401  (host_build: the fixture)

JETS, MIN_FPS = 4, 1


def write_ppm(path, rgb):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[2], rgb.shape[1]))
        f.write(np.ascontiguousarray(rgb.transpose(1, 2, 0)).tobytes())


def make_frames(root):
    """frames 10 .. 26 (start_jet 0: 10, 12, .. 18; start_jet 1: 18 .. 26), 8-bit RGB"""
    d = root / "seq"
    d.mkdir()
    for k, a in enumerate(range(10, 27, 2)):
        write_ppm(d / ("frame_%d.ppm" % a), np.clip(np.rint(texture_frame(W, H, k)[:, :, :W]), 0, 255).astype(np.uint8))
    return d


def write_cfg(root, out, extra=""):
    # acc_min_fps 1: steps 2, Jets = 200 / (25 * 2) = 4, skip 1; rate 0 has r_Jets = 0.5 * 4 = 2 (2 steps of 4 frames), rate 1 r_Jets = 4
    lines = ["jet_estimation\t%s/" % (root / "low"), "jet_estimation\t%s/" % (root / "high"), "flow_format\tframe_%i", "output\t%s" % out, "start\t10",
             "file\t%s/frame_%%i.ppm" % (root / "seq"), "ref_fps\t25", "ref_fps_F\t2", "max_fps\t200", "acc_min_fps\t%d" % MIN_FPS, "acc_skip_pixel\t1",
             "acc_discard_inconsistent\t0", "acc_consistency_threshold\t0.5", "acc_cv\t0.25"]
    cfg = root / "dense_tracking.cfg"
    cfg.write_text("\n".join(lines) + "\n" + extra)
    return cfg


def read_pfm(path):
    data = open(path, "rb").read()
    head = data.split(b"\n", 3)
    assert head[0] == b"Pf" and float(head[2]) < 0
    w, h = map(int, head[1].split())
    return np.frombuffer(head[3], "<f4").reshape(h, w)[::-1]


def expected(truth, seq_dir, start, oracle):
    """per rate (energy float32, occluded count) and the best rate, restated"""
    frames = []
    for f in range(JETS + 1):
        rgb = np.fromfile(seq_dir / ("frame_%d.ppm" % (start + 2 * f)), np.uint8)[-3 * W * H:].reshape(H, W, 3)
        fr = orc.aligned_zeros((3, H, orc.stride_of(W)))
        fr[:, :, :W] = rgb.transpose(2, 0, 1).astype(np.float32)
        frames.append(fr)
    oracle.normalize(frames, W)
    fr = np.ascontiguousarray(np.stack(frames)[..., :W])
    dx, dy = derivatives(oracle, fr, W)
    min_flows = truth[MIN_FPS, start][:4]
    out = {}
    for r in (0, 1):
        fu, fv, bu, bv, _ = truth[r, start]
        au, av, tr = accumulate(fu, fv, bu, bv, None, 0.5, 1, False)
        p = Params(skip=1, weight=float(r), acc_cv=0.25)
        e, b, _ = energies(p, fu.shape[0], au, av, tr, fr, dx, dy, flows_for_rate(r, MIN_FPS, min_flows))
        cnt = np.array([bin(int(x)).count("1") for x in b.ravel()], np.uint8).reshape(b.shape)
        out[r] = (e.astype(np.float32), cnt, int((tr == fu.shape[0]).sum()))
    e0, e1 = out[0][0], out[1][0]
    best = np.where(np.isinf(e0) & np.isinf(e1), 255, np.where(e1 < e0, 1, 0)).astype(np.uint8)
    return out, best


@pytest.mark.gpu
def test_program_energies_end_to_end(host_build, oracle, tmp_path):
    truth = make_jets(tmp_path)
    seq = make_frames(tmp_path)
    cfg = write_cfg(tmp_path, tmp_path / "result")
    r = subprocess.run([PROGRAM, str(cfg), "-energies"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    acc = tmp_path / "result" / "accumulated"
    run = json.load(open(acc / "run.json"))
    assert run["energies"] is True and run["Jets"] == JETS and len(run["segments"]) == 4 and run["timings_s"]["energy_call"] > 0
    for start in (10, 18):
        out, best = expected(truth, seq, start, oracle)
        for rate in (0, 1):
            e, cnt, created = out[rate]
            got = read_pfm(acc / str(rate) / ("energy_%d.pfm" % start))
            assert np.array_equal(got, e)
            assert np.array_equal(read_pgm(acc / str(rate) / ("occluded_%d.pgm" % start)), cnt)
            seg = [s for s in run["segments"] if s["rate"] == rate and s["sequence_start"] == start][0]
            assert seg["hypotheses"] == created and 0 < created
        assert np.array_equal(read_pgm(acc / ("best_%d.pgm" % start)), best)
        assert set(np.unique(best)) <= {0, 1, 255}
    # without the flag: the same .flo and tracked files, byte for byte, and no energy outputs
    cfg2 = write_cfg(tmp_path, tmp_path / "plain")
    r = subprocess.run([PROGRAM, str(cfg2)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = tmp_path / "plain" / "accumulated"
    for rate in (0, 1):
        for start in (10, 18):
            for name in ("frame_%d.flo" % start, "tracked_%d.pgm" % start):
                assert (plain / str(rate) / name).read_bytes() == (acc / str(rate) / name).read_bytes()
    assert not list(plain.rglob("energy_*")) and not list(plain.rglob("best_*"))


@pytest.mark.gpu
def test_program_energies_refusals_and_missing_frames(host_build, tmp_path):
    make_jets(tmp_path, seed=2)
    seq = make_frames(tmp_path)
    for extra in ("acc_occlusion\t1\n", "grayscale\t1\n"):
        cfg = write_cfg(tmp_path, tmp_path / "refused", extra)
        r = subprocess.run([PROGRAM, str(cfg), "-energies"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and extra.split("\t")[0] in r.stderr
    cfg = write_cfg(tmp_path, tmp_path / "result")
    missing = seq / "frame_22.ppm"
    missing.unlink()
    r = subprocess.run([PROGRAM, str(cfg), "-energies"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and str(missing) in r.stderr.replace("//", "/")
    # -select 0 needs frames 10 .. 18 only; a second run with -resume finds best_10.pgm and skips the start_jet
    r = subprocess.run([PROGRAM, str(cfg), "-energies", "-select", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([PROGRAM, str(cfg), "-energies", "-select", "0", "-resume"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "already exists!" in r.stdout
    assert os.path.exists(tmp_path / "result" / "accumulated" / "best_10.pgm")
