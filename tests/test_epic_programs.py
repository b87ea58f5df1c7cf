"""The programs with EpicFlow's graph searches on the GPU: slow_flow with `gpu_epic 1` and adaptiveFR with -gpu_epic write, file for file and byte for byte,
what they write without -- epic_batch returns epic()'s fields, and everything after the initial flow is the same code.  Modelled on
test_host.py::test_driver_deep_matching_initialisation and test_adaptive_fr.py::test_program_end_to_end."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from synth import texture_frame
from test_host import write_ppm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
# Both runs of a program work in the same directory (the first one's tree is moved aside), so no path differs.  What differs by design: the wall-clock
# reports (the driver's run.json and timings.json hold seconds), and for the driver the copy of the configuration, which holds the key
TIMINGS, CONFIG = ("timings.json", "run.json"), "config.cfg"


@pytest.fixture(scope="module")
def host_build():
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return HOST


def tree(root, not_compared):
    """relative path -> bytes of every file under root"""
    out = {}
    for dirpath, _, files in os.walk(root):
        for fn in files:
            if fn not in not_compared:
                p = os.path.join(dirpath, fn)
                out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def assert_same_trees(a, b, must_hold, not_compared):
    ta, tb = tree(a, not_compared), tree(b, not_compared)
    assert sorted(ta) == sorted(tb)
    for name in must_hold:
        assert name in ta, (name, sorted(ta))
    differing = [n for n in ta if ta[n] != tb[n]]
    assert not differing, differing


@pytest.mark.gpu
def test_driver_writes_the_same_files_with_gpu_epic(host_build, tmp_path):
    w, h, jets, S = 128, 96, 2, 2
    steps = S - 1
    nframes = 1 + (jets + 2) * steps
    DX, DY = 7.0, -4.0
    frames = [np.clip(np.round(texture_frame(w, h, k, dx=DX, dy=DY)[:, :, :w]), 0, 255) for k in range(nframes)]
    rng = np.random.default_rng(3)
    matches, edges = {}, {}
    for j in range(jets):
        a, b = 10 + j, 11 + j
        for (p, q, sx, sy) in ((a, b, DX, DY), (b, a, -DX, -DY)):
            rows = []
            for k in range(400):
                x, y = (rng.uniform(12, w - 13), rng.uniform(8, h - 9)) if k % 4 else (float(16 + 8 * (k // 4 % 12)), float(16 + 8 * (k // 48)))     # a quarter on a lattice
                rows.append("%.3f %.3f %.3f %.3f 3.1 1\n" % (x, y, x + sx + rng.normal(0, 0.2), y + sy + rng.normal(0, 0.2)))
            matches[(p, q)] = "".join(rows)
    for n in range(10, 11 + jets):
        e = (0.05 + 0.02 * rng.uniform(0, 1, (h, w))).astype(np.float32)
        e[:, w // 2] = 0.8
        edges[n] = e
    outs = []
    for key in (0, 1):
        root = tmp_path / "work"
        (root / "out" / "tmp").mkdir(parents=True)
        for k, f in enumerate(frames):
            write_ppm(str(root / ("f_%03d.ppm" % (10 - steps + k))), f)
        for (p, q), text in matches.items():
            (root / "out" / "tmp" / ("matches_%d_%d.dat" % (p, q))).write_text(text)
        for n, e in edges.items():
            e.tofile(str(root / "out" / "tmp" / ("edges_%d.dat" % n)))
        cfg = root / "run.cfg"
        cfg.write_text(("file\t%s/f_%%03i.ppm\noutput\t%s/out\nJets\t%d\nstart\t10\nmax_fps\t200\n16bit\t0\nraw\t0\nscale\t1.0\ndeep_matching\t1\ndm_scale\t1.0\nverbose\t00001\n"
                        "slow_flow_S\t%d\nslow_flow_layers\t1\nslow_flow_niter_alter\t1\nslow_flow_niter_outer\t3\nslow_flow_occlusion_reasoning\t0\n"
                        "slow_flow_thres_outer\t0\nslow_flow_thres_inner\t0\nslow_flow_rho_0\t1\nslow_flow_omega_0\t0\ngpus\t1\ngpu_streams\t1\ngpu_batch\t3\ngpu_epic\t%d\n")
                       % (root, root, jets, S, key))
        r = subprocess.run([os.path.join(HOST, "slow_flow"), str(cfg), "-overwrite"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        shutil.move(str(root), str(tmp_path / ("run%d" % key)))
        outs.append(str(tmp_path / ("run%d" % key) / "out"))
    assert_same_trees(outs[0], outs[1], ["f_010.flo", "f_011_back.flo", "f_011.flo", os.path.join("tmp", "frame_10_INIT.png")], TIMINGS + (CONFIG,))


@pytest.mark.gpu
def test_adaptive_fr_writes_the_same_files_with_gpu_epic(host_build, tmp_path):
    W, H, DX, DY = 256, 192, 2.0, -1.0
    scale, skip, step, samples = 0.25, 2, 3, 3
    sw, sh = int(W * scale), int(H * scale)
    fu, fv = DX * skip * scale, DY * skip * scale
    ys, xs = np.mgrid[2:sh - 2:3, 2:sw - 2:3]                          # matches on a lattice over constant edges: neighbour lists full of ties
    outs = []
    for key in (0, 1):
        seq = tmp_path / "data" / "seqA"
        seq.mkdir(parents=True)
        for k in range(step * (samples - 1) + skip + 1):
            write_ppm(str(seq / ("%07i.ppm" % k)), texture_frame(W, H, k, DX, DY)[:, :, :W])
        tmpd = seq / "adaptiveFR" / "tmp"
        tmpd.mkdir(parents=True)
        for i in range(samples):
            a = i * step
            with open(str(tmpd / ("matches_%d_%d.dat" % (a, a + skip))), "w") as f:
                for x, y in zip(xs.ravel(), ys.ravel()):
                    f.write("%d %d %g %g 1.0 0\n" % (x, y, x + fu, y + fv))
            np.ones(sw * sh, np.float32).tofile(str(tmpd / ("edges_%d.dat" % a)))
        cmd = [os.path.join(HOST, "adaptiveFR"), "-path", str(tmp_path / "data") + "/", "-folder", "seqA", "-format", "%07i.ppm", "-samples", str(samples),
               "-step", str(step), "-skip", str(skip), "-scale", str(scale)] + (["-gpu_epic"] if key else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        shutil.move(str(tmp_path / "data"), str(tmp_path / ("data%d" % key)))
        outs.append(str(tmp_path / ("data%d" % key)))
    assert_same_trees(outs[0], outs[1], ["results.info", os.path.join("seqA", "quantil.dat"), os.path.join("seqA", "adaptiveFR", "config.cfg"),
                                         os.path.join("seqA", "adaptiveFR", "%07i.flo" % 0), os.path.join("seqA", "adaptiveFR", "%07i.flo" % (step * (samples - 1)))], TIMINGS)
