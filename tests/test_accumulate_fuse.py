"""The accumulate program's -fuse flag end to end: the two-rate synthetic run of tests/test_accumulate_energies.py at a width that is a multiple of 4,
against tests/energy_ref.py (energies, adapted flows) and tests/fuse_ref.py (smoothness weight, NMS, pairwise terms, TRW-S)."""
import json
import subprocess

import numpy as np
import pytest

import fuse_ref as fr
import oracle as orc
import test_accumulate as ta
import test_accumulate_energies as tae
from accum_ref import accumulate, grid
from energy_ref import Params, derivatives, energies, flows_for_rate
from test_accumulate import PROGRAM, host_build, read_flo, read_pgm  # noqa: F401  (host_build: the fixture)

WF = 52                   # the fusion refuses a width that is not a multiple of 4; tests/test_accumulate.py's W is 53
JETS, MIN_FPS = tae.JETS, tae.MIN_FPS


@pytest.fixture
def width52(monkeypatch):
    monkeypatch.setattr(ta, "W", WF)
    monkeypatch.setattr(tae, "W", WF)


def expected(truth, seq_dir, start, oracle, p):
    """the fused outputs of one start_jet, restated: frames as the program ingests and normalises them, per rate the energies and adapted flows,
    the smoothness weight of normalised frame 0 (img_norm_* absent: avg 0, std 1), then the fusion"""
    H = ta.H
    frames = []
    for f in range(JETS + 1):
        rgb = np.fromfile(seq_dir / ("frame_%d.ppm" % (start + 2 * f)), np.uint8)[-3 * WF * H:].reshape(H, WF, 3)
        im = orc.aligned_zeros((3, H, orc.stride_of(WF)))
        im[:, :, :WF] = rgb.transpose(2, 0, 1).astype(np.float32)
        frames.append(im)
    oracle.normalize(frames, WF)
    stack = np.ascontiguousarray(np.stack(frames)[..., :WF])
    dx, dy = derivatives(oracle, stack, WF)
    gw, gh, _, _ = grid(WF, H, 1)
    K = 2
    U, V = np.zeros((K, JETS, gh, gw)), np.zeros((K, JETS, gh, gw))
    E = np.full((K, gh, gw), np.inf)
    O = np.zeros((K, gh, gw), np.uint64)
    for r in range(K):
        fu, fv, bu, bv, _ = truth[r, start]
        au, av, tr = accumulate(fu, fv, bu, bv, None, 0.5, 1, False)
        e, b, terms = energies(Params(skip=1, weight=float(r), acc_cv=0.25), fu.shape[0], au, av, tr, stack, dx, dy,
                               flows_for_rate(r, MIN_FPS, truth[MIN_FPS, start][:4]))
        E[r], O[r] = e, b
        U[r][:, terms["hy"], terms["hx"]] = terms["U"]
        V[r][:, terms["hy"], terms["hx"]] = terms["V"]
    weight = fr.smoothness_weight(oracle, frames[0], WF)
    return fr.fuse(U, V, E, O, weight, p, WF)


@pytest.mark.gpu
def test_program_fuse_end_to_end(host_build, oracle, tmp_path, width52):
    truth = ta.make_jets(tmp_path)
    seq = tae.make_frames(tmp_path)
    cfg = tae.write_cfg(tmp_path, tmp_path / "result", "acc_trws_max_iter\t6\n")
    r = subprocess.run(["timeout", "-k", "10", "300", PROGRAM, str(cfg), "-fuse"], capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "EpicFlow" in r.stdout                                           # acc_epic_interpolation 1 (the default): said, and not run
    acc = tmp_path / "result" / "accumulated"
    run = json.load(open(acc / "run.json"))
    assert run["fused"] is True and run["epic_interpolation"] is False and len(run["fusion"]) == 2
    p = fr.Params(trws_max_iter=6)
    for start in (10, 18):
        want = expected(truth, seq, start, oracle, p)
        u, v = read_flo(acc / ("frame_%d.flo" % start))
        assert np.array_equal(u, want["u"].astype(np.float32)) and np.array_equal(v, want["v"].astype(np.float32))
        assert np.array_equal(read_pgm(acc / ("labels_%d.pgm" % start)), np.where(want["slot"] < 0, 255, want["slot"]).astype(np.uint8))
        assert np.array_equal(read_pgm(acc / "occlusions" / ("frame_%d.pgm" % start)), (want["occ"] * 255).astype(np.uint8))
        assert (acc / ("frame_%d_vis.png" % start)).stat().st_size > 0
        seg = [s for s in run["fusion"] if s["sequence_start"] == start][0]
        assert seg["energy"] == want["energy"] and seg["lower_bound"] == want["bound"] and seg["iterations"] == want["iters"]
        assert seg["nodes"] == int((want["slot"] >= 0).sum()) > 0
    # -energies alone writes the same per-rate files and best_*.pgm, and none of the fused outputs
    cfg2 = tae.write_cfg(tmp_path, tmp_path / "plain", "acc_trws_max_iter\t6\n")
    r = subprocess.run(["timeout", "-k", "10", "300", PROGRAM, str(cfg2), "-energies"], capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = tmp_path / "plain" / "accumulated"
    for start in (10, 18):
        assert (plain / ("best_%d.pgm" % start)).read_bytes() == (acc / ("best_%d.pgm" % start)).read_bytes()
        for rate in (0, 1):
            for name in ("frame_%d.flo" % start, "tracked_%d.pgm" % start, "energy_%d.pfm" % start, "occluded_%d.pgm" % start):
                assert (plain / str(rate) / name).read_bytes() == (acc / str(rate) / name).read_bytes()
    assert not list(plain.glob("labels_*")) and not (plain / "occlusions").exists() and "fused" not in json.load(open(plain / "run.json"))


@pytest.mark.gpu
def test_program_fuse_without_pairwise_terms_picks_the_best_rate(host_build, tmp_path, width52):
    ta.make_jets(tmp_path, seed=3)
    tae.make_frames(tmp_path)
    cfg = tae.write_cfg(tmp_path, tmp_path / "result", "acc_beta\t0\nacc_spatial_occ\t0\n")
    r = subprocess.run(["timeout", "-k", "10", "300", PROGRAM, str(cfg), "-fuse"], capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, r.stdout + r.stderr
    acc = tmp_path / "result" / "accumulated"
    for start in (10, 18):
        assert np.array_equal(read_pgm(acc / ("labels_%d.pgm" % start)), read_pgm(acc / ("best_%d.pgm" % start)))
    # -resume skips a start_jet whose fused .flo exists
    r = subprocess.run(["timeout", "-k", "10", "300", PROGRAM, str(cfg), "-fuse", "-select", "0", "-resume"], capture_output=True, text=True, timeout=330)
    assert r.returncode == 0 and "already exists!" in r.stdout


@pytest.mark.gpu
def test_program_fuse_refusals(host_build, tmp_path):
    ta.make_jets(tmp_path, seed=2)                                          # width 53: refused by -fuse, accepted by -energies
    tae.make_frames(tmp_path)
    cases = [("acc_approach\t1\n", "acc_approach 1"), ("acc_traj_sim_method\t2\n", "acc_traj_sim_method 2"), ("", "multiple of 4"),
             ("".join("jet_estimation\t%s/\n" % (tmp_path / "low") for _ in range(15)), "more than 16 rates")]
    for extra, msg in cases:
        cfg = tae.write_cfg(tmp_path, tmp_path / "refused", extra)
        r = subprocess.run(["timeout", "-k", "10", "300", PROGRAM, str(cfg), "-fuse"], capture_output=True, text=True, timeout=330)
        assert r.returncode == 1 and msg in r.stderr, (msg, r.stdout, r.stderr)
