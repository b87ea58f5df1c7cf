"""The accumulate program's -energies / -fuse through the resident track job in groups of acc_gpu_batch start_jets: a sequence of 5 start_jets and two
rates (the sizes and keys of tests/test_accumulate_energies.py / test_accumulate_fuse.py, acc_trws_max_iter 6) gives the same bytes whatever the batch,
batch 1 equals the restatement, run.json carries the grouping, -resume redoes one start_jet only, and a batch outside 1 .. 64 is refused by name.
Not covered: the refusal of an explicit batch whose job does not fit the device ("cannot be created ... bytes needed"), which needs a memory shortage."""
import json
import subprocess

import numpy as np
import pytest

import fuse_ref as fr
import test_accumulate as ta
import test_accumulate_energies as tae
import test_accumulate_fuse as taf
from synth import texture_frame
from test_accumulate import PROGRAM, host_build, read_flo, read_pgm  # noqa: F401  (host_build: the fixture)

pytestmark = pytest.mark.gpu
STARTS = (10, 18, 26, 34, 42)
W, H = taf.WF, ta.H
# what a run.json comparison between batches leaves out: the timing values, the grouping itself, and the paths (the runs write to different folders)
VARYING = ("timings_s", "weight_s", "fuse_call_s", "kernels_ms", "stage_ms", "group", "group_size", "gpu_batch", "groups", "cfg", "flo", "jet_estimation")


def make_sequence(root, sizes=None, h=H):
    """tests/test_accumulate.py's make_jets and tests/test_accumulate_energies.py's make_frames for the five start_jets; sizes: per rate the (w, h) its
    jets are stored at (default: the frames')"""
    rng = np.random.default_rng(0)
    truth = {}
    for r, rate in enumerate(ta.RATES):
        w_r, h_r = sizes[r] if sizes else (W, h)
        d = root / rate["name"]
        (d / "occlusion").mkdir(parents=True)
        (d / "config.cfg").write_text("# slow flow\nslow_flow_S\t%d\njet_fps\t%d\n" % (rate["S"], rate["fps"]))
        step = (rate["S"] - 1) * (200 // rate["fps"])
        FF = int(np.float32(np.float32(rate["fps"]) / np.float32(100)) * np.float32(2))
        for start in STARTS:
            fu, fv, _, _ = ta.smooth_flows(rng, FF, h_r, w_r, 0.8 * w_r / W)
            bu = -fu + (rng.standard_normal(fu.shape) * 0.05 * w_r / W).astype(np.float32)
            bv = -fv
            bu[0, 2:6, 3:9] += 3.0                                          # a block that contradicts the forward flow: no hypothesis there
            for f in range(FF):
                ta.write_flo(d / ("frame_%d.flo" % (start + f * step)), fu[f], fv[f])
                ta.write_flo(d / ("frame_%d_back.flo" % (start + (f + 1) * step)), bu[f], bv[f])
            truth[r, start] = (fu, fv, bu, bv, None)
    seq = root / "seq"
    seq.mkdir()
    for k, a in enumerate(range(STARTS[0], STARTS[-1] + 2 * tae.JETS + 1, 2)):
        tae.write_ppm(seq / ("frame_%d.ppm" % a), np.clip(np.rint(texture_frame(W, h, k)[:, :, :W]), 0, 255).astype(np.uint8))
    return truth, seq


def cfg_for(root, out, batch, name):
    extra = "acc_trws_max_iter\t6\n" + ("" if batch is None else "acc_gpu_batch\t%d\n" % batch)
    cfg = tae.write_cfg(root, out, extra)
    text = cfg.read_text().replace("ref_fps_F\t2", "ref_fps_F\t%d" % len(STARTS))
    path = root / name
    path.write_text(text)
    return path


def run_program(*args):
    return subprocess.run(["timeout", "-k", "10", "300", PROGRAM] + [str(a) for a in args], capture_output=True, text=True, timeout=330)


def files(acc):
    """every output file below acc but run.json: relative name -> bytes"""
    return {str(p.relative_to(acc)): p.read_bytes() for p in sorted(acc.rglob("*")) if p.is_file() and p.name != "run.json"}


def untimed(x):
    """run.json without its timing values, the grouping and the paths"""
    if isinstance(x, dict):
        return {k: untimed(v) for k, v in x.items() if k not in VARYING}
    return [untimed(v) for v in x] if isinstance(x, list) else x


@pytest.fixture
def width52(monkeypatch):
    monkeypatch.setattr(ta, "W", W)
    monkeypatch.setattr(tae, "W", W)


def test_every_batch_writes_the_same_bytes_and_batch_1_the_restatement(host_build, oracle, tmp_path, width52):
    truth, seq = make_sequence(tmp_path)
    out, runs = {}, {}
    for batch in (1, 2, 5, None):
        r = run_program(cfg_for(tmp_path, tmp_path / ("result_%s" % batch), batch, "b%s.cfg" % batch), "-fuse")
        assert r.returncode == 0, r.stdout + r.stderr
        assert "gpu batch: %d start_jet(s)" % (batch or 5) in r.stdout, r.stdout      # absent: the largest B <= 16 and <= the start_jets to do
        acc = tmp_path / ("result_%s" % batch) / "accumulated"
        out[batch], runs[batch] = files(acc), json.load(open(acc / "run.json"))
    assert len(out[1]) == 5 * (2 * 4 + 1 + 4)                               # per rate .flo, tracked, energy, occluded; best; fused .flo, _vis.png, occlusion, labels
    for batch in (2, 5, None):
        assert out[batch].keys() == out[1].keys()
        assert [k for k in out[1] if out[batch][k] != out[1][k]] == [], batch
        assert untimed(runs[batch]) == untimed(runs[1]), batch
    assert [runs[b]["gpu_batch"] for b in (1, 2, 5, None)] == [1, 2, 5, 5]
    assert [(g["group"], g["group_size"]) for g in runs[2]["groups"]] == [(0, 2), (1, 2), (2, 1)] and all(len(g["stage_ms"]) == 8 for g in runs[2]["groups"])
    assert [(s["group"], s["group_size"]) for s in runs[2]["fusion"]] == [(0, 2), (0, 2), (1, 2), (1, 2), (2, 1)]
    for key in ("weight_s", "fuse_call_s", "kernels_ms"):
        assert runs[2]["fusion"][0][key] == runs[2]["fusion"][1][key]       # the group's value in each of its start_jets
    acc = tmp_path / "result_1" / "accumulated"
    p = fr.Params(trws_max_iter=6)
    for start in STARTS:
        want = taf.expected(truth, seq, start, oracle, p)
        u, v = read_flo(acc / ("frame_%d.flo" % start))
        assert np.array_equal(u, want["u"].astype(np.float32)) and np.array_equal(v, want["v"].astype(np.float32)), start
        assert np.array_equal(read_pgm(acc / ("labels_%d.pgm" % start)), np.where(want["slot"] < 0, 255, want["slot"]).astype(np.uint8))
        assert np.array_equal(read_pgm(acc / "occlusions" / ("frame_%d.pgm" % start)), (want["occ"] * 255).astype(np.uint8))
        seg = [s for s in runs[1]["fusion"] if s["sequence_start"] == start][0]
        assert seg["energy"] == want["energy"] and seg["lower_bound"] == want["bound"] and seg["iterations"] == want["iters"]
    # -energies alone with batch 2: the per-rate files and best_*.pgm of the -fuse run, none of the fused outputs
    r = run_program(cfg_for(tmp_path, tmp_path / "plain", 2, "plain.cfg"), "-energies")
    assert r.returncode == 0, r.stdout + r.stderr
    plain = files(tmp_path / "plain" / "accumulated")
    assert plain == {k: v for k, v in out[1].items() if k.startswith(("0/", "1/", "best_"))} and len(plain) == 5 * 9
    # -resume after one fused .flo is gone: that start_jet alone is recomputed, identically
    acc2 = tmp_path / "result_2" / "accumulated"
    (acc2 / "frame_26.flo").unlink()
    r = run_program(tmp_path / "b2.cfg", "-fuse", "-resume")
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("already exists!") == 4 and "start 26: fused" in r.stdout and r.stdout.count(": fused") == 1
    assert files(acc2) == out[1]
    again = json.load(open(acc2 / "run.json"))
    assert again["gpu_batch"] == 2 and [s["sequence_start"] for s in again["fusion"]] == [26]


def test_a_batch_outside_1_to_64_is_refused_by_name(host_build, tmp_path, width52):
    make_sequence(tmp_path)
    for batch in (0, 65):
        r = run_program(cfg_for(tmp_path, tmp_path / "refused", batch, "r%d.cfg" % batch), "-fuse")
        assert r.returncode == 1 and "acc_gpu_batch %d" % batch in r.stderr, (r.stdout, r.stderr)
        assert not (tmp_path / "refused").exists()


def test_low_rate_at_half_the_size_batch_2_against_batch_1(host_build, tmp_path, width52):
    """the layout of tests/test_accumulate_scaled.py: the low rate's jets are stored at half the frames' size and resampled on the GPU"""
    make_sequence(tmp_path, sizes=[(W // 2, 20), (W, 40)], h=40)
    out = {}
    for batch in (1, 2):
        r = run_program(cfg_for(tmp_path, tmp_path / ("result_%d" % batch), batch, "s%d.cfg" % batch), "-fuse")
        assert r.returncode == 0, r.stdout + r.stderr
        acc = tmp_path / ("result_%d" % batch) / "accumulated"
        out[batch] = files(acc)
        run = json.load(open(acc / "run.json"))
        assert [(q["source_width"], q["rescale"]) for q in run["rates"]] == [(W // 2, 2), (W, 1)]
    assert out[1] == out[2] and len(out[1]) == 5 * 13
    tracked = read_pgm(tmp_path / "result_1" / "accumulated" / "0" / "tracked_26.pgm")
    assert 0 < (tracked == 255).sum() < tracked.size                        # the resampled rate has hypotheses, and not everywhere
