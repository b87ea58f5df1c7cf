"""The accumulate program's -fill flag end to end: the two-rate synthetic run of tests/test_accumulate_fuse.py (width 52) with acc_skip_pixel 0, written
edge maps and a block of flows corrupted so that no rate tracks it.  Plain -fuse leaves UNKNOWN_FLOW there; -fill leaves none, and its fused flow,
occlusions and labels equal the chain assembled here: the library's accumulation, the fill-in trajectories of the plain host chain
(tests/host/epic_fill_tool.cpp: one epic() per step on one shared edge map), the energies of both hypotheses per rate and sfa_fuse_hypotheses with four
slots.  Everything is compared with == on bytes or bit patterns."""
import json
import subprocess

import numpy as np
import pytest

import oracle as orc
import test_accumulate as ta
import test_accumulate_energies as tae
from test_accumulate import PROGRAM, host_build, read_flo, read_pgm  # noqa: F401  (host_build: the fixture)
from test_accumulate_fuse import WF, width52  # noqa: F401  (width52: the fixture)
from test_epic_fill import tool  # noqa: F401  (the fixture that builds tests/host/epic_fill_tool.cpp)

JETS, MIN_FPS = tae.JETS, tae.MIN_FPS
STARTS = (10, 18)
BLOCK = (slice(8, 20), slice(30, 44))            # rows, columns no rate tracks
INNER = (slice(11, 17), slice(33, 41))            # its interior: trajectories that start at the block's rim may leave it and stay consistent
UNKNOWN = 1e9                                    # UNKNOWN_FLOW is 1e10


def run(args, **kw):
    return subprocess.run(["timeout", "-k", "10", "300", PROGRAM] + [str(a) for a in args], capture_output=True, text=True, timeout=330, **kw)


def make_scene(root, seed=0):
    """jets with the block's backward flows off by 5 pixels at every step (tracked stops at 1 there), the frames, and truth as make_jets returns it"""
    truth = ta.make_jets(root, seed=seed)
    for r, rate in enumerate(ta.RATES):
        step = (rate["S"] - 1) * (200 // rate["fps"])
        for start in STARTS:
            fu, fv, bu, bv, _ = truth[r, start]
            bu[(slice(None),) + BLOCK] += np.float32(5)
            for f in range(fu.shape[0]):
                ta.write_flo(root / rate["name"] / ("frame_%d_back.flo" % (start + (f + 1) * step)), bu[f], bv[f])
    seq = tae.make_frames(root)
    return truth, seq


def write_cfg(root, out, extra="", skip_pixel=0):
    cfg = tae.write_cfg(root, out, "acc_trws_max_iter\t6\n" + extra)
    cfg.write_text(cfg.read_text().replace("acc_skip_pixel\t1", "acc_skip_pixel\t%d" % skip_pixel))
    return cfg


def write_edges(out, seed=0):
    """<output>/accumulated/tmp/edges_<start>.dat: a noise edge map per start_jet; returns them"""
    d = out / "accumulated" / "tmp"
    d.mkdir(parents=True)
    maps = {}
    for k, start in enumerate(STARTS):
        maps[start] = np.random.default_rng(seed + k).uniform(0.01, 0.5, (ta.H, WF)).astype(np.float32)
        maps[start].tofile(d / ("edges_%d.dat" % start))
    return maps


def chain(ctx, oracle, tool_exe, work, truth, seq, start, edges, trws_max_iter=6):
    """the fused result of one start_jet, assembled from the stages"""
    import slowflow_amd as sfa
    H = ta.H
    raw = []
    for f in range(JETS + 1):
        rgb = np.fromfile(seq / ("frame_%d.ppm" % (start + 2 * f)), np.uint8)[-3 * WF * H:].reshape(H, WF, 3)
        im = orc.aligned_zeros((3, H, orc.stride_of(WF)))
        im[:, :, :WF] = rgb.transpose(2, 0, 1).astype(np.float32)
        raw.append(im)
    work.mkdir()
    np.ascontiguousarray(raw[0]).tofile(work / "rgb.bin")                    # the 8-bit values of frame 0, before the normalisation
    edges.tofile(work / "edges.bin")
    frames = [f.copy() for f in raw]
    oracle.normalize(frames, WF)
    stack = np.ascontiguousarray(np.stack(frames))[None]
    acc = []
    for r in range(2):
        fu, fv, bu, bv, _ = truth[r, start]
        au, av, tr = ctx.accumulate_consistent(fu[None], fv[None], bu[None], bv[None], WF, 0.5, 0, False, all_steps=True)
        acc.append((au[0], av[0], tr[0]))
        au[0].tofile(work / ("acc_u_%d.bin" % r)); av[0].tofile(work / ("acc_v_%d.bin" % r)); tr[0].tofile(work / ("tracked_%d.bin" % r))
    rates = [a[0].shape[0] for a in acc]
    r = subprocess.run([tool_exe, str(work), str(WF), str(H), "0", "2", "0.001"] + [str(J) for J in rates], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    K = 4
    U, V = np.zeros((1, K, JETS, H, WF)), np.zeros((1, K, JETS, H, WF))
    E = np.full((1, K, H, WF), np.inf)
    O = np.zeros((1, K, H, WF), np.uint64)
    filled = []
    for r in range(2):
        J = rates[r]
        cu = np.fromfile(work / ("chain_u_%d.bin" % r), np.float64).reshape(J, H, WF)
        cv = np.fromfile(work / ("chain_v_%d.bin" % r), np.float64).reshape(J, H, WF)
        ct = np.fromfile(work / ("chain_tracked_%d.bin" % r), np.int32).reshape(H, WF)
        filled.append(bool((ct == J).all()))
        flows = None if r < MIN_FPS else tuple(a[None] for a in truth[MIN_FPS, start][:4])
        p = sfa.energy_params(skip=0, weight=float(r), acc_cv=0.25)
        for kind, (au, av, tr) in enumerate((acc[r], (cu, cv, ct))):
            if kind == 1 and not filled[r]:
                continue
            e, o, u, v = ctx.hypothesis_energies(p, J, au[None], av[None], tr[None], stack, WF, flows=flows, adapted=True)
            E[0, 2 * r + kind], O[0, 2 * r + kind], U[0, 2 * r + kind], V[0, 2 * r + kind] = e[0], o[0], u[0], v[0]
    weight = ctx.smoothness_weight(frames[0], WF)
    out = ctx.fuse_hypotheses(sfa.fuse_params(skip=0, trws_max_iter=trws_max_iter), U, V, E, O, weight[None], WF, H)
    return out, filled, acc


@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_program_fill_end_to_end(host_build, tool, ctx, oracle, tmp_path, width52):
    truth, seq = make_scene(tmp_path)
    # plain -fuse: the block has no hypothesis of either rate
    cfg = write_cfg(tmp_path, tmp_path / "plain")
    r = run([cfg, "-fuse"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "EpicFlow's fill-in and the neighbour proposals are not run" in r.stdout         # the line of the program without -fill
    plain = tmp_path / "plain" / "accumulated"
    pj = json.load(open(plain / "run.json"))
    assert pj["epic_interpolation"] is False and "epic_fill" not in pj and "slots" not in pj
    for start in STARTS:
        u, v = read_flo(plain / ("frame_%d.flo" % start))
        assert (u[INNER] > UNKNOWN).all() and (v[INNER] > UNKNOWN).all()                    # the scene does exercise the gap
        assert (read_pgm(plain / ("labels_%d.pgm" % start))[INNER] == 255).all()
    # -fill
    out = tmp_path / "result"
    edges = write_edges(out)
    cfg = write_cfg(tmp_path, out)
    r = run([cfg, "-fill", "-resume"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "are not run" not in r.stdout
    acc = out / "accumulated"
    rj = json.load(open(acc / "run.json"))
    assert rj["fused"] is True and rj["epic_fill"] is True and len(rj["fusion"]) == 2
    assert rj["slots"] == [{"slot": k, "rate": k // 2, "kind": "epic_fill" if k % 2 else "accumulated"} for k in range(4)]
    for start in STARTS:
        want, filled, stage_acc = chain(ctx, oracle, tool, tmp_path / ("chain_%d" % start), truth, seq, start, edges[start])
        assert all(filled)
        u, v = read_flo(acc / ("frame_%d.flo" % start))
        assert (np.abs(u) < UNKNOWN).all() and (np.abs(v) < UNKNOWN).all()                  # no hole is left
        assert np.array_equal(u.view(np.uint32), want["u"][0].astype(np.float32).view(np.uint32))
        assert np.array_equal(v.view(np.uint32), want["v"][0].astype(np.float32).view(np.uint32))
        labels = read_pgm(acc / ("labels_%d.pgm" % start))
        assert np.array_equal(labels, want["slot"][0].astype(np.uint8)) and (want["slot"][0] >= 0).all()
        assert (labels[INNER] % 2 == 1).all() and (labels % 2 == 0).any()                   # fill-in slots in the block, accumulated ones elsewhere
        assert np.array_equal(read_pgm(acc / "occlusions" / ("frame_%d.pgm" % start)), (want["occ"][0] * 255).astype(np.uint8))
        seg = [s for s in rj["fusion"] if s["sequence_start"] == start][0]
        assert seg["energy"] == want["energy"][0] and seg["lower_bound"] == want["bound"][0] and seg["iterations"] == want["iters"][0]
        assert seg["nodes"] == ta.H * WF
        import fill_ref
        for rate in (0, 1):
            rec = [f for f in rj["fill"] if f["sequence_start"] == start and f["rate"] == rate]
            J = stage_acc[rate][0].shape[0]
            mask = fill_ref.consistent_regions(stage_acc[rate][2], J)
            xs, ys = fill_ref.fill_samples(WF, 2), fill_ref.fill_samples(ta.H, 2)
            assert rec == [{"sequence_start": start, "rate": rate, "kept_pixels": int(mask.sum()), "matches": int(mask[np.ix_(ys, xs)].sum()), "filled": True}]
    # the rates' own files do not depend on the flag: the stage calls write what the track job of -fuse writes
    cfg0 = write_cfg(tmp_path, tmp_path / "fuse0")
    r0 = run([cfg0, "-fuse"])
    assert r0.returncode == 0
    for start in STARTS:
        assert (tmp_path / "fuse0" / "accumulated" / ("best_%d.pgm" % start)).read_bytes() == (acc / ("best_%d.pgm" % start)).read_bytes()
        assert (tmp_path / "fuse0" / "accumulated" / ("frame_%d.flo" % start)).read_bytes() == (plain / ("frame_%d.flo" % start)).read_bytes()
        for rate in (0, 1):
            for name in ("frame_%d.flo" % start, "tracked_%d.pgm" % start, "energy_%d.pfm" % start, "occluded_%d.pgm" % start):
                assert (tmp_path / "fuse0" / "accumulated" / str(rate) / name).read_bytes() == (acc / str(rate) / name).read_bytes(), name
    # -resume skips a start_jet whose fused .flo exists
    before = (acc / "frame_10.flo").read_bytes()
    r = run([cfg, "-fill", "-select", "0", "-resume"])
    assert r.returncode == 0 and "already exists!" in r.stdout and (acc / "frame_10.flo").read_bytes() == before


@pytest.mark.gpu
def test_program_fill_missing_edge_file_and_refusals(host_build, tmp_path, width52):
    make_scene(tmp_path, seed=1)
    out = tmp_path / "result"
    write_edges(out)
    (out / "accumulated" / "tmp" / "edges_18.dat").unlink()
    cfg = write_cfg(tmp_path, out)
    r = run([cfg, "-fill", "-resume"])
    assert r.returncode == 2 and "edges_18.dat" in r.stderr, (r.stdout, r.stderr)
    assert sorted(p.name for p in (out / "accumulated").iterdir()) == ["tmp"]               # nothing was written
    cases = [(dict(skip_pixel=1), "acc_skip_pixel"), (dict(extra="acc_epic_interpolation\t0\n"), "acc_epic_interpolation"),
             (dict(extra="".join("jet_estimation\t%s/\n" % (tmp_path / "low") for _ in range(7))), "more than 8 rates")]
    for kw, word in cases:
        cfg = write_cfg(tmp_path, tmp_path / "refused", **kw)
        r = run([cfg, "-fill"])
        assert r.returncode == 1 and "-fill" in r.stderr and word in r.stderr, (word, r.stdout, r.stderr)
        assert not (tmp_path / "refused").exists()
    cfg = write_cfg(tmp_path, tmp_path / "refused", extra="acc_approach\t1\n")               # what -fuse refuses, -fill refuses
    r = run([cfg, "-fill"])
    assert r.returncode == 1 and "acc_approach 1" in r.stderr and not (tmp_path / "refused").exists()
