"""epic_fill_rate (slowflow_amd/host/epic_fill.cpp): dense_tracking's EpicFlow fill-in of a rate -- sfa_consistent_regions, sfa_fill_matches, ONE epic_batch of
r_Jets images, sfa_fill_trajectories -- against the plain chain on the host (tests/host/epic_fill_tool.cpp): the restated region growing, the match loop,
one epic() call per step on one shared edge map, the scaling.  The trajectories are compared by their bit patterns.  A 96 x 64 scene (test_epic.scene's
image, a noise edge map), two rates of 2 and 4 steps with the call index carried from the first to the second.  test_epic.scene is the builder that
tests/test_epic_fit.py's scenes come from (it imports it), and its strides are tests/synth.py's stride_of; only its image is used here, since the matches
come from the trajectories and the edge map is noise."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_epic import scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
W, H = 96, 64
RATES = (2, 4)


def test_the_host_call_is_declared_and_built():
    text = open(os.path.join(HOST, "epic_fill.h")).read()
    assert re.search(r"\bint\s+epic_fill_rate\s*\(", text) and re.search(r"\bvoid\s+epic_fill_params\s*\(", text)
    assert "epic_fill.o" in open(os.path.join(HOST, "Makefile")).read()
    src = open(os.path.join(HOST, "epic_fill.cpp")).read()
    assert len(re.findall(r"\bepic_batch\s*\(", src)) == 1 and not re.search(r"\bepic\s*\(", src)      # one batch, no call per step


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path_factory.mktemp("epic_fill") / "epic_fill_tool")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-pthread", "-I", HOST, os.path.join(ROOT, "tests", "host", "epic_fill_tool.cpp"), os.path.join(HOST, "libslowflow_host.a"),
                        "-L", os.path.join(ROOT, "slowflow_amd"), "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "slowflow_amd"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def trajectories(J, seed, consistent=True):
    """accumulated trajectories of J steps on the W x H grid: a piecewise-affine motion that grows with the step, and a tracked map whose consistent
    pixels (tracked == J) form one large region with holes, plus islands of 81 pixels; consistent=False: the islands only"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    right = xx > W * 0.55
    u = np.where(right, 3.0 + 0.02 * (xx - W / 2), -1.5 + 0.01 * yy)
    v = np.where(right, -2.0 + 0.015 * yy, 0.5 - 0.01 * (xx - 10))
    acc_u = np.stack([(j + 1) / J * u + rng.normal(0, 0.05, (H, W)) for j in range(J)])
    acc_v = np.stack([(j + 1) / J * v + rng.normal(0, 0.05, (H, W)) for j in range(J)])
    tracked = np.full((H, W), J, np.int32)
    tracked[20:44, 30:70] = rng.integers(0, J, (24, 40))                      # a hole no trajectory crosses
    tracked[:, 80:82] = 0                                                     # a strip that cuts the right edge off ...
    tracked[0:50, 82:] = rng.integers(0, J, (50, W - 82))
    tracked[50:, 82:] = 1 if J > 1 else 0
    tracked[52:61, 84:93] = J                                                 # ... where one island of 81 pixels is left
    if not consistent:
        keep = np.zeros((H, W), bool)
        keep[52:61, 84:93] = keep[3:12, 3:12] = keep[30:39, 40:49] = True
        tracked = np.where(keep, J, 0).astype(np.int32)
    return acc_u, acc_v, tracked


def run_tool(tool, d, rates, inputs, euc, seed=0, epic_skip=2):
    rgb, _, _ = scene(W, H, seed)
    edges = np.random.default_rng(seed + 40).uniform(0.01, 0.5, (H, W)).astype(np.float32)     # a noise edge map
    rgb.tofile(os.path.join(d, "rgb.bin"))
    edges.tofile(os.path.join(d, "edges.bin"))
    for r, (au, av, tr) in enumerate(inputs):
        au.tofile(os.path.join(d, "acc_u_%d.bin" % r))
        av.tofile(os.path.join(d, "acc_v_%d.bin" % r))
        tr.tofile(os.path.join(d, "tracked_%d.bin" % r))
    r = subprocess.run([tool, d, str(W), str(H), "0", repr(epic_skip), repr(euc)] + [str(J) for J in rates], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^rate (\d+) chain (\d) (\d+) (\d+) fill (\d) (\d+) (\d+) index (\d+)$", r.stdout, flags=re.M)
    assert len(lines) == len(rates), r.stdout
    out = []
    for k, J in enumerate(rates):
        rd = lambda name, dt, shape: np.fromfile(os.path.join(d, "%s_%d.bin" % (name, k)), dt).reshape(shape)
        out.append(dict(line=[int(x) for x in lines[k]],
                        chain=(rd("chain_u", np.float64, (J, H, W)), rd("chain_v", np.float64, (J, H, W)), rd("chain_tracked", np.int32, (H, W))),
                        fill=(rd("fill_u", np.float64, (J, H, W)), rd("fill_v", np.float64, (J, H, W)), rd("fill_tracked", np.int32, (H, W)))))
    return out


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_rate(res, J, filled, index):
    k, cf, ck, cm, ff, fk, fm, idx = res["line"]
    assert (cf, ff) == (filled, filled) and ck == fk and cm == fm and idx == index, res["line"]
    assert same_bits(res["fill"][0], res["chain"][0]) and same_bits(res["fill"][1], res["chain"][1]) and np.array_equal(res["fill"][2], res["chain"][2])
    if filled:
        assert (res["fill"][2] == J).all() and len(np.unique(res["fill"][0])) > 50 and np.isfinite(res["fill"][0]).all()
        assert ck >= 100 and cm >= 160                                        # (enough matches for nn 160: no other path of epic() is taken)
    else:
        assert (res["fill"][0] == -7).all() and (res["fill"][1] == -7).all() and (res["fill"][2] == -7).all()      # nothing written


@pytest.mark.gpu
@pytest.mark.parametrize("euc", (0.001, 0.25))
def test_two_rates_equal_the_chain_of_single_epic_calls(tool, tmp_path, euc):
    """euc 0.25: the costs are noise of 0.01 .. 0.5, so one addition more or fewer moves region borders, not only last bits -- shown by running the second
    rate's inputs as a first rate: without the two additions of rate 0's calls its result differs"""
    inputs = [trajectories(J, 10 + J) for J in RATES]
    d = tmp_path / "two"
    d.mkdir()
    res = run_tool(tool, str(d), RATES, inputs, euc)
    check_rate(res[0], RATES[0], 1, RATES[0])
    check_rate(res[1], RATES[1], 1, RATES[0] + RATES[1])
    if euc == 0.25:
        d2 = tmp_path / "alone"
        d2.mkdir()
        alone = run_tool(tool, str(d2), RATES[1:], inputs[1:], euc)
        check_rate(alone[0], RATES[1], 1, RATES[1])
        diff = np.abs(alone[0]["fill"][0] - res[1]["fill"][0])
        assert (diff > 1e-3).any(), "the call index does not change the second rate's fill-in beyond its last bits"


@pytest.mark.gpu
def test_a_rate_without_a_consistent_region_is_not_filled(tool, tmp_path):
    """rate 0 has islands of 81 pixels only: no match, stats say not filled, nothing is written -- and its two steps still count as calls for rate 1"""
    inputs = [trajectories(RATES[0], 3, consistent=False), trajectories(RATES[1], 14)]
    assert (inputs[0][2] == RATES[0]).sum() == 3 * 81
    res = run_tool(tool, str(tmp_path), RATES, inputs, 0.25)
    check_rate(res[0], RATES[0], 0, RATES[0])
    assert res[0]["line"][2] == 0 and res[0]["line"][3] == 0                  # kept 0, matches 0
    check_rate(res[1], RATES[1], 1, RATES[0] + RATES[1])
