"""accumulate -alternate: the program runs its start_jets through the track job that alternates (sfa_track_job_create_alternate), acc_gpu_batch of them
per launch sequence.  tests/test_accumulate_fill.py's scene (two rates: 4 slots with the fill-in): groups of one and of two write the same files, the
rounds stand in run.json, labels hold origin slots and proposed_<n>.pgm is 0 / 255; the limits are refused by name before anything is written; and
without the flag -fill writes what it wrote, whether or not the cfg holds the alternation's keys (its bytes are pinned to the stage chain by
tests/test_accumulate_fill.py, which is unchanged)."""
import json
import re

import numpy as np
import pytest

from test_accumulate import host_build  # noqa: F401  (the fixture)
from test_accumulate_fill import STARTS, make_scene, run, write_cfg, write_edges
from test_accumulate_fill_groups import outputs
from test_accumulate_fuse import width52  # noqa: F401  (the fixture)

KEYS = "acc_alternate\t2\nacc_perturb_keep\t3\nacc_hyp_neigh_tryouts\t6\nseed\t3\n"


def pgm(path):
    raw = path.read_bytes()
    head = raw.split(b"\n", 3)
    w, h = (int(v) for v in head[1].split())
    return np.frombuffer(raw[-w * h:], np.uint8).reshape(h, w)


@pytest.mark.gpu
def test_groups_of_one_and_of_two_write_the_same_rounds(host_build, tmp_path, width52):  # noqa: F811
    make_scene(tmp_path)
    got = {}
    for batch in (1, 2):
        out = tmp_path / ("batch%d" % batch)
        write_edges(out)
        cfg = write_cfg(tmp_path, out, extra=KEYS + "acc_gpu_batch\t%d\n" % batch)
        r = run([cfg, "-alternate", "-resume"])
        assert r.returncode == 0, r.stdout + r.stderr
        assert "gpu batch: %d start_jet(s) per run" % batch in r.stdout and "not run" not in r.stdout
        acc = out / "accumulated"
        rj = json.load(open(acc / "run.json"))
        assert rj["neighbour_proposals"] is True and rj["epic_fill"] is True and rj["acc_alternate"] == 2 and rj["acc_perturb_keep"] == 3 and rj["seed"] == 3
        assert [g["group_size"] for g in rj["groups"]] == ([1, 1] if batch == 1 else [2])
        for f in rj["fusion"]:
            assert [q["round"] for q in f["rounds"]] == [0, 1] and all(q["accepted_proposals"] > 0 and q["nodes"] == f["nodes"] for q in f["rounds"])
            assert (f["rounds"][-1]["energy"], f["rounds"][-1]["lower_bound"], f["rounds"][-1]["iterations"]) == (f["energy"], f["lower_bound"], f["iterations"])
        for start in STARTS:
            lab, prop = pgm(acc / ("labels_%d.pgm" % start)), pgm(acc / ("proposed_%d.pgm" % start))
            assert set(np.unique(prop)) <= {0, 255} and (prop == 255).any() and set(np.unique(lab)) <= {0, 1, 2, 3}   # -fill leaves no hole: every pixel a node
        got[batch] = (outputs(acc), rj)
    files1, files2 = got[1][0], got[2][0]
    assert sorted(files1) == sorted(files2) and any(n.startswith("proposed_") for n in files1)
    for name in files1:
        assert files1[name] == files2[name], name
    for a, b in zip(got[1][1]["fusion"], got[2][1]["fusion"]):
        assert a["rounds"] == b["rounds"] and all(a[k] == b[k] for k in ("sequence_start", "nodes", "energy", "lower_bound", "iterations"))


@pytest.mark.gpu
def test_fill_without_the_flag_is_what_it_was(host_build, tmp_path, width52):  # noqa: F811
    """-fill ignores the alternation's keys: the same files byte for byte, no proposed_<n>.pgm, the same lines on stdout, neighbour_proposals false"""
    make_scene(tmp_path)
    got = {}
    for name, extra in (("plain", ""), ("keys", KEYS)):
        out = tmp_path / name
        write_edges(out)
        cfg = write_cfg(tmp_path, out, extra=extra + "acc_gpu_batch\t2\n")
        r = run([cfg, "-fill", "-resume"])
        assert r.returncode == 0, r.stdout + r.stderr
        rj = json.load(open(out / "accumulated" / "run.json"))
        assert rj["neighbour_proposals"] is False and "acc_alternate" not in rj and "rounds" not in rj["fusion"][0]
        got[name] = (outputs(out / "accumulated"), r.stdout.replace(str(out), "OUT").replace(str(cfg), "CFG"))
    assert got["plain"][0] == got["keys"][0] and not any("proposed_" in n for n in got["plain"][0])
    shape = lambda text: [re.sub(r"[0-9][0-9.e+-]*", "#", l) for l in text.splitlines()]   # the lines without their figures (times among them)
    assert shape(got["plain"][1]) == shape(got["keys"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("extra,name", [
    ("acc_alternate\t2\n", "acc_perturb_keep is not set"), ("acc_alternate\t2\nacc_perturb_keep\t3\nacc_neigh_hyp\t7\n", "slots + 2 * acc_neigh_hyp"),
    ("acc_alternate\t2\nacc_perturb_keep\t6\n", "acc_perturb_keep + 1 + 2 * acc_neigh_hyp"), ("acc_alternate\t1\nacc_neigh_skip1\t0\n", "acc_neigh_skip1"),
    ("acc_alternate\t1\nacc_neigh_skip2\t0\n", "acc_neigh_skip2"), ("acc_alternate\t1\nacc_hyp_neigh_tryouts\t-1\n", "acc_hyp_neigh_tryouts"),
    ("acc_alternate\t1\nacc_neigh_hyp_radius\t0\n", "acc_neigh_hyp_radius"), ("acc_alternate\t0\n", "acc_alternate"),
])
def test_limits_are_refused_by_name_before_anything_is_written(host_build, tmp_path, width52, extra, name):  # noqa: F811
    make_scene(tmp_path)
    out = tmp_path / "out"
    write_edges(out)
    cfg = write_cfg(tmp_path, out, extra=extra)
    r = run([cfg, "-alternate", "-resume"])
    assert r.returncode == 1 and name in r.stderr, r.stdout + r.stderr
    assert outputs(out / "accumulated") == {}                               # only tmp/, which the test made
