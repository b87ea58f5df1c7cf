"""accumulate -fill in groups: the program runs its start_jets through the track job that fills in (sfa_track_job_create_fill), acc_gpu_batch of them per
launch sequence.  tests/test_accumulate_fill.py's scene with one start_jet per run and with both in one: every output file but run.json is the same,
byte for byte, and run.json names the path and the groups."""
import json

import pytest

from test_accumulate import host_build  # noqa: F401  (the fixture)
from test_accumulate_fill import make_scene, run, write_cfg, write_edges
from test_accumulate_fuse import width52  # noqa: F401  (the fixture)


def outputs(root):
    files = (p for p in sorted(root.rglob("*")) if p.is_file() and p.name != "run.json" and p.relative_to(root).parts[0] != "tmp")
    return {str(p.relative_to(root)): p.read_bytes() for p in files}


@pytest.mark.gpu
def test_groups_of_one_and_of_two_write_the_same_files(host_build, tmp_path, width52):  # noqa: F811
    make_scene(tmp_path)
    got = {}
    for batch in (1, 2):
        out = tmp_path / ("batch%d" % batch)
        write_edges(out)
        cfg = write_cfg(tmp_path, out, extra="acc_gpu_batch\t%d\n" % batch)
        r = run([cfg, "-fill", "-resume"])
        assert r.returncode == 0, r.stdout + r.stderr
        assert "gpu batch: %d start_jet(s) per run" % batch in r.stdout and "acc_gpu_batch" in r.stdout
        acc = out / "accumulated"
        rj = json.load(open(acc / "run.json"))
        assert rj["fill_path"] == "track_job" and rj["epic_fill"] is True and rj["gpu_batch"] == batch
        assert [g["group_size"] for g in rj["groups"]] == ([1, 1] if batch == 1 else [2])
        assert all(len(g["stage_ms"]) == 8 and len(g["fill_ms"]) == 4 and g["fill_ms"][2] > 0 for g in rj["groups"])
        assert [(f["group"], f["group_size"]) for f in rj["fusion"]] == ([(0, 1), (1, 1)] if batch == 1 else [(0, 2), (0, 2)])
        assert len(rj["fill"]) == 4 and all(f["filled"] for f in rj["fill"])
        assert set(rj["timings_s"]) == {"frames", "accumulate", "epic_fill", "energy_call", "fuse", "write", "total"}
        got[batch] = (outputs(acc), rj)
    files1, files2 = got[1][0], got[2][0]
    assert sorted(files1) == sorted(files2) and len(files1) >= 2 * (4 + 2 * 4 + 1)       # per start_jet: four fused files, four per rate, best
    for name in files1:
        assert files1[name] == files2[name], name
    for key in ("fill", "slots", "rates"):
        assert got[1][1][key] == got[2][1][key], key
    strip = lambda segs: [{k: v for k, v in s.items() if k != "flo"} for s in segs]      # ("flo" names the run's own output folder)
    assert strip(got[1][1]["segments"]) == strip(got[2][1]["segments"])
    for a, b in zip(got[1][1]["fusion"], got[2][1]["fusion"]):
        assert all(a[k] == b[k] for k in ("sequence_start", "nodes", "energy", "lower_bound", "iterations"))
