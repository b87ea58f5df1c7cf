"""accumulate -fill with the cfg key acc_gpu_epic_search (slowflow_amd/host/accumulate.cpp): value 1 runs the fill-in's graph searches in the library's
compact mode (sfa_ctx_set_epic_search) and writes the bytes the default mode writes; any other value is refused before anything is written.  The scene and
the helpers are tests/test_accumulate_fill.py's."""
import json

import pytest

from test_accumulate import host_build  # noqa: F401  (the fixture)
from test_accumulate_fill import make_scene, run, write_cfg, write_edges
from test_accumulate_fuse import width52  # noqa: F401  (the fixture)


def files_of(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


@pytest.mark.gpu
def test_fill_with_the_compact_search_writes_the_same_bytes(host_build, tmp_path, width52):  # noqa: F811
    make_scene(tmp_path)
    outs, stdout = {}, {}
    for name, extra in (("default", ""), ("compact", "acc_gpu_epic_search\t1\n"), ("zero", "acc_gpu_epic_search\t0\n")):
        out = tmp_path / name
        write_edges(out)
        r = run([write_cfg(tmp_path, out, extra=extra), "-fill", "-resume"])
        assert r.returncode == 0, r.stdout + r.stderr
        outs[name] = files_of(out / "accumulated")
        stdout[name] = r.stdout.replace(str(out), "<out>")
    assert sorted(outs["default"]) == sorted(outs["compact"]) == sorted(outs["zero"]) and len(outs["default"]) > 12
    for name in outs["default"]:
        if name != "run.json":
            assert outs["compact"][name] == outs["default"][name] and outs["zero"][name] == outs["default"][name], name
    assert stdout["compact"] == stdout["default"] == stdout["zero"]
    rj = {k: json.loads(v["run.json"]) for k, v in outs.items()}
    assert (rj["default"]["acc_gpu_epic_search"], rj["compact"]["acc_gpu_epic_search"], rj["zero"]["acc_gpu_epic_search"]) == (0, 1, 0)
    assert rj["compact"]["fill"] == rj["default"]["fill"] and all(f["filled"] for f in rj["compact"]["fill"])
    assert [f["energy"] for f in rj["compact"]["fusion"]] == [f["energy"] for f in rj["default"]["fusion"]]


@pytest.mark.gpu
def test_another_value_is_refused_before_anything_is_written(host_build, tmp_path, width52):  # noqa: F811
    make_scene(tmp_path, seed=1)
    for value in (2, -1):
        r = run([write_cfg(tmp_path, tmp_path / "refused", extra="acc_gpu_epic_search\t%d\n" % value), "-fill"])
        assert r.returncode == 1 and "acc_gpu_epic_search %d" % value in r.stderr, (r.stdout, r.stderr)
        assert not (tmp_path / "refused").exists()
