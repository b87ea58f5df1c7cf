"""EpicFlow's geodesic k nearest seeds on the GPU (sfa_epic_nearest_seeds_batch, slowflow_amd/csrc/epic_nn.hip) against the host function it restates
(slowflow_amd/host/epic.cpp: epic_nearest_seeds), and epic_batch against epic().  The stage's outputs are integers and float bit patterns: every comparison
is np.array_equal on all outputs of all images, no tolerance.  The host side runs in tests/host/epic_nn_tool.cpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_epic import ref_lab, refepic, run_ref, scene, stride_of  # noqa: F401  (refepic: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
HUGE = np.array([0x7F7F7F7F], np.uint32).view(np.float32)[0]
SFA_ERR_ARG = -1


# ---- CPU: the boundary -------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    header = open(os.path.join(ROOT, "include", "slowflow_amd.h")).read()
    assert re.search(r"\bint\s+sfa_epic_nearest_seeds_batch\s*\(", header)
    assert "sfa_epic_nearest_seeds_batch" in sfa.EXPORTS
    assert hasattr(C.CDLL(sfa.LIB_PATH), "sfa_epic_nearest_seeds_batch")
    assert callable(getattr(sfa.Context, "epic_nearest_seeds"))
    assert os.path.exists(os.path.join(ROOT, "slowflow_amd", "csrc", "epic_heap.h"))


# ---- the host side -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path_factory.mktemp("epic_nn") / "epic_nn_tool")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-pthread", "-I", HOST, os.path.join(ROOT, "tests", "host", "epic_nn_tool.cpp"), os.path.join(HOST, "libslowflow_host.a"),
                        "-L", os.path.join(ROOT, "slowflow_amd"), "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "slowflow_amd"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


def host_nearest_seeds(tool, d, cost, seeds, nn):
    """epic_nearest_seeds of the host code: (labels (h, w), index (ns, nn), dist (ns, nn))"""
    h, w = cost.shape
    seeds = np.ascontiguousarray(seeds, np.int32).reshape(-1, 2)
    np.ascontiguousarray(cost, np.float32).tofile(os.path.join(d, "cost.bin"))
    seeds.tofile(os.path.join(d, "seeds.bin"))
    r = subprocess.run([tool, "seeds", d, str(w), str(h), str(nn)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return (np.fromfile(os.path.join(d, "labels.bin"), np.int32).reshape(h, w), np.fromfile(os.path.join(d, "index.bin"), np.int32).reshape(len(seeds), nn),
            np.fromfile(os.path.join(d, "dist.bin"), np.float32).reshape(len(seeds), nn))


def same(got, want):
    """all three outputs, the distances by their bits"""
    return (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)))


def check_alone(ctx, tool, d, cost, seeds, nn):
    want = host_nearest_seeds(tool, d, cost, seeds, nn)
    labels, index, dist = ctx.epic_nearest_seeds([cost], [seeds], nn)
    assert same((labels[0], index[0], dist[0]), want)
    return want


def scene_cost_and_seeds(w, h, seed, n_matches=400):
    """what epic() hands to its first search on test_epic.scene: the edge map plus euc, the integer parts of the clamped matches"""
    _, edges, m = scene(w, h, seed, n_matches=n_matches)
    cost = edges + np.float32(0.001)
    x = np.clip(m[:, 0], 0, np.float32(w - 1)).astype(np.int32)
    y = np.clip(m[:, 1], 0, np.float32(h - 1)).astype(np.int32)
    return cost, np.stack([x, y], 1)


def serpentine(w, h=20):
    cost = np.full((h, w), 0.5, np.float32)
    for k, x in enumerate(range(3, w, 4)):                            # walls in every 4th column, their 2-pixel gap alternating bottom / top
        cost[:, x] = 60.0
        if k % 2 == 0:
            cost[h - 2:, x] = 0.5
        else:
            cost[:2, x] = 0.5
    return cost


# ---- GPU: nearest seeds == host ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed", [(96, 64, 0), (131, 77, 1)])
def test_scene_of_test_epic(ctx, tool, tmp_path, w, h, seed):
    cost, seeds = scene_cost_and_seeds(w, h, seed)
    for nn in (1, 26, 100, len(seeds) + 50):
        _, index, _ = check_alone(ctx, tool, str(tmp_path), cost, seeds, nn)
        if nn > len(seeds):
            assert (index[:, len(seeds):] == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("w", [24, 48, 96])
def test_serpentine_extends_the_sweeps(ctx, tool, tmp_path, w):
    """13, 25 and 40 sweeps on the host: the extension rule `end_iter = min(40, i + 3)` and its cap"""
    cost = serpentine(w)
    labels, _, _ = check_alone(ctx, tool, str(tmp_path), cost, [(0, 0)], 3)
    assert (labels == 0).all()                                        # one seed, one region
    check_alone(ctx, tool, str(tmp_path), cost, [(0, 0), (w - 1, 19), (w // 2, 10), (5, 3), (w - 2, 0), (9, 18)], 4)


@pytest.mark.gpu
def test_lattice_of_tied_distances(ctx, tool, tmp_path):
    """constant cost, seeds on a lattice: the lists are full of tied distances, whose order (and membership at the nn-th place) only the heap's order decides"""
    cost = np.full((48, 64), 0.25, np.float32)
    seeds = [(4 + 8 * a, 4 + 8 * b) for b in range(6) for a in range(8)]
    for nn in (20, 48, 60):
        _, index, dist = check_alone(ctx, tool, str(tmp_path), cost, seeds, nn)
        if nn <= 48:
            ties = sum(int((np.diff(row) == 0).sum()) for row in dist)
            assert ties > 100                                         # (the case does hold ties)
        else:
            assert (index[:, 48:] == -1).all() and (dist[:, 48:].view(np.uint32) == 0x7F7F7F7F).all()


@pytest.mark.gpu
def test_unreachable_pixels_keep_no_label(ctx, tool, tmp_path):
    cost = np.full((30, 40), 0.3, np.float32)
    cost[8:19, 10:21] = np.inf
    labels, _, _ = check_alone(ctx, tool, str(tmp_path), cost, [(2, 2), (35, 25), (30, 3)], 3)
    assert (labels == -1).sum() == 121 and (labels[8:19, 10:21] == -1).all()


@pytest.mark.gpu
def test_degenerate_sizes_and_duplicate_seeds(ctx, tool, tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(7)
    _, index, _ = check_alone(ctx, tool, d, rng.uniform(0.1, 1, (1, 50)).astype(np.float32), [(3, 0), (20, 0), (44, 0)], 3)        # one row: no graph
    assert (index[:, 1:] == -1).all()
    check_alone(ctx, tool, d, rng.uniform(0.1, 1, (50, 1)).astype(np.float32), [(0, 3), (0, 20), (0, 44)], 3)                      # one column
    check_alone(ctx, tool, d, rng.uniform(0.1, 1, (2, 2)).astype(np.float32), [(0, 0), (1, 1)], 2)
    cost = rng.uniform(0.05, 0.5, (15, 20)).astype(np.float32)
    labels, _, _ = check_alone(ctx, tool, d, cost, [(5, 5), (12, 7), (5, 5)], 3)                                                  # the later seed of a pixel wins
    assert labels[5, 5] == 2 and not (labels == 0).any()
    check_alone(ctx, tool, d, cost, [(3, 4)], 2)                                                                                  # a single seed


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(521, 515), (515, 521), (600, 40), (40, 600)])
def test_diagonals_longer_than_the_sweeps_workgroup(ctx, tool, tmp_path, w, h):
    """k_epic_sweeps runs 512 threads: diagonals of up to 515 cells take a second round, in both orientations of the diagonal's LDS index"""
    rng = np.random.default_rng(w)
    cost = rng.uniform(0.02, 0.5, (h, w)).astype(np.float32)
    seeds = np.stack([rng.integers(0, w, 300), rng.integers(0, h, 300)], 1)
    check_alone(ctx, tool, str(tmp_path), cost, seeds, 12)


@pytest.mark.gpu
def test_batch_sub_batches_and_the_flag(ctx, tool, tmp_path):
    """images of different ns in one call equal the same images one by one -- also when the call has to run in several sub-batches, and an image that fits
    no sub-batch comes back flagged, the others untouched by it"""
    w, h, nn = 96, 64, 5
    rng = np.random.default_rng(11)
    costs, seeds, want = [], [], []
    for k, ns in enumerate((250, 300, 262, 287, 275, 700)):
        costs.append(rng.uniform(0.02, 0.6, (h, w)).astype(np.float32))
        seeds.append(np.stack([rng.integers(0, w, ns), rng.integers(0, h, ns)], 1))
        want.append(host_nearest_seeds(tool, str(tmp_path), costs[k], seeds[k], nn))
    labels, index, dist = ctx.epic_nearest_seeds(costs[:5], seeds[:5], nn)
    for k in range(5):
        assert same((labels[k], index[k], dist[k]), want[k]), k
    # a budget of 1.25 MB.  Each of the first five needs more than 344 KB (planes 74 KB, lists 20 KB, ns * ns floats >= 250 KB) -- together more than the
    # budget, so several sub-batches -- and at most 97 + 393 + 360 KB for planes, lists, the largest table these 6144 pixels can ask for (2^15 slots of 12
    # bytes) and `done`, which leaves 400 KB for the heaps, (1 + 4 * largest degree) * ns * 8 B: each fits alone up to a largest degree of 40 (these
    # regions of about 22 pixels have fewer than 20 neighbours).  The sixth needs 700 * 700 floats = 1.96 MB for `done` alone: flagged.
    labels, index, dist, status = ctx.epic_nearest_seeds(costs, seeds, nn, workspace_bytes=1250000, with_status=True)
    assert status == [0, 0, 0, 0, 0, 1]
    for k in range(5):
        assert same((labels[k], index[k], dist[k]), want[k]), k
    labels, index, dist = ctx.epic_nearest_seeds(costs, seeds, nn)      # and with room for all six
    assert same((labels[5], index[5], dist[5]), want[5])


# ---- GPU: epic_batch == epic() ----------------------------------------------------------------------------------------------------------------------
def run_epic_tool(tool, d, scenes, method, sal, pref_nn, nn, budget=None):
    """epic() and epic_batch of the host code on the scenes [(rgb, edges, m, w, h)]: [(fx, fy, bfx, bfy)] per scene"""
    with open(os.path.join(d, "sizes.txt"), "w") as f:
        for k, (rgb, edges, m, w, h) in enumerate(scenes):
            f.write("%d %d\n" % (w, h))
            rgb.tofile(os.path.join(d, "rgb_%d.bin" % k))
            edges.tofile(os.path.join(d, "edges_%d.bin" % k))
            with open(os.path.join(d, "matches_%d.txt" % k), "w") as g:
                for r in m:
                    g.write("%.9g %.9g %.9g %.9g 1.0 17\n" % tuple(float(x) for x in r))
    r = subprocess.run([tool, "epic", d, str(len(scenes)), method, repr(sal), str(pref_nn), "5.0", str(nn), "0.8", "0.001"] + ([str(budget)] if budget else []),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rcs = re.findall(r"^rc (\d+) (-?\d+) (-?\d+)$", r.stdout, flags=re.M)
    assert len(rcs) == len(scenes) and all(a == "0" and b == "0" for _, a, b in rcs), r.stdout
    out = []
    for k, (_, _, _, w, h) in enumerate(scenes):
        out.append(tuple(np.fromfile(os.path.join(d, "%s_%d.bin" % (n, k)), np.float32).reshape(h, stride_of(w)) for n in ("fx", "fy", "bfx", "bfy")))
    return out


@pytest.fixture(scope="module")
def epic_scenes():
    scenes = [scene(96, 64, 0) + (96, 64), scene(131, 77, 1) + (131, 77)]
    rgb, edges, m = scene(131, 77, 5, n_matches=600)                  # the saliency scene of test_epic_with_saliency_filter_gpu
    rgb[:, :30, :40] = 128.0
    return scenes + [(rgb, edges, m, 131, 77)]


@pytest.mark.gpu
@pytest.mark.parametrize("method,sal,pref_nn,nn", [("NW", 0.0, 25, 100), ("NW", 0.0, 0, 30), ("LA", 0.0, 25, 100), ("NW", 0.045, 25, 100), ("LA", 0.045, 25, 100)])
def test_epic_batch_equals_epic(tool, refepic, epic_scenes, tmp_path, method, sal, pref_nn, nn):
    """three scenes of two sizes in one epic_batch: the flow fields of epic() bit for bit -- and for Nadaraya-Watson the compiled reference's, on the
    scenes and parameter sets the golden file knows"""
    res = run_epic_tool(tool, str(tmp_path), epic_scenes, method, sal, pref_nn, nn)
    for k, (fx, fy, bfx, bfy) in enumerate(res):
        assert np.array_equal(bfx.view(np.uint32), fx.view(np.uint32)) and np.array_equal(bfy.view(np.uint32), fy.view(np.uint32)), k
        assert len(np.unique(bfx)) > 50
    if method == "NW":
        for k in ((0, 1) if sal == 0.0 else (2,)):
            rgb, edges, m, w, h = epic_scenes[k]
            rx, ry = run_ref(refepic, ref_lab(refepic, rgb, w, h), edges, m, w, h, "NW", sal, pref_nn, nn)
            assert np.array_equal(res[k][2][:, :w], rx[:, :w]) and np.array_equal(res[k][3][:, :w], ry[:, :w]), k


@pytest.mark.gpu
def test_epic_batch_computes_flagged_images_on_the_host(tool, epic_scenes, tmp_path):
    """a workspace of 200 KB holds none of these images (their lists alone are larger): every one comes back flagged, and epic_batch still returns epic()'s fields"""
    for k, (fx, fy, bfx, bfy) in enumerate(run_epic_tool(tool, str(tmp_path), epic_scenes, "LA", 0.0, 25, 100, budget=200000)):
        assert np.array_equal(bfx.view(np.uint32), fx.view(np.uint32)) and np.array_equal(bfy.view(np.uint32), fy.view(np.uint32)), k


# ---- GPU: refusals --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_name_the_argument(ctx):
    import slowflow_amd as sfa
    L = sfa.lib()
    _f, _i = C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.sfa_epic_nearest_seeds_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(_f), C.POINTER(_i), _i, C.c_int, C.POINTER(_i), C.POINTER(_i),
                                               C.POINTER(_f), C.c_size_t, _i]
    w, h, nn = 8, 6, 2
    cost = np.full((h, w), 0.5, np.float32)
    seeds = np.array([[1, 1], [6, 4]], np.int32)
    labels, index, dist = np.full((h, w), -7, np.int32), np.full((2, nn), -7, np.int32), np.zeros((2, nn), np.float32)
    fp, ip = (lambda a: a.ctypes.data_as(_f)), (lambda a: a.ctypes.data_as(_i))

    def call(named, n=1, w=w, h=h, nn=nn, ns=2, seeds=seeds, null=None):
        a = dict(cost=(_f * 1)(fp(cost)), seeds_xy=(_i * 1)(ip(seeds)), ns=(C.c_int * 1)(ns), labels=(_i * 1)(ip(labels)), nn_index=(_i * 1)(ip(index)),
                 nn_dist=(_f * 1)(fp(dist)), status=(C.c_int * 1)(5))
        if null in a:
            a[null] = None
        elif null:                                                    # "cost[0]": the image's own pointer
            a[null[:-3]] = type(a[null[:-3]])()
        rc = L.sfa_epic_nearest_seeds_batch(ctx.h, n, w, h, a["cost"], a["seeds_xy"], a["ns"], nn, a["labels"], a["nn_index"], a["nn_dist"], 0, a["status"])
        msg = L.sfa_last_error(ctx.h).decode()
        assert rc == SFA_ERR_ARG and "sfa_epic_nearest_seeds_batch" in msg and named in msg, (rc, msg, named)
        assert (labels == -7).all() and (index == -7).all()           # nothing was computed

    call("n =", n=0)
    call("w x h", w=0)
    call("w x h", h=-1)
    call("nn =", nn=0)
    call("ns[0]", ns=0)
    for name in ("cost", "seeds_xy", "ns", "labels", "nn_index", "nn_dist", "status"):
        call(name + " is null", null=name)
    for name in ("cost", "seeds_xy", "labels", "nn_index", "nn_dist"):
        call(name + "[0] is null", null=name + "[0]")
    call("seeds_xy[0]: seed 1 = (8, 4)", seeds=np.array([[1, 1], [8, 4]], np.int32))
    call("seeds_xy[0]: seed 0 = (1, -1)", seeds=np.array([[1, -1], [6, 4]], np.int32))
    call("w * h", w=1 << 15, h=(1 << 14) + 1)                         # more than 2^29 pixels
    call("ns[0] * nn", nn=1 << 30)                                    # 2 * 2^30 list entries
    out = ctx.epic_nearest_seeds([cost], [seeds], nn)                 # and the call that is not refused computes
    assert (out[0][0] >= 0).all()
