"""EpicFlow's whole interpolation of a batch as one chain on the GPU (sfa_epic_batch, slowflow_amd/csrc/epic_batch.hip and epic_filter.hip) against the host
code it restates: saliency(), the two filters and their survivors, and epic()'s flow fields.  The host side runs in tests/host/epic_batch_tool.cpp, which
builds the chain out of the public pieces of slowflow_amd/host/epic.cpp.  Every comparison is on bit patterns (np.array_equal on uint32 views)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_epic import ref_lab, refepic, run_ref, scene, stride_of  # noqa: F401  (refepic: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
SFA_OK, SFA_ERR_ARG = 0, -1
EUC = 0.001
NAMES = ("sfa_epic_batch", "sfa_epic_saliency_batch", "sfa_epic_batch_stage_ms")


# ---- CPU: the boundary -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    header = open(os.path.join(ROOT, "include", "slowflow_amd.h")).read()
    L = C.CDLL(sfa.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in sfa.EXPORTS, name
        assert hasattr(L, name), name
    assert "typedef struct sfa_epic_params" in header
    for name in ("epic_batch", "epic_saliency", "epic_batch_stage_ms"):
        assert callable(getattr(sfa.Context, name)), name
    p = sfa.epic_params(method="NW", nn=30)
    assert (p.method, p.nn, p.pref_nn) == (1, 30, 25) and C.sizeof(sfa.EpicParams) == 28
    assert abs(p.saliency_th - 0.045) < 1e-7 and abs(p.coef_kernel - 0.8) < 1e-7 and p.pref_th == 5.0
    mk = open(os.path.join(ROOT, "slowflow_amd", "csrc", "Makefile")).read()
    assert "epic_batch.hip" in mk and "epic_filter.hip" in mk
    # the stage functions the chain is made of are declared at device level; the weights kernel stands beside the one restatement of glibc's expf
    internal = open(os.path.join(ROOT, "slowflow_amd", "csrc", "sfa_internal.h")).read()
    for name in ("epic_nn_device", "epic_fit_device", "epic_apply_device", "epic_saliency_device", "epic_compact_device"):
        assert re.search(r"\b%s\s*\(" % name, internal), name
    kernels = open(os.path.join(ROOT, "slowflow_amd", "csrc", "kernels.hip")).read()
    assert "k_epic_weights" in kernels and len(re.findall(r"float\s+expf_glibc\s*\(", kernels)) == 1
    for name in ("sfa_device.h", "epic_filter.hip", "epic_batch.hip"):
        assert "kExp2fTab" not in open(os.path.join(ROOT, "slowflow_amd", "csrc", name)).read(), name


# ---- the host side -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path_factory.mktemp("epic_batch") / "epic_batch_tool")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-pthread", "-I", HOST, os.path.join(ROOT, "tests", "host", "epic_batch_tool.cpp"), os.path.join(HOST, "libslowflow_host.a"),
                        "-L", os.path.join(ROOT, "slowflow_amd"), "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "slowflow_amd"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("epic_batch_runs")


_runs = {}


def host_run(tool, workdir, key, scenes, method, sal, pref_nn, nn, coef=0.8, budget=None, euc=EUC):
    """the tool's `run` on the scenes [(rgb, edges, m, w, h)], once per key: a list of dicts per scene (lab, sal, keep1, keep2, fx, fy, bfx, bfy, rc, brc) and
    the stage times of the library's chain after epic_batch.  euc = 0: epic() adds nothing to the edges"""
    full = (key, method, sal, pref_nn, nn, coef, budget, euc)
    if full in _runs:
        return _runs[full]
    d = str(workdir / ("run%d" % len(_runs)))
    os.makedirs(d)
    with open(os.path.join(d, "sizes.txt"), "w") as f:
        for k, (rgb, edges, m, w, h) in enumerate(scenes):
            f.write("%d %d\n" % (w, h))
            rgb.tofile(os.path.join(d, "rgb_%d.bin" % k))
            edges.tofile(os.path.join(d, "edges_%d.bin" % k))
            np.ascontiguousarray(m, np.float32).tofile(os.path.join(d, "matches_%d.bin" % k))
    r = subprocess.run([tool, "run", d, str(len(scenes)), method, repr(sal), str(pref_nn), "5.0", str(nn), repr(coef), repr(euc)] + ([str(budget)] if budget else []),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rcs = re.findall(r"^rc (\d+) (-?\d+) (-?\d+)$", r.stdout, flags=re.M)
    assert len(rcs) == len(scenes), r.stdout
    stage = [float(v) for v in re.search(r"^stage_ms (.*)$", r.stdout, flags=re.M).group(1).split()]
    out = []
    for k, (_, _, _, w, h) in enumerate(scenes):
        st = stride_of(w)
        rd = lambda n, shape: np.fromfile(os.path.join(d, "%s_%d.bin" % (n, k)), np.float32).reshape(shape)
        o = dict(lab=rd("lab", (3, h, st)), keep1=rd("keep1", (-1, 4)), keep2=rd("keep2", (-1, 4)), rc=int(rcs[k][1]), brc=int(rcs[k][2]), stderr=r.stderr)
        for n in ("fx", "fy", "bfx", "bfy"):
            o[n] = rd(n, (h, st))
        if sal:
            o["sal"] = rd("sal", (h, st))
        out.append(o)
    _runs[full] = (out, stage)
    return _runs[full]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def lib_batch(ctx, scenes, host, method, sal, pref_nn, nn, coef=0.8, euc=EUC, **kw):
    """ctx.epic_batch on scenes of ONE size with the Lab images the tool wrote.  euc = 0: the edges as they are (epic()'s `if (euc)`; -0.0 + 0.0 would be +0.0)"""
    import slowflow_amd as sfa
    w = scenes[0][3]
    costs = [s[1] + np.float32(euc) if euc else s[1] for s in scenes]    # epic()'s in-place `c += euc`, one fp32 addition
    p = sfa.epic_params(method=method, saliency_th=sal, pref_nn=pref_nn, nn=nn, coef_kernel=coef, euc=euc)
    return ctx.epic_batch([o["lab"] for o in host], costs, [s[2] for s in scenes], p, stride=stride_of(w), **kw)


def by_size(scenes):
    groups = {}
    for k, s in enumerate(scenes):
        groups.setdefault((s[3], s[4]), []).append(k)
    return list(groups.values())


@pytest.fixture(scope="module")
def epic_scenes():
    """test_epic_nn.py's three scenes of two sizes"""
    scenes = [scene(96, 64, 0) + (96, 64), scene(131, 77, 1) + (131, 77)]
    rgb, edges, m = scene(131, 77, 5, n_matches=600)                  # the saliency scene of test_epic_with_saliency_filter_gpu
    rgb[:, :30, :40] = 128.0
    return scenes + [(rgb, edges, m, 131, 77)]


# ---- 1. saliency -----------------------------------------------------------------------------------------------------------------------------------------
def host_saliency(tool, d, labs, w, h):
    with open(os.path.join(d, "sizes.txt"), "w") as f:
        for k, a in enumerate(labs):
            f.write("%d %d\n" % (w, h))
            a.tofile(os.path.join(d, "lab_%d.bin" % k))
    r = subprocess.run([tool, "sal", d, str(len(labs)), "0.8", "1.0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return [np.fromfile(os.path.join(d, "sal_%d.bin" % k), np.float32).reshape(h, stride_of(w)) for k in range(len(labs))]


def lab_like(w, h, seed, constant=False):
    rng = np.random.default_rng(seed)
    a = np.zeros((3, h, stride_of(w)), np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    for c in range(3):
        a[c, :, :w] = 41.5 if constant else (50 + 30 * np.sin(0.3 * xx + c) * np.cos(0.23 * yy) + rng.uniform(-5, 5, (h, w)))
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,kinds", [(131, 77, (0,)), (64, 16, (0,)), (9, 9, (0,)), (33, 21, (0, 1, 0))])
def test_saliency_equals_the_host(ctx, tool, tmp_path, w, h, kinds):
    """stride != w (131 -> 132), a flat image, the smallest size the Gaussian of sigma 1.0 takes (order 4: more than 8 columns and rows), and a batch of
    three whose middle image is constant: every eigenvalue of it is 0 up to the rounding of the filters at the border"""
    labs = [lab_like(w, h, 10 + k, constant=bool(c)) for k, c in enumerate(kinds)]
    want = host_saliency(tool, str(tmp_path), labs, w, h)
    got = ctx.epic_saliency(labs, 0.8, 1.0, w=w)
    for k in range(len(labs)):
        assert same(got[k], want[k]), k
        assert not got[k][:, w:].any()                                   # the padding, as image_erase left it
        if kinds[k]:
            assert got[k].max() < 1e-3                                   # (rounding of the smoothed constant at the border, nothing else)
        else:
            assert got[k][:, :w].max() > 0.045


@pytest.mark.gpu
def test_saliency_refusals(ctx):
    import slowflow_amd as sfa
    with pytest.raises(sfa.SlowflowError, match="smaller than the filter"):
        ctx.epic_saliency([lab_like(8, 9, 0)], w=8)
    with pytest.raises(sfa.SlowflowError, match="stride"):
        ctx.epic_saliency([lab_like(12, 12, 0)], w=13)


# ---- 2. the filters ------------------------------------------------------------------------------------------------------------------------------------------
def filter_scene():
    """131 x 77 (stride 132) with a textureless corner, 600 matches with outliers, and on top: matches whose float index y * stride + x names another pixel
    than the integer parts do, matches outside the image, duplicate seeds"""
    w, h = 131, 77
    rgb, edges, m = scene(w, h, 5, n_matches=600, outliers=30)
    rgb[:, :30, :40] = 128.0
    rng = np.random.default_rng(77)
    extra = []
    # x1 one ulp below an integer: y * 132 + x rounds up to the next pixel (ulp 3e-5 at 400) where (int)x stays behind; around the corner's border, where
    # the saliency crosses the threshold
    for y in range(2, 60, 3):
        for c in (34, 38, 41, 44):
            extra.append([np.nextafter(np.float32(c), np.float32(0)), float(y), c + 2.0, y + 1.0])
    # fractional y1: (int)(y * 132 + x) lies in row floor(y) only while frac(y) * 132 + x < 132; otherwise the float index names the row below
    for y in np.arange(20.5, 40, 1.75):
        for x in (10.25, 70.5, 100.75, 129.5):
            extra.append([x, y, x - 1.5, y + 0.5])
    # a column that falls into the padding: frac(y) * 132 + x in [131, 132)
    extra.append([0.5, 50.0 + 131.0 / 132.0, 2.0, 51.0])
    # outside the image on every side: clamped (epic.cpp:15-28)
    extra += [[-7.5, 30.0, 4.0, 31.0], [w + 9.0, 40.2, w + 12.0, 41.0], [60.0, -2.0, 61.0, -4.0], [61.0, h + 3.0, 62.0, h + 8.5], [-1.0, -1.0, w + 1.0, h + 1.0]]
    m = np.concatenate([m, np.array(extra, np.float32)])
    dup = m[rng.choice(600, 25, replace=False)].copy()                # duplicate seeds: the same x1, y1 with another target
    dup[:, 2:] += rng.uniform(-0.5, 0.5, (25, 2)).astype(np.float32)
    return rgb, edges, np.concatenate([m, dup]).astype(np.float32), w, h


def test_the_filter_scene_pins_the_float_index():
    """(CPU) some of the scene's matches name, through the host's float expression, another pixel than y * stride + x of their integer parts"""
    _, _, m, w, h = filter_scene()
    m = m.copy()
    m[:, 0::2] = np.clip(m[:, 0::2], 0, w - 1); m[:, 1::2] = np.clip(m[:, 1::2], 0, h - 1)
    st = np.float32(stride_of(w))
    fl = (m[:, 1] * st + m[:, 0]).astype(np.float32).astype(np.int64)
    it = m[:, 1].astype(np.int64) * stride_of(w) + m[:, 0].astype(np.int64)
    assert (fl != it).sum() >= 40 and ((fl % stride_of(w)) >= w).any()


@pytest.mark.gpu
@pytest.mark.parametrize("sal,pref_nn", [(0.045, 25), (0.045, 0), (0.0, 25), (0.0, 0), (-1.0, 25), (1e9, 25)])
def test_filters_keep_the_hosts_matches(ctx, tool, workdir, sal, pref_nn):
    """kept_matches and counts against the survivors of the chain built from the host's public pieces: both filters, each alone, neither, a saliency
    threshold that keeps everything and one that keeps nothing (rc 1, planes untouched)"""
    sc = filter_scene()
    (host,), _ = host_run(tool, workdir, "filter", [sc], "NW", sal, pref_nn, 100)
    fx, fy, rc, counts, kept = lib_batch(ctx, [sc], [host], "NW", sal, pref_nn, 100)
    nm = len(sc[2])
    assert list(counts[0]) == [nm, len(host["keep1"]), len(host["keep2"])]
    assert same(kept[0], host["keep2"])
    assert rc[0] == host["rc"] == host["brc"]
    if sal == 1e9:
        assert rc[0] == 1 and list(counts[0]) == [nm, 0, 0] and np.isnan(fx[0]).all() and np.isnan(fy[0]).all()
        return
    assert rc[0] == 0 and len(kept[0]) > 100
    if sal == -1.0 or sal == 0.0:
        assert counts[0][1] == nm
    else:
        assert 100 < counts[0][1] < nm
    assert (counts[0][2] < counts[0][1]) == bool(pref_nn)              # the outliers go
    w = sc[3]
    assert same(fx[0][:, :w], host["fx"][:, :w]) and same(fy[0][:, :w], host["fy"][:, :w])


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------------------------------
GRID = [(method, sal, pref_nn, 100 if pref_nn else 30) for method in ("NW", "LA") for sal in (0.0, 0.045) for pref_nn in (25, 0)]
GOLDEN = {("NW", 0.0, 25, 100): (0, 1), ("NW", 0.0, 0, 30): (0, 1), ("NW", 0.045, 25, 100): (2,)}     # what tests/golden/ref_epic.npz knows


@pytest.mark.gpu
@pytest.mark.parametrize("method,sal,pref_nn,nn", GRID)
def test_epic_batch_equals_epic(ctx, tool, workdir, refepic, epic_scenes, method, sal, pref_nn, nn):
    """three scenes of two sizes, the images of one size in one call: epic()'s fields bit for bit; the host's epic_batch, which goes through the same call,
    too (its filter stage time is not 0); and for Nadaraya-Watson the compiled reference's"""
    host, stage = host_run(tool, workdir, "scenes", epic_scenes, method, sal, pref_nn, nn)
    assert stage[1] > 0                                                  # epic_batch went through sfa_epic_batch
    for group in by_size(epic_scenes):
        fx, fy, rc, counts, kept = lib_batch(ctx, [epic_scenes[k] for k in group], [host[k] for k in group], method, sal, pref_nn, nn)
        for j, k in enumerate(group):
            w = epic_scenes[k][3]
            assert rc[j] == 0 and host[k]["rc"] == 0 and host[k]["brc"] == 0 and counts[j][2] > 100, k
            assert same(fx[j][:, :w], host[k]["fx"][:, :w]) and same(fy[j][:, :w], host[k]["fy"][:, :w]), k
            assert np.isnan(fx[j][:, w:]).all()                          # columns >= w are not written
            assert same(host[k]["bfx"], host[k]["fx"]) and same(host[k]["bfy"], host[k]["fy"]), k
            assert len(np.unique(fx[j][:, :w])) > 50
            if k in GOLDEN.get((method, sal, pref_nn, nn), ()):
                rgb, edges, m, w, h = epic_scenes[k]
                rx, ry = run_ref(refepic, ref_lab(refepic, rgb, w, h), edges, m, w, h, "NW", sal, pref_nn, nn)
                assert np.array_equal(fx[j][:, :w], rx[:, :w]) and np.array_equal(fy[j][:, :w], ry[:, :w]), k


# ---- 4. neighbour counts per image -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("method", ["LA", "NW"])
def test_neighbour_counts_are_per_image(ctx, tool, workdir, method):
    """a 20-match image between 600-match images with nn 100 and pref_nn 25: it searches 20 and then fewer neighbours where the others search 26 and 100 (both
    "not enough matches" cases), in the same launches; each result is the image's result alone, and epic()'s"""
    w, h = 131, 77
    big0, big1 = scene(w, h, 21, n_matches=600), scene(w, h, 22, n_matches=600)
    rgb, edges, m = scene(w, h, 23, n_matches=600)
    small = (rgb, edges, m[40:60].copy())
    scenes = [s + (w, h) for s in (big0, small, big1)]
    host, _ = host_run(tool, workdir, "mixed", scenes, method, 0.0, 25, 100)
    assert "not enough matches for prefiltering" in host[0]["stderr"] and "not enough matches for interpolating" in host[0]["stderr"]
    together = lib_batch(ctx, scenes, host, method, 0.0, 25, 100)
    assert together[2] == [0, 0, 0] and 0 < together[3][1][2] <= 20 and together[3][0][2] > 100
    for k in range(3):
        alone = lib_batch(ctx, [scenes[k]], [host[k]], method, 0.0, 25, 100)
        for part in (0, 1, 4):                                           # flow_x, flow_y, the survivors
            assert same(together[part][k], alone[part][0]), (k, part)
        assert together[2][k] == alone[2][0] and np.array_equal(together[3][k], alone[3][0]), k
        assert same(together[0][k][:, :w], host[k]["fx"][:, :w]) and same(together[1][k][:, :w], host[k]["fy"][:, :w]), k


# ---- 5. the weights over their range ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("method", ["LA", "NW"])
def test_weights_from_one_to_underflow(ctx, tool, workdir, method):
    """costs of 2.0 across 131 columns, coef_kernel 0.8 and lists that hold every seed (nn = the number of matches): the distances run from 2 (a seed's own pixel) past
    87.3 / 0.8 = 109 (expf subnormal) and 104 / 0.8 = 130 (expf 0: the weight is exactly 1e-08f) up to about 260"""
    w, h = 131, 77
    rgb, edges, m = scene(w, h, 31, n_matches=300, outliers=0)
    edges[:] = 2.0
    sc = (rgb, edges, m, w, h)
    (host,), _ = host_run(tool, workdir, "weights", [sc], method, 0.0, 25, 300)
    fx, fy, rc, counts, kept = lib_batch(ctx, [sc], [host], method, 0.0, 25, 300)
    assert rc == [0] and host["rc"] == 0 and counts[0][2] > 50
    assert same(fx[0][:, :w], host["fx"][:, :w]) and same(fy[0][:, :w], host["fy"][:, :w])
    assert same(kept[0], host["keep2"])
    # the range is reached: the raw lists of the survivors
    seeds = np.stack([kept[0][:, 0].astype(np.int32), kept[0][:, 1].astype(np.int32)], 1)
    _, _, dist = ctx.epic_nearest_seeds([edges + np.float32(EUC)], [seeds], len(seeds))
    d = dist[0][dist[0] < 1e30]
    assert d.min() < 2.5 and ((d > 87.4 / 0.8) & (d < 103.0 / 0.8)).any() and (d > 104.5 / 0.8).any()


# ---- 6. batch invariance and the flag ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def six_scenes():
    w, h = 96, 64
    return [scene(w, h, 40 + k, n_matches=300 + 4 * k) + (w, h) for k in range(6)]


@pytest.mark.gpu
def test_batch_invariance_and_the_flag(ctx, tool, workdir, six_scenes):
    """six images as one batch, in sub-batches of one, and in reversed order: identical bits per image.  With nn 30 an image of 300 - 320 matches owns about
    200 KB for the whole chain (four planes of 24.5 KB, two lists of 38 KB, the matches) and its search allocates 0.67 - 1.2 MB more (dmap, its own lists,
    a table of 2^13 slots, `done` = ns * ns floats, heaps of ns * (1 + 29 * largest degree) entries of 8 bytes, for some 190 survivors and a largest degree
    of 8 - 20).  A budget of 1.6 MB therefore holds one image and never two (at least 2 * (0.2 + 0.67) MB); 200 KB holds none (`done` alone is 360 KB):
    every status is 1 and nothing is written"""
    import slowflow_amd as sfa
    w, h = 96, 64
    host, _ = host_run(tool, workdir, "six", six_scenes, "LA", 0.045, 25, 30)
    whole = lib_batch(ctx, six_scenes, host, "LA", 0.045, 25, 30)
    assert whole[2] == [0] * 6
    ones = lib_batch(ctx, six_scenes, host, "LA", 0.045, 25, 30, workspace_bytes=1600000)
    back = lib_batch(ctx, six_scenes[::-1], host[::-1], "LA", 0.045, 25, 30)
    for k in range(6):
        assert same(whole[0][k][:, :w], host[k]["fx"][:, :w]) and same(whole[1][k][:, :w], host[k]["fy"][:, :w]), k
        for other, j in ((ones, k), (back, 5 - k)):
            assert same(whole[0][k], other[0][j]) and same(whole[1][k], other[1][j]) and same(whole[4][k], other[4][j]), k
            assert whole[2][k] == other[2][j] and np.array_equal(whole[3][k], other[3][j]), k
    # the flag, through the raw call: sentinels everywhere
    L = sfa.lib()
    n = 6
    _f, _i = C.POINTER(C.c_float), C.POINTER(C.c_int)
    fp = lambda a: a.ctypes.data_as(_f)
    costs = [s[1] + np.float32(EUC) for s in six_scenes]
    ms = [np.ascontiguousarray(s[2], np.float32) for s in six_scenes]
    labs = [o["lab"] for o in host]
    fx = [np.full((h, w), -77.0, np.float32) for _ in range(n)]
    fy = [np.full((h, w), -78.0, np.float32) for _ in range(n)]
    rc = (C.c_int * n)(*([-9] * n)); status = (C.c_int * n)(*([5] * n)); counts = ((C.c_int * 3) * n)(*[(C.c_int * 3)(-4, -4, -4) for _ in range(n)])
    p = sfa.epic_params(method="LA", nn=30)
    r = L.sfa_epic_batch(ctx.h, n, w, h, C.byref(p), (_f * n)(*[fp(a) for a in labs]), stride_of(w), (_f * n)(*[fp(a) for a in costs]), (_f * n)(*[fp(a) for a in ms]),
                         (C.c_int * n)(*[len(a) for a in ms]), (_f * n)(*[fp(a) for a in fx]), (_f * n)(*[fp(a) for a in fy]), w, rc, counts, None, 200000, status)
    assert r == SFA_OK, L.sfa_last_error(ctx.h)
    assert list(status) == [1] * n and list(rc) == [-9] * n and all(list(c) == [-4, -4, -4] for c in counts)
    assert all((a == -77.0).all() for a in fx) and all((a == -78.0).all() for a in fy)
    assert all(v == 0.0 for v in ctx.epic_batch_stage_ms().values())


@pytest.mark.gpu
def test_host_epic_batch_computes_flagged_images_on_the_staged_path(tool, workdir, six_scenes):
    """at 200 KB the library flags every image: the host's epic_batch runs them stage by stage (the chain's stage times stay 0) and still returns epic()'s fields"""
    host, stage = host_run(tool, workdir, "six", six_scenes, "LA", 0.045, 25, 30, budget=200000)
    assert all(v == 0.0 for v in stage)
    for k, o in enumerate(host):
        assert o["rc"] == 0 and o["brc"] == 0 and same(o["bfx"], o["fx"]) and same(o["bfy"], o["fy"]), k


# ---- 7. dropping out mid-batch -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_image_that_loses_all_matches_in_the_consistency_filter(ctx, tool, workdir):
    """the middle image's 40 matches point in 40 unrelated directions: none agrees with the estimate from its neighbours to 5 px.  rc 1, planes untouched;
    the neighbours' fields are their fields alone"""
    w, h = 96, 64
    a, b = scene(w, h, 51), scene(w, h, 52)
    rgb, edges, m = scene(w, h, 53, n_matches=40, outliers=0)
    rng = np.random.default_rng(53)
    ang = rng.uniform(0, 2 * np.pi, 40)
    m[:, 0] = rng.uniform(20, w - 20, 40); m[:, 1] = rng.uniform(20, h - 20, 40)      # (away from the border: the clamp does not shorten the vectors)
    m[:, 2] = m[:, 0] + (np.arange(40) % 2 * 2 - 1) * 19 * np.cos(ang); m[:, 3] = m[:, 1] + 19 * np.sin(ang) * (1 - np.arange(40) % 4 // 2 * 2)
    scenes = [s + (w, h) for s in (a, (rgb, edges, m.astype(np.float32)), b)]
    host, _ = host_run(tool, workdir, "dropout", scenes, "LA", 0.0, 25, 100)
    assert len(host[1]["keep2"]) == 0 and host[1]["rc"] == 1 and host[1]["brc"] == 1
    fx, fy, rc, counts, kept = lib_batch(ctx, scenes, host, "LA", 0.0, 25, 100)
    assert rc == [0, 1, 0] and list(counts[1]) == [40, 40, 0] and len(kept[1]) == 0
    assert np.isnan(fx[1]).all() and np.isnan(fy[1]).all()
    assert not host[1]["bfx"].any() and not host[1]["bfy"].any()         # the host's planes too (the tool erased them)
    for k in (0, 2):
        alone = lib_batch(ctx, [scenes[k]], [host[k]], "LA", 0.0, 25, 100)
        assert same(fx[k], alone[0][0]) and same(fy[k], alone[1][0]) and same(fx[k][:, :w], host[k]["fx"][:, :w]), k


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, named, n=1, w=12, h=10, nm=3, null=None, m=None, **pk):
    import slowflow_amd as sfa
    L = sfa.lib()
    _f, _i = C.POINTER(C.c_float), C.POINTER(C.c_int)
    fp = lambda a: a.ctypes.data_as(_f)
    W, H = 12, 10
    lab = np.zeros((3, H, 12), np.float32); cost = np.full((H, W), 0.5, np.float32)
    mm = np.array([[1, 1, 2, 2], [6, 4, 7, 5], [9, 8, 9, 7]], np.float32) if m is None else m
    fx, fy = np.full((H, W), -7.0, np.float32), np.full((H, W), -7.0, np.float32)
    strides = dict(lab_stride=pk.pop("lab_stride", 12), flow_stride=pk.pop("flow_stride", W))
    a = dict(p=sfa.epic_params(**pk), lab=(_f * 1)(fp(lab)), cost=(_f * 1)(fp(cost)), matches=(_f * 1)(fp(mm)), nm=(C.c_int * 1)(nm), flow_x=(_f * 1)(fp(fx)),
             flow_y=(_f * 1)(fp(fy)), rc=(C.c_int * 1)(-9), status=(C.c_int * 1)(5))
    rc = a["rc"]
    if null in a:
        a[null] = None
    elif null:                                                        # "cost[0]": the image's own pointer
        a[null[:-3]] = type(a[null[:-3]])()
    before = ctx.epic_batch_stage_ms()
    r = L.sfa_epic_batch(ctx.h, n, w, h, C.byref(a["p"]) if a["p"] is not None else None, a["lab"], strides["lab_stride"], a["cost"], a["matches"], a["nm"], a["flow_x"],
                         a["flow_y"], strides["flow_stride"], a["rc"], None, None, 0, a["status"])
    msg = L.sfa_last_error(ctx.h).decode()
    assert r == SFA_ERR_ARG and "sfa_epic_batch" in msg and named in msg, (r, msg, named)
    assert (fx == -7.0).all() and (fy == -7.0).all() and rc[0] == -9      # nothing was computed
    assert ctx.epic_batch_stage_ms() == before                          # and nothing launched: the stage times are the last call's


@pytest.fixture(scope="module")
def after_a_call(ctx):
    """a call that is not refused, so that the stage times the refusals must leave alone are not all 0"""
    import slowflow_amd as sfa
    w, h = 12, 10
    m = np.array([[1, 1, 2, 2], [6, 4, 7, 5], [9, 8, 9, 7]], np.float32)
    fx, fy, rc, counts, kept = ctx.epic_batch([np.zeros((3, h, 12), np.float32)], [np.full((h, w), 0.5, np.float32)], [m], sfa.epic_params(saliency_th=0.0, pref_nn=0, nn=2))
    assert rc == [0] and np.isfinite(fx[0]).all() and ctx.epic_batch_stage_ms()["filters"] > 0
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("named,kw", [
    ("n =", dict(n=0)), ("w x h", dict(w=0)), ("w x h", dict(h=-1)), ("nn =", dict(nn=0)), ("pref_nn =", dict(pref_nn=-1)), ("method =", dict(method=2)),
    ("lab_stride =", dict(lab_stride=11)), ("flow_stride =", dict(flow_stride=11)), ("nm[0] =", dict(nm=-1)), ("w * h", dict(w=1 << 15, h=(1 << 14) + 1, saliency_th=0.0, flow_stride=1 << 15)),
    ("nm[0] * nn", dict(nm=1 << 17, nn=1 << 17, pref_nn=0)), ("w x h", dict(w=4001, h=4001, flow_stride=4001, lab_stride=4004)),
    ("matches[0]: match 1", dict(m=np.array([[1, 1, 2, 2], [6, np.nan, 7, 5], [9, 8, 9, 7]], np.float32))),
    ("matches[0]: match 2", dict(m=np.array([[1, 1, 2, 2], [6, 4, 7, 5], [9, 8, np.inf, 7]], np.float32))),
    ("Gaussian", dict(w=8, h=10, flow_stride=8, lab_stride=8)),
] + [(name + " is null", dict(null=name)) for name in ("p", "lab", "cost", "matches", "nm", "flow_x", "flow_y", "rc", "status")]
  + [(name + "[0] is null", dict(null=name + "[0]")) for name in ("lab", "cost", "matches", "flow_x", "flow_y")])
def test_refusals_name_the_argument(after_a_call, named, kw):
    _raw(after_a_call, named, **kw)
