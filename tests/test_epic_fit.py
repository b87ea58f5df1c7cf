"""EpicFlow's model fit and dense application on the GPU (sfa_epic_interpolate_batch, slowflow_amd/csrc/epic_fit.hip) against the host code it restates
(slowflow_amd/host/epic.cpp: epic_fit_localaffine, epic_fit_nadarayawatson, the apply loops of epic()), and epic_batch, which now runs this stage on the GPU
too, against epic().  Models and flow planes are compared by their bit patterns (np.array_equal on uint32 views), no tolerance; the one exception: where the
host's Nadaraya-Watson result is NaN (weights summing to 0) only NaN-ness is compared -- the sign of a 0/0 NaN differs between x86 and the GPU.  The host
side runs in tests/host/epic_fit_tool.cpp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_epic import scene
from test_epic_nn import epic_scenes, run_epic_tool, scene_cost_and_seeds  # noqa: F401  (epic_scenes: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "slowflow_amd", "host")
SFA_OK, SFA_ERR_ARG = 0, -1
METHODS = ("LA", "NW")


# ---- CPU: the boundary -------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    header = open(os.path.join(ROOT, "include", "slowflow_amd.h")).read()
    L = C.CDLL(sfa.LIB_PATH)
    for name in ("sfa_epic_interpolate_batch", "sfa_epic_fit_stage_ms"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in sfa.EXPORTS, name
        assert hasattr(L, name), name
    assert callable(getattr(sfa.Context, "epic_interpolate")) and callable(getattr(sfa.Context, "epic_fit_stage_ms"))
    assert "epic_fit.hip" in open(os.path.join(ROOT, "slowflow_amd", "csrc", "Makefile")).read()


def test_the_kernel_regression_fit_is_public():
    text = open(os.path.join(HOST, "epic.h")).read()
    assert re.search(r"\bvoid\s+epic_fit_nadarayawatson\s*\(", text) and re.search(r"\bvoid\s+epic_fit_localaffine\s*\(", text)
    assert not re.search(r"static\s+void\s+fit_nadarayawatson", open(os.path.join(HOST, "epic.cpp")).read())


# ---- the host side -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    r = subprocess.run(["make", "-C", HOST], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path_factory.mktemp("epic_fit") / "epic_fit_tool")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-pthread", "-I", HOST, os.path.join(ROOT, "tests", "host", "epic_fit_tool.cpp"), os.path.join(HOST, "libslowflow_host.a"),
                        "-L", os.path.join(ROOT, "slowflow_amd"), "-lslowflow_amd", "-lz", "-Wl,-rpath," + os.path.join(ROOT, "slowflow_amd"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


def host_fit(tool, d, labels, seeds, vects, index, weight, method, stride=None):
    """the host's fit and apply loop: (fx (h, stride), fy, model (ns, 6 or 2)); the planes' columns >= w hold NaN"""
    h, w = labels.shape
    ns, nn = index.shape
    stride = w if stride is None else stride
    for name, a, t in (("labels", labels, np.int32), ("seeds", seeds, np.int32), ("vects", vects, np.float32), ("index", index, np.int32), ("weight", weight, np.float32)):
        np.ascontiguousarray(a, t).tofile(os.path.join(d, name + ".bin"))
    r = subprocess.run([tool, "fit", d, str(w), str(h), str(ns), str(nn), method, str(stride)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return (np.fromfile(os.path.join(d, "fx.bin"), np.float32).reshape(h, stride), np.fromfile(os.path.join(d, "fy.bin"), np.float32).reshape(h, stride),
            np.fromfile(os.path.join(d, "model.bin"), np.float32).reshape(ns, 6 if method == "LA" else 2))


def same_bits(got, want, nan_ok=False):
    """the same bit patterns; with nan_ok a NaN of the host's may be any NaN"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    if not nan_ok:
        return np.array_equal(got.view(np.uint32), want.view(np.uint32))
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def check(ctx, tool, d, labels, seeds, vects, index, weight, method, stride=None):
    """one image through both sides: model and both planes; returns the host's (fx, fy, model)"""
    labels, seeds, vects = np.asarray(labels, np.int32), np.asarray(seeds, np.int32).reshape(-1, 2), np.asarray(vects, np.float32).reshape(-1, 2)
    index, weight = np.asarray(index, np.int32), np.asarray(weight, np.float32)
    want = host_fit(tool, d, labels, seeds, vects, index, weight, method, stride)
    fx, fy, model = ctx.epic_interpolate([labels], [seeds], [vects], [index], [weight], method=method, stride=stride)
    w = labels.shape[1]
    nan_ok = method == "NW"
    assert same_bits(model[0], want[2], nan_ok), (method, "model")
    assert same_bits(fx[0][:, :w], want[0][:, :w], nan_ok) and same_bits(fy[0][:, :w], want[1][:, :w], nan_ok), (method, "flow")
    assert np.isnan(fx[0][:, w:]).all() and np.isnan(fy[0][:, w:]).all()          # the pad columns keep what they held
    return want


def kernel_weights(dist):
    """exp(-0.8 d) + 1e-8 as fp32, formed once: both sides get this array"""
    with np.errstate(under="ignore"):
        return (np.exp(np.float32(-0.8) * dist.astype(np.float32)) + np.float32(1e-8)).astype(np.float32)


def scene_inputs(w, h, seed, n_matches=400):
    cost, seeds = scene_cost_and_seeds(w, h, seed, n_matches=n_matches)
    _, _, m = scene(w, h, seed, n_matches=n_matches)
    lim = np.array([w - 1, h - 1, w - 1, h - 1], np.float32)
    m = np.clip(m, 0, lim)
    return cost, np.ascontiguousarray(seeds, np.int32), np.ascontiguousarray(m[:, 2:4] - m[:, 0:2], np.float32)


# ---- GPU: 1. real lists --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed", [(96, 64, 0), (131, 77, 1)])
def test_lists_of_the_scene(ctx, tool, tmp_path, w, h, seed):
    cost, seeds, vects = scene_inputs(w, h, seed)
    ns = len(seeds)
    for nn in (1, 26, 100, ns + 50):                                  # the last: every row ends in -1 entries
        labels, index, dist = ctx.epic_nearest_seeds([cost], [seeds], nn)
        weight = kernel_weights(dist[0])
        if nn > ns:
            assert (index[0][:, ns:] == -1).all()
        for method in METHODS:
            for stride in (w, w + 5):
                check(ctx, tool, str(tmp_path), labels[0], seeds, vects, index[0], weight, method, stride)


# ---- GPU: 2. batches, sub-batches and the flag -----------------------------------------------------------------------------------------------------------
def raw_call(ctx, method, w, h, labels, seeds, vects, index, weight, fx, fy, stride, model, budget, n=None, nn=None, ns=None, null=()):
    """sfa_epic_interpolate_batch through ctypes on lists of arrays (None: a null array of pointers); returns (rc, message, status)"""
    import slowflow_amd as sfa
    L = sfa.lib()
    _f, _i = C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.sfa_epic_interpolate_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_i), C.POINTER(_i), C.POINTER(_f), _i, C.c_int, C.POINTER(_i),
                                             C.POINTER(_f), C.POINTER(_f), C.POINTER(_f), C.c_int, C.POINTER(_f), C.c_size_t, _i]
    k = len(seeds)

    def ptrs(name, arrs, t):
        if arrs is None or name in null:
            return None
        out = (t * k)(*[a.ctypes.data_as(t) for a in arrs])
        if name + "[0]" in null:
            out[0] = t()
        return out
    status = (C.c_int * k)(*([5] * k))
    nsv = (C.c_int * k)(*(ns if ns is not None else [len(s) for s in seeds]))
    rc = L.sfa_epic_interpolate_batch(ctx.h, k if n is None else n, w, h, method, ptrs("labels", labels, _i), ptrs("seeds_xy", seeds, _i), ptrs("vects", vects, _f),
                                      None if "ns" in null else nsv, index[0].shape[1] if nn is None else nn, ptrs("nn_index", index, _i), ptrs("nn_weight", weight, _f),
                                      ptrs("flow_x", fx, _f), ptrs("flow_y", fy, _f), stride, ptrs("model", model, _f), budget, None if "status" in null else status)
    return rc, L.sfa_last_error(ctx.h).decode(), list(status)


@pytest.mark.gpu
def test_batch_sub_batches_and_the_flag(ctx):
    """three images of different ns in one call equal the three single calls -- also when the workspace holds one image at a time; with a workspace that holds
    none, every image comes back flagged and nothing is written"""
    w, h, nn = 96, 64, 26
    costs, seeds, vects = zip(*[scene_inputs(w, h, 20 + k, n_matches=ns) for k, ns in enumerate((300, 400, 350))])
    labels, index, dist = ctx.epic_nearest_seeds(list(costs), list(seeds), nn)
    weight = [kernel_weights(d) for d in dist]
    for method in METHODS:
        single = [ctx.epic_interpolate([labels[k]], [seeds[k]], [vects[k]], [index[k]], [weight[k]], method=method) for k in range(3)]
        # An image needs its lists (2 * ns * nn * 4 bytes), seeds, vectors and models (ns * (16 + 24) bytes at most), labels and two planes (3 * 24 576 bytes)
        # and less than 2 KB of alignment: 149 KB .. 174 KB for ns = 300 .. 400.  200 000 bytes hold any one of them and no two
        for budget in (0, 200000):
            fx, fy, model, status = ctx.epic_interpolate(labels, list(seeds), list(vects), index, weight, method=method, workspace_bytes=budget, with_status=True)
            assert status == [0, 0, 0]
            for k in range(3):
                assert same_bits(model[k], single[k][2][0]) and same_bits(fx[k], single[k][0][0]) and same_bits(fy[k], single[k][1][0]), (method, budget, k)
        mf = 6 if method == "LA" else 2
        fx = [np.full((h, w), -7.0, np.float32) for _ in range(3)]
        fy = [np.full((h, w), -7.0, np.float32) for _ in range(3)]
        model = [np.full((len(s), mf), -7.0, np.float32) for s in seeds]
        rc, msg, status = raw_call(ctx, METHODS.index(method), w, h, labels, seeds, vects, index, weight, fx, fy, w, model, 60000)   # less than any image's lists
        assert rc == SFA_OK and status == [1, 1, 1], (rc, msg, status)
        assert all((a == -7.0).all() for a in fx + fy + model)


# ---- GPU: 3. the branches of the fit ---------------------------------------------------------------------------------------------------------------------
W, H = 24, 16


def some_labels(ns, seed=0):
    return np.random.default_rng(seed).integers(0, ns, (H, W)).astype(np.int32)


def both(ctx, tool, tmp_path, seeds, vects, index, weight, labels=None):
    labels = some_labels(len(seeds)) if labels is None else labels
    return {m: check(ctx, tool, str(tmp_path), labels, seeds, vects, index, weight, m) for m in METHODS}


@pytest.mark.gpu
def test_one_seed_one_neighbour(ctx, tool, tmp_path):
    res = both(ctx, tool, tmp_path, [(3, 2)], [(1.5, -0.25)], [[0]], [[0.7]])
    assert np.array_equal(res["NW"][2], np.array([[1.5, -0.25]], np.float32))


@pytest.mark.gpu
def test_two_seeds_on_one_pixel_and_a_row_without_its_own_seed(ctx, tool, tmp_path):
    """seeds 0 and 1 share a pixel: the search hands both the list of seed 1, so row 0 does not contain 0 and coefi stays 0 (no 0.1 px points)"""
    seeds = [(5, 5), (5, 5), (9, 3), (2, 7), (14, 11)]
    vects = [(1.0, 0.5), (-2.0, 0.25), (0.5, 0.5), (3.0, -1.0), (0.0, 2.0)]
    index = [[1, 2, 3, 4], [1, 2, 3, 4], [2, 1, 4, 3], [3, 1, 2, 4], [4, 2, 1, 3]]
    weight = np.array([[1.0, 0.4, 0.3, 0.05]] * 5, np.float32)
    both(ctx, tool, tmp_path, seeds, vects, index, weight)


@pytest.mark.gpu
def test_a_seed_listed_twice_in_its_own_row(ctx, tool, tmp_path):
    """the last occurrence decides coefi, and both are scaled by 0.96"""
    seeds = [(4, 4), (12, 6), (20, 13), (7, 10)]
    vects = [(1.0, 1.0), (-1.0, 2.0), (0.5, -3.0), (2.0, 0.0)]
    index = [[0, 1, 0, 2, 3], [1, 0, 2, 1, 3], [3, 2, 1, 2, 2], [0, 1, 2, 3, 3]]
    weight = np.array([[0.9, 0.5, 0.3, 0.2, 0.1], [1.0, 0.8, 0.1, 0.6, 0.2], [0.2, 0.9, 0.3, 0.4, 0.7], [0.3, 0.2, 0.1, 0.6, 0.9]], np.float32)
    both(ctx, tool, tmp_path, seeds, vects, index, weight)


@pytest.mark.gpu
def test_all_weights_zero(ctx, tool, tmp_path):
    """the normal matrix is all zeros: solve3 returns on its zero pivot, the model is 0 and the flow (-x, -y); Nadaraya-Watson divides 0 by 0"""
    seeds = [(4, 4), (12, 6), (20, 13)]
    res = both(ctx, tool, tmp_path, seeds, [(1.0, 1.0), (-1.0, 2.0), (0.5, -3.0)], [[0, 1, 2], [1, 0, 2], [2, 1, 0]], np.zeros((3, 3), np.float32))
    fx, fy, model = res["LA"]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    assert (model == 0).all() and np.array_equal(fx, -xx) and np.array_equal(fy, -yy)
    assert np.isnan(res["NW"][2]).all()


@pytest.mark.gpu
def test_collinear_seeds_on_one_row(ctx, tool, tmp_path):
    """every seed has y = 4: without the four 0.1 px points the y column is a multiple of the constant one"""
    seeds = [(2, 4), (7, 4), (11, 4), (15, 4), (21, 4)]
    vects = [(1.0, 0.5), (1.5, 0.25), (2.0, 0.0), (2.5, -0.25), (3.0, -0.5)]
    index = [[k] + [j for j in range(5) if j != k] for k in range(5)]
    weight = np.array([[1.0, 0.5, 0.25, 0.125, 0.0625]] * 5, np.float32)
    res = both(ctx, tool, tmp_path, seeds, vects, index, weight)
    assert np.isfinite(res["LA"][2]).all() and (res["LA"][2] != 0).any()


@pytest.mark.gpu
def test_seeds_in_the_far_corner_with_large_vectors(ctx, tool, tmp_path):
    seeds = [(W - 1, H - 1), (W - 1, 0), (0, H - 1), (W - 2, H - 2)]
    vects = [(1e3, -1e3), (-1e3, 1e3), (1e3, 1e3), (999.5, -1000.25)]
    index = [[0, 3, 1, 2], [1, 0, 3, 2], [2, 3, 0, 1], [3, 0, 2, 1]]
    weight = np.array([[1.0, 0.7, 0.01, 0.02]] * 4, np.float32)
    both(ctx, tool, tmp_path, seeds, vects, index, weight)


@pytest.mark.gpu
def test_weights_of_1e_8_next_to_1(ctx, tool, tmp_path):
    rng = np.random.default_rng(3)
    ns, nn = 70, 37                                                   # two waves of seeds, two tiles of columns, both ragged
    seeds = np.stack([rng.integers(0, W, ns), rng.integers(0, H, ns)], 1)
    vects = rng.uniform(-4, 4, (ns, 2)).astype(np.float32)
    index = np.stack([np.concatenate([[k], rng.permutation(np.delete(np.arange(ns), k))[:nn - 1]]) for k in range(ns)]).astype(np.int32)
    weight = np.where(rng.uniform(0, 1, (ns, nn)) < 0.5, np.float32(1.0), np.float32(1e-8)).astype(np.float32)
    both(ctx, tool, tmp_path, seeds, vects, index, weight)


@pytest.mark.gpu
def test_the_plain_form_gives_the_same_bits(ctx, switches):
    """SFA_EPIC_FIT_PLAIN (full build): the lists read row by row from global memory instead of through the LDS tiles"""
    w, h, nn = 96, 64, 40
    cost, seeds, vects = scene_inputs(w, h, 2, n_matches=333)
    labels, index, dist = ctx.epic_nearest_seeds([cost], [seeds], nn)
    weight = kernel_weights(dist[0])
    for method in METHODS:
        staged = ctx.epic_interpolate(labels, [seeds], [vects], index, [weight], method=method)
        switches.set("SFA_EPIC_FIT_PLAIN", "1")
        plain = ctx.epic_interpolate(labels, [seeds], [vects], index, [weight], method=method)
        switches.unset("SFA_EPIC_FIT_PLAIN")
        assert all(same_bits(a[0], b[0]) for a, b in zip(staged, plain)), method


# ---- GPU: 4. guards -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_indices_and_labels_outside_the_seeds(ctx, tool, tmp_path):
    """a bounds check: list entries >= ns are skipped like the negative ones, pixels labelled -1 or ns get 0.0f; everything else equals the host's result on the
    same input with those entries removed"""
    rng = np.random.default_rng(5)
    ns, nn = 20, 6
    seeds = np.stack([rng.integers(0, W, ns), rng.integers(0, H, ns)], 1).astype(np.int32)
    vects = rng.uniform(-4, 4, (ns, 2)).astype(np.float32)
    index = np.stack([np.concatenate([[k], rng.permutation(np.delete(np.arange(ns), k))[:nn - 1]]) for k in range(ns)]).astype(np.int32)
    weight = rng.uniform(0.05, 1, (ns, nn)).astype(np.float32)
    labels = some_labels(ns, 1)
    bad_index, bad_labels = index.copy(), labels.copy()
    bad_index[3, 2] = ns; bad_index[7, 0] = ns + 5; bad_index[11, 5] = 2 ** 31 - 1; bad_index[15, 1] = -1
    bad_labels[0, 0] = -1; bad_labels[5, 7] = ns; bad_labels[H - 1, W - 1] = -1; bad_labels[9, 3] = 2 ** 31 - 1
    off = (bad_labels < 0) | (bad_labels >= ns)
    for method in METHODS:
        want = host_fit(tool, str(tmp_path), labels, seeds, vects, np.where((bad_index < 0) | (bad_index >= ns), -1, bad_index), weight, method)
        mf = want[2].shape[1]
        fx, fy, model = np.full((H, W), -7.0, np.float32), np.full((H, W), -7.0, np.float32), np.full((ns, mf), -7.0, np.float32)
        rc, msg, status = raw_call(ctx, METHODS.index(method), W, H, [bad_labels], [seeds], [vects], [bad_index], [weight], [fx], [fy], W, [model], 0)
        assert rc == SFA_OK and status == [0], (rc, msg)
        assert same_bits(model, want[2])
        assert (fx[off] == 0).all() and (fy[off] == 0).all() and not np.signbit(fx[off]).any() and not np.signbit(fy[off]).any()
        assert same_bits(fx[~off], want[0][~off]) and same_bits(fy[~off], want[1][~off])


# ---- GPU: 5. refusals ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_name_the_argument(ctx):
    w, h, ns, nn = 8, 6, 2, 2
    a = dict(labels=[np.zeros((h, w), np.int32)], seeds=[np.array([[1, 1], [6, 4]], np.int32)], vects=[np.ones((ns, 2), np.float32)],
             index=[np.array([[0, 1], [1, 0]], np.int32)], weight=[np.ones((ns, nn), np.float32)], fx=[np.full((h, w), -7.0, np.float32)],
             fy=[np.full((h, w), -7.0, np.float32)], model=[np.full((ns, 6), -7.0, np.float32)])

    def call(named, method=0, w=w, h=h, stride=w, drop=(), **kw):
        b = {k: (None if k in drop else v) for k, v in a.items()}
        rc, msg, _ = raw_call(ctx, method, w, h, b["labels"], b["seeds"], b["vects"], b["index"], b["weight"], b["fx"], b["fy"], stride, b["model"], 0, **kw)
        assert rc == SFA_ERR_ARG and "sfa_epic_interpolate_batch" in msg and named in msg, (rc, msg, named)
        assert all((x[0] == -7.0).all() for x in (a["fx"], a["fy"], a["model"]))              # nothing was written

    call("n =", n=0)
    call("w x h", w=0, stride=8)
    call("w x h", h=-1)
    call("nn =", nn=0)
    call("ns[0]", ns=[0])
    call("method =", method=2)
    call("method =", method=-1)
    call("stride =", stride=w - 1)
    for name in ("seeds_xy", "vects", "ns", "nn_index", "nn_weight", "status"):
        call(name + " is null", null=(name,))
    call("flow_x is null", drop=("fx",))
    call("flow_y is null", drop=("fy",))
    call("labels is null", drop=("labels",))
    call("model is null", drop=("fx", "fy", "model"))
    for name in ("labels", "seeds_xy", "vects", "nn_index", "nn_weight", "flow_x", "flow_y", "model"):
        call(name + "[0] is null", null=(name + "[0]",))
    call("w * h", w=1 << 15, h=(1 << 14) + 1, stride=1 << 15)         # more than 2^29 pixels
    call("ns[0] * nn", nn=1 << 30)                                    # 2 * 2^30 list entries
    fx, fy, model = ctx.epic_interpolate(a["labels"], a["seeds"], a["vects"], a["index"], a["weight"])      # and the call that is not refused computes
    assert np.isfinite(fx[0]).all() and np.isfinite(model[0]).all()


# ---- GPU: 6. models only ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_models_only(ctx):
    w, h, nn = 96, 64, 26
    cost, seeds, vects = scene_inputs(w, h, 0)
    labels, index, dist = ctx.epic_nearest_seeds([cost], [seeds], nn)
    weight = kernel_weights(dist[0])
    for method in METHODS:
        _, _, full = ctx.epic_interpolate(labels, [seeds], [vects], index, [weight], method=method)
        fx, fy, model = ctx.epic_interpolate(None, [seeds], [vects], index, [weight], method=method)         # flow_x = flow_y = labels = NULL
        assert fx is None and fy is None and same_bits(model[0], full[0])
    ms = ctx.epic_fit_stage_ms()
    assert set(ms) == {"fit", "apply"} and ms["fit"] > 0 and ms["apply"] == 0


# ---- GPU: 7. epic_batch == epic() ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("method,pref_nn,nn,budget", [("LA", 25, 100, None), ("NW", 25, 100, None), ("LA", 0, 100, None), ("NW", 0, 30, None),
                                                      ("LA", 25, 100, 200000), ("NW", 25, 100, 200000)])
def test_epic_batch_equals_epic(tool, epic_scenes, tmp_path, method, pref_nn, nn, budget):
    """three scenes of two sizes in one epic_batch, its searches, model fits and dense fields on the GPU: epic()'s flow fields bit for bit.  A workspace of
    200 KB holds none of these images in either GPU stage (their lists alone are larger): every image goes through the host code, the fields are the same"""
    for k, (fx, fy, bfx, bfy) in enumerate(run_epic_tool(tool, str(tmp_path), epic_scenes, method, 0.0, pref_nn, nn, budget=budget)):
        assert np.array_equal(bfx.view(np.uint32), fx.view(np.uint32)) and np.array_equal(bfy.view(np.uint32), fy.view(np.uint32)), (k, method)
        assert len(np.unique(bfx)) > 50
