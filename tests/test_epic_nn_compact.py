"""The compact search of EpicFlow's nearest-seeds stage (sfa_ctx_set_epic_search, slowflow_amd/csrc/epic_nn.hip: k_epic_search over a dense row or a sparse
map per seed, in slices that share one workspace; epic_nn_plan.h plans them) against the host's epic_nearest_seeds: every output bit for bit, in both forms of
the visited set, whole and in slices, and sfa_epic_nn_search_info to show which code ran.  The default mode's behaviour is pinned by tests/test_epic_nn.py."""
import ctypes as C

import numpy as np
import pytest

from test_epic_batch import host_run, lib_batch, six_scenes, workdir  # noqa: F401  (six_scenes, workdir: fixtures)
from test_epic_batch import same as same_planes
from test_epic_batch import tool as batch_tool  # noqa: F401  (a fixture: the host side of epic_batch)
from test_epic_nn import host_nearest_seeds, same, scene_cost_and_seeds, tool  # noqa: F401  (tool: the fixture)

pytestmark = pytest.mark.gpu
SFA_ERR_ARG = -1
FORMS = ("dense", "sparse")


@pytest.fixture(scope="module")
def ctx():
    """a context of its own in compact mode"""
    import slowflow_amd as sfa
    c = sfa.Context(0)
    c.set_epic_search("compact")
    yield c
    c.close()


def run(ctx, costs, seeds, nn, **kw):
    labels, index, dist = ctx.epic_nearest_seeds(costs, seeds, nn, **kw)
    return list(zip(labels, index, dist)), ctx.epic_nn_search_info()


def check_forms(ctx, switches, tool, d, cost, seeds, nn, forms=FORMS):
    """one image alone in each forced form: the host's bits, and search_info names the form"""
    want = host_nearest_seeds(tool, d, cost, seeds, nn)
    for form in forms:
        switches.set("SFA_EPIC_NN_SET", form)
        got, info = run(ctx, [cost], [seeds], nn)
        assert same(got[0], want), form
        assert (info["dense"], info["sparse"]) == ((1, 0) if form == "dense" else (0, 1)) and info["slices"] >= 1 and info["workspace_bytes"] > 0, (form, info)
    return want


# ---- 1. both forms against the host ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,seed", [(96, 64, 0), (131, 77, 1)])
def test_both_forms_equal_the_host(ctx, switches, tool, tmp_path, w, h, seed):
    cost, seeds = scene_cost_and_seeds(w, h, seed)
    for nn in (1, 26, 100, len(seeds) + 50):
        _, index, _ = check_forms(ctx, switches, tool, str(tmp_path), cost, seeds, nn)
        if nn > len(seeds):
            assert (index[:, len(seeds):] == -1).all()


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------------------------------------
def test_lattice_of_tied_distances_in_the_sparse_form(ctx, switches, tool, tmp_path):
    """constant cost, seeds on a lattice: only the heap's order decides the order of tied distances and who is the nn-th, so a visited set that answers
    differently at any node changes the lists"""
    cost = np.full((48, 64), 0.25, np.float32)
    seeds = [(4 + 8 * a, 4 + 8 * b) for b in range(6) for a in range(8)]
    for nn in (20, 48, 60):
        _, index, dist = check_forms(ctx, switches, tool, str(tmp_path), cost, seeds, nn, forms=("sparse",))
        if nn <= 48:
            assert sum(int((np.diff(row) == 0).sum()) for row in dist) > 100       # (the case does hold ties)
        else:
            assert (index[:, 48:] == -1).all() and (dist[:, 48:].view(np.uint32) == 0x7F7F7F7F).all()


# ---- 3. degenerate graphs in the sparse form -------------------------------------------------------------------------------------------------------------
def test_degenerate_graphs_in_the_sparse_form(ctx, switches, tool, tmp_path):
    d = str(tmp_path)
    rng = np.random.default_rng(7)
    sparse = ("sparse",)
    _, index, _ = check_forms(ctx, switches, tool, d, rng.uniform(0.1, 1, (1, 50)).astype(np.float32), [(3, 0), (20, 0), (44, 0)], 3, sparse)   # one row: E = 0, maps of 2 slots
    assert (index[:, 1:] == -1).all()
    assert ctx.epic_nn_search_info()["workspace_bytes"] == 2 * 256    # 3 maps of 16 bytes and 3 heaps of one entry, each rounded to 256 bytes
    check_forms(ctx, switches, tool, d, rng.uniform(0.1, 1, (2, 2)).astype(np.float32), [(0, 0), (1, 1)], 2, sparse)
    cost = rng.uniform(0.05, 0.5, (15, 20)).astype(np.float32)
    check_forms(ctx, switches, tool, d, cost, [(3, 4)], 2, sparse)                                                                               # a single seed
    labels, _, _ = check_forms(ctx, switches, tool, d, cost, [(5, 5), (12, 7), (5, 5)], 3, sparse)                                               # duplicate seeds: seed 0 owns no region
    assert labels[5, 5] == 2 and not (labels == 0).any()
    cost = np.full((30, 40), 0.3, np.float32)
    cost[8:19, 10:21] = np.inf
    labels, _, _ = check_forms(ctx, switches, tool, d, cost, [(2, 2), (35, 25), (30, 3)], 3, sparse)                                             # unreachable pixels
    assert (labels == -1).sum() == 121


# ---- 4 - 7: the six images of test_epic_nn.py::test_batch_sub_batches_and_the_flag ----------------------------------------------------------------------------
NS6 = (250, 300, 262, 287, 275, 700)


@pytest.fixture(scope="module")
def six(tool, tmp_path_factory):
    """(costs, seeds, the host's results) of six 96 x 64 images, nn 5 -- computed once, read by every test below"""
    w, h, nn = 96, 64, 5
    d = str(tmp_path_factory.mktemp("six_nn"))
    rng = np.random.default_rng(11)
    costs, seeds, want = [], [], []
    for k, ns in enumerate(NS6):
        costs.append(rng.uniform(0.02, 0.6, (h, w)).astype(np.float32))
        seeds.append(np.stack([rng.integers(0, w, ns), rng.integers(0, h, ns)], 1))
        want.append(host_nearest_seeds(tool, d, costs[k], seeds[k], nn))
    return costs, seeds, want, nn


def test_slices_of_64_and_128_seeds(ctx, switches, six):
    """SFA_EPIC_NN_SLICE caps a slice: at 64 the 700-seed image takes 11 slices, the last of 60 seeds; the count of slices is the sum of ceil(ns / slice)"""
    costs, seeds, want, nn = six
    for form in FORMS:
        switches.set("SFA_EPIC_NN_SET", form)
        for cap in (64, 128):
            switches.set("SFA_EPIC_NN_SLICE", cap)
            got, info = run(ctx, costs, seeds, nn)
            for k in range(6):
                assert same(got[k], want[k]), (form, cap, k)
            assert info["slices"] == sum(-(-ns // cap) for ns in NS6), (form, cap, info)
            assert (info["dense"], info["sparse"]) == ((6, 0) if form == "dense" else (0, 6))
        switches.set("SFA_EPIC_NN_SLICE", 64)
        got, info = run(ctx, costs[5:], seeds[5:], nn)
        assert same(got[0], want[5]) and info["slices"] == 11 and 700 - 10 * 64 == 60, (form, info)


def test_an_image_too_large_for_the_default_mode_is_computed_in_slices(ctx, switches, six):
    """1.25 MB: `done` alone is 700 * 700 floats = 1.96 MB for the sixth image, so the default mode flags it and the dense form can only run it in slices"""
    import slowflow_amd as sfa
    costs, seeds, want, nn = six
    switches.set("SFA_EPIC_NN_SET", "dense")
    labels, index, dist, status = ctx.epic_nearest_seeds(costs, seeds, nn, workspace_bytes=1250000, with_status=True)
    info = ctx.epic_nn_search_info()
    assert status == [0] * 6
    for k in range(6):
        assert same((labels[k], index[k], dist[k]), want[k]), k
    assert info["slices"] > 6 and info["dense"] == 6 and info["sparse"] == 0 and info["workspace_bytes"] < 1250000, info
    other = sfa.Context(0)                                            # the same call in the default mode
    try:
        assert other.epic_nearest_seeds(costs, seeds, nn, workspace_bytes=1250000, with_status=True)[3] == [0, 0, 0, 0, 0, 1]
        assert other.epic_nn_search_info()["sparse"] == 0
    finally:
        other.close()
    switches.unset("SFA_EPIC_NN_SET")                                 # the form the planner chooses
    labels, index, dist, status = ctx.epic_nearest_seeds(costs, seeds, nn, workspace_bytes=1250000, with_status=True)
    info = ctx.epic_nn_search_info()
    assert status == [0] * 6 and info["dense"] + info["sparse"] == 6, info
    for k in range(6):
        assert same((labels[k], index[k], dist[k]), want[k]), k


def test_batch_invariance(ctx, six):
    """the six images as one call, one by one, and in reversed order: identical bits per image"""
    costs, seeds, want, nn = six
    whole, _ = run(ctx, costs, seeds, nn)
    back, _ = run(ctx, costs[::-1], seeds[::-1], nn)
    for k in range(6):
        alone, _ = run(ctx, [costs[k]], [seeds[k]], nn)
        assert same(whole[k], want[k]) and same(alone[0], whole[k]) and same(back[5 - k], whole[k]), k


def test_the_flag_survives(ctx):
    """200 KB is less than the lists of these images alone (400 seeds, nn 100: 160 KB each, held twice): every image is flagged in compact mode too and
    nothing is written"""
    import slowflow_amd as sfa
    L = sfa.lib()
    _f, _i = C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.sfa_epic_nearest_seeds_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(_f), C.POINTER(_i), _i, C.c_int, C.POINTER(_i), C.POINTER(_i),
                                               C.POINTER(_f), C.c_size_t, _i]
    w, h, nn, n = 96, 64, 100, 2
    made = [scene_cost_and_seeds(w, h, s) for s in (0, 3)]
    costs = [np.ascontiguousarray(c, np.float32) for c, _ in made]
    seeds = [np.ascontiguousarray(s, np.int32) for _, s in made]
    labels = [np.full((h, w), -7, np.int32) for _ in range(n)]
    index = [np.full((len(s), nn), -7, np.int32) for s in seeds]
    dist = [np.full((len(s), nn), -3.0, np.float32) for s in seeds]
    status = (C.c_int * n)(5, 5)
    fp, ip = (lambda a: a.ctypes.data_as(_f)), (lambda a: a.ctypes.data_as(_i))
    rc = L.sfa_epic_nearest_seeds_batch(ctx.h, n, w, h, (_f * n)(*[fp(a) for a in costs]), (_i * n)(*[ip(a) for a in seeds]), (C.c_int * n)(*[len(s) for s in seeds]), nn,
                                        (_i * n)(*[ip(a) for a in labels]), (_i * n)(*[ip(a) for a in index]), (_f * n)(*[fp(a) for a in dist]), 200000, status)
    assert rc == 0, L.sfa_last_error(ctx.h)
    assert list(status) == [1, 1]
    assert all((a == -7).all() for a in labels + index) and all((a == -3.0).all() for a in dist)
    assert ctx.epic_nn_search_info()["slices"] == 0


# ---- 8. through the chain ------------------------------------------------------------------------------------------------------------------------------------
def test_epic_batch_in_compact_mode_equals_the_default_mode(ctx, switches, batch_tool, workdir, six_scenes):  # noqa: F811
    import slowflow_amd as sfa
    host, _ = host_run(batch_tool, workdir, "six", six_scenes, "LA", 0.045, 25, 30)
    other = sfa.Context(0)
    try:
        want = lib_batch(other, six_scenes, host, "LA", 0.045, 25, 30)
        assert other.epic_nn_search_info()["slices"] == 6             # the default mode: one per image
    finally:
        other.close()
    switches.set("SFA_EPIC_NN_SLICE", 64)
    for form in (None,) + FORMS:
        if form:
            switches.set("SFA_EPIC_NN_SET", form)
        got = lib_batch(ctx, six_scenes, host, "LA", 0.045, 25, 30)
        info = ctx.epic_nn_search_info()
        assert got[2] == want[2] == [0] * 6
        for k in range(6):
            assert same_planes(got[0][k], want[0][k]) and same_planes(got[1][k], want[1][k]) and np.array_equal(got[3][k], want[3][k]), (form, k)
        assert info["slices"] >= 3 and info["slices"] == sum(-(-int(c[2]) // 64) for c in got[3]), (form, info)
        assert info["dense"] + info["sparse"] == 6 and (form is None or info[form] == 6), (form, info)


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_an_unknown_mode_is_refused_and_changes_nothing(ctx, six):
    import slowflow_amd as sfa
    L = sfa.lib()
    for mode in (2, -1):
        assert L.sfa_ctx_set_epic_search(ctx.h, mode) == SFA_ERR_ARG
        msg = L.sfa_last_error(ctx.h).decode()
        assert "sfa_ctx_set_epic_search" in msg and "mode = %d" % mode in msg, msg
    with pytest.raises(sfa.SlowflowError):
        ctx.set_epic_search(2)
    with pytest.raises(sfa.SlowflowError):
        ctx.set_epic_search("sparse")
    costs, seeds, want, nn = six                                      # still compact: the sixth image at 1.25 MB is computed, not flagged
    assert ctx.epic_nearest_seeds(costs[5:], seeds[5:], nn, workspace_bytes=1250000, with_status=True)[3] == [0]
    assert L.sfa_ctx_set_epic_search(None, 1) == SFA_ERR_ARG
    info = (C.c_longlong * 4)()
    assert L.sfa_epic_nn_search_info(ctx.h, None) == SFA_ERR_ARG and "info is null" in L.sfa_last_error(ctx.h).decode()
    assert L.sfa_epic_nn_search_info(ctx.h, info) == 0
