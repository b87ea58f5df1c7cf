"""sfa_consistent_regions (slowflow_amd/csrc/fill.hip): dense_tracking's removeSmallSegments on (tracked == r_Jets), computed on the GPU by connected-component
labelling (64 x 16 tiles in LDS, a union across tile borders, sizes summed at the roots), against the reference's region growing in its own scan order
(tests/fill_ref.py).  Masks are compared with ==; nothing here is approximate.  The maps are 70 x 45 and 131 x 67 (no multiple of the tile in either
direction, 2 x 3 and 3 x 5 tiles), three to a batch with a different r_Jets each, and one map of 1024 x 436."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fill_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((70, 45), (131, 67))
FULLS = (2, 4, 7)
SFA_ERR_ARG = -1


# ---- the scenes: 0/1 maps of w x h --------------------------------------------------------------------------------------------------------------
def rect(m, x0, y0, rw, rh):
    m[y0:y0 + rh, x0:x0 + rw] = 1


def scene_sizes_99_100(w, h):
    m = np.zeros((h, w), np.int32)
    rect(m, 58, 10, 11, 9)                       # 99 pixels over the tile corner (64, 16)
    rect(m, 30, 12, 10, 10)                      # 100 pixels over the tile border y = 16
    return m


def scene_diagonal(w, h, joined=False):
    m = np.zeros((h, w), np.int32)
    rect(m, 54, 10, 10, 6)                       # 60 pixels ending at (63, 15), the last pixel of a tile
    rect(m, 64, 16, 6, 10)                       # 60 pixels starting at (64, 16), the first pixel of the tile diagonally below
    if joined:
        m[15, 64] = 1
    return m


def scene_serpentine(w, h, vertical=False):
    if vertical:
        return np.ascontiguousarray(scene_serpentine(h, w).T)
    m = np.zeros((h, w), np.int32)
    m[0::2, :] = 1                               # every other row, joined at alternating ends: one path that crosses every tile border many times
    for k, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 1
    return m


def scene_u(w, h):
    m = np.zeros((h, w), np.int32)
    m[:, 3] = 1
    m[:, w - 4] = 1                              # two arms of h < 100 pixels each ...
    m[h - 1, 3:w - 3] = 1                        # ... that meet only in the last row
    return m


def scene_frame(w, h):
    m = np.zeros((h, w), np.int32)
    m[0, :] = m[h - 1, :] = 1
    m[:, 0] = m[:, w - 1] = 1
    return m


def scene_random(w, h, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.int32)


def scenes(w, h):
    out = [("sizes_99_100", scene_sizes_99_100(w, h)), ("diagonal", scene_diagonal(w, h)), ("joined", scene_diagonal(w, h, True)),
           ("serpentine_rows", scene_serpentine(w, h)), ("serpentine_columns", scene_serpentine(w, h, True)), ("u", scene_u(w, h)),
           ("frame", scene_frame(w, h)), ("ones", np.ones((h, w), np.int32)), ("zeros", np.zeros((h, w), np.int32))]
    for density in (0.3, 0.5, 0.593):            # 0.593: the site-percolation threshold of the square lattice, the largest and most ragged components
        for seed in range(3):
            out.append(("random_%g_%d" % (density, seed), scene_random(w, h, density, 100 * seed + int(1000 * density))))
    return out


def tracked_of(m, full, seed):
    """a tracked map whose (tracked == full) is m: the other pixels hold values below and above full"""
    other = np.random.default_rng(seed).choice(np.array([0, full - 1, full + 1, full + 5], np.int32), size=m.shape)
    return np.where(m == 1, np.int32(full), other).astype(np.int32)


@pytest.fixture(scope="module")
def cases():
    """per size: the scene names, the tracked maps, their full values and the restatement's masks, computed once"""
    out = {}
    for (w, h) in SIZES:
        sc = scenes(w, h)
        assert len(sc) % 3 == 0
        fulls = [FULLS[i % 3] for i in range(len(sc))]
        tracked = [tracked_of(m, f, i) for i, ((_, m), f) in enumerate(zip(sc, fulls))]
        want = [fill_ref.consistent_regions(t, f) for t, f in zip(tracked, fulls)]
        for a in tracked + want:
            a.setflags(write=False)
        out[(w, h)] = dict(names=[n for n, _ in sc], maps=[m for _, m in sc], tracked=tracked, fulls=fulls, want=want)
    return out


@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


# ---- CPU: the boundary, and that the scenes are what they claim ---------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    import slowflow_amd as sfa
    if not os.path.exists(sfa.LIB_PATH):
        sfa.build()
    header = open(os.path.join(ROOT, "include", "slowflow_amd.h")).read()
    L = C.CDLL(sfa.LIB_PATH)
    for name in ("sfa_consistent_regions", "sfa_fill_samples", "sfa_fill_matches", "sfa_fill_trajectories"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in sfa.EXPORTS, name
        assert hasattr(L, name), name
    for name in ("consistent_regions", "fill_matches", "fill_trajectories"):
        assert callable(getattr(sfa.Context, name)), name
    assert callable(sfa.fill_samples)
    assert "fill.hip" in open(os.path.join(ROOT, "slowflow_amd", "csrc", "Makefile")).read()


def test_the_device_launch_functions_are_declared():
    text = open(os.path.join(ROOT, "slowflow_amd", "csrc", "sfa_internal.h")).read()
    for name in ("consistent_regions_device", "fill_matches_device", "fill_trajectories_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_the_scenes_exercise_what_they_claim(cases):
    for (w, h), c in cases.items():
        want, maps = dict(zip(c["names"], c["want"])), dict(zip(c["names"], c["maps"]))
        m = want["sizes_99_100"]
        assert m.sum() == 100 and m[12:22, 30:40].all() and not m[10:19, 58:69].any()
        assert maps["diagonal"].sum() == 120 and want["diagonal"].sum() == 0          # the blobs touch only diagonally: each stays at 60 and vanishes
        assert want["joined"].sum() == 121                                              # one pixel joins them
        for name in ("serpentine_rows", "serpentine_columns", "u", "frame", "ones"):
            assert maps[name].sum() >= 100 and np.array_equal(want[name], maps[name]), name   # one component each, kept whole
        assert h < 100 and want["u"].sum() == 2 * h + (w - 8)                          # an arm alone is below 100
        assert want["zeros"].sum() == 0
        for name, mp, wt in zip(c["names"], c["maps"], c["want"]):
            if name.startswith("random"):
                assert wt.sum() < mp.sum(), name                                        # some components go ...
                assert wt.sum() > 0 or not name.startswith("random_0.593"), name         # ... and at the threshold some stay


def test_the_restatement_does_not_depend_on_its_scan_order(cases):
    """the claim the GPU form rests on, checked on the restatement itself: a transposed map (a row-major scan of the original) gives the transposed mask"""
    c = cases[(70, 45)]
    for name, m in zip(c["names"], c["maps"]):
        if name.startswith("random_0.593") or name in ("diagonal", "joined", "sizes_99_100"):
            a = fill_ref.remove_small_segments(m.copy())
            b = fill_ref.remove_small_segments(np.ascontiguousarray(m.T)).T
            assert np.array_equal(a, b), name


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_masks(ctx, cases):
    """every scene through the GPU, three maps with three different `full` to a batch"""
    out = {}
    for size, c in cases.items():
        masks, kept = [], []
        for b in range(0, len(c["tracked"]), 3):
            m, k = ctx.consistent_regions(np.stack(c["tracked"][b:b + 3]), c["fulls"][b:b + 3], 100)
            masks += list(m)
            kept += list(k)
        out[size] = (masks, kept)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_masks_equal_the_region_growing(gpu_masks, cases, size):
    c = cases[size]
    masks, kept = gpu_masks[size]
    for name, got, k, want in zip(c["names"], masks, kept, c["want"]):
        assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1}, name
        assert np.array_equal(got, want), "%s: %d pixels differ" % (name, int((got != want).sum()))
        assert int(k) == int(got.sum()), name


@pytest.mark.gpu
def test_a_map_alone_and_in_any_batch_position_gives_the_same_mask(ctx, cases):
    """labels cannot leak between the maps of a batch: the same tracked map, at every position of a batch of unlike maps and alone, with unlike `full`"""
    c = cases[(131, 67)]
    i = c["names"].index("random_0.593_1")
    base, full = c["tracked"][i], c["fulls"][i]
    alone, _ = ctx.consistent_regions(base[None], [full], 100)
    assert np.array_equal(alone[0], c["want"][i])
    others = [c["tracked"][c["names"].index("ones")], c["tracked"][c["names"].index("serpentine_rows")]]
    ofull = [c["fulls"][c["names"].index("ones")], c["fulls"][c["names"].index("serpentine_rows")]]
    for pos in range(3):
        tr, fl = list(others), list(ofull)
        tr.insert(pos, base)
        fl.insert(pos, full)
        m, k = ctx.consistent_regions(np.stack(tr), fl, 100)
        assert np.array_equal(m[pos], alone[0]) and int(k[pos]) == int(alone[0].sum()), pos


@pytest.mark.gpu
def test_min_size_is_the_argument_not_a_constant(ctx, cases):
    c = cases[(70, 45)]
    i = c["names"].index("sizes_99_100")
    for min_size, total in ((99, 199), (100, 100), (101, 0), (1, 199)):
        m, k = ctx.consistent_regions(c["tracked"][i][None], [c["fulls"][i]], min_size)
        assert int(m.sum()) == total == int(k[0]), min_size
    rnd = c["names"].index("random_0.5_0")
    m, _ = ctx.consistent_regions(c["tracked"][rnd][None], [c["fulls"][rnd]], 7)
    assert np.array_equal(m[0], fill_ref.consistent_regions(c["tracked"][rnd], c["fulls"][rnd], 7))


@pytest.mark.gpu
def test_a_frame_of_1024_x_436(ctx):
    """the tracking frames' size: a percolation-threshold map with a serpentine and a frame laid over it (components that span hundreds of tiles)"""
    w, h = 1024, 436
    m = scene_random(w, h, 0.593, 7)
    m[100:200] = 0
    m[102:198] = scene_serpentine(w, 96)
    m |= scene_frame(w, h)
    tracked = tracked_of(m, 32, 1)
    want = fill_ref.consistent_regions(tracked, 32)
    got, kept = ctx.consistent_regions(tracked[None], [32], 100)
    assert np.array_equal(got[0], want), "%d pixels differ" % int((got[0] != want).sum())
    assert int(kept[0]) == int(want.sum()) and 0 < want.sum() < m.sum()


@pytest.mark.gpu
def test_refusals_name_the_argument_and_write_nothing(ctx):
    import slowflow_amd as sfa
    L = sfa.lib()
    L.sfa_consistent_regions.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    w, h = 8, 4
    tracked, full = np.ones((1, h, w), np.int32), np.ones(1, np.int32)
    mask, kept = np.full((1, h, w), 9, np.uint8), np.full(1, -5, np.int32)
    ptr = lambda a: a.ctypes.data
    good = dict(n=1, w=w, h=h, tracked=ptr(tracked), full=ptr(full), min_size=1, mask=ptr(mask), kept=ptr(kept))
    bad = [("n", 0), ("n", -1), ("w", 0), ("h", 0), ("min_size", 0), ("tracked", None), ("full", None), ("mask", None), ("kept", None)]
    for name, value in bad:
        a = dict(good)
        a[name] = value
        rc = L.sfa_consistent_regions(ctx.h, a["n"], a["w"], a["h"], a["tracked"], a["full"], a["min_size"], a["mask"], a["kept"])
        msg = L.sfa_last_error(ctx.h).decode()
        assert rc == SFA_ERR_ARG and "sfa_consistent_regions" in msg and re.search(r"\b%s\b" % name, msg), (name, value, rc, msg)
    rc = L.sfa_consistent_regions(ctx.h, 1, 32768, 16385, ptr(tracked), ptr(full), 1, ptr(mask), ptr(kept))      # w * h = 2^29 + 2^15
    assert rc == SFA_ERR_ARG and "w * h" in L.sfa_last_error(ctx.h).decode()
    assert (mask == 9).all() and kept[0] == -5
    m, k = ctx.consistent_regions(tracked, full, 1)                                                               # (the good arguments do run)
    assert m.all() and k[0] == w * h
