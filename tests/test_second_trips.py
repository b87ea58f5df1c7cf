"""The second trip of every chunked scan and capped grid that the stage tests' shapes of about 100 x 70 never take, at the counts the workload has (DESIGN
section 3, "Second trips", lists every such loop of slowflow_amd/csrc and the test that crosses it):

  k_fill_offsets, k_ef_offsets   a block-level scan over chunks of 256 block counts with a carry: a second chunk from 65 537 samples / matches on
  k_group_keys_hist, k_group_digit_hist   grid stride under min(ceil(values / 256), max(1, 4 CU / G)) blocks per group
  k_jet_resample                 grid stride under min(ceil(total / 256), 16 CU) blocks, with the plane index i / (w h) inside the loop
  k_jet_occ_decode               k += gridDim.z under a grid of at most 65 535 planes, barriers inside the loop

Every GPU test computes the launch's block count from the device's CU count and the constants mirrored below, and asserts that its input crosses the cap
before it calls the GPU; test_the_mirrored_constants_are_the_sources reads the sources, so a change of a cap fails there instead of un-covering a loop.
Every comparison is exact (`==` or bit patterns), against the references of the stage's own tests."""
import os
import re

import numpy as np
import pytest

try:                                             # torch brings its own HIP runtime: it has to be loaded before the library opens the GPU through the system's,
    import torch                                 # as in the modules that importorskip it at their top; the CPU tests here do not need it
except ImportError:
    torch = None

import fill_ref
from jet_resample_ref import crop_rect, decode_occlusion_scaled, resample_flow
from test_epic_batch import filter_scene, host_run, lib_batch, same, tool, workdir  # noqa: F401  (tool, workdir: fixtures)
from test_fill_matches import bits
from test_fill_matches import scene as fill_scene  # noqa: F401  (a fixture: the 70 x 45 scene)
from test_jet_resample import padded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slowflow_amd", "csrc")

# ---- the mirrors of slowflow_amd/csrc -----------------------------------------------------------------------------------------------------------------
K_EF_THREADS = K_FILL_THREADS = K_Q_THREADS = K_JET_THREADS = 256
Q_BLOCKS_PER_CU, JET_BLOCKS_PER_CU, OCC_MAX_PLANES_IN_GRID = 4, 16, 65535


def scan_chunks(count, threads):
    """(blocks of `threads` entries, chunks of `threads` block counts): what k_fill_offsets / k_ef_offsets loop over"""
    nblocks = -(-count // threads)
    return nblocks, -(-nblocks // threads)


def quantile_blocks(cu, G, key_stride):
    """blocks per group of sfa_flow_magnitude_quantiles_device"""
    return min(-(-key_stride // K_Q_THREADS), max(1, cu * Q_BLOCKS_PER_CU // G))


def jet_blocks(cu, total):
    return min(-(-total // K_JET_THREADS), cu * JET_BLOCKS_PER_CU)


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def body_of(text, head):
    """the definition that starts with `head` up to its closing brace in column 0"""
    m = re.search(re.escape(head) + r".*?\n}\n", text, flags=re.S)
    assert m, head
    return m.group(0)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_mirrored_constants_are_the_sources():
    ef, fill, q, jet = source("epic_filter.hip"), source("fill.hip"), source("quantile.hip"), source("jet_resample.hip")
    for text, name, want in ((ef, "kEfThreads", K_EF_THREADS), (fill, "kFillThreads", K_FILL_THREADS), (q, "kQThreads", K_Q_THREADS), (jet, "kJetThreads", K_JET_THREADS)):
        found = re.findall(r"constexpr int [^;]*\b%s = (\d+)[,;]" % name, text)
        assert found == [str(want)], (name, found)
    # the chunked scans: one chunk per trip, the carry added once per chunk
    for text, kernel, threads in ((ef, "k_ef_offsets", "kEfThreads"), (fill, "k_fill_offsets", "kFillThreads")):
        body = body_of(text, "__global__ void __launch_bounds__(%s) %s(" % (threads, kernel))
        assert len(re.findall(r"for \(int b0 = 0; b0 < nblocks; b0 \+= %s\)" % threads, body)) == 1, kernel
        assert len(re.findall(r"carry \+= part\[%s - 1\];" % threads, body)) == 1, kernel
    assert "const int nblocks = (im.count + kEfThreads - 1) / kEfThreads;" in ef
    assert "size_t fill_matches_blocks(int nx, int ny) { return ((size_t)nx * ny + kFillThreads - 1) / kFillThreads; }" in fill
    # the grouped quantile: blocks per group, and the strides of the two kernels it launches
    grouped = body_of(q, "int sfa_flow_magnitude_quantiles_device(")
    assert re.search(r"const int blocks = \(int\)std::min<size_t>\(\(key_stride \+ kQThreads - 1\) / kQThreads, \(size_t\)std::max\(1, ctx->cu_count \* %d / G\)\);" % Q_BLOCKS_PER_CU,
                     grouped)
    assert "k_group_keys_hist, dim3(blocks, G), dim3(kQThreads)" in grouped and "k_group_digit_hist, dim3(blocks, G), dim3(kQThreads)" in grouped
    stride = "i < N; i += (size_t)gridDim.x * kQThreads)"
    assert stride in body_of(q, "__global__ void __launch_bounds__(kQThreads) k_group_keys_hist(") and stride in body_of(q, "__device__ __forceinline__ void digit_hist(")
    # the jet kernels
    launch = body_of(jet, "int launch_jet_resample(")
    assert re.search(r"std::min<size_t>\(\(total \+ kJetThreads - 1\) / kJetThreads, \(size_t\)ctx->cu_count \* %d\)" % JET_BLOCKS_PER_CU, launch)
    assert "dim3(blocks), dim3(kJetThreads)" in launch
    assert "i < total; i += (size_t)gridDim.x * kJetThreads)" in body_of(jet, "__global__ void __launch_bounds__(kJetThreads) k_jet_resample(")
    assert re.search(r"\(unsigned\)std::min<size_t>\(np, %d\)\);" % OCC_MAX_PLANES_IN_GRID, body_of(jet, "int launch_jet_occ_decode("))
    assert "for (int k = blockIdx.z; k < np; k += gridDim.z)" in body_of(jet, "__global__ void __launch_bounds__(kOccTX * kOccTY) k_jet_occ_decode(")
    # the CU count is the device's
    assert "c->cu_count = prop.multiProcessorCount;" in source("api.hip")


@pytest.mark.parametrize("J", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("divisor", (1, 3))
def test_the_vectorised_matches_equal_the_match_loop(fill_scene, J, divisor):
    xs, ys = fill_scene["xs"], fill_scene["ys"]
    for i in range(3):
        au, av, mask = fill_scene["acc_u"][i, :J], fill_scene["acc_v"][i, :J], fill_scene["mask"][i]
        want, got = fill_ref.fill_matches(au, av, mask, xs, ys, divisor), fill_ref.fill_matches_vec(au, av, mask, xs, ys, divisor)
        assert len(got) == len(want) == J
        for j in range(J):
            assert got[j].dtype == np.float32 and got[j].shape == want[j].shape and np.array_equal(bits(got[j]), bits(want[j])), (i, j)
    # and on values whose sum leaves the floats, with a mask value that is not 1 (the loop tests == 1)
    au = np.array([[[1e39, -1.7e308, np.nan, np.inf, 5e-324, 3.0]]])
    mask = np.array([[1, 1, 1, 1, 1, 2]], np.uint8)
    with np.errstate(over="ignore"):
        want, got = [f(au, -au, mask, np.arange(6), [0], 3) for f in (fill_ref.fill_matches, fill_ref.fill_matches_vec)]
    assert len(want[0]) == 5 and np.array_equal(bits(got[0]), bits(want[0]))


# ---- 1. k_fill_offsets / k_fill_rows ------------------------------------------------------------------------------------------------------------------
FILL_CASES = {  # samples: (nx, ny, every other column, every other row, J, divisor, chunks of the scan)
    65536: (256, 256, True, True, 1, 1, 1),       # exactly one full chunk
    65792: (257, 256, False, True, 2, 3, 2),      # 257 blocks: one block in the second chunk
    131584: (514, 256, True, False, 1, 1, 3),     # 514 blocks: a third chunk of 2 blocks
    65537: (65537, 1, False, False, 2, 3, 2),     # one sample alone in block 256
}
FILL_MASKS = {"a": ("ones", "random", "tail"), "b": ("last", "none", "random")}


def fill_case(ns, which):
    """three maps: xs, ys, the masks through their flags per sample, the accumulated flows"""
    nx, ny, skip_x, skip_y, J, divisor, chunks = FILL_CASES[ns]
    assert nx * ny == ns
    xs = (1 + 2 * np.arange(nx) if skip_x else np.arange(nx)).astype(np.int32)
    ys = (1 + 2 * np.arange(ny) if skip_y else np.arange(ny)).astype(np.int32)
    w, h = int(xs[-1]) + 1 + skip_x, int(ys[-1]) + 1 + skip_y
    rng = np.random.default_rng(ns + ord(which))
    flags = np.zeros((3, ns), np.uint8)
    mask = (rng.random((3, h, w)) < 0.5).astype(np.uint8)            # what lies between the samples is not read
    for i, kind in enumerate(FILL_MASKS[which]):
        if kind == "ones":
            flags[i] = 1
        elif kind == "random":
            flags[i] = rng.random(ns) < 0.4
            flags[i, -1] = 1                                          # the last block writes a row behind the carry
        elif kind == "tail":
            flags[i, K_FILL_THREADS * K_FILL_THREADS:] = 1          # the first chunk sums to 0
        elif kind == "last":
            flags[i, -1] = 1
        if kind == "none":
            mask[i] = 1                                               # 1 everywhere but on the samples
        mask[i][np.ix_(ys, xs)] = flags[i].reshape(ny, nx)
    acc_u, acc_v = rng.normal(0, 9, (3, J, h, w)), rng.normal(0, 9, (3, J, h, w))
    return xs, ys, mask, flags, acc_u, acc_v, J, divisor, chunks


@pytest.mark.parametrize("ns", sorted(FILL_CASES))
def test_fill_masks_are_what_their_names_say(ns):
    """(CPU) the sample counts, the block and chunk counts of the scan and the sums of the first chunk that the GPU test relies on"""
    full = K_FILL_THREADS * K_FILL_THREADS
    for which in FILL_MASKS:
        xs, ys, mask, flags, _, _, _, _, chunks = fill_case(ns, which)
        nblocks, nchunks = scan_chunks(len(xs) * len(ys), K_FILL_THREADS)
        assert len(xs) * len(ys) == ns and nchunks == chunks and nblocks == -(-ns // 256)
        assert np.array_equal(mask[:, ys][:, :, xs].reshape(3, ns), flags)
        for i, kind in enumerate(FILL_MASKS[which]):
            total, first = int(flags[i].sum()), int(flags[i, :full].sum())
            if kind == "ones":
                assert total == ns and first == full                 # every block count is 256: the carry is 65 536 and more
            elif kind == "tail":
                assert first == 0 and total == ns - full
            elif kind == "last":
                assert total == 1 and flags[i, -1] == 1
            elif kind == "none":
                assert total == 0 and mask[i].sum() == mask[i].size - ns
            else:
                assert 0.35 * ns < total < 0.45 * ns and (ns == full or first < total)
    assert {k: scan_chunks(k, 256) for k in FILL_CASES} == {65536: (256, 1), 65792: (257, 2), 131584: (514, 3), 65537: (257, 2)}


@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(FILL_MASKS))
@pytest.mark.parametrize("ns", sorted(FILL_CASES))
def test_fill_matches_across_the_scans_chunks(ctx, ns, which):
    xs, ys, mask, flags, acc_u, acc_v, J, divisor, chunks = fill_case(ns, which)
    nblocks, nchunks = scan_chunks(len(xs) * len(ys), K_FILL_THREADS)
    assert nchunks == chunks and (nblocks > K_FILL_THREADS if chunks > 1 else nblocks == K_FILL_THREADS)      # the second trip is taken (or the first is full)
    got, count = ctx.fill_matches(acc_u, acc_v, mask, xs, ys, divisor)
    assert got.shape == (3, J, ns, 4) and got.dtype == np.float32
    for i in range(3):
        want = fill_ref.fill_matches_vec(acc_u[i], acc_v[i], mask[i], xs, ys, divisor)
        assert int(count[i]) == len(want[0]) == int(flags[i].sum()), (i, FILL_MASKS[which][i], count[i])
        for j in range(J):
            assert np.array_equal(bits(got[i, j, :count[i]]), bits(want[j])), (i, j, FILL_MASKS[which][i])
            assert np.isnan(got[i, j, count[i]:]).all(), (i, j)                                  # nothing is written behind the count


# ---- 2. k_ef_block_count / k_ef_offsets / k_ef_scatter ------------------------------------------------------------------------------------------------
EPIC_COUNTS = (65535, 65536, 65537, 131073, 300)
EPIC_CHUNKS = (1, 1, 2, 3, 1)
CORNER_W, CORNER_H, REACH = 40, 30, 12           # filter_scene's flat corner; the saliency's three filters reach 4 + 1 + 4 pixels, 12 leaves room
FILLER_TARGET = (100.0, 70.0)
WORKSPACE = 1 << 40                              # the default search plans `done` = nm x nm floats per image before a filter has run: 69 GB for 131 073


def textured_ranges(nm):
    """the index ranges of a long list that hold the scene's textured matches"""
    r = {"the first block": range(0, K_EF_THREADS), "across the chunk boundary": range(65500, min(65581, nm)),
         "the last block": range((nm - 1) // K_EF_THREADS * K_EF_THREADS, nm)}
    if nm > 2 * K_EF_THREADS * K_EF_THREADS:
        r["the third chunk"] = range(2 * K_EF_THREADS * K_EF_THREADS, nm)
    return r


_long = []


def long_scenes():
    """five images of 131 x 77: filter_scene's image with lists of 65 535, 65 536, 65 537 and 131 073 matches -- fillers inside the flat corner, the scene's
    textured matches on textured_ranges -- and the scene's first 300 matches"""
    if _long:
        return _long
    rgb, edges, m, w, h = filter_scene()
    rng = np.random.default_rng(131)
    for nm in EPIC_COUNTS:
        if nm == 300:
            _long.append((rgb, edges, m[:300].copy(), w, h))
            continue
        lst = np.empty((nm, 4), np.float32)
        lst[:, 0] = rng.uniform(1.0, CORNER_W - REACH - 1, nm)        # (int)(y1 * stride + x1) is column (int)x1 of row y1: y1 is whole
        lst[:, 1] = rng.integers(1, CORNER_H - REACH - 1, nm)
        lst[:, 2:] = FILLER_TARGET
        idx = textured_indices(nm)
        lst[idx] = m[:len(idx)]                                       # scene()'s own 600: random positions, every target another
        lst.setflags(write=False)
        _long.append((rgb, edges, lst, w, h))
    return _long


def textured_indices(nm):
    return np.array(sorted(set().union(*textured_ranges(nm).values())))


def clamped(m, w, h):
    """epic.cpp:15-28"""
    m = m.copy()
    m[:, 0::2] = np.clip(m[:, 0::2], 0, w - 1); m[:, 1::2] = np.clip(m[:, 1::2], 0, h - 1)
    return m


def target_key(row):
    return bits(row[2:4]).tobytes()


def test_long_lists_are_what_the_filter_test_needs():
    """(CPU) counts, blocks and chunks; the fillers sample flat pixels away from the corner's border by more than the filters' reach; the textured rows lie
    on the ranges and a clamped target names its row"""
    scenes = long_scenes()
    assert [len(s[2]) for s in scenes] == list(EPIC_COUNTS)
    assert [scan_chunks(nm, K_EF_THREADS) for nm in EPIC_COUNTS] == [(256, 1), (256, 1), (257, 2), (513, 3), (2, 1)]
    assert [scan_chunks(nm, K_EF_THREADS)[1] for nm in EPIC_COUNTS] == list(EPIC_CHUNKS)
    for rgb, edges, m, w, h in scenes[:4]:
        nm, st = len(m), ((w + 3) // 4) * 4
        assert (rgb[:, :CORNER_H, :CORNER_W] == 128).all() and rgb[:, :CORNER_H + 1, :CORNER_W + 1].std() > 0
        r = textured_ranges(nm)
        assert r["across the chunk boundary"][0] // 256 == 255 and (nm <= 65536 or r["across the chunk boundary"][-1] // 256 == 256)
        assert len(r["the last block"]) == (nm - 1) % 256 + 1 and (nm != 131073 or list(r["the third chunk"]) == [131072])
        idx = textured_indices(nm)
        assert 250 < len(idx) <= 600
        filler = np.ones(nm, bool)
        filler[idx] = False
        f = m[filler]
        index = (f[:, 1] * np.float32(st) + f[:, 0]).astype(np.float32).astype(np.int64)    # the host's float index
        assert (index // st < CORNER_H - REACH).all() and (index % st < CORNER_W - REACH).all() and (index >= 0).all()
        assert np.array_equal(index // st, f[:, 1].astype(np.int64)) and (index % st - f[:, 0].astype(np.int64) <= 1).all()    # (the fp32 sum may round x1 up)
        assert (f[:, 2:] == np.float32(FILLER_TARGET)).all()
        c = clamped(m[idx], w, h)
        keys = {target_key(row) for row in c}
        assert len(keys) == len(idx) and target_key(np.array((0, 0) + FILLER_TARGET, np.float32)) not in keys
        assert any(not (set(range(b * 256, min(nm, b * 256 + 256))) & set(idx.tolist())) for b in range(-(-nm // 256)))


def traced(kept, m, w, h):
    """the input index of every kept row, through its target; a filler has none"""
    idx = textured_indices(len(m))
    where = {target_key(row): int(i) for row, i in zip(clamped(m[idx], w, h), idx)}
    out = []
    for row in kept:
        assert target_key(row) in where, "a filler match survived the host's saliency filter: %r" % (row,)
        out.append(where[target_key(row)])
    return out


@pytest.mark.gpu
def test_saliency_compaction_of_lists_longer_than_one_chunk(ctx, tool, workdir):
    scenes = long_scenes()
    w, h = scenes[0][3:]
    assert max(scan_chunks(len(s[2]), K_EF_THREADS)[1] for s in scenes) == 3 and [scan_chunks(len(s[2]), K_EF_THREADS)[1] for s in scenes] == list(EPIC_CHUNKS)
    host, _ = host_run(tool, workdir, "long", scenes, "NW", 0.045, 0, 30)
    # the reference alone: a few hundred survivors, some from every range, whole blocks of fillers gone, the order kept
    for s, o in zip(scenes[:4], host):
        nm = len(s[2])
        assert 100 <= len(o["keep1"]) <= 2000, (nm, len(o["keep1"]))
        src = traced(o["keep1"], s[2], w, h)
        assert src == sorted(src) and len(set(src)) == len(src), nm
        for name, r in textured_ranges(nm).items():
            assert any(i in r for i in src), (nm, name)
        assert len({i // K_EF_THREADS for i in src}) < scan_chunks(nm, K_EF_THREADS)[0], nm
        assert same(o["keep2"], o["keep1"]) and o["rc"] == 0
    fx, fy, rc, counts, kept = lib_batch(ctx, scenes, host, "NW", 0.045, 0, 30, workspace_bytes=WORKSPACE)
    for k, (s, o) in enumerate(zip(scenes, host)):
        assert list(counts[k]) == [len(s[2]), len(o["keep1"]), len(o["keep2"])], k
        assert same(kept[k], o["keep2"]), k
        assert rc[k] == o["rc"] == o["brc"] == 0, k
        assert same(fx[k][:, :w], o["fx"][:, :w]) and same(fy[k][:, :w], o["fy"][:, :w]), k


@pytest.mark.gpu
def test_saliency_compaction_that_keeps_nothing_of_long_lists(ctx, tool, workdir):
    """every chunk sums to 0"""
    scenes = long_scenes()
    assert max(scan_chunks(len(s[2]), K_EF_THREADS)[1] for s in scenes) == 3
    host, _ = host_run(tool, workdir, "long", scenes, "NW", 1e9, 0, 30)
    fx, fy, rc, counts, kept = lib_batch(ctx, scenes, host, "NW", 1e9, 0, 30, workspace_bytes=WORKSPACE)
    for k, (s, o) in enumerate(zip(scenes, host)):
        assert len(o["keep1"]) == len(o["keep2"]) == 0 and o["rc"] == o["brc"] == 1, k
        assert rc[k] == 1 and list(counts[k]) == [len(s[2]), 0, 0] and len(kept[k]) == 0, k
        assert np.isnan(fx[k]).all() and np.isnan(fy[k]).all(), k                                # the planes are untouched


# ---- 3. the grouped quantile ---------------------------------------------------------------------------------------------------------------------------
def cu_count():
    if torch is None:
        pytest.skip("torch is not installed")
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def many_groups():
    """G = 64 groups of n fields of 37 x 19 with more values than one trip of the group's blocks reads (n = 6 at 256 CUs), magnitudes 1e-3, 1, 1e3 by group"""
    from test_quantile_device import H, W, noise
    G = 64
    per_trip = K_Q_THREADS * max(1, cu_count() * Q_BLOCKS_PER_CU // G)
    n = per_trip // (W * H) + 1
    flow = noise(11, G, n)
    for g in range(G):
        flow[g] *= np.float32((1e-3, 1.0, 1e3)[g % 3])
    flow.setflags(write=False)
    return flow, per_trip


@pytest.mark.gpu
@pytest.mark.parametrize("q", [0.99, 0.5, 1.0])
def test_grouped_quantile_with_more_values_than_a_trip(ctx, many_groups, q):
    from test_quantile_device import check, expected, run
    flow, per_trip = many_groups
    G, n = flow.shape[:2]
    N = flow[0, :, 0].size
    blocks = quantile_blocks(cu_count(), G, N)
    assert blocks * K_Q_THREADS == per_trip < N and N - flow[0, 0, 0].size <= per_trip         # a second trip, and no field more than it takes
    want = expected(ctx, flow, 1.0, q)
    assert len({w[0] for w in want}) == G                                                      # (no two groups share a quantile)
    assert want[0][1] < 1e-2 and 1 < want[1][1] < 10 and want[2][1] > 1e3                      # the chosen bins differ between groups
    check(run(ctx, torch.tensor(flow, device="cuda"), q), want)


@pytest.mark.gpu
def test_grouped_quantile_with_groups_under_and_over_a_trip(ctx, many_groups):
    from test_quantile_device import check, expected, run
    base, per_trip = many_groups
    G, n = base.shape[:2]
    per = base[0, 0, 0].size
    counts = [(1, 2, n, n - 1 if (n - 1) * per > per_trip else n)[g % 4] for g in range(G)]
    flow = base.copy()
    for g in range(G):
        flow[g, counts[g]:] = np.inf                                                           # the unused fields
    blocks = quantile_blocks(cu_count(), G, n * per)
    assert blocks * K_Q_THREADS == per_trip and 2 * per <= per_trip < n * per                  # groups of 1 and 2 fields stay under one trip, the full ones do not
    want = expected(ctx, flow, 1.0, 0.99, counts)
    assert all(np.isfinite(w[1]) for w in want)
    check(run(ctx, torch.tensor(flow, device="cuda"), 0.99, 1.0, counts), want)


@pytest.mark.gpu
def test_three_strided_groups_with_more_values_than_a_trip(ctx):
    from test_quantile_device import check, expected, noise, run
    G, n, w = 3, 3, 173
    per_trip = K_Q_THREADS * max(1, cu_count() * Q_BLOCKS_PER_CU // G)
    h = per_trip // (n * w) + 1                                                                # 169 rows at 256 CUs: 87 711 values against 87 296
    flow = noise(12, G, n, h, w)
    N = n * h * w
    assert quantile_blocks(cu_count(), G, N) * K_Q_THREADS == per_trip < N
    want = expected(ctx, flow, 0.5, 0.99)
    last = torch.tensor(flow, device="cuda").permute(0, 1, 3, 4, 2).contiguous()                    # [G,n,h,w,2] in memory
    view = last.permute(0, 1, 4, 2, 3)
    assert view.stride()[-1] == 2 and not view.is_contiguous()
    check(run(ctx, view, 0.99, 0.5), want)


# ---- 4. k_jet_resample ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("crop", [None, ((8, 6), (7, 5))])
def test_flow_resample_of_more_elements_than_the_grid_has_threads(ctx, crop):
    """a 16 x 12 source at rescale 4.0, whole (64 x 48) and cropped (28 x 20): eight random planes in turn, and so many of them that the grid of
    16 CU blocks comes round again; ten planes and more lie in the second trip (at 256 CUs it starts inside plane 341 and plane 1872)"""
    import slowflow_amd as sfa
    sw, sh = 16, 12
    rect = crop_rect(*crop) if crop else None
    stride = sfa.stride_of(sw) + 4
    src = sfa.jet_source(sw, sh, stride, crop=rect, rescale=4.0)
    w, h = src.target()
    assert (w, h) == ((28, 20) if crop else (64, 48))
    threads = cu_count() * JET_BLOCKS_PER_CU * K_JET_THREADS
    n = 8 * -(-(threads // (w * h) + 11) // 8)                                                  # 352 whole planes at 256 CUs
    assert jet_blocks(cu_count(), n * w * h) * K_JET_THREADS == threads and n * w * h >= threads + 10 * w * h
    rng = np.random.default_rng(16 + bool(crop))
    u8, v8 = ((rng.standard_normal((8, sh, sw)) * 3).astype(np.float32) for _ in range(2))
    turn = np.arange(n) % 8
    gu, gv = ctx.jet_flow_resample(padded(u8[turn], stride, np.nan, np.float32), padded(v8[turn], stride, np.nan, np.float32), src)   # NaN in the padding: never read
    ref = [resample_flow(u8[k], v8[k], src.rescale, rect) for k in range(8)]
    assert ref[0][0].shape == (h, w) and gu.shape == (n, h, w)
    ru, rv = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    bad = [k for k in range(n) if not (np.array_equal(gu[k], ru[k % 8]) and np.array_equal(gv[k], rv[k % 8]))]
    assert not bad, "planes %s (the second trip starts in plane %d)" % (bad[:8], threads // (w * h))


# ---- 5. k_jet_occ_decode -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_occlusion_decode_of_more_planes_than_the_grid_is_deep(ctx):
    import slowflow_amd as sfa
    sw, sh, n = 5, 4, OCC_MAX_PLANES_IN_GRID + 2
    assert n == 65537 and min(n, OCC_MAX_PLANES_IN_GRID) < n                                     # planes 65 535 and 65 536 are the second trip of blocks z = 0 and 1
    rng = np.random.default_rng(5)
    img = rng.choice(np.array([0, 127, 255], np.uint8), (8, sh, sw))
    stride = sfa.stride_of(sw) + 4
    src = sfa.jet_source(sw, sh, stride, rescale=4.0)
    ref = np.stack([decode_occlusion_scaled(img[k], src.rescale) for k in range(8)])
    assert len({r.tobytes() for r in ref}) == 8
    turn = np.arange(n) % 8
    got = ctx.jet_occlusion_decode(padded(img[turn], stride, 77, np.uint8), src)
    assert got.shape == (n,) + ref.shape[1:]
    bad = np.flatnonzero((got != ref[turn]).any(axis=(1, 2)))
    assert bad.size == 0, "planes %s differ (planes 65535 and 65536 are the second trip: %s)" % (bad[:8].tolist(), [k in bad for k in (65535, 65536)])
