"""Value-range parity of the EpicFlow chain (epic_nn.hip, epic_filter.hip, epic_fit.hip, epic_batch.hip, k_epic_weights) against slowflow_amd/host/epic.cpp: edge
costs over the whole domain +0 ... +Inf -- a magnitude ladder from subnormal to 2^60, +0, subnormals, FLT_MIN, FLT_MAX, +Inf, sums beyond 0x7F7F7F7F, planes of
zeros and of -0.0 -- where the rest of the suite feeds costs of 0.02 ... 2.  tests/value_ranges.py builds the inputs.  Before any GPU comparison the CPU tests
run the host function on the same inputs and prove which classes they reach: the counts beside the assertions are the host tool's on these seeds.  Every
comparison is on bit patterns; only where the host itself gives a NaN is NaN-ness compared instead (test_epic_fit.same_bits).  Nothing here hands a NaN or
a negative cost to a kernel: those are refused at the entry points, and the refusals are tested."""
import os

import numpy as np
import pytest

import value_ranges as vr
from test_epic import scene, stride_of
from test_epic_batch import host_run, lib_batch, workdir  # noqa: F401  (workdir: a fixture)
from test_epic_batch import tool as batch_tool  # noqa: F401  (a fixture: the host side of epic_batch)
from test_epic_fit import host_fit, kernel_weights, same_bits
from test_epic_fit import tool as fit_tool  # noqa: F401  (a fixture: the host side of the fit)
from test_epic_nn import host_nearest_seeds, same, tool  # noqa: F401  (tool: the fixture that builds tests/host/epic_nn_tool.cpp)

SEED = 5
BIG, MID, TINY = vr.EPIC_SIZES
PLANES = {"ladder": vr.cost_ladder, "sprinkled": vr.cost_ladder_sprinkled, "zeros": vr.cost_zeros, "minus_zeros": vr.cost_minus_zeros,
          "all_zero": lambda w, h, seed: np.zeros((h, w), np.float32), "plain": vr.cost_plain}
HUGE = np.array([0x7F7F7F7F], np.uint32).view(np.float32)[0]


def plane_and_seeds(name, w, h, ns):
    cost = PLANES[name](w, h, SEED)
    return cost, vr.epic_seeds(w, h, ns, SEED, cost if name == "sprinkled" else None)


@pytest.fixture(scope="module")
def hostnn(tool, tmp_path_factory):
    """the host's epic_nearest_seeds on a named plane: (cost, seeds, (labels, index, dist)), computed once per (plane, size, nn) and never written to"""
    d = str(tmp_path_factory.mktemp("epic_value_ranges"))
    done = {}

    def get(name, w, h, ns, nn):
        key = (name, w, h, ns, nn)
        if key not in done:
            cost, seeds = plane_and_seeds(name, w, h, ns)
            done[key] = (cost, seeds, host_nearest_seeds(tool, d, cost, seeds, nn))
        return done[key]
    return get


# ---- CPU: 1. what the planes hold and what the host reaches on them -------------------------------------------------------------------------------------
def test_the_planes_hold_their_values():
    for w, h, ns in vr.EPIC_SIZES:
        for name in PLANES:
            cost, seeds = plane_and_seeds(name, w, h, ns)
            assert cost.dtype == np.float32 and cost.shape == (h, w) and not np.isnan(cost).any() and (cost >= 0).all(), name      # the domain (-0.0 >= 0)
            assert np.signbit(cost).any() == (name == "minus_zeros"), name
            assert seeds.shape == (ns, 2) and (seeds >= 0).all() and (seeds[:, 0] < w).all() and (seeds[:, 1] < h).all()
        ladder, sprinkled = PLANES["ladder"](w, h, SEED), PLANES["sprinkled"](w, h, SEED)
        assert vr.is_subnormal(ladder).any() and (ladder > 0).all() and ladder.max() < 2.0 ** 60
        if w >= 64:
            for e in vr.EPIC_EXPS:                                     # every band in every eight rows
                assert all(((ladder[y:y + 8] >= 0.05 * 2.0 ** e) & (ladder[y:y + 8] < 2.0 ** e)).any() for y in range(0, h, 8)), e
            top = (sprinkled >= 0.05 * 2.0 ** vr.EPIC_TOP) & (sprinkled < 2.0 ** vr.EPIC_TOP)
            assert top.sum() > 100                                     # 259: the band whose sums pass 0x7F7F7F7F
            assert 0.04 < (sprinkled.view(np.uint32)[..., None] == vr.EPIC_SPECIALS.view(np.uint32)).any(-1).mean() < 0.08           # one pixel in sixteen
        seeds = plane_and_seeds("sprinkled", w, h, ns)[1]
        on = sprinkled[seeds[:, 1], seeds[:, 0]].view(np.uint32)
        for v in vr.EPIC_SPECIALS[:max(1, ns // 2)]:                  # the plane holds every special value, and a seed stands on one pixel of each
            assert (sprinkled.view(np.uint32) == v.view(np.uint32)).any() and (on == v.view(np.uint32)).any(), v
        zeros, minus = PLANES["zeros"](w, h, SEED), PLANES["minus_zeros"](w, h, SEED)
        assert np.array_equal(zeros, minus) and np.array_equal(zeros == 0, np.signbit(minus)) and not np.signbit(zeros).any()
        assert (zeros == 0).any() and (w * h < 100 or 0.25 < (zeros == 0).mean() < 0.42)       # a third of the pixels


# the host tool's counts on these inputs, nn = min(25, ns): (zero, subnormal, +Inf distances, absent entries, tied neighbouring entries, unlabelled pixels of
# finite cost, unlabelled pixels).  The assertions below ask for the class, with room below the measured count
MEASURED = {
    (136, 24, "ladder"): (0, 47, 0, 0, 3885, 0, 0), (136, 24, "sprinkled"): (3, 48, 196, 260, 4239, 55, 85), (136, 24, "zeros"): (149, 0, 0, 0, 1049, 0, 0),
    (136, 24, "minus_zeros"): (149, 0, 0, 0, 1049, 0, 0), (136, 24, "all_zero"): (7500, 0, 0, 0, 7200, 0, 0),
    (12, 10, "ladder"): (0, 1, 0, 364, 80, 0, 0), (12, 10, "sprinkled"): (1, 3, 1, 384, 147, 1, 1), (12, 10, "zeros"): (13, 0, 0, 208, 27, 0, 0),
    (12, 10, "minus_zeros"): (13, 0, 0, 208, 27, 0, 0), (12, 10, "all_zero"): (546, 0, 0, 104, 520, 0, 0),
}


@pytest.mark.parametrize("w,h,ns", [BIG, MID])
def test_the_host_reaches_every_class(hostnn, w, h, ns):
    nn = min(25, ns)
    got = {}
    for name in ("ladder", "sprinkled", "zeros", "minus_zeros", "all_zero"):
        cost, seeds, (labels, index, dist) = hostnn(name, w, h, ns, nn)
        c = vr.list_classes(index, dist)
        got[name] = c
        c["unlabelled_finite"], c["unlabelled"] = int(((labels < 0) & np.isfinite(cost)).sum()), int((labels < 0).sum())
        print(w, h, name, c, "measured", MEASURED[w, h, name])
        assert (index < ns).all() and (dist[index < 0] >= HUGE).all(), name    # an absent entry is -1 / the seed's own distance + 0x7F7F7F7F
        assert not np.isnan(dist).any() and not np.signbit(dist).any(), name
        if name != "sprinkled":
            assert c["unlabelled"] == 0, name                           # fully labelled: what the chain tests may use (the host's LA apply loop reads aff[label * 6])
    big = (w, h) == BIG[:2]
    assert got["ladder"]["subnormal"] >= (30 if big else 1)             # 47 / 1
    assert got["ladder"]["ties"] >= (3000 if big else 50)               # 3885 of 7500 / 80 of 650: small costs are absorbed into large sums
    s = got["sprinkled"]
    assert s["zero"] >= 1 and s["subnormal"] >= (30 if big else 1) and s["inf"] >= 1 and s["absent"] >= 200 and s["ties"] >= (3000 if big else 50)    # 3, 48, 196, 260, 4239 / 1, 3, 1, 384, 147
    if big:
        assert s["inf"] >= 100 and s["unlabelled_finite"] >= 30         # 196; 55: finite costs behind +Inf, or reached only by sums of 0x7F7F7F7F and more
    assert got["zeros"]["zero"] >= (100 if big else 8) and got["zeros"]["ties"] >= (500 if big else 15)     # 149, 1049 / 13, 27
    a = got["all_zero"]
    assert a["zero"] + a["absent"] == ns * nn and a["zero"] >= (7500 if big else 500) and a["ties"] >= (7200 if big else 500)    # only the heap's order decides


@pytest.mark.parametrize("w,h,ns", vr.EPIC_SIZES)
def test_the_host_takes_minus_zero_for_zero(hostnn, w, h, ns):
    """the expected output on -0.0 is well defined: the bits of the same plane with +0.0"""
    for nn in (1, min(25, ns), ns + 5):
        assert same(hostnn("minus_zeros", w, h, ns, nn)[2], hostnn("zeros", w, h, ns, nn)[2]), nn


# ---- GPU: 2. nearest seeds ---------------------------------------------------------------------------------------------------------------------------------
MODES = ("default", "dense", "sparse")


@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def compact():
    """a context of its own in compact mode"""
    import slowflow_amd as sfa
    c = sfa.Context(0)
    c.set_epic_search("compact")
    yield c
    c.close()


def in_mode(mode, ctx, compact, switches):
    if mode == "default":
        return ctx
    switches.set("SFA_EPIC_NN_SET", mode)
    return compact


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("w,h,ns", vr.EPIC_SIZES)
@pytest.mark.parametrize("name", ["ladder", "sprinkled", "zeros", "all_zero", "minus_zeros"])
def test_nearest_seeds_equal_the_host(ctx, compact, switches, hostnn, name, w, h, ns, mode):
    """labels, indices and the bits of the distances, with 1, 25 and ns + 5 neighbours.  minus_zeros: a border between two seeds' pixels of cost -0.0 has the
    length -0.0 = 0x80000000, which k_epic_insert's atomicMin on the bits ranked above every positive length until border_pairs made it +0.0"""
    c = in_mode(mode, ctx, compact, switches)
    for nn in (1, 25, ns + 5):
        cost, seeds, want = hostnn(name, w, h, ns, nn)
        labels, index, dist = c.epic_nearest_seeds([cost], [seeds], nn)
        differ = int((index[0] != want[1]).sum() + (dist[0].view(np.uint32) != want[2].view(np.uint32)).sum())
        assert same((labels[0], index[0], dist[0]), want), (nn, "labels differ at %d pixels, the lists at %d entries of %d" % ((labels[0] != want[0]).sum(), differ, 2 * index[0].size))
        if mode != "default":
            info = c.epic_nn_search_info()
            assert (info["dense"], info["sparse"]) == ((1, 0) if mode == "dense" else (0, 1)), (mode, info)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_batch_of_three_kinds_equals_each_alone(ctx, compact, switches, hostnn, mode):
    """an ordinary plane, the sprinkled ladder and the all-zero plane in one call: no image's +Inf, 0x7F7F7F7F sums or ties reach its neighbours"""
    c = in_mode(mode, ctx, compact, switches)
    w, h, ns = BIG
    each = [hostnn(name, w, h, ns, 25) for name in ("plain", "sprinkled", "all_zero")]
    labels, index, dist = c.epic_nearest_seeds([e[0] for e in each], [e[1] for e in each], 25)
    for k, (cost, seeds, want) in enumerate(each):
        assert same((labels[k], index[k], dist[k]), want), k
        alone = c.epic_nearest_seeds([cost], [seeds], 25)
        assert same((labels[k], index[k], dist[k]), (alone[0][0], alone[1][0], alone[2][0])), k


# ---- 3. the whole chain ---------------------------------------------------------------------------------------------------------------------------------------
CHAIN_PLANES = ("ladder", "zeros", "minus_zeros")                       # fully labelled (test_the_host_reaches_every_class); all their costs are finite, so every
CHAIN_SIZES = (BIG[:2], MID[:2])                                        # pixel is reached from any seed: no label of -1 for the host's LA apply loop


def chain_scene(name, w, h, flat_corner=False):
    """test_epic.scene's image and about 300 matches, the plane `name` for its edges, and vr.epic_edge_matches at the ends of the clamp.  flat_corner: a
    textureless corner, as in test_epic_batch's saliency scene: the matches in it do not pass the saliency filter"""
    rgb, _, m = scene(w, h, SEED, n_matches=300)
    if flat_corner:
        rgb[:, :h // 2, :40] = 128.0
    return rgb, PLANES[name](w, h, SEED), np.concatenate([m, vr.epic_edge_matches(w, h)]).astype(np.float32), w, h


def clamped(m, w, h):
    """epic.cpp:15-28 and the seeds of its integer parts"""
    m = np.minimum(m, np.array([w - 1, h - 1, w - 1, h - 1], np.float32))
    m = np.where(m > 0, m, np.float32(0))                              # std::max(0.f, x): +0 for -0.0
    return m, np.stack([m[:, 0].astype(np.int32), m[:, 1].astype(np.int32)], 1)


def test_the_edge_matches_meet_the_clamp():
    for w, h in CHAIN_SIZES:
        e = vr.epic_edge_matches(w, h)
        assert np.isfinite(e).all() and np.signbit(e[e == 0]).any() and vr.is_subnormal(e).any() and (np.abs(e) == vr.FLT_MAX).any()
        m, seeds = clamped(e, w, h)
        assert not np.signbit(m).any() and (m[:, 0::2] <= w - 1).all() and (m[:, 1::2] <= h - 1).all()
        assert (e[:, 0] > w - 1).any() and (e[:, 1] > h - 1).any() and (seeds[:, 0] == w - 1).any() and (seeds[:, 1] == h - 1).any()
        assert ((m[:, 0] < w - 1) & (seeds[:, 0] == w - 2)).any()     # the float before w - 1: another pixel than w - 1


@pytest.mark.parametrize("w,h", CHAIN_SIZES)
def test_the_chains_weights_reach_both_ends(tool, tmp_path, w, h):
    """the lists of the survivors without filters (every clamped match) on the chain's planes: expf(-0.8 d) is exactly 1 for a zero or subnormal distance
    (|0.8 d| < 2^-25) and exactly 0 from d = 2^14 on (0.8 d > 104), where the weight is 1e-08f.  And every pixel carries a label"""
    for name in CHAIN_PLANES:
        _, cost, m, _, _ = chain_scene(name, w, h)
        _, seeds = clamped(m, w, h)
        labels, index, dist = host_nearest_seeds(tool, str(tmp_path), cost, seeds, 30)
        assert (labels >= 0).all(), name
        d = dist[index >= 0]
        one, floor = int(((d == 0) | vr.is_subnormal(d)).sum()), int((d >= 2.0 ** 14).sum())
        print(w, h, name, "weights of exactly 1:", one, "of exactly 1e-08f:", floor, "of", d.size)
        assert one >= 10 and np.isfinite(d).all(), name                # 136 x 24: 52 (ladder), 170 (zeros and minus_zeros); 12 x 10: 157, 270
        if name == "ladder":
            assert floor >= 1000                                      # 136 x 24: 3050 of 9330; 12 x 10: 4484 of 9156


GRID = [(method, pref_nn, 100 if pref_nn else 30) for method in ("LA", "NW") for pref_nn in (25, 0)]


def check_chain(ctx, batch_tool, workdir, key, scenes, method, sal, pref_nn, nn):  # noqa: F811
    host, _ = host_run(batch_tool, workdir, key, scenes, method, sal, pref_nn, nn, euc=0.0)
    for w, h in sorted({s[3:] for s in scenes}):
        group = [k for k, s in enumerate(scenes) if s[3:] == (w, h)]
        fx, fy, rc, counts, kept = lib_batch(ctx, [scenes[k] for k in group], [host[k] for k in group], method, sal, pref_nn, nn, euc=0.0)
        for j, k in enumerate(group):
            assert rc[j] == 0 and host[k]["rc"] == 0 and host[k]["brc"] == 0, (k, rc[j], host[k]["rc"], host[k]["brc"])
            assert list(counts[j]) == [len(scenes[k][2]), len(host[k]["keep1"]), len(host[k]["keep2"])] and counts[j][2] > 100, (k, counts[j])
            assert same_bits(kept[j], host[k]["keep2"]), k
            assert same_bits(fx[j][:, :w], host[k]["fx"][:, :w], nan_ok=True) and same_bits(fy[j][:, :w], host[k]["fy"][:, :w], nan_ok=True), k
            assert same_bits(host[k]["bfx"], host[k]["fx"], nan_ok=True) and same_bits(host[k]["bfy"], host[k]["fy"], nan_ok=True), k
            assert len(np.unique(fx[j][:, :w])) > 20, k
    return host


@pytest.mark.gpu
@pytest.mark.parametrize("method,pref_nn,nn", GRID)
def test_epic_batch_equals_epic_over_the_value_range(ctx, batch_tool, workdir, method, pref_nn, nn):  # noqa: F811
    """ladder, zeros and minus_zeros at both sizes, euc = 0 (so that -0.0 and the small bands reach the search), no saliency filter: epic()'s fields bit for
    bit, the survivors too; the three images of a size in one call"""
    scenes = [chain_scene(name, w, h) for w, h in CHAIN_SIZES for name in CHAIN_PLANES]
    host = check_chain(ctx, batch_tool, workdir, "value_ranges", scenes, method, 0.0, pref_nn, nn)
    for k in (1, 4):                                                   # minus_zeros gives what zeros gives
        assert same_bits(host[k + 1]["fx"], host[k]["fx"], nan_ok=True) and same_bits(host[k + 1]["fy"], host[k]["fy"], nan_ok=True), k


@pytest.mark.gpu
def test_epic_batch_with_the_saliency_filter_on_the_ladder(ctx, batch_tool, workdir):  # noqa: F811
    """an ordinary Lab image (test_epic.scene's) with saliency_th 0.045 over the ladder's costs"""
    w, h = BIG[:2]
    sc = chain_scene("ladder", w, h, flat_corner=True)
    host = check_chain(ctx, batch_tool, workdir, "value_ranges_saliency", [sc], "LA", 0.045, 25, 100)
    assert 100 < len(host[0]["keep1"]) < len(sc[2])                     # the filter is live


# ---- 4. the fit stage ---------------------------------------------------------------------------------------------------------------------------------------------
FIT_EXPS = (-140, -70, -20, 0, 14, 40)
FIT_SPECIALS = np.array([0.0, vr.SUB_MIN, vr.SUB_MAX, vr.FLT_MAX, np.inf], np.float32)


def fit_inputs(hostnn):
    """the plain plane's lists with their kernel weights times a ladder 2^-140 ... 2^40 (bands of eight seeds and four entries) and +0, subnormals, FLT_MAX and
    +Inf on one entry in sixteen"""
    w, h, ns = BIG
    _, seeds, (labels, index, dist) = hostnn("plain", w, h, ns, 25)
    rng = np.random.default_rng(SEED + 4000)
    e = np.asarray(FIT_EXPS, np.float64)[((np.arange(ns)[:, None] // 8) + (np.arange(25)[None, :] // 4)) % len(FIT_EXPS)]
    with np.errstate(under="ignore"):
        weight = (kernel_weights(dist).astype(np.float64) * np.exp2(e)).astype(np.float32)
    pos = rng.choice(weight.size, weight.size // 16, replace=False)
    weight.reshape(-1)[pos] = FIT_SPECIALS[np.arange(len(pos)) % len(FIT_SPECIALS)]
    vects = rng.uniform(-4, 4, (ns, 2)).astype(np.float32)
    return labels, seeds, vects, index, weight


@pytest.fixture(scope="module")
def fit_host(hostnn, fit_tool, tmp_path_factory):  # noqa: F811
    d = str(tmp_path_factory.mktemp("epic_value_ranges_fit"))
    args = fit_inputs(hostnn)
    return args, {method: host_fit(fit_tool, d, *args, method) for method in ("LA", "NW")}


def test_the_fits_weights_reach_their_classes(fit_host):
    (labels, seeds, vects, index, weight), want = fit_host
    assert (labels >= 0).all() and (index >= 0).all() and (weight >= 0).all()
    assert vr.is_subnormal(weight).sum() > 300 and (weight == 0).sum() > 50 and (weight == np.inf).sum() > 50 and (weight == vr.FLT_MAX).sum() > 50
    assert (weight[np.isfinite(weight)] > 2.0 ** 30).any()
    for method in ("LA", "NW"):
        model = want[method][2]
        nan, fin = int(np.isnan(model).any(1).sum()), int(np.isfinite(model).all(1).sum())
        print(method, "seeds with a NaN model:", nan, "with a finite model:", fin, "of", len(model))
        assert nan >= 50 and fin >= 100, method                        # LA 147 and 153, NW 92 and 160 of 300: an overflowing x * c or weight sum gives NaN on both sides


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["LA", "NW"])
def test_the_fit_equals_the_host_over_the_weight_range(ctx, fit_host, method):
    (labels, seeds, vects, index, weight), want = fit_host
    fx, fy, model = ctx.epic_interpolate([labels], [seeds], [vects], [index], [weight], method=method)
    w = labels.shape[1]
    hx, hy, hm = want[method]
    assert same_bits(model[0], hm, nan_ok=True), "model"
    assert same_bits(fx[0][:, :w], hx[:, :w], nan_ok=True) and same_bits(fy[0][:, :w], hy[:, :w], nan_ok=True), "flow"


# ---- 5. the domain ---------------------------------------------------------------------------------------------------------------------------------------------------
OUTSIDE = [np.nan, -np.inf, -1.0, -float(vr.SUB_MIN)]                  # (-0.0 is inside: every test on minus_zeros above)


@pytest.mark.gpu
def test_costs_outside_the_domain_are_refused(ctx):
    """a NaN or a cost below 0 in any image: SFA_ERR_ARG naming image and pixel before anything is allocated or launched (the stage times are still the last
    call's).  No such plane reaches a kernel"""
    import slowflow_amd as sfa
    w, h = MID[:2]
    cost, seeds = plane_and_seeds("plain", w, h, 26)
    m = chain_scene("plain", w, h)[2]
    p = sfa.epic_params(saliency_th=0.0, pref_nn=0, nn=5, euc=0.0)
    ctx.epic_nearest_seeds([cost], [seeds], 3)
    ctx.epic_batch(None, [cost], [m], p)
    nn_ms, batch_ms = ctx.epic_nn_stage_ms(), ctx.epic_batch_stage_ms()
    assert nn_ms["sweeps"] > 0 and batch_ms["filters"] > 0
    for k, v in enumerate(OUTSIDE):
        bad = cost.copy()
        x, y = 3 + k, 2 * k
        bad[y, x] = v
        named = r"cost\[1\]: pixel \(%d, %d\)" % (x, y)
        with pytest.raises(sfa.SlowflowError, match="sfa_epic_nearest_seeds_batch: " + named):
            ctx.epic_nearest_seeds([cost, bad], [seeds, seeds], 3)
        with pytest.raises(sfa.SlowflowError, match="sfa_epic_batch: " + named):
            ctx.epic_batch(None, [cost, bad], [m, m], p)
        assert ctx.epic_nn_stage_ms() == nn_ms and ctx.epic_batch_stage_ms() == batch_ms


@pytest.mark.gpu
def test_a_fill_jobs_edges_outside_the_domain_are_refused(ctx):
    import fill_inputs as fi
    import slowflow_amd as sfa
    case = fi.Case("value_ranges", 24, 16, 0, [(1,)])
    job = sfa.TrackJob(ctx, case.params(), case.fill(epic=sfa.epic_params(saliency_th=0.0, pref_nn=25, nn=160, coef_kernel=1.1, euc=0.0)))
    try:
        edges = PLANES["minus_zeros"](case.gw, case.gh, SEED)
        job.upload_fill(0, None, edges)                                  # -0.0 is inside the domain
        for k, v in enumerate(OUTSIDE):
            bad = edges.copy()
            bad[k, 2 * k + 1] = v
            with pytest.raises(sfa.SlowflowError, match=r"sfa_track_job_upload_fill: edges of start_jet 0: pixel \(%d, %d\)" % (2 * k + 1, k)):
                job.upload_fill(0, None, bad)
    finally:
        job.close()
