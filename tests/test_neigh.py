"""dense_tracking's alternation around the fusion (sfa_prune_hypotheses, sfa_neighbour_proposals): Philox against the published
known-answer vectors, the restatement (tests/neigh_ref.py) against its own properties on the CPU, and the GPU kernels against the restatement with ==
on every output."""
import functools

import numpy as np
import pytest

import fuse_ref as fr
import neigh_ref as nr

K16 = nr.KMAX

# Random123's kat_vectors for philox4x32 with 10 rounds: (counter, key, result)
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# synthetic lists (one segment)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def make_lists(seed, gw, gh, J=3, slots=4, holes=0.15, flows="random", pruned=False):
    """flows: "random" (every pixel's slots far from everything: proposals are accepted), "blocks" (constant over 5 x 5 blocks: a draw from the
    pixel's own block is discarded as similar), "constant" (every proposal is discarded).  holes: the share of pixels without any hypothesis.
    pruned: the present slots are a prefix of the positions (what the prune leaves, for rounds > 0)."""
    rng = np.random.default_rng(seed)
    U, V = np.zeros((K16, J, gh, gw)), np.zeros((K16, J, gh, gw))
    if flows == "random":
        U[:slots], V[:slots] = rng.normal(0, 3, (2, slots, J, gh, gw))
    elif flows == "blocks":
        by, bx = (gh + 4) // 5, (gw + 4) // 5
        b = rng.normal(0, 3, (2, slots, J, by, bx))
        U[:slots], V[:slots] = np.repeat(np.repeat(b, 5, -2), 5, -1)[..., :gh, :gw]
    else:
        U[:slots], V[:slots] = 1.25, -0.5
    energy = np.full((K16, gh, gw), np.inf)
    energy[:slots] = rng.uniform(0, 50, (slots, gh, gw)).astype(np.float32)
    if not pruned:
        energy[:slots][rng.random((slots, gh, gw)) < 0.3] = np.inf
        energy[0, ::7, ::5] = np.nan                                            # NaN is absent
    energy[:, rng.random((gh, gw)) < holes] = np.inf
    if pruned:                                                                  # a prefix of random length
        m = rng.integers(1, slots + 1, (gh, gw))
        energy[np.arange(K16).reshape(K16, 1, 1) >= m] = np.inf
    occ = rng.integers(0, 1 << (J + 1), (K16, gh, gw)).astype(np.uint64)
    origin = np.broadcast_to(np.arange(K16, dtype=np.uint8).reshape(K16, 1, 1), (K16, gh, gw)).copy()
    return dict(U=U, V=V, energy=energy, occ=occ, origin=origin)


def batch(*lists):
    return {k: np.stack([l[k] for l in lists]) for k in lists[0]}


def assert_lists_equal(got, want, s=0):
    for k in ("energy", "occ", "origin", "U", "V"):
        assert np.array_equal(got[k][s], want[k], equal_nan=False), k           # the outputs hold no NaN: an absent position is +Inf


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# CPU: Philox and the restatement's own properties
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_restatement_known_answers(ctr, key, want):
    assert tuple(nr.philox4x32_10(ctr, key)) == want


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_library_known_answers_on_the_host(ctr, key, want):
    import slowflow_amd as sfa
    assert tuple(sfa.philox4x32_10(ctr, key)) == want


def test_draw_scales_the_first_word():
    r = nr.philox4x32_10((7, 1, 3, 0), (5 + 2, 11))[0]
    assert nr.draw(5, 2, 11, 7, 1, 3, 13) == r * 13 // 2 ** 32
    assert all(0 <= nr.draw(0, 0, 0, p, 0, 0, 3) < 3 for p in range(200))
    assert {nr.draw(0, 0, 0, p, 0, 0, 3) for p in range(200)} == {0, 1, 2}


def test_distance_is_fuse_refs():
    rng = np.random.default_rng(0)
    for method in (0, 1):
        for _ in range(50):
            a = rng.normal(0, 2, (4, 5))
            want = fr.distance(a[0:1], a[1:2], a[2:3], a[3:4], method)[0]
            assert nr.distance(*[r.tolist() for r in a], method) == want


def lattice(gw, gh, first, skip):
    return [(y, x) for y in range(first, gh, skip) for x in range(first, gw, skip)]


def test_search_disc_fallback_and_rounding():
    c = lattice(40, 36, 1, 2)
    # away from the borders radius^2 100 on the skip-2 lattice holds at least 50 candidates: the disc, the pixel itself removed
    got = nr.search(c, 21, 17, 0, 100.0, True)
    want = [(y, x) for y, x in c if (x - 21) ** 2 + (y - 17) ** 2 <= 100 and (y, x) != (17, 21)]
    assert got == want and len(got) >= 50
    assert len(nr.search(c, 21, 17, 0, 100.0, False)) == len(got) + 1          # without a hypothesis at the pixel nothing is removed
    assert nr.search(c, 20, 17, 0, 100.0, True) == nr.search(c, 20, 17, 0, 100.0, False)   # (20, 17) is no lattice point
    # in the corner fewer than 50 lie inside: the 50 nearest, ties of d^2 to the lower (y, x)
    got = nr.search(c, 0, 0, 0, 100.0, False)
    assert len(got) == 50 and len([q for q in c if q[0] ** 2 + q[1] ** 2 <= 100]) < 50
    far = max(q[0] ** 2 + q[1] ** 2 for q in got)
    ring = sorted(q for q in c if q[0] ** 2 + q[1] ** 2 == far)
    assert [q for q in got if q[0] ** 2 + q[1] ** 2 == far] == ring[:len([q for q in got if q[0] ** 2 + q[1] ** 2 == far])]
    assert all(q in got for q in c if q[0] ** 2 + q[1] ** 2 < far)
    # fewer than 50 in the whole set: all of them
    assert nr.search(c[:30], 5, 5, 0, 1.0, False) == sorted(c[:30])
    assert nr.search([], 5, 5, 0, 100.0, True) == []
    # 49.9999999 is 50 as a float: d^2 = 50 is inside; set 1 doubles the radius
    d = lattice(40, 36, 1, 1)
    assert (17 + 5, 21 + 5) in nr.search(d, 21, 17, 0, 49.9999999, True) and (17 + 5, 21 + 5) not in nr.search(d, 21, 17, 0, 49.99999, True)
    assert (17 + 10, 21) in nr.search(d, 21, 17, 1, 50.0, True) and (17 + 10, 21) not in nr.search(d, 21, 17, 0, 50.0, True)


def test_candidate_sets_follow_the_reference_loops():
    l = make_lists(1, 13, 11, holes=0.0, pruned=True)
    sets, holds, source = nr.candidate_sets(l, 1, None, 2, 4)
    assert sets[0] == lattice(13, 11, 1, 2) and sets[1] == lattice(13, 11, 2, 4) and holds.all() and not source.any()
    sets, _, _ = nr.candidate_sets(l, 1, None, 1, 1)                            # (1 - 2) % 1 == 0 in C: skip 1 admits row and column 1 in set 1
    assert sets[0] == lattice(13, 11, 1, 1) and sets[1] == lattice(13, 11, 1, 1)
    cons = np.zeros((11, 13), np.uint8)
    cons[3, 3] = cons[2, 2] = 1
    cons[5, 5] = 2                                                              # only == 1 counts (:1445)
    sets, _, _ = nr.candidate_sets(l, 0, cons, 2, 4)
    assert sets == ([(3, 3)], [(2, 2)])
    l["energy"][:, 3, 3] = np.inf                                               # a candidate holds a hypothesis
    assert nr.candidate_sets(l, 0, cons, 2, 4)[0][0] == []
    m = make_lists(2, 9, 8, holes=0.0)
    _, holds, source = nr.candidate_sets(m, 0, np.ones((8, 9), np.uint8), 2, 4)
    e = np.where(m["energy"] < np.inf, m["energy"], np.inf)
    assert np.array_equal(holds, (e < np.inf).any(0)) and np.array_equal(source[holds], np.argmin(e, 0)[holds])


def test_prune_restatement_properties():
    l = make_lists(3, 9, 7, slots=6)
    l["energy"][1, 2, 2] = l["energy"][4, 2, 2] = l["energy"][5, 2, 2] = 7.0   # ties: the lower position first
    l["energy"][0, 2, 2], l["energy"][2, 2, 2], l["energy"][3, 2, 2] = 9.0, np.inf, 8.0
    sel = np.full((7, 9), -1)
    sel[2, 2] = 3
    out = nr.prune(l, sel, 2)
    assert out["origin"][:, 2, 2].tolist()[:3] == [3, 1, 4] and not (out["energy"][3:, 2, 2] < np.inf).any()
    out = nr.prune(l, np.full((7, 9), -1), 2)                                   # no selection: the top keep + 1
    assert out["origin"][:3, 2, 2].tolist() == [1, 4, 5] and not (out["energy"][3:, 2, 2] < np.inf).any()
    out = nr.prune(l, sel, 0)                                                   # keep 0: the selection alone
    assert out["origin"][0, 2, 2] == 3 and not (out["energy"][1:, 2, 2] < np.inf).any()
    out = nr.prune(l, sel, 15)                                                  # the largest value: everything present stays
    assert (out["energy"] < np.inf).sum() == (l["energy"] < np.inf).sum()


@functools.lru_cache(maxsize=None)
def quota_case(flows, tryouts):
    l = make_lists(4, 23, 19, flows=flows, pruned=True)
    trace = {}
    out = nr.propose(l, nr.Params(hyp_neigh_tryouts=tryouts, neigh_hyp=2, perturb_keep=3), 1, 9, trace=trace)
    return l, out, trace


def test_quota_paths_of_the_restatement():
    # far flows: the quota of 2, then 4, is reached before the tryouts run out
    l, (out, _, _, acc), trace = quota_case("random", 20)
    new = ((out["origin"] & nr.PROPOSAL) != 0).sum(0)
    full = (l["energy"] < np.inf).sum(0) > 0
    assert (new[full] == 4).all() and acc == new.sum() and max(t for _, t in trace.values()) < 20
    # block-constant flows: some pixels exhaust their tryouts with the quota open
    l, (out, _, _, acc), trace = quota_case("blocks", 6)
    new = ((out["origin"] & nr.PROPOSAL) != 0).sum(0)
    assert (new < 4).any() and (new > 0).any() and any(t == 6 for _, t in trace.values())
    # a constant field: every proposal is similar to what the pixel holds; a pixel without a hypothesis takes the first
    l, (out, _, _, acc), _ = quota_case("constant", 6)
    new = ((out["origin"] & nr.PROPOSAL) != 0).sum(0)
    holds = (l["energy"] < np.inf).any(0)
    assert not new[holds].any() and (new[~holds] == 1).all() and (~holds).any()


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_gpu_philox_known_answers(ctx):
    got = ctx.philox4x32_10(np.array([k[0] for k in KAT], np.uint32), np.array([k[1] for k in KAT], np.uint32))
    assert [tuple(int(v) for v in row) for row in got] == [k[2] for k in KAT]
    rng = np.random.default_rng(0)
    ctr, key = rng.integers(0, 2 ** 32, (300, 4), dtype=np.uint64), rng.integers(0, 2 ** 32, (300, 2), dtype=np.uint64)
    got = ctx.philox4x32_10(ctr, key)
    assert [list(map(int, r)) for r in got] == [nr.philox4x32_10(c, k) for c, k in zip(ctr.tolist(), key.tolist())]


PRUNE = [(3, 9, 7, 6, 2), (5, 23, 19, 4, 0), (6, 40, 36, 4, 1), (7, 17, 5, 16, 15), (8, 300, 3, 5, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,gw,gh,slots,keep", PRUNE)
def test_gpu_prune_equals_restatement(ctx, seed, gw, gh, slots, keep):
    l = make_lists(seed, gw, gh, slots=slots)
    rng = np.random.default_rng(seed)
    l["energy"][:slots] = np.where(rng.random((slots, gh, gw)) < 0.3, np.float64(7.0), l["energy"][:slots])   # ties
    sel = rng.integers(-1, slots, (gh, gw)).astype(np.int32)                    # -1, present and absent positions alike
    sel[0, 0] = 16
    got = ctx.prune_hypotheses(batch(l), sel[None], keep)
    assert_lists_equal(got, nr.prune(l, sel, keep))


@pytest.mark.gpu
def test_gpu_prune_segments_are_independent(ctx):
    a, b = make_lists(11, 23, 19, slots=5), make_lists(12, 23, 19, slots=5)
    rng = np.random.default_rng(1)
    sel = rng.integers(-1, 5, (2, 19, 23)).astype(np.int32)
    got = ctx.prune_hypotheses(batch(a, b), sel, 2)
    assert_lists_equal(got, nr.prune(a, sel[0], 2), 0)
    assert_lists_equal(got, nr.prune(b, sel[1], 2), 1)


def round0_mask(kind, gw, gh, seed):
    rng = np.random.default_rng(seed)
    if kind == "all":
        return np.ones((gh, gw), np.uint8)
    if kind == "none":
        return np.zeros((gh, gw), np.uint8)
    if kind == "few":                                                           # fewer than 50 candidates in the whole grid
        m = np.zeros((gh, gw), np.uint8)
        m[rng.random((gh, gw)) < 0.06] = 1
        return m
    m = (rng.random((gh, gw)) < 0.6).astype(np.uint8)                           # "patch": more than 50 candidates, all in one corner
    m[:, gw // 2:] = 0
    m[rng.random((gh, gw)) < 0.1] = 2                                           # only == 1 counts
    return m


# (name, grid, round, mask, list arguments, parameter arguments)
PROPOSE = [
    ("disc_and_corners", (40, 36), 1, None, dict(), dict()),
    ("round0_all", (40, 36), 0, "all", dict(), dict(hyp_neigh_tryouts=8)),
    ("rounding_up", (23, 19), 1, None, dict(holes=0.0), dict(neigh_hyp_radius=49.9999999, neigh_skip1=1, neigh_skip2=1, hyp_neigh_tryouts=8)),
    ("rounding_down", (23, 19), 1, None, dict(holes=0.0), dict(neigh_hyp_radius=49.99999, neigh_skip1=1, neigh_skip2=1, hyp_neigh_tryouts=8)),
    ("sparse_few", (40, 36), 0, "few", dict(), dict(hyp_neigh_tryouts=6)),
    ("sparse_none", (23, 19), 0, "none", dict(), dict()),
    ("sparse_patch", (40, 36), 0, "patch", dict(), dict(hyp_neigh_tryouts=6)),
    ("quota_first", (23, 19), 1, None, dict(), dict(neigh_hyp=2)),
    ("tryouts_first", (23, 19), 1, None, dict(flows="blocks"), dict(neigh_hyp=2, hyp_neigh_tryouts=6)),
    ("similar", (23, 19), 1, None, dict(flows="constant"), dict(neigh_hyp=2, hyp_neigh_tryouts=6)),
    ("adj_skip3", (23, 19), 1, None, dict(flows="blocks", J=5), dict(traj_sim_method=0, neigh_skip1=3, neigh_skip2=5, traj_sim_thres=0.5)),
    ("many_tryouts_list_fills_exactly", (23, 19), 1, None, dict(flows="blocks", slots=6), dict(neigh_hyp=5, hyp_neigh_tryouts=70, neigh_hyp_radius=30.0, perturb_keep=5)),
    ("round0_six_slots_fill_exactly", (23, 19), 0, "all", dict(slots=6), dict(slots=6, hyp_neigh_tryouts=30)),
    ("no_tryouts", (23, 19), 1, None, dict(), dict(hyp_neigh_tryouts=0)),
    ("no_quota", (23, 19), 1, None, dict(), dict(neigh_hyp=0)),
    ("one_row", (61, 2), 1, None, dict(), dict(hyp_neigh_tryouts=6)),
    ("one_pixel", (1, 1), 1, None, dict(holes=0.0), dict()),
]


@functools.lru_cache(maxsize=None)
def propose_case(name):
    _, (gw, gh), rnd, mask, la, pa = next(c for c in PROPOSE if c[0] == name)
    l = make_lists(len(name) * 7 + gw, gw, gh, pruned=rnd > 0, **la)
    p = nr.Params(seed=3, **{"perturb_keep": 3, **pa})
    cons = None if mask is None else round0_mask(mask, gw, gh, gw + gh)
    return l, p, rnd, cons, nr.propose(l, p, rnd, 1234, cons)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in PROPOSE])
def test_gpu_proposals_equal_restatement(ctx, name):
    import slowflow_amd as sfa
    l, p, rnd, cons, (want, wpix, wpos, wacc) = propose_case(name)
    got, pix, pos, acc = ctx.neighbour_proposals(p.to_c(sfa), batch(l), rnd, [1234], None if cons is None else cons[None])
    assert acc[0] == wacc
    assert np.array_equal(pix[0], wpix) and np.array_equal(pos[0], wpos)
    assert_lists_equal(got, want)
    if name in ("similar", "sparse_none", "no_tryouts", "no_quota"):
        holds = (l["energy"] < np.inf).any(0)
        assert not (pix[0] >= 0)[:, holds].any()
    if name == "sparse_none":
        assert acc[0] == 0
    if name in ("disc_and_corners", "quota_first", "round0_all"):
        assert acc[0] > 0


@pytest.mark.gpu
def test_gpu_holes_become_nodes_and_self_is_never_drawn(ctx):
    """every pixel without a hypothesis that has a candidate and a draw holds one afterwards; no pixel draws itself"""
    import slowflow_amd as sfa
    l, p, rnd, cons, _ = propose_case("round0_all")
    got, pix, pos, acc = ctx.neighbour_proposals(p.to_c(sfa), batch(l), rnd, [1234], cons[None])
    holds = (l["energy"] < np.inf).any(0)
    after = (got["energy"][0] < np.inf).any(0)
    assert (~holds).any() and after.all()
    gh, gw = holds.shape
    own = np.arange(gh * gw).reshape(gh, gw)
    assert not (pix[0] == own[None]).any()
    src = pix[0][pix[0] >= 0]
    assert holds.reshape(-1)[src].all()                                        # a source holds a hypothesis


@pytest.mark.gpu
def test_gpu_proposals_segments_and_keys(ctx):
    """segments of one call equal single calls; the draws depend on the seed + round and on sequence_start"""
    import slowflow_amd as sfa
    a, b = make_lists(21, 23, 19, pruned=True), make_lists(22, 23, 19, pruned=True, flows="blocks")
    p = nr.Params(seed=5, hyp_neigh_tryouts=6, perturb_keep=3)
    got, pix, pos, acc = ctx.neighbour_proposals(p.to_c(sfa), batch(a, b), 2, [7, 8])
    for s, (l, seq) in enumerate(((a, 7), (b, 8))):
        want, wpix, wpos, wacc = nr.propose(l, p, 2, seq)
        assert acc[s] == wacc and np.array_equal(pix[s], wpix) and np.array_equal(pos[s], wpos)
        assert_lists_equal(got, want, s)
    one, pix1, _, _ = ctx.neighbour_proposals(nr.Params(seed=6, hyp_neigh_tryouts=6, perturb_keep=3).to_c(sfa), batch(a), 1, [7])   # seed + round is the key
    assert np.array_equal(pix1[0], pix[0])
    _, pix2, _, _ = ctx.neighbour_proposals(p.to_c(sfa), batch(a), 2, [9])
    assert not np.array_equal(pix2[0], pix[0])


REFUSED = [
    (dict(neigh_hyp_radius=0.0), "acc_neigh_hyp_radius"), (dict(neigh_hyp_radius=-1.0), "acc_neigh_hyp_radius"),
    (dict(neigh_hyp_radius=float("nan")), "acc_neigh_hyp_radius"), (dict(neigh_skip1=0), "acc_neigh_skip1"), (dict(neigh_skip2=0), "acc_neigh_skip2"),
    (dict(hyp_neigh_tryouts=-1), "acc_hyp_neigh_tryouts"), (dict(neigh_hyp=-1), "acc_neigh_hyp"), (dict(traj_sim_method=2), "acc_traj_sim_method"),
    # the issue's limits: acc_perturb_keep + 1 + 2 * acc_neigh_hyp > 16, and acc_perturb_keep absent, in rounds after the first
    (dict(perturb_keep=6), r"acc_perturb_keep \+ 1 \+ 2 \* acc_neigh_hyp"), (dict(neigh_hyp=7), r"acc_perturb_keep \+ 1 \+ 2 \* acc_neigh_hyp"),
    (dict(perturb_keep=-1), "acc_perturb_keep is not set"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kw,name", REFUSED)
def test_gpu_proposals_refusals_by_name(ctx, kw, name):
    import slowflow_amd as sfa
    l = batch(make_lists(1, 9, 7, pruned=True))
    with pytest.raises(sfa.SlowflowError, match=name):
        ctx.neighbour_proposals(sfa.neigh_params(**{"perturb_keep": 3, **kw}), l, 1, [0])


@pytest.mark.gpu
def test_gpu_list_limits_are_refused_by_name(ctx):
    """slots + 2 * acc_neigh_hyp > 16 in round 0; a list longer than the limit counts on, in either kind of round; the largest that fits is taken"""
    import slowflow_amd as sfa
    l = batch(make_lists(1, 9, 7, slots=4))
    cons = np.ones((1, 7, 9), np.uint8)
    for kw in (dict(slots=7), dict(slots=4, neigh_hyp=7), dict(slots=17), dict(slots=0)):
        with pytest.raises(sfa.SlowflowError, match="slots"):
            ctx.neighbour_proposals(sfa.neigh_params(**kw), l, 0, [0], cons)
    with pytest.raises(sfa.SlowflowError, match="holds a hypothesis at position 3"):
        ctx.neighbour_proposals(sfa.neigh_params(slots=3), l, 0, [0], cons)
    pr = batch(make_lists(1, 9, 7, slots=4, pruned=True, holes=0.0))
    pr["energy"][0, :4] = 1.0
    with pytest.raises(sfa.SlowflowError, match="holds a hypothesis at position 3"):
        ctx.neighbour_proposals(sfa.neigh_params(perturb_keep=2), pr, 1, [0])
    ctx.neighbour_proposals(sfa.neigh_params(slots=6), l, 0, [0], cons)          # 6 + 10 = 16
    ctx.neighbour_proposals(sfa.neigh_params(perturb_keep=5), pr, 1, [0])        # 5 + 1 + 10 = 16


@pytest.mark.gpu
def test_gpu_stage_refusals(ctx):
    import slowflow_amd as sfa
    l = batch(make_lists(1, 9, 7, pruned=True))
    with pytest.raises(sfa.SlowflowError, match="consistent"):
        ctx.neighbour_proposals(sfa.neigh_params(), l, 0, [0])                  # round 0 without the mask
    with pytest.raises(sfa.SlowflowError, match="round"):
        ctx.neighbour_proposals(sfa.neigh_params(perturb_keep=3), l, -1, [0])
    for keep in (-1, 16):
        with pytest.raises(sfa.SlowflowError, match="acc_perturb_keep"):
            ctx.prune_hypotheses(l, np.zeros((1, 7, 9), np.int32), keep)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the fusion with position 0 pinned (sfa_fuse_params.pin_first)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_unpinned_labels_are_fuse_refs():
    l = make_lists(31, 12, 9, slots=5, flows="blocks")
    l["V"][1] = l["V"][0] + 0.01                                                # NMS active
    l["U"][1] = l["U"][0]
    want = fr.labels(l["U"], l["V"], l["energy"], 1, 0.1)
    assert nr.labels(l["U"], l["V"], l["energy"], 1, 0.1, False) == want
    pinned = nr.labels(l["U"], l["V"], l["energy"], 1, 0.1, True)
    assert pinned != want and all(a[0] == 0 for a, b in zip(pinned, want) if 0 in b)


def pinned_pixel():
    """position 0 is worse than position 1 and similar to it; position 2 is far from both"""
    U, V = np.zeros((3, 2, 1, 1)), np.zeros((3, 2, 1, 1))
    U[0, :, 0, 0], U[1, :, 0, 0], U[2, :, 0, 0] = (1, 1), (1.01, 1), (5, 5)
    return U, V, np.array([3.0, 1.0, 2.0]).reshape(3, 1, 1)


def test_pinned_position_survives_in_the_restatement():
    U, V, e = pinned_pixel()
    assert nr.labels(U, V, e, 1, 0.1, False) == [[1, 2]]                        # sorted 1, 2, 0: 2 is far and kept, 0 is similar to 1 and discarded
    assert nr.labels(U, V, e, 1, 0.1, True) == [[0]]                            # pinned: 0 first; 1 is similar: discarded, and the break drops 2
    e[1] = np.inf
    assert nr.labels(U, V, e, 1, 0.1, True) == [[0, 2]]
    e[0], e[1] = np.inf, 1.0                                                    # position 0 absent: the plain sort
    assert nr.labels(U, V, e, 1, 0.1, True) == [[1, 2]]


@pytest.mark.gpu
def test_gpu_pinned_position_survives(ctx):
    import slowflow_amd as sfa
    U, V, e = pinned_pixel()
    occ, weight = np.zeros((1, 3, 1, 1), np.uint64), np.ones((1, 1, 1), np.float32)
    got = ctx.fuse_hypotheses(sfa.fuse_params(skip=0, pin_first=1), U[None], V[None], e[None], occ, weight, 1, 1)
    assert got["slot"][0, 0, 0] == 0 and got["energy"][0] == 3.0
    got = ctx.fuse_hypotheses(sfa.fuse_params(skip=0), U[None], V[None], e[None], occ, weight, 1, 1)
    assert got["slot"][0, 0, 0] == 1 and got["energy"][0] == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("gw,gh,slots,J,method", [(23, 19, 4, 3, 1), (12, 9, 16, 4, 0), (40, 36, 7, 3, 1)])
def test_gpu_pinned_fusion_equals_restatement(ctx, gw, gh, slots, J, method):
    """skip 0: the grid is the image.  Position 1 is a near copy of position 0 at many pixels, so the pin decides what the NMS keeps"""
    import slowflow_amd as sfa
    l = make_lists(gw + slots, gw, gh, J=J, slots=slots, flows="blocks")
    rng = np.random.default_rng(gw)
    near = rng.random((gh, gw)) < 0.5
    l["U"][1][:, near], l["V"][1][:, near] = l["U"][0][:, near] + 0.01, l["V"][0][:, near]
    weight = rng.uniform(0.01, 0.5, (gh, gw)).astype(np.float32)
    p = fr.Params(traj_sim_method=method, skip=0, trws_max_iter=5)
    cp = p.to_c(sfa)
    cp.pin_first = 1
    got = ctx.fuse_hypotheses(cp, l["U"][None, :slots], l["V"][None, :slots], l["energy"][None, :slots], l["occ"][None, :slots], weight[None], gw, gh)
    want = nr.fuse(l["U"][:slots], l["V"][:slots], l["energy"][:slots], l["occ"][:slots], weight, p, gw, True)
    for k in ("slot", "u", "v", "occ"):
        assert np.array_equal(got[k][0], want[k]), k
    assert got["energy"][0] == want["energy"] and got["bound"][0] == want["bound"] and got["iters"][0] == want["iters"]
    plain = fr.fuse(l["U"][:slots], l["V"][:slots], l["energy"][:slots], l["occ"][:slots], weight, p, gw)
    assert not np.array_equal(plain["slot"], want["slot"])                      # the pin changes the result here


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the rescoring of accepted proposals (sfa_rescore_proposals) and the rounds as stage calls
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def scene(seed, w, h, J):
    rng = np.random.default_rng(seed)
    stride = (w + 3) // 4 * 4
    frames = np.zeros((1, J + 1, 3, h, stride), np.float32)
    frames[..., :w] = rng.normal(0, 1, (1, J + 1, 3, h, w))
    flows = [np.zeros((1, J, h, stride), np.float32) for _ in range(4)]
    for a in flows:
        a[..., :w] = rng.normal(0, 1.5, (1, J, h, w))
    return frames, flows


SLOT_WEIGHT = [0.0, 0.0, 1.25, 1.25]                                            # two rates with fill-in: slots 2 r + kind


@pytest.mark.gpu
@pytest.mark.parametrize("skip,w,h,with_flows", [(1, 46, 38, True), (0, 23, 19, True), (1, 46, 38, False)])
def test_gpu_rescore_equals_restatement_and_the_energy_stage(ctx, oracle, skip, w, h, with_flows):
    import energy_ref as er
    import slowflow_amd as sfa
    J = 3
    gw, gh = sfa.accumulate_grid(w, h, skip)
    assert (gw, gh) == (23, 19)
    l = make_lists(41 + skip, gw, gh, J=J)
    l["U"], l["V"] = l["U"] / 2, l["V"] / 2                                      # most trajectories stay inside the image
    p = nr.Params(seed=1, hyp_neigh_tryouts=8)
    got, pix, _, acc = ctx.neighbour_proposals(p.to_c(sfa), batch(l), 0, [3], np.ones((1, gh, gw), np.uint8))
    assert acc[0] > 0
    frames, flows = scene(5, w, h, J)
    if not with_flows:
        flows = None
    ep = er.Params(skip=skip, weight=7.0)                                       # the weight of the parameters is ignored
    out = ctx.rescore_proposals(ep.to_c(sfa), got, pix, frames, w, flows, SLOT_WEIGHT)
    dx, dy = er.derivatives(oracle, frames[0], w)
    want = nr.rescore({k: v[0] for k, v in got.items()}, pix[0], ep, frames[0], dx, dy, None if flows is None else [a[0] for a in flows], SLOT_WEIGHT, w)
    assert_lists_equal(out, want)
    new = pix[0] >= 0
    assert not np.array_equal(out["energy"][0][new], got["energy"][0][new])     # the source's energy is replaced
    assert np.array_equal(out["energy"][0][~new], got["energy"][0][~new]) and np.array_equal(out["occ"][0][~new], got["occ"][0][~new])
    # the same numbers from the energy stage itself, position by position
    e0 = ep.to_c(sfa)
    e0.weight = 0.0
    for k in np.flatnonzero(new.any((1, 2))):
        tr = np.where(new[k], J, 0).astype(np.int32)[None]
        e, o = ctx.hypothesis_energies(e0, J, got["U"][:, k], got["V"][:, k], tr, frames, w, flows)
        wk = np.asarray(SLOT_WEIGHT + [0.0] * 124, np.float32)[got["origin"][0, k] & 0x7f]
        assert np.array_equal(out["energy"][0, k][new[k]], (e[0].astype(np.float32) + wk).astype(np.float64)[new[k]])
        assert np.array_equal(out["occ"][0, k][new[k]], o[0][new[k]])


@pytest.mark.gpu
def test_gpu_rounds_as_stage_calls(ctx, oracle):
    """three rounds of prune -> propose -> rescore -> fuse through the stage calls equal the restatements chained the same way; in a grid with
    holes every pixel is a node after round 0"""
    import energy_ref as er
    import slowflow_amd as sfa
    J, skip, w, h, keep = 3, 0, 23, 19, 2
    gw, gh = w, h
    l = make_lists(51, gw, gh, J=J, flows="blocks")
    l["U"], l["V"] = l["U"] / 2, l["V"] / 2
    frames, flows = scene(6, w, h, J)
    dx, dy = er.derivatives(oracle, frames[0], w)
    weight = np.random.default_rng(2).uniform(0.01, 0.5, (h, w)).astype(np.float32)
    p, ep, fp = nr.Params(seed=9, hyp_neigh_tryouts=6, neigh_hyp=3, perturb_keep=keep), er.Params(skip=skip), fr.Params(skip=skip, trws_max_iter=4)
    cons = (np.random.default_rng(3).random((gh, gw)) < 0.8).astype(np.uint8)
    g, r = batch(l), l
    for rnd in range(3):
        if rnd > 0:
            g, r = ctx.prune_hypotheses(g, gsel, keep), nr.prune(r, rsel, keep)
            assert_lists_equal(g, r)
        g, pix, _, _ = ctx.neighbour_proposals(p.to_c(sfa), g, rnd, [77], cons[None] if rnd == 0 else None)
        r, rpix, _, _ = nr.propose(r, p, rnd, 77, cons)
        assert np.array_equal(pix[0], rpix)
        g = ctx.rescore_proposals(ep.to_c(sfa), g, pix, frames, w, flows, SLOT_WEIGHT)
        r = nr.rescore(r, rpix, ep, frames[0], dx, dy, [a[0] for a in flows], SLOT_WEIGHT, w)
        assert_lists_equal(g, r)
        cf = fp.to_c(sfa)
        cf.pin_first = int(rnd > 0)
        gf = ctx.fuse_hypotheses(cf, g["U"], g["V"], g["energy"], g["occ"], weight[None], w, h)
        rf = nr.fuse(r["U"], r["V"], r["energy"], r["occ"], weight, fp, w, rnd > 0)
        for k in ("slot", "u", "v", "occ"):
            assert np.array_equal(gf[k][0], rf[k]), (rnd, k)
        assert gf["energy"][0] == rf["energy"] and gf["bound"][0] == rf["bound"] and gf["iters"][0] == rf["iters"]
        if rnd == 0:
            assert (~(l["energy"] < np.inf).any(0)).any() and (gf["slot"][0] >= 0).all()
        gsel, rsel = gf["slot"], rf["slot"]


@pytest.mark.gpu
def test_gpu_rescore_nan_in_the_stride_padding_changes_nothing(ctx):
    """frames and flows at a row stride of w + 3: the columns past w are never read.  The smallest shape the kernels take (h >= 4), odd width and stride
    so that no alignment hides a wrong pitch; the proposals are named by hand, a handful over four positions"""
    import energy_ref as er
    import slowflow_amd as sfa
    J, skip, w, h = 2, 1, 13, 9
    stride = w + 3
    gw, gh = sfa.accumulate_grid(w, h, skip)
    l = make_lists(61, gw, gh, J=J, pruned=True)
    l["U"], l["V"] = l["U"] / 2, l["V"] / 2
    pix = np.full((1, K16, gh, gw), -1, np.int32)
    for k, y, x in [(0, 0, 0), (1, 1, 2), (1, 3, 5), (2, 2, 1), (3, 0, 4), (3, 3, 3)]:
        pix[0, k, y, x] = (gh - 1 - y) * gw + x                                 # any source pixel: the rescoring asks only whether there is one
    new = pix[0] >= 0
    rng = np.random.default_rng(7)
    valid_frames = rng.normal(0, 1, (1, J + 1, 3, h, w))
    valid_flows = rng.normal(0, 1.5, (4, 1, J, h, w))
    out = []
    for pad in (0.0, np.nan):
        frames = np.full((1, J + 1, 3, h, stride), pad, np.float32)
        frames[..., :w] = valid_frames
        flows = [np.full((1, J, h, stride), pad, np.float32) for _ in range(4)]
        for a, v in zip(flows, valid_flows):
            a[..., :w] = v
        out.append(ctx.rescore_proposals(er.Params(skip=skip).to_c(sfa), batch(l), pix, frames, w, flows, SLOT_WEIGHT))
    zero, nan = out
    assert np.isfinite(zero["energy"][0][new]).all() and not np.array_equal(zero["energy"][0][new], l["energy"][new])   # they were scored
    assert np.array_equal(zero["energy"].view(np.uint64), nan["energy"].view(np.uint64)) and np.array_equal(zero["occ"], nan["occ"])
