"""The track job that alternates (sfa_track_job_create_alternate, csrc/track_alt.hip): every start_jet of a run equals, with ==, the loop of stage calls
(prune -> neighbour proposals -> rescoring -> fusion) on that start_jet alone, for 1, 2 and 3 rounds and for groups of 1 and 3 start_jets; the results do
not depend on the group.  Inputs: tests/track_inputs.py's T1 (K 3, Jets 2, a 20 x 12 grid; rate 0 sees no flows, rate 2 is stored at half the size)."""
import numpy as np
import pytest

import slowflow_amd as sfa
import track_inputs as ti
from energy_ref import Params as EnergyRefParams
from test_track_job import same, upload

pytestmark = pytest.mark.gpu

CASE = ti.T1
KEYS = dict(hyp_neigh_tryouts=6, perturb_keep=3, seed=4)
SEQ = {11: 100, 12: 101, 13: 102}


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def segments():
    return {seed: ti.segment(CASE, seed) for seed in SEQ}


def slots_of(ctx, case, seg):
    """the job's slots of one start_jet by the stage calls: lists of 16 positions, the consistent mask, the smoothness weight"""
    K, J, w = case.K, case.Jets, case.w
    U, V = np.zeros((1, K, J, case.gh, case.gw)), np.zeros((1, K, J, case.gh, case.gw))
    E, O = np.zeros((1, K, case.gh, case.gw)), np.zeros((1, K, case.gh, case.gw), np.uint64)
    cons = np.zeros((1, case.gh, case.gw), np.uint8)
    mf = case.min_fps_idx
    for r in range(K):
        fu, fv, bu, bv = (a[None] for a in seg["flows"][r])
        au, av, tr = ctx.accumulate_consistent(fu, fv, bu, bv, w, ti.EPSILON, case.skip, 1, True, source=case.jet_source(r))
        ep = EnergyRefParams(skip=case.skip, weight=ti.WEIGHTS[r]).to_c(sfa)
        flows = tuple(a[None] for a in seg["flows"][mf]) if r >= mf else None
        e, o, au2, av2 = ctx.hypothesis_energies(ep, case.r_Jets[r], au, av, tr, seg["frames"][None], w, flows=flows, adapted=True)
        E[0, r], O[0, r], U[0, r], V[0, r] = e[0], o[0], au2[0], av2[0]
        cons |= (tr == case.r_Jets[r]).astype(np.uint8)
    weight = ctx.smoothness_weight(np.ascontiguousarray(seg["frames"][0]), w)
    return sfa.hyp_lists(U, V, E, O), cons, weight


def stage_loop(ctx, case, seg, seq, rounds):
    """-> the last round's fusion, the chosen origins and the per-round figures"""
    lists, cons, weight = slots_of(ctx, case, seg)
    p = sfa.neigh_params(slots=case.K, **KEYS)
    ep = EnergyRefParams(skip=case.skip).to_c(sfa)
    flows = tuple(a[None] for a in seg["flows"][case.min_fps_idx])
    per = dict(energy=[], bound=[], iters=[], nodes=[], accepted=[])
    for r in range(rounds):
        if r > 0:
            lists = ctx.prune_hypotheses(lists, f["slot"], KEYS["perturb_keep"])
        lists, pix, _, acc = ctx.neighbour_proposals(p, lists, r, [seq], cons if r == 0 else None)
        lists = ctx.rescore_proposals(ep, lists, pix, seg["frames"][None], case.w, flows, ti.WEIGHTS[:case.K])
        fp = sfa.fuse_params(trws_max_iter=case.trws_max_iter, trws_eps=case.trws_eps, skip=case.skip, pin_first=int(r > 0))
        f = ctx.fuse_hypotheses(fp, lists["U"], lists["V"], lists["energy"], lists["occ"], weight[None], case.w, case.h)
        for k, v in (("energy", f["energy"][0]), ("bound", f["bound"][0]), ("iters", f["iters"][0]), ("nodes", (f["slot"][0] >= 0).sum()), ("accepted", acc[0])):
            per[k].append(v)
    slot = f["slot"][0]
    yy, xx = np.indices(slot.shape)
    origin = np.where(slot >= 0, lists["origin"][0][slot.clip(0), yy, xx], 255).astype(np.uint8)
    return {k: f[k][0] for k in ("slot", "u", "v", "occ")}, origin, per, lists


@pytest.fixture(scope="module")
def wanted(ctx, segments):
    """the stage-call loop once per (start_jet, rounds)"""
    return {(seed, R): stage_loop(ctx, CASE, segments[seed], SEQ[seed], R) for seed in SEQ for R in (1, 2, 3)}


def check(job, s, want, rounds):
    fused, origin, per, _ = want
    got = job.download_fused(s)
    for k in ("slot", "u", "v", "occ"):
        assert same(got[k], fused[k]), (s, k)
    alt = job.download_alternation(s)
    assert same(alt["origin"], origin), s
    for k in ("energy", "bound"):
        assert same(alt[k], np.asarray(per[k], np.float64)), (s, k)
    for k in ("iters", "nodes", "accepted"):
        assert alt[k].tolist() == [int(v) for v in per[k]], (s, k)
    assert same(np.float64(got["energy"]), np.float64(per["energy"][-1])) and got["iters"] == int(per["iters"][-1])


@pytest.mark.parametrize("rounds", [1, 2, 3])
@pytest.mark.parametrize("group", [1, 3])
def test_job_equals_the_stage_call_loop(ctx, segments, wanted, rounds, group):
    seeds = list(SEQ)
    job = sfa.TrackJob(ctx, CASE.params(n=group), alt=sfa.track_alt_params(rounds, **KEYS))
    for g0 in range(0, len(seeds), group):
        part = seeds[g0:g0 + group]
        for s, seed in enumerate(part):
            upload(job, CASE, s, segments[seed], 0)
        job.set_sequence_starts([SEQ[seed] for seed in part])
        job.run(len(part))
        for s, seed in enumerate(part):
            check(job, s, wanted[seed, rounds], rounds)                          # the same expectation for every group size
    job.close()


def test_proposals_change_the_result_and_holes_become_nodes(ctx, segments, wanted):
    """a job without fill-in: every pixel without a hypothesis is a node after round 0 (candidates exist, and an empty list takes its first draw); a
    plain job leaves those pixels without a flow"""
    plain = sfa.TrackJob(ctx, CASE.params(n=1))
    seen_holes = 0
    for seed in SEQ:
        upload(plain, CASE, 0, segments[seed], 0)
        plain.run(1)
        before = plain.download_fused(0)["slot"]
        fused, origin, per, lists = wanted[seed, 1]
        holes = before < 0
        seen_holes += int(holes.sum())
        assert per["accepted"][0] > 0 and (fused["slot"][holes] >= 0).all() and (origin[holes] & 0x80).all()
        assert per["nodes"][0] == holes.size
    assert seen_holes > 0
    plain.close()


def test_creation_refusals_and_unchanged_byte_counts(ctx):
    p = CASE.params(n=2)
    assert sfa.track_job_bytes(p) < bytes_alt(p, sfa.track_alt_params(2, **KEYS))
    for alt, name in ((sfa.track_alt_params(0, **KEYS), "rounds"), (sfa.track_alt_params(2, **{**KEYS, "perturb_keep": -1}), "acc_perturb_keep is not set"),
                      (sfa.track_alt_params(2, **{**KEYS, "neigh_hyp": 7}), "slots"), (sfa.track_alt_params(2, **{**KEYS, "perturb_keep": 6}), "acc_perturb_keep"),
                      (sfa.track_alt_params(1, **{**KEYS, "neigh_skip1": 0}), "acc_neigh_skip1"), (sfa.track_alt_params(1, **{**KEYS, "neigh_hyp_radius": 0.0}),
                                                                                                    "acc_neigh_hyp_radius")):
        with pytest.raises(sfa.SlowflowError, match=name):
            sfa.TrackJob(ctx, p, alt=alt)
    sfa.TrackJob(ctx, p, alt=sfa.track_alt_params(1, **{**KEYS, "perturb_keep": -1})).close()   # one round needs no acc_perturb_keep
    with pytest.raises(sfa.SlowflowError, match="do_fuse"):
        sfa.TrackJob(ctx, CASE.params(n=1, do_fuse=0), alt=sfa.track_alt_params(1, **KEYS))
    plain = sfa.TrackJob(ctx, p)
    with pytest.raises(sfa.SlowflowError, match="does not alternate"):
        plain.set_sequence_starts([1, 2])
    plain.close()


def bytes_alt(p, alt):
    import ctypes as C
    L = sfa.lib()
    L.sfa_track_job_bytes_alternate.argtypes = [C.POINTER(sfa.TrackParams), C.c_void_p, C.POINTER(sfa.TrackAltParams), C.POINTER(C.c_size_t)]
    b = C.c_size_t()
    assert L.sfa_track_job_bytes_alternate(C.byref(p), None, C.byref(alt), C.byref(b)) == 0
    return b.value
