"""dense_tracking's alternation around the fusion (reference dense_tracking.cpp:1381-1583) restated in plain Python as INTEGRATION.md 4d defines it:
Philox4x32-10 from the paper (Salmon, Moraes, Dror, Shaw, SC'11), the prune (:1384-1416), the candidate sets (:1442-1474), the search (:1503-1528) by
brute force over every candidate, the draws and the acceptance (:1533-1568).  The distance is fuse_ref.distance's arithmetic on Python floats (IEEE
doubles, every operation rounded on its own; test_neigh.py holds the two against each other).

One segment: a list is a dict U, V (16, Jets, gh, gw) float64, energy (16, gh, gw) float64 (+Inf or NaN: absent), occ (16, gh, gw) uint64, origin
(16, gh, gw) uint8 (the slot a hypothesis was born in, | 0x80 once it has arrived as a proposal).
"""
import math

import numpy as np

KMAX = 16
NEAREST = 50
PROPOSAL = 0x80
F32 = np.float32
M32 = 0xFFFFFFFF


class Params:
    """sfa_neigh_params: setDefault's values (dense_tracking.cpp:136-159), seed 0"""
    def __init__(self, **kw):
        self.traj_sim_thres, self.traj_sim_method, self.neigh_hyp, self.neigh_hyp_radius = 0.1, 1, 5, 100.0
        self.neigh_skip1, self.neigh_skip2, self.hyp_neigh_tryouts, self.seed = 2, 4, 20, 0
        self.slots, self.perturb_keep = 4, -1                                  # the lists' capacity in round 0 / acc_perturb_keep (no default)
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, type(getattr(self, k))(v))

    def to_c(self, sfa):
        return sfa.neigh_params(**vars(self))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Philox4x32-10
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """the paper's Philox-4x32 with 10 rounds: multipliers 0xD2511F53, 0xCD9E8D57, the key bumped by the Weyl constants between the rounds"""
    c = [int(v) & M32 for v in ctr]
    k = [int(v) & M32 for v in key]
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
    return c


def draw(seed, round, seq_start, pixel, t, tryout, found):
    """ridx of one tryout: the first word scaled to 0 .. found - 1"""
    r = philox4x32_10((pixel, t, tryout, 0), ((seed + round) & M32, seq_start))[0]
    return (r * found) >> 32


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# lists
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def present(e):
    return e < math.inf                                                         # NaN is absent, as in the fusion


def empty_like(lists):
    out = {k: np.zeros_like(v) for k, v in lists.items()}
    out["energy"][:] = np.inf
    return out


def _put(out, k, y, x, src, sk, sy, sx, flag=0):
    out["U"][k, :, y, x], out["V"][k, :, y, x] = src["U"][sk, :, sy, sx], src["V"][sk, :, sy, sx]
    out["energy"][k, y, x], out["occ"][k, y, x] = src["energy"][sk, sy, sx], src["occ"][sk, sy, sx]
    out["origin"][k, y, x] = src["origin"][sk, sy, sx] | flag


def by_score(energy, positions):
    """compareHypotheses: the float score, ties to the lower position"""
    with np.errstate(over="ignore"):
        return sorted(positions, key=lambda k: (float(F32(energy[k])), k))


def prune(lists, selected, keep):
    """:1384-1416.  selected (gh, gw): the position the last fusion chose, -1 none (an absent position counts as none)"""
    _, gh, gw = lists["energy"].shape
    out = empty_like(lists)
    for y in range(gh):
        for x in range(gw):
            e = lists["energy"][:, y, x]
            last = int(selected[y, x])
            if not (0 <= last < KMAX and present(e[last])):
                last = -1
            new = [last] if last >= 0 else []
            for k in by_score(e, [k for k in range(KMAX) if k != last and present(e[k])]):
                if len(new) <= keep:                                            # `size() <= perturb_keep` before each push
                    new.append(k)
            for i, k in enumerate(new[:KMAX]):
                _put(out, i, y, x, lists, k, y, x)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# candidates and search
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def c_rem(a, b):
    """C's a % b for b > 0: truncation towards zero"""
    return a - b * int(a / b)


def candidate_sets(lists, round, consistent, skip1, skip2):
    """:1442-1474.  Returns (sets, holds, source): sets[t] the candidates (y, x) of set t in raster order; holds (gh, gw) bool; source (gh, gw): the
    position a neighbour copies -- round 0: the best score, later: position 0 of the pruned list"""
    _, gh, gw = lists["energy"].shape
    holds, source = np.zeros((gh, gw), bool), np.zeros((gh, gw), int)
    sets = ([], [])
    for y in range(gh):
        for x in range(gw):
            e = lists["energy"][:, y, x]
            if round > 0:
                holds[y, x] = present(e[0])
            else:
                have = [k for k in range(KMAX) if present(e[k])]
                holds[y, x] = bool(have)
                if have:
                    source[y, x] = by_score(e, have)[0]
            if y < 1 or x < 1 or not holds[y, x] or (round == 0 and consistent[y, x] != 1):
                continue
            if c_rem(y - 1, skip1) == 0 and c_rem(x - 1, skip1) == 0:
                sets[0].append((y, x))
            if c_rem(y - 2, skip2) == 0 and c_rem(x - 2, skip2) == 0:
                sets[1].append((y, x))
    return sets, holds, source


def search(cands, x, y, t, radius, holds_here):
    """:1503-1528 as defined: FLANN's radius is a squared distance compared in fp32; fewer than 50 inside: the 50 nearest by (d^2, y, x); the pixel
    itself removed where it holds a hypothesis; raster order.  cands: the set's (y, x) list"""
    if not cands:
        return []
    c = np.asarray(cands)
    dx, dy = (c[:, 1] - x).astype(F32), (c[:, 0] - y).astype(F32)
    inside = c[dx * dx + dy * dy <= F32(t + 1) * F32(radius)]
    if len(inside) < NEAREST:
        d2 = (c[:, 1] - x) ** 2 + (c[:, 0] - y) ** 2
        inside = c[np.lexsort((c[:, 1], c[:, 0], d2))[:NEAREST]]
    found = sorted((int(cy), int(cx)) for cy, cx in inside)
    if holds_here:
        found = [q for q in found if q != (y, x)]
    return found


def distance(ua, va, ub, vb, method):
    """hypothesis::distance of two full-length trajectories given as Python lists"""
    J = len(ua)
    s = 0.0
    for f in range(J):
        if method == 1:
            ysq = va[f] - vb[f]
            xsq = ua[f] - ub[f]
            s = s + math.sqrt(xsq * xsq + ysq * ysq) / (f + 1)
        else:
            pau, pav, pbu, pbv = (ua[f - 1], va[f - 1], ub[f - 1], vb[f - 1]) if f > 0 else (0.0, 0.0, 0.0, 0.0)
            ysq = (va[f] - pav) - (vb[f] - pbv)
            xsq = (ua[f] - pau) - (ub[f] - pbu)
            s = s + math.sqrt(xsq * xsq + ysq * ysq)
    if method != 1:
        s = s / J
    return s


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the proposals of one round
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def propose(lists, p, round, seq_start, consistent=None, trace=None):
    """:1432-1583 for one segment.  Returns (lists, src_pixel, src_position, accepted): src_pixel, src_position (16, gh, gw): the source of a position
    filled in this round, -1 / 0 elsewhere.  trace: a dict that receives per (y, x, t) the pair (found, tryouts made)"""
    _, gh, gw = lists["energy"].shape
    cap = p.slots if round == 0 else p.perturb_keep + 1                         # the limits refused by name: no list can fill up
    assert 1 <= cap and cap + 2 * p.neigh_hyp <= KMAX and not (lists["energy"][cap:] < np.inf).any(), "limits"
    sets, holds, source = candidate_sets(lists, round, consistent, p.neigh_skip1, p.neigh_skip2)
    out = {k: v.copy() for k, v in lists.items()}
    absent = ~(lists["energy"] < np.inf)
    for k in ("U", "V"):
        out[k][np.broadcast_to(absent[:, None], out[k].shape)] = 0
    out["energy"][absent], out["occ"][absent], out["origin"][absent] = np.inf, 0, 0
    src_pixel, src_pos = np.full((KMAX, gh, gw), -1, np.int32), np.zeros((KMAX, gh, gw), np.uint8)
    Ul, Vl = lists["U"], lists["V"]
    accepted = 0
    for y in range(gh):
        for x in range(gw):
            pix = y * gw + x
            # the list as it stands: position -> (flows u, flows v)
            here = {k: (Ul[k, :, y, x].tolist(), Vl[k, :, y, x].tolist()) for k in range(KMAX) if not absent[k, y, x]}
            added = 0
            for t in range(2):
                found_set = search(sets[t], x, y, t, p.neigh_hyp_radius, holds[y, x])
                found = len(found_set)
                tryouts = 0
                while found > 0 and tryouts < p.hyp_neigh_tryouts and added < (t + 1) * p.neigh_hyp:
                    cy, cx = found_set[draw(p.seed, round, seq_start, pix, t, tryouts, found)]
                    tryouts += 1
                    sk = int(source[cy, cx])
                    pu, pv = Ul[sk, :, cy, cx].tolist(), Vl[sk, :, cy, cx].tolist()
                    if any(not (distance(hu, hv, pu, pv, p.traj_sim_method) > p.traj_sim_thres) for hu, hv in here.values()):
                        continue
                    k = min(k for k in range(KMAX) if k not in here)
                    here[k] = (pu, pv)
                    _put(out, k, y, x, lists, sk, cy, cx, PROPOSAL)
                    src_pixel[k, y, x], src_pos[k, y, x] = cy * gw + cx, sk
                    added += 1
                    accepted += 1
                if trace is not None:
                    trace[(y, x, t)] = (found, tryouts)
    return out, src_pixel, src_pos, accepted


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the fusion of a round: fuse_ref's, with position 0 pinned in rounds p > 0
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def labels(U, V, energy, method, thres, pin):
    """fuse_ref.labels pixel by pixel, with the pin: position 0, where present, is the first label whatever its score and the sort covers the
    others (:1601-1602); the NMS with its `break` (:1609-1626) then measures them against it"""
    K, _, gh, gw = U.shape
    out = []
    for y in range(gh):
        for x in range(gw):
            e = energy[:, y, x]
            have = [k for k in range(K) if present(e[k])]
            order = ([0] + by_score(e, [k for k in have if k != 0])) if pin and have and have[0] == 0 else by_score(e, have)
            flows = {k: (U[k, :, y, x].tolist(), V[k, :, y, x].tolist()) for k in order}
            kept = order[:1]
            for c in order[1:]:
                if any(distance(*flows[c], *flows[q], method) < thres for q in kept):
                    break
                kept.append(c)
            out.append(kept)
    return out


def fuse(U, V, energy, occ, weight, p, w, pin):
    """fuse_ref.fuse with the labels above: p a fuse_ref.Params.  The same dict"""
    import fuse_ref as fr
    from accum_ref import grid
    K, J, gh, gw = U.shape
    _, _, incr, _ = grid(w, weight.shape[0], p.skip)
    lab = labels(U, V, energy, p.traj_sim_method, p.traj_sim_thres, pin)
    PR, PD = fr.pairwise(U, V, occ, weight, lab, p, w)
    theta = [np.array([energy[k, pi // gw, pi % gw] for k in lab[pi]], dtype=np.float64) for pi in range(gh * gw)]
    x, E, lb, its = fr.trws_diag(theta, PR, PD, gw, gh, p.trws_eps, p.trws_max_iter)
    slot = np.full((gh, gw), -1, np.int32)
    u, v = np.full((gh, gw), fr.UNKNOWN_FLOW), np.full((gh, gw), fr.UNKNOWN_FLOW)
    oc = np.zeros((gh, gw), np.uint8)
    for pi in range(gh * gw):
        if lab[pi]:
            y, xx = divmod(pi, gw)
            k = lab[pi][x[pi]]
            slot[y, xx], u[y, xx], v[y, xx] = k, U[k, J - 1, y, xx] / incr, V[k, J - 1, y, xx] / incr
            oc[y, xx] = 1 if (int(occ[k, y, xx]) & ((1 << (J + 1)) - 1)) else 0
    return dict(slot=slot, u=u, v=v, occ=oc, energy=E, bound=lb, iters=its, lab=lab)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the rescoring of a round's accepted proposals (:1549-1553): energy_ref's energies of the lists' flows as full-length trajectories
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def rescore(lists, src_pixel, p, frames, dx, dy, flows, slot_weight, w):
    """p: an energy_ref.Params (its weight is ignored); frames, dx, dy: (Jets + 1, 3, h, stride); flows: None or four (Jets, h, stride) arrays (the
    first w columns of each are the image);
    slot_weight: weight_jet_estimation of the rate each slot belongs to.  Positions with src_pixel >= 0 get the energy
    ((JC + BCGC) + OC) + slot_weight[origin & 0x7f] in fp32 and the occlusion word of their new place"""
    import copy

    import energy_ref as er
    J = lists["U"].shape[1]
    q = copy.copy(p)
    q.weight = F32(0.0)
    out = {k: v.copy() for k, v in lists.items()}
    wt = np.zeros(128, F32)
    wt[:len(slot_weight)] = slot_weight
    frames, dx, dy = (np.ascontiguousarray(a[..., :w]) for a in (frames, dx, dy))
    flows = None if flows is None else [np.ascontiguousarray(a[..., :w]) for a in flows]
    for k in range(KMAX):
        new = src_pixel[k] >= 0
        if not new.any():
            continue
        e, b, _ = er.energies(q, J, lists["U"][k], lists["V"][k], np.where(new, J, 0).astype(np.int32), frames, dx, dy, flows)
        total = (e.astype(F32) + wt[lists["origin"][k] & 0x7f]).astype(np.float64)
        out["energy"][k][new], out["occ"][k][new] = total[new], b[new]
    return out
