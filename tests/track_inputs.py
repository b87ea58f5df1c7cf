"""Seeded inputs of the track-job tests (tests/test_track_job.py, test_track_device.py, test_track_inputs.py) and their restatement through
tests/jet_resample_ref.py -> accum_ref -> energy_ref -> fuse_ref, one segment (start_jet) at a time.

A segment is smooth forward flows per rate (a translation of about two pixels over the segment plus a low-frequency wave, each rate with an offset of its
own so that the rates' hypotheses survive the NMS), backward flows that undo them, and per rate one rectangle where the backward flow contradicts the
forward one: there that rate loses its hypotheses and the other rates win the fusion.  One small rectangle is shared by all rates, so some pixels have
no hypothesis at all."""
import numpy as np

import fuse_ref as fr
import oracle as orc
import slowflow_amd as sfa
from accum_ref import accumulate, grid
from energy_ref import Params as EnergyRefParams, derivatives, energies
from jet_resample_ref import decode_occlusion_scaled, resample_flow

F32 = np.float32
PAD = F32(1e30)                                     # what the stride padding holds: never read


class Case:
    def __init__(self, name, w, h, skip, Jets, r_Jets, min_fps_idx, scaled=(), seeds=(), n=1, trws_max_iter=10, trws_eps=1e-5):
        self.name, self.w, self.h, self.skip, self.Jets, self.r_Jets, self.min_fps_idx = name, w, h, skip, Jets, tuple(r_Jets), min_fps_idx
        self.scaled, self.seeds, self.n, self.trws_max_iter, self.trws_eps = dict(scaled), tuple(seeds), n, trws_max_iter, trws_eps
        self.K = len(r_Jets)
        self.stride = sfa.stride_of(w)
        self.gw, self.gh, self.incr, self.start = grid(w, h, skip)

    def source(self, r):
        """rate r's planes: (sw, sh, stride, rescale); an identity source has the frames' stride"""
        if r in self.scaled:
            sw, sh = self.scaled[r]
            return sw, sh, sw, F32(self.w) / F32(sw)
        return self.w, self.h, self.stride, F32(1.0)

    def jet_source(self, r):
        sw, sh, stride, rs = self.source(r)
        return sfa.jet_source(sw, sh, stride, rescale=rs)

    def params(self, n=None, use_occlusions=0, discard=1, do_fuse=1):
        return sfa.track_params(self.w, self.h, self.Jets, self.r_Jets, n=self.n if n is None else n, sources=[self.jet_source(r) for r in range(self.K)],
                                weights=WEIGHTS[:self.K], fuse=sfa.fuse_params(trws_max_iter=self.trws_max_iter, trws_eps=self.trws_eps), min_fps_idx=self.min_fps_idx,
                                use_occlusions=use_occlusions, discard=discard, do_fuse=do_fuse, skip=self.skip, epsilon=EPSILON)


EPSILON = 0.75
WEIGHTS = (0.0, 0.5, 0.25) + (0.0,) * 13            # weight_jet_estimation[r]
# T1, the indexing case: rate 0 sees no flows, rate 2 is stored at half the size; five segments over two runs.  With 12 iterations at most and a bound
# step of 1e-3 one of the five segments stops early (tests/test_track_inputs.py)
T1 = Case("T1", 40, 24, 1, 2, (1, 2, 4), 1, scaled={2: (20, 12)}, seeds=(11, 12, 13, 14, 15), n=3, trws_max_iter=12, trws_eps=1e-3)
# T2, the pitch / offset case: row pitch 44 for 42 columns, xy_start 1, xy_incr 3
T2 = Case("T2", 42, 25, 2, 3, (3, 6), 0, seeds=(21, 22), n=2)


def segment(case, seed):
    """-> dict: flows[r] = (fu, fv, bu, bv) fp32 (r_Jets, sh, stride), occ[r] = raw uint8 occlusion images of that shape, frames fp32 (Jets + 1, 3, h, stride)"""
    rng = np.random.default_rng(seed)
    total = np.array([2.0, 1.2]) * rng.uniform(0.8, 1.2, 2) * rng.choice([-1, 1], 2)
    phase = rng.uniform(0, 2 * np.pi, 4)
    common = (rng.uniform(0.15, 0.7), rng.uniform(0.15, 0.7))           # centre of the rectangle every rate loses, as a fraction of the plane
    flows, occ = [], []
    for r in range(case.K):
        sw, sh, stride, rs = case.source(r)
        rJ = case.r_Jets[r]
        scale = 1.0 / float(rs)                                         # a field stored at another size holds that size's pixels
        y, x = np.mgrid[0:sh, 0:sw]
        fx, fy = x / sw, y / sh
        off = rng.uniform(-0.6, 0.6, 2)
        own = (rng.uniform(0.1, 0.6), rng.uniform(0.1, 0.6))
        f = np.full((4, rJ, sh, stride), PAD, F32)
        o = np.zeros((rJ, sh, stride), np.uint8)
        for k in range(rJ):
            u = (total[0] + off[0] + 0.5 * np.sin(2 * np.pi * fx + phase[0] + 0.3 * k) * np.cos(2 * np.pi * fy + phase[1])) / rJ * scale
            v = (total[1] + off[1] + 0.5 * np.cos(2 * np.pi * fx + phase[2]) * np.sin(2 * np.pi * fy + phase[3] + 0.3 * k)) / rJ * scale
            bu, bv = -u, -v
            if k == 0:                                                  # the contradiction: an error of 3 target pixels
                for cx, cy, ex, ey in ((own[0], own[1], 0.3, 0.35), (common[0], common[1], 0.12, 0.2)):
                    bad = (fx >= cx) & (fx < cx + ex) & (fy >= cy) & (fy < cy + ey)
                    bu = np.where(bad, bu + 3.0 * scale, bu)
            f[0, k, :, :sw], f[1, k, :, :sw], f[2, k, :, :sw], f[3, k, :, :sw] = u, v, bu, bv
            if k == rJ - 1:                                             # an occluded block in the last step
                o[k, :, :sw] = np.where((fx > 0.8) & (fy < 0.3 + 0.1 * r), 255, 0)
        flows.append(tuple(f))
        occ.append(o)
    y, x = np.mgrid[0:case.h, 0:case.w]
    frames = np.full((case.Jets + 1, 3, case.h, case.stride), PAD, F32)
    tex = rng.uniform(0.15, 0.45, (3, 2))
    for t in range(case.Jets + 1):
        sx, sy = x - total[0] * t / case.Jets, y - total[1] * t / case.Jets     # the texture moves with the segment's translation
        for c in range(3):
            frames[t, c, :, :case.w] = np.sin(tex[c, 0] * sx + c) * np.cos(tex[c, 1] * sy - c) + 0.05 * rng.standard_normal((case.h, case.w))
    return dict(flows=flows, occ=occ, frames=frames)


def restate(oracle, case, seg, use_occlusions=False, discard=True):
    """one segment through the restatements: {"rate": [dict(u, v, tracked, energy, occ_bits)], "best", "occluded": [..], "fused": fuse_ref.fuse's dict, "E", "U", "V"}"""
    w, h, J, K = case.w, case.h, case.Jets, case.K
    at_size = []
    for r in range(K):
        sw, sh, stride, rs = case.source(r)
        fu, fv, bu, bv = (a[:, :, :sw] for a in seg["flows"][r])
        if r in case.scaled:
            f = [resample_flow(fu[k], fv[k], rs) for k in range(fu.shape[0])]
            b = [resample_flow(bu[k], bv[k], rs) for k in range(fu.shape[0])]
            fu, fv, bu, bv = (np.stack([q[0] for q in f]), np.stack([q[1] for q in f]), np.stack([q[0] for q in b]), np.stack([q[1] for q in b]))
        masks = np.stack([decode_occlusion_scaled(g[:, :sw], rs) for g in seg["occ"][r]]) if use_occlusions else None
        at_size.append((fu, fv, bu, bv, masks))
    full = orc.aligned_zeros(seg["frames"].shape)                       # the 5-tap derivatives on the strided planes, padding zero
    full[..., :w] = seg["frames"][..., :w]
    dx, dy = (np.ascontiguousarray(d[..., :w]) for d in derivatives(oracle, full, w))
    stack = np.ascontiguousarray(full[..., :w])
    U, V = np.zeros((K, J, case.gh, case.gw)), np.zeros((K, J, case.gh, case.gw))
    E = np.full((K, case.gh, case.gw), np.inf)
    O = np.zeros((K, case.gh, case.gw), np.uint64)
    rates = []
    for r in range(K):
        fu, fv, bu, bv, masks = at_size[r]
        au, av, tr = accumulate(fu, fv, bu, bv, masks, EPSILON, case.skip, discard)
        flows = at_size[case.min_fps_idx][:4] if r >= case.min_fps_idx else None
        e, b, terms = energies(EnergyRefParams(skip=case.skip, weight=WEIGHTS[r]), case.r_Jets[r], au, av, tr, stack, dx, dy, flows)
        E[r], O[r] = e, b
        U[r][:, terms["hy"], terms["hx"]] = terms["U"]
        V[r][:, terms["hy"], terms["hx"]] = terms["V"]
        rates.append(dict(u=au[-1], v=av[-1], tracked=tr, energy=e, occ_bits=b))
    best, occluded = best_and_occluded(E, O)
    fused = fr.fuse(U, V, E, O, fr.smoothness_weight(oracle, full[0], w), fr.Params(trws_max_iter=case.trws_max_iter, trws_eps=case.trws_eps, skip=case.skip), w)
    return dict(rate=rates, best=best, occluded=occluded, fused=fused, E=E, U=U, V=V)


def best_and_occluded(E, O):
    """the accumulate program's host loop over the rates: best = the rate of the lowest fp32 energy, strict, so ties keep the lower rate; 255 for none;
    occluded = the popcount of each rate's occlusion word.  E (K, gh, gw) float64, O (K, gh, gw) uint64"""
    best_e = np.full(E.shape[1:], np.inf, F32)
    best = np.full(E.shape[1:], 255, np.uint8)
    for r in range(E.shape[0]):
        ef = E[r].astype(F32)
        win = ef < best_e
        best_e[win], best[win] = ef[win], r
    return best, [fr.popcount(O[r]).astype(np.uint8) for r in range(E.shape[0])]
