"""dense_tracking's unary hypothesis energies restated afresh in float64 numpy (reference dense_tracking.cpp:1219-1257): adaptFPS (utils/hypothesis.h:136-175),
setOcclusions (utils/hypothesis.cpp:172-215), addJC (dense_tracking.cpp:176-232), addBCGC (:240-349), addOC (:351-365) and the fp32 sum of the four terms.

Two forms:
  energies()         vectorised over the hypotheses (and their neighbours), with switches that turn each quirk of the reference off (QUIRKS); it also
                     returns the intermediate terms so that the hand-worked cases can look at them,
  energies_scalar()  a plain transliteration, hypothesis by hypothesis in the reference's loop order, for small sizes.
Inputs: acc_u, acc_v (r_Jets, gh, gw) float64 and tracked (gh, gw) as accumulateConsistentBatches leaves them (tests/accum_ref.py); frames, dx, dy
(Jets + 1, 3, h, w) fp32 with the channels c1, c2, c3; flows None (the empty Mats of a rate before acc_min_fps) or (fu, fv, bu, bv), (Jets, h, w) fp32.
Every double operation is evaluated on its own, in the order written; fp32 roundings are np.float32 conversions, as the reference's float types make them.
"""
import numpy as np

from accum_ref import grid

QUIRKS = ("float_skip", "cv_continue", "visible_hole", "offx_outer", "empty_flows", "fp32_sum", "edge_weight", "channel_order")

# what the reference's statements do with values no smooth trajectory reaches (tests/test_track_value_ranges.py pins them): a tap of weight zero is still
# multiplied (0 * Inf = NaN, utils.h:216 / utils.cpp:441-444), addJC stops at the first step beyond UNKNOWN_FLOW_THRESH (dense_tracking.cpp:190), and a
# NaN position fails every `>= 0 && < extent` test
VALUE_QUIRKS = ("zero_weight_tap", "unknown_break", "nan_outside")

F32 = np.float32


class Params:
    """sfa_energy_params: setDefault's values (dense_tracking.cpp:118-165), weight 0, skip 1"""
    def __init__(self, **kw):
        self.acc_jc, self.acc_bc, self.acc_gc, self.acc_occ = F32(1.0), F32(0.1), F32(1.0), F32(500.0)
        self.acc_cv, self.acc_temporal_occ = 0.0, 10.0
        self.occlusion_threshold, self.occlusion_fb_threshold = F32(5.0), F32(5.0)
        self.penalty, self.penalty_eps, self.weight, self.skip = 1, 0.001, F32(0.0), 1
        for k, v in kw.items():
            assert hasattr(self, k), k
            cur = getattr(self, k)
            setattr(self, k, F32(v) if isinstance(cur, F32) else type(cur)(v))

    def to_c(self, sfa):
        return sfa.energy_params(**{k: (float(v) if isinstance(v, (float, F32)) else v) for k, v in vars(self).items()})


def flows_for_rate(r, min_fps_idx, flows, off=()):
    """forward_flow / backward_flow are filled only while rate acc_min_fps is read (:1148-1151); a rate before it sees empty Mats"""
    if "empty_flows" not in off and r < min_fps_idx:
        return None
    return flows


def derivatives(oracle, frames, w):
    """dx, dy of (Jets + 1, 3, h, stride) fp32 frames: color_image_convolve_hv with {0, -8/12, 1/12} (:918-925), the pinned CPU oracle's 5-tap"""
    dx, dy = np.zeros_like(frames), np.zeros_like(frames)
    for f in range(frames.shape[0]):
        for c in range(3):
            src = np.ascontiguousarray(frames[f, c])
            dx[f, c] = oracle.convolve(src, w, 2, True)
            dy[f, c] = oracle.convolve(src, w, 2, False)
    return dx, dy


def adapt_table(F, nF, off=()):
    """adaptFPS(nF) of F steps (hypothesis.h:139-171): (up, skip, off[i], offm1[i]) in float arithmetic"""
    if "float_skip" in off:
        skip = F / nF
        up = skip >= 1
        o = [int(i * skip + (skip - 1)) if up else int(np.floor(i * skip)) for i in range(nF)]
        m = [0 if up else int(np.floor((i - 1) * skip)) for i in range(nF)]
        return up, skip, o, m
    skip = F32(F32(1.0) * F32(F)) / F32(nF)
    up = bool(skip >= 1)
    o = [int(F32(F32(i) * skip) + F32(skip - F32(1))) if up else int(np.floor(F32(F32(i) * skip))) for i in range(nF)]
    m = [0 if up else int(np.floor(F32(F32(i - 1) * skip))) for i in range(nF)]
    return up, skip, o, m


def phi(kind, eps, xsq):
    """PenaltyFunction::apply(float) -> float; epsilon_sq = e * e in float, kept in a double; sqrt / log in double (penalty_functions/*.h)"""
    xsq = F32(xsq)
    e = F32(eps)
    esq = np.float64(F32(e * e))
    if kind == 0:
        return xsq
    if kind == 1:
        return F32(np.sqrt(np.float64(xsq) + esq))
    return F32(np.log(1 + 0.5 * np.float64(xsq) / esq))


def _bil(p, x, y, edge_weight=True, zero_taps=True):
    """bilinearInterp (utils.h:182-217 / utils.cpp:415-446) at arrays of in-image points of an (h, w) fp32 plane.  Every index formed is asserted to lie in
    the plane (numpy would wrap a negative one silently).  zero_taps=False: the slip that leaves a tap of weight zero out of the sum"""
    h, w = p.shape
    assert np.all((x >= 0) & (x < w) & (y >= 0) & (y < h)), "bilinearInterp outside the plane"      # NaN fails it as well
    x0, y0 = x.astype(np.int64), y.astype(np.int64)
    if edge_weight:
        wx = np.where(x0 + 1 < w, x - x0, 0.0)
        wy = np.where(y0 + 1 < h, y - y0, 0.0)
        x1 = np.where(x0 + 1 < w, x0 + 1, x0)
        y1 = np.where(y0 + 1 < h, y0 + 1, y0)
    else:                                                       # the slip: the neighbour wraps round to column / row 0
        wx, wy = x - x0, y - y0
        x1, y1 = (x0 + 1) % w, (y0 + 1) % h
    assert np.all((x0 >= 0) & (x0 < w) & (x1 >= 0) & (x1 < w) & (y0 >= 0) & (y0 < h) & (y1 >= 0) & (y1 < h)), "tap outside the plane"
    d = p.astype(np.float64)
    if not zero_taps:
        def term(wgt, val):
            return np.where(wgt == 0, 0.0, wgt * val)
        return term((1 - wy) * (1 - wx), d[y0, x0]) + term((1 - wy) * wx, d[y0, x1]) + term(wy * (1 - wx), d[y1, x0]) + term(wy * wx, d[y1, x1])
    return (1 - wy) * (1 - wx) * d[y0, x0] + (1 - wy) * wx * d[y0, x1] + wy * (1 - wx) * d[y1, x0] + wy * wx * d[y1, x1]


def energies(p, r_Jets, acc_u, acc_v, tracked, frames, dx, dy, flows, off=()):
    """-> energy (gh, gw) float64 (+Inf where tracked != r_Jets), occ_bits (gh, gw) uint64 and a dict of intermediate terms over the hypotheses"""
    off = set(off)
    assert off <= set(QUIRKS) | set(VALUE_QUIRKS), off
    J = frames.shape[0] - 1
    h, w = frames.shape[2:]
    gw, gh, incr, start = grid(w, h, p.skip)
    ew = "edge_weight" not in off
    zt = "zero_weight_tap" not in off

    def lookup(pl, x, y, ew_):                                   # every bilinearInterp below, with this call's switches
        if "nan_outside" in off:
            x, y = np.nan_to_num(x), np.nan_to_num(y)
        return _bil(pl, x, y, ew_, zt)
    hy, hx = np.nonzero(tracked == r_Jets)
    H = len(hy)
    px, py = (hx * incr + start).astype(np.float64), (hy * incr + start).astype(np.float64)
    # ---- adaptFPS
    up, skip, o, m = adapt_table(r_Jets, J, off)
    AU, AV = acc_u[:, hy, hx], acc_v[:, hy, hx]                     # (r_Jets, H)
    U, V = np.zeros((J, H)), np.zeros((J, H))
    for i in range(J):
        if up:
            U[i], V[i] = AU[o[i]], AV[o[i]]
        else:
            lx, ly = np.zeros(H), np.zeros(H)
            if i > 0:
                lx, ly = AU[m[i]], AV[m[i]]
                if "float_skip" not in off:                     # last_x, last_y are float
                    lx, ly = lx.astype(F32).astype(np.float64), ly.astype(F32).astype(np.float64)
            U[i] = lx + np.float64(skip) * (AU[o[i]] - lx)
            V[i] = ly + np.float64(skip) * (AV[o[i]] - ly)
    # ---- setOcclusions
    fw, fh = (w, h) if flows is not None else (0, 0)
    occ = np.zeros((J + 1, H), bool)

    def inside(x, y, W, Hh):
        if "nan_outside" in off:                                # the slip: `!(outside)`, which lets a NaN position through (read at pixel 0 here)
            return ~((y < 0) | (y >= Hh) | (x < 0) | (x >= W)) & (W > 0)
        return (y >= 0) & (y < Hh) & (x >= 0) & (x < W)

    for t in range(J):
        u_tm1 = 0 + U[t - 1] if t > 0 else np.zeros(H)
        v_tm1 = 0 + V[t - 1] if t > 0 else np.zeros(H)
        xm, ym = px + u_tm1, py + v_tm1
        o_t = np.ones(H, bool)
        a = ~occ[t] & inside(xm, ym, fw, fh)
        if a.any():
            fu, fv, bu, bv = (q[t] for q in flows)
            Fx, Fy = lookup(fu, xm[a], ym[a], ew), lookup(fv, xm[a], ym[a], ew)
            ysq = V[t][a] - v_tm1[a] - Fy
            xsq = U[t][a] - u_tm1[a] - Fx
            xt, yt = px[a] + U[t][a], py[a] + V[t][a]
            b = inside(xt, yt, fw, fh)
            ok = np.zeros(a.sum(), bool)
            if b.any():
                bFx, bFy = lookup(bu, xt[b], yt[b], ew), lookup(bv, xt[b], yt[b], ew)
                fby, fbx = bFy + Fy[b], bFx + Fx[b]
                ok[b] = (np.sqrt(fby * fby + fbx * fbx) < np.float64(p.occlusion_fb_threshold)) & (
                    np.sqrt(ysq[b] * ysq[b] + xsq[b] * xsq[b]) < np.float64(p.occlusion_threshold))
            o_t[a] = ~ok
        occ[t + 1] = occ[t] | o_t
    # ---- addJC
    jen, cven, contr = np.zeros(H), np.zeros(H), np.zeros(H, np.int64)
    alive = np.ones(H, bool)
    for j in range(J):
        u_j, v_j = U[j], V[j]
        u_jm1, v_jm1 = (U[j - 1], V[j - 1]) if j > 0 else (np.zeros(H), np.zeros(H))
        if "unknown_break" not in off:
            alive &= ~((u_j > 1e9) | (v_j > 1e9))               # break
        xi, yi = px + u_jm1, py + v_jm1
        ins = alive & inside(xi, yi, fw, fh)
        skipped = ins & (occ[j] | occ[j + 1])
        use = ins & ~skipped
        if use.any():
            Ix, Iy = lookup(flows[0][j], xi[use], yi[use], ew), lookup(flows[1][j], xi[use], yi[use], ew)
            du, dv = u_j[use] - u_jm1[use] - Ix, v_j[use] - v_jm1[use] - Iy
            arg = (du * du + dv * dv).astype(F32)
            jen[use] = jen[use] + 0.5 * np.array([np.float64(phi(p.penalty, p.penalty_eps, x)) for x in arg])
            contr[use] += 1
        u_jp1, v_jp1 = (U[j + 1], V[j + 1]) if j + 1 < J else (np.zeros(H), np.zeros(H))
        us, vs = 2 * u_j - u_jm1 - u_jp1, 2 * v_j - v_jm1 - v_jp1
        us, vs = us * us, vs * vs
        cvm = alive & ~skipped if "cv_continue" not in off else alive   # the `continue` skips the constant-velocity term too
        cven[cvm] = cven[cvm] + np.sqrt(us[cvm] + vs[cvm])
    jen = np.where(contr > 0, jen / np.maximum(contr, 1), jen)
    jc = (np.float64(p.acc_jc) * jen + p.acc_cv * cven).astype(F32)
    # ---- addOC
    noc = occ.sum(0)
    chg = (occ[:-1] != occ[1:]).sum(0)
    oc = (np.float64(p.acc_occ) * noc + p.acc_temporal_occ * chg).astype(F32)
    # ---- addBCGC, one row per (hypothesis, neighbour)
    r = int(F32(0.5) * F32(p.skip + 1))
    side = 2 * r + 1
    ks = np.arange(side * side)
    a_, b_ = ks // side, ks % side                               # off_x outer, off_y inner
    if "offx_outer" in off:
        a_, b_ = b_, a_
    ox = (px[:, None] - r + a_[None, :]).astype(np.int64)        # (H, NN)
    oy = (py[:, None] - r + b_[None, :]).astype(np.int64)
    valid = (ox >= 0) & (ox < w) & (oy >= 0) & (oy < h)
    hi, ki = np.nonzero(valid)
    X0, Y0 = ox[hi, ki], oy[hi, ki]
    R = len(hi)
    chans = (2, 1, 0) if "channel_order" not in off else (0, 1, 2)
    ins = np.zeros((J + 1, R), bool)
    ins[0] = True
    for j in range(1, J + 1):
        ins[j] = inside(X0 + U[j - 1][hi], Y0 + V[j - 1][hi], w, h)
    vis = ins.sum(0)
    vals = np.zeros((J + 1, 9, R))
    for j in range(J + 1):
        if j == 0:
            for q, pl in enumerate((frames, dx, dy)):
                for c, ch in enumerate(chans):
                    vals[0, 3 * q + c] = pl[0, ch][Y0, X0].astype(np.float64)
        else:
            sel = ins[j]
            xj, yj = X0[sel] + U[j - 1][hi][sel], Y0[sel] + V[j - 1][hi][sel]
            for q, pl in enumerate((frames, dx, dy)):
                for c, ch in enumerate(chans):
                    vals[j, 3 * q + c, sel] = lookup(pl[j, ch], xj, yj, ew)
    occR = occ[:, hi]
    bcw, gcw = np.float64(p.acc_bc) * 0.3334, np.float64(p.acc_gc) * 0.3334
    e_p, cnt = np.zeros(R), np.zeros(R, np.int64)
    for i in range(J + 1):
        for j in range(i + 1, J + 1):
            take = ins[i] & ins[j] & ~occR[i] & ~occR[j]
            if "visible_hole" not in off:
                take &= j < vis                                  # i < j < visible
            if not take.any():
                continue
            d = np.abs(vals[i] - vals[j])
            bc = (d[0] + d[1]) + d[2]
            gc = ((((d[3] + d[4]) + d[5]) + d[6]) + d[7]) + d[8]
            e_p = np.where(take, e_p + bcw * bc, e_p)
            e_p = np.where(take, e_p + gcw * gc, e_p)
            cnt += take
    e_p = np.where(cnt > 0, e_p / np.maximum(cnt, 1), e_p)
    ep_full = np.full((H, side * side), np.nan)
    ep_full[hi, ki] = e_p
    wen, neighs = np.zeros(H), np.zeros(H)
    for k in range(side * side):                                 # in the order of the loops
        v = valid[:, k]
        wen[v] = wen[v] + ep_full[v, k]
        neighs[v] += 1
    wen = np.where(neighs > 0, wen / np.maximum(neighs, 1), wen)
    bcgc = wen.astype(F32)
    # ---- the sum
    if "fp32_sum" in off:
        tot = ((jc.astype(np.float64) + bcgc.astype(np.float64)) + oc.astype(np.float64)) + np.float64(p.weight)
    else:
        tot = (((jc + bcgc).astype(F32) + oc).astype(F32) + F32(p.weight)).astype(F32).astype(np.float64)
    energy = np.full((gh, gw), np.inf)
    energy[hy, hx] = tot
    bits = np.zeros((gh, gw), np.uint64)
    word = np.zeros(H, np.uint64)
    for t in range(J + 1):
        word |= occ[t].astype(np.uint64) << np.uint64(t)
    bits[hy, hx] = word
    terms = dict(hy=hy, hx=hx, U=U, V=V, occ=occ, jc=jc, oc=oc, bcgc=bcgc, bcgc_double=wen, ep=ep_full, contribution=contr, cv=cven)
    return energy, bits, terms


def energies_scalar(p, r_Jets, acc_u, acc_v, tracked, frames, dx, dy, flows):
    """the same, hypothesis by hypothesis in the reference's statement order"""
    J = frames.shape[0] - 1
    h, w = frames.shape[2:]
    gw, gh, incr, start = grid(w, h, p.skip)
    energy = np.full((gh, gw), np.inf)
    bits = np.zeros((gh, gw), np.uint64)
    fw, fh = (w, h) if flows is not None else (0, 0)
    up, skip, o, m = adapt_table(r_Jets, J)
    r = int(F32(0.5) * F32(p.skip + 1))

    def bil(pl, x, y):
        return float(_bil(pl, np.array([x]), np.array([y]))[0])

    def inside(x, y, W, Hh):
        return y >= 0 and y < Hh and x >= 0 and x < W

    for y in range(gh):
        for x in range(gw):
            if tracked[y, x] != r_Jets:
                continue
            PX, PY = float(x * incr + start), float(y * incr + start)
            fx, fy = [float(acc_u[f, y, x]) for f in range(r_Jets)], [float(acc_v[f, y, x]) for f in range(r_Jets)]
            U, V = [0.0] * J, [0.0] * J
            for i in range(J):
                if up:
                    U[i], V[i] = fx[o[i]], fy[o[i]]
                else:
                    lx = ly = 0.0
                    if i > 0:
                        lx, ly = float(F32(fx[m[i]])), float(F32(fy[m[i]]))
                    U[i] = lx + float(skip) * (fx[o[i]] - lx)
                    V[i] = ly + float(skip) * (fy[o[i]] - ly)
            occ = [0] * (J + 1)
            for t in range(J):
                if occ[t] == 1:
                    occ[t + 1] = 1
                    continue
                u_tm1 = v_tm1 = 0.0
                if t > 0:
                    u_tm1 += U[t - 1]
                    v_tm1 += V[t - 1]
                xm, ym = PX + u_tm1, PY + v_tm1
                occ[t + 1] = 1
                if inside(xm, ym, fw, fh):
                    Fx, Fy = bil(flows[0][t], xm, ym), bil(flows[1][t], xm, ym)
                    ysq, xsq = V[t] - v_tm1 - Fy, U[t] - u_tm1 - Fx
                    xt, yt = PX + U[t], PY + V[t]
                    if inside(xt, yt, fw, fh):
                        bFx, bFy = bil(flows[2][t], xt, yt), bil(flows[3][t], xt, yt)
                        fby, fbx = bFy + Fy, bFx + Fx
                        if np.sqrt(fby * fby + fbx * fbx) < float(p.occlusion_fb_threshold) and np.sqrt(ysq * ysq + xsq * xsq) < float(p.occlusion_threshold):
                            occ[t + 1] = 0
            # addJC
            jen = cven = 0.0
            contribution = 0
            for j in range(J):
                u_j, v_j = U[j], V[j]
                u_jm1 = v_jm1 = 0.0
                if j > 0:
                    u_jm1, v_jm1 = U[j - 1], V[j - 1]
                if u_j > 1e9 or v_j > 1e9:
                    break
                if inside(PX + u_jm1, PY + v_jm1, fw, fh):
                    if occ[j] == 1 or occ[j + 1] == 1:
                        continue
                    Ix, Iy = bil(flows[0][j], PX + u_jm1, PY + v_jm1), bil(flows[1][j], PX + u_jm1, PY + v_jm1)
                    jen += 0.5 * float(phi(p.penalty, p.penalty_eps, F32((u_j - u_jm1 - Ix) * (u_j - u_jm1 - Ix) + (v_j - v_jm1 - Iy) * (v_j - v_jm1 - Iy))))
                    contribution += 1
                u_jp1 = v_jp1 = 0.0
                if j + 1 < J:
                    u_jp1, v_jp1 = U[j + 1], V[j + 1]
                us, vs = 2 * u_j - u_jm1 - u_jp1, 2 * v_j - v_jm1 - v_jp1
                us *= us
                vs *= vs
                cven += float(np.sqrt(us + vs))
            if contribution > 0:
                jen /= contribution
            jc = F32(float(p.acc_jc) * jen + p.acc_cv * cven)
            # addBCGC
            wen = neighs = 0.0
            for off_x in range(int(PX - r), int(PX + r) + 1):
                for off_y in range(int(PY - r), int(PY + r) + 1):
                    if off_x < 0 or off_x >= w or off_y < 0 or off_y >= h:
                        continue
                    visible = 0
                    I = np.zeros((9, J + 1))
                    for j in range(J + 1):
                        if j == 0:
                            for q, pl in enumerate((frames, dx, dy)):
                                for c, ch in enumerate((2, 1, 0)):
                                    I[3 * q + c, 0] = float(pl[0, ch, off_y, off_x])
                            visible += 1
                        else:
                            xj, yj = off_x + U[j - 1], off_y + V[j - 1]
                            if inside(xj, yj, w, h):
                                for q, pl in enumerate((frames, dx, dy)):
                                    for c, ch in enumerate((2, 1, 0)):
                                        I[3 * q + c, j] = bil(pl[j, ch], xj, yj)
                                visible += 1
                    contribution = 0
                    e_p = 0.0
                    for i in range(visible):
                        for j in range(i + 1, visible):
                            xi, yi = float(off_x), float(off_y)
                            if i > 0:
                                xi += U[i - 1]
                                yi += V[i - 1]
                            xj, yj = off_x + U[j - 1], off_y + V[j - 1]
                            if inside(xi, yi, w, h) and inside(xj, yj, w, h):
                                if occ[i] == 1 or occ[j] == 1:
                                    continue
                                d = [abs(I[k, i] - I[k, j]) for k in range(9)]
                                e_p += float(p.acc_bc) * 0.3334 * (d[0] + d[1] + d[2])
                                e_p += float(p.acc_gc) * 0.3334 * (d[3] + d[4] + d[5] + d[6] + d[7] + d[8])
                                contribution += 1
                    if contribution > 0:
                        e_p /= contribution
                    wen += e_p
                    neighs += 1
            if neighs > 0:
                wen /= neighs
            bcgc = F32(wen)
            # addOC
            occlusions = change = 0
            for i in range(J + 1):
                occlusions += occ[i]
                if i < J and occ[i] != occ[i + 1]:
                    change += 1
            oc = F32(float(p.acc_occ) * occlusions + p.acc_temporal_occ * change)
            energy[y, x] = float(F32(F32(F32(jc + bcgc) + oc) + p.weight))
            bits[y, x] = np.uint64(sum(b << t for t, b in enumerate(occ)))
    return energy, bits
