"""dense_tracking's fusion of the trajectory hypotheses restated afresh in float64 numpy (reference dense_tracking.cpp:1588-1905): the smoothness
weight (computeSmoothnessWeight, :367-405), the per-pixel sort and non-maximum suppression (:1592-1630), the pairwise potentials (:1716-1797) with
hypothesis::distance (utils/hypothesis.cpp:223-285), and TRW-S in sequential raster order as INTEGRATION.md 4c defines it.

TRW-S comes in two forms that must give the same bits:
  trws_scalar()  node by node in raster order, label by label,
  trws_diag()    vectorised over the nodes of one anti-diagonal x + y = d (what the GPU kernel does).
Every double operation is evaluated on its own, in the order written; fp32 roundings are np.float32 conversions.  Sums of many terms run in a
fixed sequential order (a Python loop or np.cumsum, never np.sum, which is pairwise).

A grid MRF here: theta, a list over the gw * gh nodes of float64 arrays (empty = no node); PR[p], PD[p]: the (len(theta[p]), len(theta[t])) cost
of the right / down edge of node p (None where either end is no node).
"""
import struct
from decimal import Decimal, getcontext

import numpy as np

from accum_ref import grid

QUIRKS = ("nms_break", "float_score", "img_norm_keys", "acc_unnormalised", "occ_jets_plus_1", "fp32_weight_sum", "float_dist")

# this project's own rule (the reference's std::sort on a NaN score is undefined): a hypothesis whose energy is NaN is absent, as +Inf is
VALUE_QUIRKS = ("nan_energy_absent",)

F32 = np.float32
INF = np.inf
UNKNOWN_FLOW = 1e10


class Params:
    """sfa_fuse_params: setDefault's values (dense_tracking.cpp:136-152), skip 1"""
    def __init__(self, **kw):
        self.acc_beta, self.acc_spatial_occ, self.traj_sim_method, self.traj_sim_thres = 10.0, 10.0, 1, 0.1
        self.trws_eps, self.trws_max_iter, self.skip = 1e-5, 10, 1
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, type(getattr(self, k))(v))

    def to_c(self, sfa):
        return sfa.fuse_params(**vars(self))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# smoothness weight
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def program_norm(cfg, off=()):
    """the statistics the smoothness weight de-normalises with: dense_tracking reads img_norm_avg_* / img_norm_std_* with defaults 0 / 1 (:971-972),
    keys nothing publishes (normalize() publishes slow_flow_img_norm_*, variational_mt.cpp:79-84)"""
    pre = "slow_flow_img_norm_" if "img_norm_keys" in off else "img_norm_"
    avg = [float(cfg.get(pre + "avg_%d" % k, 0)) for k in (1, 2, 3)]
    std = [float(cfg.get(pre + "std_%d" % k, 1)) for k in (1, 2, 3)]
    return avg, std


def _exp_table():
    getcontext().prec = 60
    T = []
    for i in range(32):
        v = float(Decimal(2) ** (Decimal(i) / Decimal(32)))
        T.append((struct.unpack("<Q", struct.pack("<d", v))[0] - (i << 47)) & 0xFFFFFFFFFFFFFFFF)
    return np.array(T, dtype=np.uint64)


_T = None


def expf(x):
    """glibc's expf algorithm (N = 32 table, degree-3 polynomial in fp64), the formulation the device uses"""
    global _T
    if _T is None:
        _T = _exp_table()
    x = np.asarray(x, dtype=F32)
    inv = float.fromhex("0x1.71547652b82fep+0") * 32
    c0, c1, c2 = float.fromhex("0x1.c6af84b912394p-5") / 32 / 32 / 32, float.fromhex("0x1.ebfce50fac4f3p-3") / 32 / 32, float.fromhex("0x1.62e42ff0c52d6p-1") / 32
    shift = float.fromhex("0x1.8p+52")
    z = inv * x.astype(np.float64)
    kd = z + shift
    ki = kd.view(np.uint64)
    kd = kd - shift
    r = z - kd
    t = _T[(ki % np.uint64(32)).astype(np.int64)] + (ki << np.uint64(47))
    s = t.view(np.float64)
    zz = c0 * r + c1
    r2 = r * r
    y = c2 * r + 1
    y = zz * r2 + y
    y = y * s
    out = y.astype(F32)
    out = np.where(x < F32(float.fromhex("-0x1.9fe368p6")), F32(0), out)
    return out


def smoothness_weight(oracle, frame, w, avg=(0, 0, 0), std=(1, 1, 1), hbit=0, coef=5.0):
    """computeSmoothnessWeight of a (3, h, stride) fp32 frame: packed (h, w) fp32.  The 5-tap derivatives are the pinned CPU oracle's."""
    c1, c2, c3 = (frame[k].astype(F32) for k in range(3))
    a, s = [F32(v) for v in avg], [F32(v) for v in std]
    lum = (F32(0.299) * (c1 * s[0] + a[0]) + F32(0.587) * (c2 * s[1] + a[1])) + F32(0.114) * (c3 * s[2] + a[2])
    lum = (lum / (F32(65535.0) if hbit else F32(255.0))).astype(F32)
    lum = np.ascontiguousarray(lum)
    lx = oracle.convolve(lum, w, 2, True)
    ly = oracle.convolve(lum, w, 2, False)
    n = F32(-coef) * np.sqrt(lx * lx + ly * ly).astype(F32)
    return (F32(0.5) * expf(n)).astype(F32)[:, :w]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# hypotheses: distance, sort + NMS, pairwise
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def distance(ua, va, ub, vb, method, off=()):
    """hypothesis::distance of two adapted hypotheses (first 0, length Jets): arrays (..., Jets); the sum runs over the steps in order"""
    J = ua.shape[-1]
    s = np.zeros(ua.shape[:-1])
    for f in range(J):
        if method == 1:
            ysq = va[..., f] - vb[..., f]
            xsq = ua[..., f] - ub[..., f]
            s = s + np.sqrt(xsq * xsq + ysq * ysq) / (f + 1)
        else:
            pa_u = ua[..., f - 1] if f > 0 else 0.0
            pa_v = va[..., f - 1] if f > 0 else 0.0
            pb_u = ub[..., f - 1] if f > 0 else 0.0
            pb_v = vb[..., f - 1] if f > 0 else 0.0
            ysq = (va[..., f] - pa_v) - (vb[..., f] - pb_v)
            xsq = (ua[..., f] - pa_u) - (ub[..., f] - pb_u)
            s = s + np.sqrt(xsq * xsq + ysq * ysq)
    if method != 1 or "acc_unnormalised" in off:
        s = s / J
    return s


def labels(U, V, energy, method, thres, off=()):
    """one segment: U, V (K, Jets, gh, gw), energy (K, gh, gw).  Returns lab, a list over the gh * gw pixels of slot lists (sorted, after NMS).
    Vectorised over the pixels; per pixel the loop of :1609-1626."""
    K, J, gh, gw = U.shape
    N = gh * gw
    Uf, Vf = U.reshape(K, J, N), V.reshape(K, J, N)
    e = energy.reshape(K, N).T
    absent = ~(e < INF)                                                         # +Inf: no hypothesis; a NaN energy is absent too
    if "nan_energy_absent" in off:                                              # the rule before: only +Inf is absent
        absent = e == INF
    with np.errstate(over="ignore"):                                            # (float) of a score beyond FLT_MAX is +-Inf, as in C
        key32 = e.astype(F32).astype(np.float64)
    key = e if "float_score" in off else key32
    slots = np.broadcast_to(np.arange(K), (N, K))
    order = np.lexsort((slots, np.where(absent, 0, key), absent), axis=-1)      # present first, by score, ties: the lower slot
    m = (~absent).sum(1)
    kept = np.full((N, K), -1)
    kept[:, 0] = order[:, 0]
    nk = (m > 0).astype(int)
    alive = np.ones(N, bool)
    pix = np.arange(N)
    for c in range(1, K):
        cand = order[:, c]
        act = (c < m) & alive
        discard = np.zeros(N, bool)
        for q in range(K):
            qa = pix[act & (q < nk)]
            if not len(qa):
                continue
            kq = kept[qa, q]
            d = distance(Uf[cand[qa], :, qa], Vf[cand[qa], :, qa], Uf[kq, :, qa], Vf[kq, :, qa], method, off)
            discard[qa] |= d < thres
        if "nms_break" not in off:
            alive &= ~(act & discard)
        add = pix[act & ~discard]
        kept[add, nk[add]] = cand[add]
        nk[add] += 1
    return [[int(k) for k in kept[p, :nk[p]]] for p in range(N)]


def popcount(x):
    x = np.ascontiguousarray(x, dtype=np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(-1)


def pair_cost(ua, va, oa, ub, vb, ob, w1, w2, J, p, off=(), trace=None):
    """P(h1, h2) of :1752-1766 for arrays of pairs.  trace: a list that receives the distances before their rounding to float"""
    dist = distance(ua, va, ub, vb, p.traj_sim_method, off)
    if trace is not None:
        trace.append(dist.copy())
    if "float_dist" not in off:
        with np.errstate(over="ignore"):                                    # (float) of a distance beyond FLT_MAX is +Inf, as in C
            dist = dist.astype(F32).astype(np.float64)
    nb = J + 1 if "occ_jets_plus_1" not in off else J
    smooth = popcount(np.bitwise_xor(oa, ob) & np.uint64((1 << nb) - 1)).astype(np.float64)
    wsum = (np.float64(w1) + np.float64(w2)) if "fp32_weight_sum" in off else (F32(w1) + F32(w2)).astype(np.float64)
    return wsum * (p.acc_beta * dist + p.acc_spatial_occ * smooth)


def pairwise(U, V, occ, weight, lab, p, w, off=(), trace=None):
    """PR, PD of one segment: lists over the pixels of (n1, n2) arrays or None.  All pairs of a direction in one vectorised evaluation."""
    K, J, gh, gw = U.shape
    N = gh * gw
    _, _, incr, start = grid(w, weight.shape[0], p.skip)
    W = weight.reshape(-1).astype(F32)
    Uf, Vf, Of = U.reshape(K, J, N), V.reshape(K, J, N), occ.reshape(K, N)
    out = []
    for dx, dy in ((1, 0), (0, 1)):
        P = [None] * N
        rows = []                                                           # (pixel, t, i, j, slot a, slot b)
        for pi in range(N):
            y, x = divmod(pi, gw)
            if not lab[pi] or x + dx >= gw or y + dy >= gh:
                continue
            t = pi + dx + dy * gw
            if not lab[t]:
                continue
            for i, a in enumerate(lab[pi]):
                for j, b in enumerate(lab[t]):
                    rows.append((pi, t, i, j, a, b))
        if rows:
            r = np.array(rows)
            pi_, t_, a_, b_ = r[:, 0], r[:, 1], r[:, 4], r[:, 5]
            y, x = pi_ // gw, pi_ % gw
            o1 = (y * incr + start) * w + x * incr + start
            o2 = ((y + dy) * incr + start) * w + (x + dx) * incr + start
            assert np.all((o1 >= 0) & (o1 < W.size) & (o2 >= 0) & (o2 < W.size)), "weight lookup outside the plane"
            c = pair_cost(Uf[a_, :, pi_], Vf[a_, :, pi_], Of[a_, pi_], Uf[b_, :, t_], Vf[b_, :, t_], Of[b_, t_], W[o1], W[o2], J, p, off, trace)
            for pi in np.unique(pi_):
                P[pi] = np.zeros((len(lab[pi]), len(lab[pi + dx + dy * gw])))
            for k in range(len(rows)):
                P[pi_[k]][r[k, 2], r[k, 3]] = c[k]
        out.append(P)
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# TRW-S
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _nbrs(theta, gw, gh, p):
    y, x = divmod(p, gw)
    L = p - 1 if x > 0 and len(theta[p - 1]) else None
    Up = p - gw if y > 0 and len(theta[p - gw]) else None
    R = p + 1 if x + 1 < gw and len(theta[p + 1]) else None
    D = p + gw if y + 1 < gh and len(theta[p + gw]) else None
    return L, Up, R, D


def energy_of(theta, PR, PD, gw, gh, x):
    """sum over rows top to bottom, nodes left to right: unary, right edge, down edge"""
    E = 0.0
    for p in range(gw * gh):
        if not len(theta[p]):
            continue
        _, _, R, D = _nbrs(theta, gw, gh, p)
        E = E + theta[p][x[p]]
        if R is not None:
            E = E + PR[p][x[p], x[R]]
        if D is not None:
            E = E + PD[p][x[p], x[D]]
    return E


def trws_scalar(theta, PR, PD, gw, gh, eps, max_iter):
    """returns (labels, energy, bound, iterations); labels -1 where there is no node"""
    N = gw * gh
    M = [[np.zeros(len(theta[p])) for _ in range(4)] for p in range(N)]     # into p from left, up, right, down
    nb = [_nbrs(theta, gw, gh, p) for p in range(N)]
    xcur = [-1] * N
    best, best_x, lb_prev, it_run = None, None, 0.0, 0
    lb = 0.0

    def hat(p):
        th = theta[p].copy()
        for k in range(4):
            if nb[p][k] is not None:
                for i in range(len(th)):
                    th[i] = th[i] + M[p][k][i]
        return th

    def gamma(p):
        L, Up, R, D = nb[p]
        nin, nout = (L is not None) + (Up is not None), (R is not None) + (D is not None)
        return 1.0 / max(nin, nout, 1)

    for it in range(1, max_iter + 1):
        for p in range(N):                                                  # forward
            m = len(theta[p])
            if not m:
                continue
            L, Up, R, D = nb[p]
            th, g = hat(p), gamma(p)
            xs, bv = 0, None
            for i in range(m):
                v = theta[p][i]
                if L is not None:
                    v = v + PR[L][xcur[L], i]
                if Up is not None:
                    v = v + PD[Up][xcur[Up], i]
                if R is not None:
                    v = v + M[p][2][i]
                if D is not None:
                    v = v + M[p][3][i]
                if bv is None or v < bv:
                    bv, xs = v, i
            xcur[p] = xs
            for k, t, P in ((0, R, PR), (1, D, PD)):
                if t is None:
                    continue
                a = [g * th[i] - M[p][2 + k][i] for i in range(m)]
                out = []
                for j in range(len(theta[t])):
                    v = None
                    for i in range(m):
                        c = a[i] + P[p][i, j]
                        if v is None or c < v:
                            v = c
                    out.append(v)
                mn = None
                for v in out:
                    if mn is None or v < mn:
                        mn = v
                M[t][k] = np.array([v - mn for v in out])
        for p in range(N - 1, -1, -1):                                      # backward
            m = len(theta[p])
            if not m:
                continue
            L, Up, R, D = nb[p]
            th, g = hat(p), gamma(p)
            for k, t, P in ((0, L, PR), (1, Up, PD)):
                if t is None:
                    continue
                a = [g * th[i] - M[p][k][i] for i in range(m)]
                out = []
                for j in range(len(theta[t])):
                    v = None
                    for i in range(m):
                        c = a[i] + P[t][j, i]
                        if v is None or c < v:
                            v = c
                    out.append(v)
                mn = None
                for v in out:
                    if mn is None or v < mn:
                        mn = v
                M[t][2 + k] = np.array([v - mn for v in out])
        E, lb = 0.0, 0.0
        for p in range(N):
            m = len(theta[p])
            if not m:
                continue
            L, Up, R, D = nb[p]
            th = hat(p)
            E = E + theta[p][xcur[p]]
            mn = None
            for v in th:
                if mn is None or v < mn:
                    mn = v
            lb = lb + mn
            for k, t, P in ((0, R, PR), (1, D, PD)):
                if t is None:
                    continue
                E = E + P[p][xcur[p], xcur[t]]
                v = None
                for i in range(m):
                    for j in range(len(theta[t])):
                        r = (P[p][i, j] - M[p][2 + k][i]) - M[t][k][j]
                        if v is None or r < v:
                            v = r
                lb = lb + v
        if it == 1 or E < best:
            best, best_x = E, list(xcur)
        it_run = it
        stop = it >= 2 and lb - lb_prev < eps
        lb_prev = lb
        if stop:
            break
    return np.array(best_x), best, lb, it_run


def trws_diag(theta, PR, PD, gw, gh, eps, max_iter):
    """trws_scalar vectorised over the nodes of each anti-diagonal; labels padded to K with +Inf (costs) and 0 (messages)"""
    N = gw * gh
    K = max([len(t) for t in theta] + [1])
    nl = np.array([len(t) for t in theta])
    TH = np.full((N, K), INF)
    for p in range(N):
        TH[p, :nl[p]] = theta[p]
    PRa, PDa = np.full((N, K, K), INF), np.full((N, K, K), INF)
    hasR, hasD = np.zeros(N, bool), np.zeros(N, bool)
    for p in range(N):
        if PR[p] is not None:
            PRa[p, :PR[p].shape[0], :PR[p].shape[1]] = PR[p]
            hasR[p] = True
        if PD[p] is not None:
            PDa[p, :PD[p].shape[0], :PD[p].shape[1]] = PD[p]
            hasD[p] = True
    idx = np.arange(N)
    xs_, ys_ = idx % gw, idx // gw
    hasL = np.zeros(N, bool)
    hasU = np.zeros(N, bool)
    hasL[1:] = hasR[:-1] & (xs_[1:] > 0)
    hasU[gw:] = hasD[:-gw]
    NB = np.stack([hasL, hasU, hasR, hasD], 1)
    nin, nout = hasL.astype(int) + hasU, hasR.astype(int) + hasD
    G = 1.0 / np.maximum(np.maximum(nin, nout), 1)
    valid = np.arange(K)[None, :] < nl[:, None]
    M = np.zeros((N, 4, K))
    xcur = np.zeros(N, int)
    diags = [idx[(xs_ + ys_ == d) & (nl > 0)] for d in range(gw + gh - 1)]

    def hat(ps):
        th = TH[ps].copy()
        for k in range(4):
            th = np.where(NB[ps, k][:, None], th + M[ps, k], th)
        return th

    def send(ps, k_into, Pm, tgt, k_from, transpose):
        th = hat(ps)
        a = G[ps][:, None] * th - M[ps, k_from]
        a = np.where(valid[ps], a, INF)
        C = a[:, :, None] + (np.transpose(Pm, (0, 2, 1)) if transpose else Pm)     # [node, i, j]
        out = C[:, 0, :]
        for i in range(1, K):
            out = np.where(C[:, i, :] < out, C[:, i, :], out)
        mn = out[:, 0]
        for j in range(1, K):
            mn = np.where(out[:, j] < mn, out[:, j], mn)
        res = out - mn[:, None]
        M[tgt, k_into] = np.where(valid[tgt], res, 0.0)

    best, best_x, lb_prev, it_run, lb = None, None, 0.0, 0, 0.0
    for it in range(1, max_iter + 1):
        for ps in diags:
            if not len(ps):
                continue
            v = TH[ps].copy()
            L, Up = ps - 1, ps - gw
            mL, mU = NB[ps, 0], NB[ps, 1]
            v = np.where(mL[:, None], v + PRa[np.where(mL, L, 0), np.where(mL, xcur[np.where(mL, L, 0)], 0)], v)
            v = np.where(mU[:, None], v + PDa[np.where(mU, Up, 0), np.where(mU, xcur[np.where(mU, Up, 0)], 0)], v)
            v = np.where(NB[ps, 2][:, None], v + M[ps, 2], v)
            v = np.where(NB[ps, 3][:, None], v + M[ps, 3], v)
            v = np.where(valid[ps], v, INF)
            xb, bv = np.zeros(len(ps), int), v[:, 0]
            for i in range(1, K):
                b = v[:, i] < bv
                xb, bv = np.where(b, i, xb), np.where(b, v[:, i], bv)
            xcur[ps] = xb
            for k, has, Pm, off in ((0, hasR, PRa, 1), (1, hasD, PDa, gw)):
                q = ps[has[ps]]
                if len(q):
                    send(q, k, Pm[q], q + off, 2 + k, False)
        for ps in diags[::-1]:
            for k, has, Pm, off in ((0, hasL, PRa, 1), (1, hasU, PDa, gw)):
                q = ps[has[ps]]
                if len(q):
                    send(q, 2 + k, Pm[q - off], q - off, k, True)
        # terms per node, then one sequential sum (np.cumsum) in the fixed order
        nodes = idx[nl > 0]
        th = np.where(valid[nodes], hat(nodes), INF)
        tE, tL = np.zeros((N, 3)), np.zeros((N, 3))
        tE[nodes, 0] = TH[nodes, xcur[nodes]]
        mn = th[:, 0]
        for i in range(1, K):
            mn = np.where(th[:, i] < mn, th[:, i], mn)
        tL[nodes, 0] = mn
        for k, has, Pm, off in ((0, hasR, PRa, 1), (1, hasD, PDa, gw)):
            q = idx[has]
            if not len(q):
                continue
            t = q + off
            tE[q, 1 + k] = Pm[q, xcur[q], xcur[t]]
            R = (Pm[q] - M[q, 2 + k][:, :, None]) - M[t, k][:, None, :]
            R = np.where(valid[q][:, :, None] & valid[t][:, None, :], R, INF)
            R = R.reshape(len(q), -1)
            v = R[:, 0]
            for c in range(1, K * K):
                v = np.where(R[:, c] < v, R[:, c], v)
            tL[q, 1 + k] = v
        E = float(np.cumsum(np.concatenate([[0.0], tE.reshape(-1)]))[-1])
        lb = float(np.cumsum(np.concatenate([[0.0], tL.reshape(-1)]))[-1])
        if it == 1 or E < best:
            best, best_x = E, np.where(nl > 0, xcur, -1)
        it_run = it
        stop = it >= 2 and lb - lb_prev < eps
        lb_prev = lb
        if stop:
            break
    return np.array(best_x), best, lb, it_run


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the whole fusion of one segment
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def fuse(U, V, energy, occ, weight, p, w, off=(), solver=trws_diag, trace=None):
    """one segment: U, V (K, Jets, gh, gw) float64; energy (K, gh, gw) (+Inf: none); occ uint64 (K, gh, gw); weight (h, w) fp32.  Returns a dict like
    Context.fuse_hypotheses' for n = 1 (without the leading axis)"""
    K, J, gh, gw = U.shape
    _, _, incr, _ = grid(w, weight.shape[0], p.skip)
    lab = labels(U, V, energy, p.traj_sim_method, p.traj_sim_thres, off)
    PR, PD = pairwise(U, V, occ, weight, lab, p, w, off, trace)
    theta = [np.array([energy[k, pi // gw, pi % gw] for k in lab[pi]], dtype=np.float64) for pi in range(gh * gw)]
    x, E, lb, its = solver(theta, PR, PD, gw, gh, p.trws_eps, p.trws_max_iter)
    slot = np.full((gh, gw), -1, np.int32)
    u, v = np.full((gh, gw), UNKNOWN_FLOW), np.full((gh, gw), UNKNOWN_FLOW)
    oc = np.zeros((gh, gw), np.uint8)
    mask = (1 << (J + 1)) - 1
    for pi in range(gh * gw):
        if not lab[pi]:
            continue
        y, xx = divmod(pi, gw)
        k = lab[pi][x[pi]]
        slot[y, xx] = k
        u[y, xx] = U[k, J - 1, y, xx] / incr
        v[y, xx] = V[k, J - 1, y, xx] / incr
        oc[y, xx] = 1 if (int(occ[k, y, xx]) & mask) else 0
    return dict(slot=slot, u=u, v=v, occ=oc, energy=E, bound=lb, iters=its, labels=x, lab=lab)
