"""Independent float64 derivations of the three operators whose bit-level parity with the reference cannot be pinned
(DESIGN.md section 3): compute_smoothness, add_data_and_match / add_data_and_match_ref and the data costs of
optimizeOcc.  Written as whole-plane numpy from the text of epic_flow_extended/variational_aux_mt.cpp and
penalty_functions/*.h (line numbers below are that file's), independently of oracle/slowflow_oracle.c and the kernels.

Every quantity is a `V`: its float64 value and a magnitude companion `m`, the same expression evaluated with the
absolute value of every term.  A fp32 evaluation of the expression then differs from the value by at most
K * 2^-24 * m for a K that counts the roundings along the chain (tests/test_indep_ref.py).  Two rules extend the
plain absolute-value evaluation so that the bound stays true:
  - a penalty factor f(x) (psi or psi') gets m = |f(x)| + |f'(x)| * m_x: the first-order effect of the rounding
    error of its argument, which is bounded relative to m_x, not to x;
  - a quotient a / b gets m = m_a / |b| + |a| * m_b / b^2.
`V.k` marks elements whose argument lies within KINK_REL of a penalty's kink (truncated modified L1), where fp32
may legitimately take the other branch; the tests exclude them.

Keyword arguments named after a reference quirk or a plausible slip produce deliberately wrong variants; the tests
assert that each variant is rejected, which shows that the inputs exercise that branch.
"""
import numpy as np

KINK_REL = 1e-5
DT_SCALE_GRAPHC = float(np.float32(0.01))                     # variational_aux_mt.h:24, a float constant
DATANORM = float(np.float32(0.1) * np.float32(0.1))           # variational_aux_mt.h:23: 0.1f * 0.1f, a float product


class V:
    """float64 value `v`, magnitude companion `m`, near-kink flags `k` (see the module docstring)"""
    __slots__ = ("v", "m", "k")

    def __init__(self, v, m=None, k=False):
        self.v = np.asarray(v, np.float64)
        self.m = np.abs(self.v) if m is None else m
        self.k = k

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def __add__(self, o):
        o = V.of(o)
        return V(self.v + o.v, self.m + o.m, self.k | o.k)

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return V(self.v - o.v, self.m + o.m, self.k | o.k)

    def __rsub__(self, o):
        return V.of(o) - self

    def __neg__(self):
        return V(-self.v, self.m, self.k)

    def __mul__(self, o):
        o = V.of(o)
        return V(self.v * o.v, self.m * o.m, self.k | o.k)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            return V(self.v / o.v, self.m / np.abs(o.v) + np.abs(self.v) * o.m / (o.v * o.v), self.k | o.k)

    def sq(self):
        return self * self


# ------------------------------------------------------------------------------------------------------------------
# penalty functions (penalty_functions/*.h; ids as in the switch of variational_aux_mt.cpp:909-925)
# ------------------------------------------------------------------------------------------------------------------
def _consts(pen):
    """pen = (id, eps, trunc).  The classes store epsilon_sq(e*e) with e a float: the square is a float product."""
    pid, eps, trunc = pen
    return int(pid), float(np.float32(eps) * np.float32(eps)), float(np.float32(trunc))


def _near_kink(pid, tr, x):
    """trunc_modified_l1_norm.h: the branch `sqrt(xsq) > truncation` switches at xsq = truncation^2"""
    if pid != 3:
        return np.zeros(x.v.shape, bool)
    return np.abs(x.v - tr * tr) <= KINK_REL * np.maximum(x.m, tr * tr)


def dpsi(pen, x):
    """psi'(x) as the `derivative` members define it, with |d psi'/dx| for the magnitude companion"""
    pid, e2, tr = _consts(pen)
    xv = x.v
    if pid == 0:                                      # quadratic_function.h:23-28: 1
        d, dd = np.ones_like(xv), np.zeros_like(xv)
    elif pid == 2:                                    # lorentzian.h:36-42: 1 / (2 eps^2 + x)
        d = 1.0 / (2.0 * e2 + xv)
        dd = d * d
    elif pid == 4:                                    # geman_mcclure.h:28-38: (eps^2 + 2x) / (eps^2 + x)^2
        t = e2 + xv
        d = (e2 + 2.0 * xv) / (t * t)
        dd = np.abs(2.0 * xv / (t * t * t))
    else:                                             # modified_l1_norm.h:28-34, trunc_modified_l1_norm.h:40-56
        r = np.sqrt(xv + e2)
        d = 1.0 / (2.0 * r)
        dd = d / (2.0 * (xv + e2))
        if pid == 3:                                  # 0 beyond the truncation
            cut = np.sqrt(xv) > tr
            d, dd = np.where(cut, 0.0, d), np.where(cut, 0.0, dd)
    return V(d, np.abs(d) + dd * x.m, x.k | _near_kink(pid, tr, x))


def psi(pen, x):
    """psi(x) as the `apply` members define it, with |d psi/dx| for the magnitude companion"""
    pid, e2, tr = _consts(pen)
    xv = x.v
    if pid == 0:                                      # quadratic_function.h:14-20: x
        f, df = xv.copy(), np.ones_like(xv)
    elif pid == 2:                                    # lorentzian.h:24-32: log(1 + x / (2 eps^2))
        f = np.log1p(0.5 * xv / e2)
        df = 1.0 / (2.0 * e2 + xv)
    elif pid == 4:                                    # geman_mcclure.h:20-26: x / (x + 1)^2 -- no epsilon in `apply`
        f = xv / ((xv + 1.0) * (xv + 1.0))
        df = np.abs((1.0 - xv) / (xv + 1.0) ** 3)
    else:                                             # modified_l1_norm.h:20-26, trunc_modified_l1_norm.h:22-36
        f = np.sqrt(xv + e2)
        df = 0.5 / f
        if pid == 3:                                  # beyond the truncation: sqrt(truncation + eps^2) -- truncation, not its square
            cut = np.sqrt(xv) > tr
            f, df = np.where(cut, np.sqrt(tr + e2), f), np.where(cut, 0.0, df)
    return V(f, np.abs(f) + df * x.m, x.k | _near_kink(pid, tr, x))


def _in(a, w):
    """valid region of a (..., h, stride) fp32 plane as float64"""
    return np.asarray(a, np.float32)[..., :w].astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------
# compute_smoothness, variational_aux_mt.cpp:18-127
# ------------------------------------------------------------------------------------------------------------------
def smoothness(method, uu, vv, dpsis, alpha, pen, w, method2_uses_width=False):
    """-> (dst_horiz, dst_vert) as V over the valid (h, w) region"""
    u, v, d = V(_in(uu, w)), V(_in(vv, w)), V(_in(dpsis, w))
    alpha = float(np.float32(alpha))
    h = u.v.shape[0]
    zero = V(np.zeros((h, w)))

    def sl(a, ys, xs):
        return V(a.v[ys, xs], a.m[ys, xs])

    def put(dst, ys, xs, src):
        out = V(dst.v.copy(), dst.m.copy(), np.array(dst.k | np.zeros(dst.v.shape, bool)))
        out.v[ys, xs], out.m[ys, xs] = src.v, src.m
        out.k[ys, xs] = src.k
        return out

    allr, allc = slice(None), slice(None)
    # forward differences [-1 1] (:23-38); the last column / row is never written and never read below
    ux1 = put(zero, allr, slice(0, w - 1), sl(u, allr, slice(1, w)) - sl(u, allr, slice(0, w - 1)))
    vx1 = put(zero, allr, slice(0, w - 1), sl(v, allr, slice(1, w)) - sl(v, allr, slice(0, w - 1)))
    uy1 = put(zero, slice(0, h - 1), allc, sl(u, slice(1, h), allc) - sl(u, slice(0, h - 1), allc))
    vy1 = put(zero, slice(0, h - 1), allc, sl(v, slice(1, h), allc) - sl(v, slice(0, h - 1), allc))

    # central differences [-0.5 0 0.5] (:41-44, convolve_horiz / convolve_vert with the 3-tap deriv_flow): for three taps
    # both border rules amount to repeating the edge sample
    def cdx(a):
        xi = np.arange(w)
        return 0.5 * sl(a, allr, np.minimum(xi + 1, w - 1)) - 0.5 * sl(a, allr, np.maximum(xi - 1, 0))

    def cdy(a):
        yi = np.arange(h)
        return 0.5 * sl(a, np.minimum(yi + 1, h - 1), allc) - 0.5 * sl(a, np.maximum(yi - 1, 0), allc)

    if method <= 1:
        # horizontal weight (:47-69), zero in the last column
        L, R = slice(0, w - 1), slice(1, w)
        t = V(np.zeros((h, w - 1)))
        t2 = V(np.zeros((h, w - 1)))
        if method == 1:
            uy2, vy2 = cdy(u), cdy(v)
            t = 0.5 * (sl(uy2, allr, L) + sl(uy2, allr, R))
            t2 = 0.5 * (sl(vy2, allr, L) + sl(vy2, allr, R))
        arg = (sl(ux1, allr, L).sq() + t.sq()) + (sl(vx1, allr, L).sq() + t2.sq())
        val = (sl(d, allr, L) + sl(d, allr, R)) * alpha * dpsi(pen, arg)
        dh = put(zero, allr, L, val)
        # vertical weight (:71-93), zero in the last row
        T, B = slice(0, h - 1), slice(1, h)
        t = V(np.zeros((h - 1, w)))
        t2 = V(np.zeros((h - 1, w)))
        if method == 1:
            ux2, vx2 = cdx(u), cdx(v)
            t = 0.5 * (sl(ux2, T, allc) + sl(ux2, B, allc))
            t2 = 0.5 * (sl(vx2, T, allc) + sl(vx2, B, allc))
        arg = (sl(uy1, T, allc).sq() + t.sq()) + (sl(vy1, T, allc).sq() + t2.sq())
        val = (sl(d, T, allc) + sl(d, B, allc)) * alpha * dpsi(pen, arg)
        dv = put(zero, T, allc, val)
        return dh, dv

    # method 2 (:95-117): one weight for both directions.  `float w = dpsis_weight->data[offset]` (:100) shadows the
    # image width, so the horizontal test `i < w - 1` (:103) compares the column index with (weight - 1).
    xi = np.broadcast_to(np.arange(w, dtype=np.float64), (h, w))
    wm1 = d.v - 1.0                                   # exact in fp32 for every weight that can pass the test (weight >= 1)
    hor = (xi < w - 1) if method2_uses_width else (xi < wm1)
    if np.any(hor[:, w - 1]):
        raise ValueError("a weight above the width in the last column makes the reference read an unwritten ux1/vx1 "
                         "sample and the next row's weight: no defined value to derive")
    vert = np.zeros((h, w), bool)
    vert[:h - 1] = True
    d_right = put(zero, allr, slice(0, w - 1), sl(d, allr, slice(1, w)))
    d_down = put(zero, slice(0, h - 1), allc, sl(d, slice(1, h), allc))
    hterm = ux1.sq() + vx1.sq()
    vterm = vy1.sq() + uy1.sq()
    tmp = V(np.where(hor, hterm.v, 0.0), np.where(hor, hterm.m, 0.0))
    tmp = tmp + V(np.where(vert, vterm.v, 0.0), np.where(vert, vterm.m, 0.0))
    wgt = d + V(np.where(hor, d_right.v, 0.0), np.where(hor, d_right.m, 0.0))
    wgt = wgt + V(np.where(vert, d_down.v, 0.0), np.where(vert, d_down.m, 0.0))
    out = wgt * alpha * dpsi(pen, tmp)
    return out, out


# ------------------------------------------------------------------------------------------------------------------
# add_data_and_match (:166-403) and add_data_and_match_ref (:408-634)
# ------------------------------------------------------------------------------------------------------------------
IX, IY, IZ, IXX, IXY, IYY, IXZ, IYZ = range(8)         # the order of the stack orc.derivative_stack builds


def data_term(sys, mask, du, dv, D, chw, hd, hg, s, dt_norm, color, grad, ref_term, w,
              ch3_keeps_weight=False, no_extra_factorsq=False):
    """sys: the five planes (a11, a12, a22, b1, b2) the term is added to.  Returns the five sums as V over (h, w)."""
    a11, a12, a22, b1, b2 = (V(_in(a, w)) for a in sys)
    m, u, v = V(_in(mask, w)), V(_in(du, w)), V(_in(dv, w))
    Dv = _in(D, w)

    def g(i, k):
        return V(Dv[i, k])

    wk = [V(_in(c, w)) for c in chw]
    s = float(np.float32(s))
    hd, hg = float(np.float32(hd)), float(np.float32(hg))

    if not ref_term:
        f, fp1 = s, s + 1.0
        if hd != 0:                                   # `if (delta_over3)` (:188)
            r = [wk[k] * (g(IZ, k) + g(IX, k) * f * u + g(IY, k) * f * v - g(IX, k) * fp1 * u - g(IY, k) * fp1 * v) for k in range(3)]
            tx = [f * g(IX, k) - fp1 * g(IX, k) for k in range(3)]
            ty = [f * g(IY, k) - fp1 * g(IY, k) for k in range(3)]
            if not dt_norm:                           # :194-226
                t = m * hd * dpsi(color, r[0].sq() + r[1].sq() + r[2].sq())
                tk = [t * wk[k] for k in range(3)]
            else:                                     # :227-266
                n = [tx[k].sq() + ty[k].sq() + DATANORM for k in range(3)]
                t = m * hd * dpsi(color, r[0].sq() / n[0] + r[1].sq() / n[1] + r[2].sq() / n[2])
                tk = [t / n[k] * wk[k] for k in range(3)]
            for k in range(3):
                a11 = a11 + tk[k] * tx[k] * tx[k]
                a12 = a12 + tk[k] * tx[k] * ty[k]
                a22 = a22 + tk[k] * ty[k] * ty[k]
                b1 = b1 - tk[k] * g(IZ, k) * tx[k]
                b2 = b2 - tk[k] * g(IZ, k) * ty[k]
        # gradient constancy (:269-364)
        r = []
        for k in range(3):
            r.append(wk[k] * (g(IXZ, k) + g(IXX, k) * f * u + g(IXY, k) * f * v - g(IXX, k) * fp1 * u - g(IXY, k) * fp1 * v))
            r.append(wk[k] * (g(IYZ, k) + g(IXY, k) * f * u + g(IYY, k) * f * v - g(IXY, k) * fp1 * u - g(IYY, k) * fp1 * v))
        X = [f * g(IXX, k) - fp1 * g(IXX, k) for k in range(3)]
        Y = [f * g(IYY, k) - fp1 * g(IYY, k) for k in range(3)]
        Z = [f * g(IXY, k) - fp1 * g(IXY, k) for k in range(3)]
        if not dt_norm:                               # :278-313
            t = m * hg * dpsi(grad, sum((x.sq() for x in r[1:]), r[0].sq()))
            ta = tb = [t * wk[k] for k in range(3)]
        else:                                         # :314-364
            n = []
            for k in range(3):
                n += [X[k].sq() + Z[k].sq() + DATANORM, Y[k].sq() + Z[k].sq() + DATANORM]
            t = m * hg * dpsi(grad, sum((r[j].sq() / n[j] for j in range(1, 6)), r[0].sq() / n[0]))
            ta = [t / n[2 * k] * wk[k] for k in range(3)]
            tb = [t / n[2 * k + 1] * wk[k] for k in range(3)]
        for k in range(3):
            a11 = a11 + (ta[k] * X[k] * X[k] + tb[k] * Z[k] * Z[k])
            a12 = a12 + (ta[k] * X[k] * Z[k] + tb[k] * Z[k] * Y[k])
            a22 = a22 + (tb[k] * Y[k] * Y[k] + ta[k] * Z[k] * Z[k])
            b1 = b1 - (ta[k] * g(IXZ, k) * X[k] + tb[k] * g(IYZ, k) * Z[k])
            b2 = b2 - (tb[k] * g(IYZ, k) * Y[k] + ta[k] * g(IXZ, k) * Z[k])
        return a11, a12, a22, b1, b2

    # reference-frame term: I_ref - I_s, so the factor changes sign for s >= 0 (:416-426)
    if s == 0:
        raise ValueError("s == 0: the reference throws logic_error (:419-420)")
    fsq = s * s
    f = -s if s >= 0 else s
    if hd != 0:                                       # :439
        r = [wk[k] * (g(IZ, k) + g(IX, k) * f * u + g(IY, k) * f * v) for k in range(3)]
        if not dt_norm:                               # :445-472
            t = m * hd * dpsi(color, r[0].sq() / fsq + r[1].sq() / fsq + r[2].sq() / fsq) / fsq
            for k in range(3):
                t2 = t * wk[k] * f
                b1 = b1 - t2 * g(IZ, k) * g(IX, k)
                b2 = b2 - t2 * g(IZ, k) * g(IY, k)
                # :469 forms channel 3's matrix factor from tmp, not tmp2: its weight drops out of a11, a12, a22
                t2 = t2 * f if (k < 2 or ch3_keeps_weight) else t * f
                a11 = a11 + t2 * g(IX, k) * g(IX, k)
                a12 = a12 + t2 * g(IX, k) * g(IY, k)
                a22 = a22 + t2 * g(IY, k) * g(IY, k)
        else:                                         # :473-508
            n = [fsq * g(IX, k) * g(IX, k) + fsq * g(IY, k) * g(IY, k) + DATANORM for k in range(3)]
            t = m * hd * dpsi(color, r[0].sq() / n[0] + r[1].sq() / n[1] + r[2].sq() / n[2])
            for k in range(3):
                tk = t / n[k] * wk[k] * f
                b1 = b1 - tk * g(IZ, k) * g(IX, k)
                b2 = b2 - tk * g(IZ, k) * g(IY, k)
                tk = tk * f
                a11 = a11 + tk * g(IX, k) * g(IX, k)
                a12 = a12 + tk * g(IX, k) * g(IY, k)
                a22 = a22 + tk * g(IY, k) * g(IY, k)
    # gradient constancy (:511-593)
    r = []
    for k in range(3):
        r.append(wk[k] * (g(IXZ, k) + g(IXX, k) * f * u + g(IXY, k) * f * v))
        r.append(wk[k] * (g(IYZ, k) + g(IXY, k) * f * u + g(IYY, k) * f * v))
    if not dt_norm:                                   # :518-546
        t = m * hg * dpsi(grad, sum((x.sq() / fsq for x in r[1:]), r[0].sq() / fsq)) / fsq
        for k in range(3):
            t2 = t * wk[k] * f
            b1 = b1 - (t2 * g(IXX, k) * g(IXZ, k) + t2 * g(IXY, k) * g(IYZ, k))
            b2 = b2 - (t2 * g(IYY, k) * g(IYZ, k) + t2 * g(IXY, k) * g(IXZ, k))
            t2 = t2 * f
            # :528-530: channel 1's matrix factors carry factorsq once more than channels 2 and 3
            q = t2 * fsq if (k == 0 and not no_extra_factorsq) else t2
            a11 = a11 + (q * g(IXX, k) * g(IXX, k) + q * g(IXY, k) * g(IXY, k))
            a12 = a12 + (q * g(IXX, k) * g(IXY, k) + q * g(IXY, k) * g(IYY, k))
            a22 = a22 + (q * g(IYY, k) * g(IYY, k) + q * g(IXY, k) * g(IXY, k))
    else:                                             # :547-593
        n = []
        for k in range(3):
            n += [fsq * g(IXX, k) * g(IXX, k) + fsq * g(IXY, k) * g(IXY, k) + DATANORM,
                  fsq * g(IYY, k) * g(IYY, k) + fsq * g(IXY, k) * g(IXY, k) + DATANORM]
        t = m * hg * dpsi(grad, sum((r[j].sq() / n[j] for j in range(1, 6)), r[0].sq() / n[0]))
        for k in range(3):
            ta = t / n[2 * k] * wk[k] * f
            tb = t / n[2 * k + 1] * wk[k] * f
            b1 = b1 - (ta * g(IXX, k) * g(IXZ, k) + tb * g(IXY, k) * g(IYZ, k))
            b2 = b2 - (tb * g(IYY, k) * g(IYZ, k) + ta * g(IXY, k) * g(IXZ, k))
            ta, tb = ta * f, tb * f
            a11 = a11 + (ta * g(IXX, k) * g(IXX, k) + tb * g(IXY, k) * g(IXY, k))
            a12 = a12 + (ta * g(IXX, k) * g(IXY, k) + tb * g(IXY, k) * g(IYY, k))
            a22 = a22 + (tb * g(IYY, k) * g(IYY, k) + ta * g(IXY, k) * g(IXY, k))
    return a11, a12, a22, b1, b2


# ------------------------------------------------------------------------------------------------------------------
# optimizeOcc's data costs, variational_aux_mt.cpp:783-866
# ------------------------------------------------------------------------------------------------------------------
def occlusion_costs(masks, succ, toref, ref, rho, omega, hd, hg, penalty, color, grad, w,
                    labels_swapped=False, idx_off_by_one=False, no_norm_guard=False, no_dt_scale=False,
                    penalty_on_label0=False):
    """masks (2ref, h, stride); succ / toref (2ref, 8, 3, h, stride) derivative stacks (successive pair, pair with the
    reference frame).  -> (d0, d1) as V over (h, w): label 0 = occluded in the past, 1 = in the future."""
    hd, hg, penalty = float(np.float32(hd)), float(np.float32(hg)), float(np.float32(penalty))
    h = masks.shape[1]
    E = [V(np.zeros((h, w))), V(np.zeros((h, w)))]
    N = [V(np.zeros((h, w))), V(np.zeros((h, w)))]
    for s in range(2 * ref):
        idx = min(abs(s - ref), ref - 1) if idx_off_by_one else max(ref - s - 1, s - ref)    # :812
        r, o = float(np.float32(rho[idx])), float(np.float32(omega[idx]))
        m = V(_in(masks[s], w))
        S, R = _in(succ[s], w), _in(toref[s], w)
        col = lambda st: V((st[IZ] ** 2).sum(axis=0))                                           # sum over the 3 channels
        grd = lambda st: V((st[IXZ] ** 2).sum(axis=0) + (st[IYZ] ** 2).sum(axis=0))
        term = r * hd * m * psi(color, col(S))                                                  # :815 successive term
        term = term + r * hg * m * psi(grad, grd(S))                                            # :816-817
        term = term + o * hd * m * psi(color, col(R))                                           # :820 reference term
        term = term + o * hg * m * psi(grad, grd(R))                                            # :821-825
        l = 0 if s >= ref else 1                                                                # :827-836
        if labels_swapped:
            l = 1 - l
        E[l] = E[l] + term
        N[l] = N[l] + m * (r + r + o + o)
    out = []
    for l in range(2):
        n = N[l]
        if not no_norm_guard:                                                                   # :843-847
            n = V(np.where(n.v == 0, 1.0, n.v), np.where(n.v == 0, 1.0, n.m), n.k)
        e = (E[l] if no_dt_scale else DT_SCALE_GRAPHC * E[l]) / n
        out.append(e + penalty * ((1 - l) if penalty_on_label0 else l))                          # :848
    return out[0], out[1]
