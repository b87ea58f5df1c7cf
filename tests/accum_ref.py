"""dense_tracking's first stage restated afresh in float64 numpy: accumulateConsistentBatches (reference utils/utils.cpp:517-617) with the
bilinearInterp<double> it calls (utils/utils.h:182-217).

Two forms:
  accumulate()         vectorised over the grid pixels, looping over f, with switches that turn each quirk of the reference off (QUIRKS), so that the
                       tests can show that every quirk is pinned by at least one case,
  accumulate_scalar()  a plain transliteration, pixel by pixel in the reference's loop order, for small sizes.
Both take the flows as (FF, h, w) fp32 planes u (x) and v (y); the reference's Vec2d holds (v, u), channel 0 being v (utils.cpp:364-369).  numpy
evaluates every double operation on its own, in the order written: no contraction, so equality with the GPU is bit for bit.

The occlusion masks the reference reads (dense_tracking.cpp:1157-1199): grey file -> medianBlur 3 -> 255 - x, occluded where 0 (decode_occlusion).
"""
import numpy as np

QUIRKS = ("last_init", "occ_zero", "tracked_once", "in_image_double", "out_diff", "edge_weight", "occ_trunc", "err_l2")
# what the reference's statements do with values no smooth flow reaches (tests/test_track_value_ranges.py pins them; the hand-worked cases of
# test_accumulate.py cannot): a tap of weight zero is still multiplied (0 * Inf = NaN, utils.h:216), and a NaN position fails `>= 0 && < extent` (:556)
VALUE_QUIRKS = ("zero_weight_tap", "nan_outside")


def grid(w, h, skip):
    """utils.cpp:522-526: (gw, gh, xy_incr, xy_start), float arithmetic as there"""
    incr = skip + 1
    start = int(np.float32(0.5) * np.float32(skip))
    gh = int(np.floor(np.float32(h) / np.float32(incr)))
    gw = int(np.floor(np.float32(w) / np.float32(incr)))
    return gw, gh, incr, start


def _bilinear(p, x, y, edge_weight=True, zero_taps=True):
    """bilinearInterp<double>(x, y, p) (utils.h:182-217) at arrays of in-image points; p: (h, w) fp32.  Every index formed is asserted to lie in the plane
    (numpy would wrap a negative one silently).  zero_taps=False: the slip that leaves a tap of weight zero out of the sum"""
    h, w = p.shape
    assert np.all((x >= 0) & (x < w) & (y >= 0) & (y < h)), "bilinearInterp outside the plane"      # NaN fails it as well
    x0, y0 = x.astype(np.int64), y.astype(np.int64)            # (int) of non-negative doubles
    if edge_weight:                                             # the weight is 0 on the last column / row (:198-209)
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


def accumulate(fwd_u, fwd_v, bwd_u, bwd_v, masks, epsilon, skip, discard, off=(), trace=None):
    """-> acc_u, acc_v (FF, gh, gw) float64 and tracked (gh, gw) int32.  masks: (FF, h, w) uint8, 0 = occluded, or None.
    off: names from QUIRKS / VALUE_QUIRKS whose reference behaviour is replaced by the obvious alternative (tests only).
    trace: a list that receives one dict per step: the positions tested (cy, cx; NaN where the pixel is occluded), which of them are inside, and the
    targets tested (ny, nx; NaN where the position is not inside) -- what tests/value_ranges.py classifies"""
    off = set(off)
    assert off <= set(QUIRKS) | set(VALUE_QUIRKS), off
    zt = "zero_weight_tap" not in off
    FF, h, w = np.shape(fwd_u)
    gw, gh, incr, start = grid(w, h, skip)
    oy = (np.arange(gh) * incr + start)[:, None].repeat(gw, 1).ravel()
    ox = (np.arange(gw) * incr + start)[None, :].repeat(gh, 0).ravel()
    n = gw * gh
    if "last_init" in off:
        last_u, last_v = np.zeros(n), np.zeros(n)
    else:                                                       # forward[0] at the grid point (:530-535)
        last_u = np.asarray(fwd_u[0], np.float64)[oy, ox].copy()
        last_v = np.asarray(fwd_v[0], np.float64)[oy, ox].copy()
    occluded = np.zeros(n, bool)
    tracked = np.full(n, FF, np.int32)
    carried_u, carried_v = np.zeros(n), np.zeros(n)             # what an occluded pixel keeps in the "occ_zero" variant
    acc_u, acc_v = np.zeros((FF, n)), np.zeros((FF, n))

    def mark(sel, f):
        if "tracked_once" in off:
            tracked[sel] = 0 if discard else f + 1
        else:                                                   # change only once (:561-566, :586-591, :602-607)
            once = sel & (tracked == FF)
            tracked[once] = 0 if discard else f + 1

    def inside(yy, xx):
        if "nan_outside" in off:                                # the slip: `!(outside)`, which lets a NaN position through (read at pixel 0 here)
            return ~((yy < 0) | (yy >= h) | (xx < 0) | (xx >= w))
        if "in_image_double" in off:                            # the slip: the test on truncated coordinates
            return (np.trunc(yy) >= 0) & (yy < h) & (np.trunc(xx) >= 0) & (xx < w)
        return (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)

    for f in range(FF):
        act = ~occluded                                         # an occluded pixel `continue`s (:547-548)
        cy, cx = oy.astype(np.float64), ox.astype(np.float64)
        au, av = np.zeros(n), np.zeros(n)
        if f > 0:
            cy = cy + acc_v[f - 1]
            cx = cx + acc_u[f - 1]
            au, av = acc_u[f - 1].copy(), acc_v[f - 1].copy()
        ins = act & inside(cy, cx)
        out = act & ~ins
        if masks is not None:
            idx = np.nonzero(ins)[0]
            if "occ_trunc" in off:
                ry = np.minimum(np.rint(cy[idx]).astype(np.int64), h - 1)
                rx = np.minimum(np.rint(cx[idx]).astype(np.int64), w - 1)
            else:                                               # at<uchar>(double, double) truncates (:557)
                ry, rx = cy[idx].astype(np.int64), cx[idx].astype(np.int64)
            if "nan_outside" in off:
                ry, rx = np.nan_to_num(cy[idx]).astype(np.int64), np.nan_to_num(cx[idx]).astype(np.int64)
            assert np.all((ry >= 0) & (ry < h) & (rx >= 0) & (rx < w)), "occlusion lookup outside the mask"
            occ_now = np.zeros(n, bool)
            occ_now[idx] = np.asarray(masks[f])[ry, rx] == 0
            occluded |= occ_now
            mark(occ_now, f)
        idx = np.nonzero(ins)[0]
        ew = "edge_weight" not in off
        pyc, pxc = np.maximum(cy[idx], 0), np.maximum(cx[idx], 0)   # only the "in_image_double" variant lets (-1, 0) through
        if "nan_outside" in off:
            pyc, pxc = np.nan_to_num(pyc), np.nan_to_num(pxc)
        vu = _bilinear(np.asarray(fwd_u[f]), pxc, pyc, ew, zt)
        vv = _bilinear(np.asarray(fwd_v[f]), pxc, pyc, ew, zt)
        ny, nx = cy[idx] + vv, cx[idx] + vu
        if "out_diff" in off:                                   # the slip: no backward flow -> the forward vector alone
            dv, du = vv.copy(), vu.copy()
        else:                                                   # diff = vec - last_flow (:574)
            dv, du = vv - last_v[idx], vu - last_u[idx]
        tin = inside(ny, nx)
        t = np.nonzero(tin)[0]
        tx, ty = np.maximum(nx[t], 0), np.maximum(ny[t], 0)
        if "nan_outside" in off:
            tx, ty = np.nan_to_num(tx), np.nan_to_num(ty)
        bu = _bilinear(np.asarray(bwd_u[f]), tx, ty, ew, zt)
        bv = _bilinear(np.asarray(bwd_v[f]), tx, ty, ew, zt)
        if trace is not None:
            full_ny, full_nx = np.full(n, np.nan), np.full(n, np.nan)
            full_ny[idx], full_nx[idx] = ny, nx
            tgt_in = np.zeros(n, bool)
            tgt_in[idx[t]] = True
            trace.append(dict(cy=np.where(act, cy, np.nan), cx=np.where(act, cx, np.nan), act=act.copy(), ins=ins.copy(), ny=full_ny, nx=full_nx,
                              tgt=ins.copy(), tgt_in=tgt_in))
        dv[t] = vv[t] + bv
        du[t] = vu[t] + bu
        if "err_l2" in off:
            err = np.abs(dv) + np.abs(du)
        else:
            err = np.sqrt(dv * dv + du * du)                    # :579
        bad = err > epsilon
        bi, gi = idx[bad], idx[~bad]
        au[bi] = au[bi] + last_u[bi]                            # constant velocity (:583)
        av[bi] = av[bi] + last_v[bi]
        au[gi] = au[gi] + vu[~bad]                              # :593-595
        av[gi] = av[gi] + vv[~bad]
        last_u[gi], last_v[gi] = vu[~bad], vv[~bad]
        fail = np.zeros(n, bool)
        fail[bi] = True
        au[out] = au[out] + last_u[out]                         # :598-599
        av[out] = av[out] + last_v[out]
        fail |= out
        mark(fail, f)
        if "occ_zero" in off:                                   # the slip: an occluded pixel keeps its last accumulated flow
            au[~act], av[~act] = carried_u[~act], carried_v[~act]
        else:
            au[~act], av[~act] = 0.0, 0.0
        carried_u[act], carried_v[act] = au[act], av[act]
        acc_u[f], acc_v[f] = au, av                             # acc_forward[f] starts at zero (:541): occluded pixels stay 0
    return acc_u.reshape(FF, gh, gw), acc_v.reshape(FF, gh, gw), tracked.reshape(gh, gw)


def _bilinear_scalar(p, x, y):
    h, w = p.shape
    y0, x0 = int(y), int(x)
    assert 0 <= y0 < h and 0 <= x0 < w, "bilinearInterp outside the plane"
    y1, x1 = y0, x0
    wx = 0.0
    if x0 + 1 < w:
        wx = x - x0
        x1 += 1
    wy = 0.0
    if y0 + 1 < h:
        wy = y - y0
        y1 += 1
    f00, f10, f01, f11 = float(p[y0, x0]), float(p[y0, x1]), float(p[y1, x0]), float(p[y1, x1])
    return (1 - wy) * (1 - wx) * f00 + (1 - wy) * wx * f10 + wy * (1 - wx) * f01 + wy * wx * f11


def accumulate_scalar(fwd_u, fwd_v, bwd_u, bwd_v, masks, epsilon, skip, discard):
    """the reference's loops as they stand (utils.cpp:517-617), one pixel at a time with Python floats (IEEE doubles); small sizes only"""
    FF, h, w = np.shape(fwd_u)
    gw, gh, incr, start = grid(w, h, skip)
    last = {}
    for y in range(gh):
        for x in range(gw):
            last[y, x] = [float(fwd_v[0][y * incr + start, x * incr + start]), float(fwd_u[0][y * incr + start, x * incr + start])]
    occluded = np.zeros((gh, gw), bool)
    tracked = np.full((gh, gw), FF, np.int32)
    acc = np.zeros((FF, gh, gw, 2))
    for f in range(FF):
        for y in range(gh):
            for x in range(gw):
                if occluded[y, x]:
                    continue
                c = [float(y * incr + start), float(x * incr + start)]
                if f > 0:
                    c = [c[0] + acc[f - 1, y, x, 0], c[1] + acc[f - 1, y, x, 1]]
                    acc[f, y, x] = acc[f - 1, y, x]
                if c[0] >= 0 and c[0] < h and c[1] >= 0 and c[1] < w:
                    if masks is not None and masks[f][int(c[0]), int(c[1])] == 0:
                        occluded[y, x] = True
                        if tracked[y, x] == FF:
                            tracked[y, x] = 0 if discard else f + 1
                    vec = [_bilinear_scalar(fwd_v[f], c[1], c[0]), _bilinear_scalar(fwd_u[f], c[1], c[0])]
                    cn = [c[0] + vec[0], c[1] + vec[1]]
                    diff = [vec[0] - last[y, x][0], vec[1] - last[y, x][1]]
                    if cn[0] >= 0 and cn[0] < h and cn[1] >= 0 and cn[1] < w:
                        diff = [vec[0] + _bilinear_scalar(bwd_v[f], cn[1], cn[0]), vec[1] + _bilinear_scalar(bwd_u[f], cn[1], cn[0])]
                    err = float(np.sqrt(diff[0] * diff[0] + diff[1] * diff[1]))
                    if err > epsilon:
                        acc[f, y, x, 0] += last[y, x][0]
                        acc[f, y, x, 1] += last[y, x][1]
                        if tracked[y, x] == FF:
                            tracked[y, x] = 0 if discard else f + 1
                    else:
                        acc[f, y, x, 0] += vec[0]
                        acc[f, y, x, 1] += vec[1]
                        last[y, x] = vec
                else:
                    acc[f, y, x, 0] += last[y, x][0]
                    acc[f, y, x, 1] += last[y, x][1]
                    if tracked[y, x] == FF:
                        tracked[y, x] = 0 if discard else f + 1
    return acc[..., 1].copy(), acc[..., 0].copy(), tracked


def median3(img):
    """3 x 3 median with a replicated border (OpenCV's medianBlur, ksize 3, uses BORDER_REPLICATE); uint8"""
    p = np.pad(np.asarray(img, np.uint8), 1, mode="edge")
    h, w = np.shape(img)
    stack = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return np.median(stack, axis=0).astype(np.uint8)


def decode_occlusion(grey):
    """the mask the reference forms from a jet's occlusion file (dense_tracking.cpp:1179-1193): medianBlur 3, then 255 - x; 0 = occluded.
    The slow_flow drivers write 255 where the occlusion label is +1 (reference slow_flow.cpp:896-898: 0.5 (occ + 1) * 255; this project's
    writePGM(offset 1, scale 127.5)), so grey 255 -> 0 -> occluded."""
    return (255 - median3(grey).astype(np.int32)).astype(np.uint8)
