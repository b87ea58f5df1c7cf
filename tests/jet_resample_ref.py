"""dense_tracking's treatment of jets of another size than the tracking frames (reference dense_tracking.cpp:1134-1146 for the flows, :1171-1189 for
the occlusion images), restated in scalar numpy: crop (utils/utils.cpp:308-318), cv::resize by `rescale`, `flow *= rescale`; for an occlusion image
the cubic resize, medianBlur(3) and 255 - x.

OpenCV is not in the tree, so nothing here is pinned against the reference's own binary: this is the documented arithmetic of cv::resize written down
once more, the same status as the pyramid's resize (oracle/slowflow_oracle.c:1158-1187, resize_linear_scaled, whose coordinate rule is followed).

  INTER_LINEAR on CV_64FC2 (readGTMiddlebury widens the floats of the file): HResizeLinear<double, double, float> then VResizeLinear: the weights
  1.f - f and f are floats, the samples, products and sums doubles, rows first.
  INTER_CUBIC on CV_8U: HResizeCubic<uchar, int, short> then VResizeCubic with FixedPtCast<int, uchar, 22>: Keys' cubic with A = -0.75 in float
  (interpolateCubic), each coefficient saturate_cast<short>(c * 2048) (cvRound: halves to even), integer sums, (sum + 2^21) >> 22 saturated.
  OpenCV's SIMD build rounds the column pass in float instead: a departure of one grey level is possible there, within two source pixels of an edge.

Every operation is written on its own, so numpy rounds it on its own: no contraction."""
import numpy as np

from accum_ref import median3

f32 = np.float32


def crop_rect(center, extent):
    """crop() (utils.cpp:308-318): output pixel (x, y) is source pixel (x - extent.x / 2 + center.x, y - extent.y / 2 + center.y) in integer
    division, the output extent.x x extent.y: (x0, y0, cw, ch).  It applies where center.x > 0 (dense_tracking.cpp:1135)"""
    (cx, cy), (ex, ey) = center, extent
    return cx - int(ex / 2), cy - int(ey / 2), ex, ey                    # C's division truncates


def rescale_of(w, cw):
    """float rescale = (1.0f * sequence[0].cols) / flow.cols (:1142)"""
    return f32(f32(1.0) * f32(w)) / f32(cw)


def target_size(cw, ch, rescale):
    """cv::resize with Size(0, 0): dsize = (cvRound(cols * fx), cvRound(rows * fy)), fx = fy = (double)rescale; cvRound rounds halves to even"""
    r = np.float64(f32(rescale))
    return int(np.rint(np.float64(cw) * r)), int(np.rint(np.float64(ch) * r))


def _linear_taps(n_dst, n_src, scale):
    """per destination index: the left tap and the float weight of the right tap (resize_linear_scaled: slowflow_oracle.c:1161-1168)"""
    idx, frac = np.zeros(n_dst, np.int64), np.zeros(n_dst, f32)
    for d in range(n_dst):
        f = f32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = f32(f - f32(s))
        if s < 0:
            f, s = f32(0), 0
        if s >= n_src - 1:
            f, s = f32(0), n_src - 1
        idx[d], frac[d] = s, f
    return idx, frac


def resize_linear_64f(src, rescale, zero_taps=True):
    """cv::resize(src, dst, Size(0, 0), rescale, rescale, INTER_LINEAR) of one float64 plane; scale = 1.0 / (double)rescale.  A tap of weight zero (the
    clamped last row / column, an exact sample position) is still multiplied: 0 * Inf = NaN.  zero_taps=False: the slip that leaves it out (tests only)"""
    def mul(v, wgt):
        return v * wgt if zero_taps or wgt != 0 else 0.0

    src = np.asarray(src, np.float64)
    sh, sw = src.shape
    dw, dh = target_size(sw, sh, rescale)
    scale = 1.0 / np.float64(f32(rescale))
    xo, xa = _linear_taps(dw, sw, scale)
    yo, ya = _linear_taps(dh, sh, scale)
    out = np.zeros((dh, dw), np.float64)
    for dy in range(dh):
        sy = int(yo[dy])
        sy1 = sy + 1 if sy + 1 < sh else sy
        b0, b1 = np.float64(f32(1) - ya[dy]), np.float64(ya[dy])
        for dx in range(dw):
            sx = int(xo[dx])
            sx1 = sx + 1 if sx + 1 < sw else sx
            a0, a1 = np.float64(f32(1) - xa[dx]), np.float64(xa[dx])
            assert 0 <= sy <= sy1 < sh and 0 <= sx <= sx1 < sw, "tap outside the plane"
            h0 = mul(src[sy, sx], a0) + mul(src[sy, sx1], a1)            # the row pass of both rows
            h1 = mul(src[sy1, sx], a0) + mul(src[sy1, sx1], a1)
            out[dy, dx] = mul(h0, b0) + mul(h1, b1)                      # the column pass
    return out


def resample_flow(u, v, rescale, crop=None, zero_taps=True):
    """one flow field as dense_tracking reads it (:1131-1146): widened to double, cropped to crop = (x0, y0, cw, ch), resized, multiplied by
    (double)rescale.  u, v: fp32 (sh, sw) planes (only the valid columns).  -> float64 (h, w) planes"""
    with np.errstate(invalid="ignore", over="ignore"):
        out = []
        for p in (u, v):
            p = np.asarray(p, np.float32).astype(np.float64)
            if crop is not None:
                x0, y0, cw, ch = crop
                assert x0 >= 0 and y0 >= 0 and cw >= 1 and ch >= 1 and x0 + cw <= p.shape[1] and y0 + ch <= p.shape[0], "the crop leaves the flow"
                p = p[y0:y0 + ch, x0:x0 + cw]
            out.append(resize_linear_64f(p, rescale, zero_taps) * np.float64(f32(rescale)))
    return out[0], out[1]


def _cubic_coeffs(x):
    """interpolateCubic(x, coeffs) with A = -0.75f in float, then saturate_cast<short>(coeffs[k] * INTER_RESIZE_COEF_SCALE) (2048)"""
    A, one, x = f32(-0.75), f32(1), f32(x)
    xp = f32(x + one)
    xm = f32(one - x)
    c = [f32(0)] * 4
    c[0] = f32(f32(f32(f32(f32(f32(A * xp) - f32(f32(5) * A)) * xp) + f32(f32(8) * A)) * xp) - f32(f32(4) * A))
    c[1] = f32(f32(f32(f32(f32(f32(A + f32(2)) * x) - f32(A + f32(3))) * x) * x) + one)
    c[2] = f32(f32(f32(f32(f32(f32(A + f32(2)) * xm) - f32(A + f32(3))) * xm) * xm) + one)
    c[3] = f32(f32(f32(one - c[0]) - c[1]) - c[2])
    return [int(np.clip(np.rint(f32(k * f32(2048))), -32768, 32767)) for k in c]


def _cubic_taps(n_dst, scale):
    idx, co = [], []
    for d in range(n_dst):
        f = f32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        idx.append(s)
        co.append(_cubic_coeffs(f32(f - f32(s))))
    return idx, co


def resize_cubic_8u(src, rescale):
    """cv::resize(src, dst, Size(0, 0), rescale, rescale, INTER_CUBIC) of one uint8 image: taps s - 1 .. s + 2 with clamped indices"""
    src = np.asarray(src, np.uint8).astype(np.int64)
    sh, sw = src.shape
    dw, dh = target_size(sw, sh, rescale)
    scale = 1.0 / np.float64(f32(rescale))
    xo, xc = _cubic_taps(dw, scale)
    yo, yc = _cubic_taps(dh, scale)
    out = np.zeros((dh, dw), np.uint8)
    for dy in range(dh):
        rows = [min(max(yo[dy] - 1 + j, 0), sh - 1) for j in range(4)]
        for dx in range(dw):
            cols = [min(max(xo[dx] - 1 + i, 0), sw - 1) for i in range(4)]
            total = 0
            for j in range(4):
                hs = sum(int(src[rows[j], cols[i]]) * xc[dx][i] for i in range(4))    # the row pass: an int
                total += hs * yc[dy][j]
            out[dy, dx] = min(max((total + (1 << 21)) >> 22, 0), 255)   # FixedPtCast<int, uchar, 22>
    return out


def decode_occlusion_scaled(grey, rescale):
    """a jet's occlusion image as dense_tracking reads it (:1169-1189): cubic resize, medianBlur 3 (replicated border), 255 - x; 0 = occluded"""
    return (255 - median3(resize_cubic_8u(grey, rescale)).astype(np.int32)).astype(np.uint8)
