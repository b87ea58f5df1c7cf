"""The driver's raw ingest restated pixel by pixel in numpy scalars: bayer2rgbGR (utils/utils.cpp:1242-1334), cv::cvtColor(CV_Bayer*2RGB) on 8-bit data as
slow_flow.cpp:502-520 uses it, rawWeighting (utils.cpp:1336-1374).  One statement per statement of slowflow_amd/host/ingest.cpp, in the C types of its
expressions: a float sum stays np.float32, `0.25 * sum` and `g * 0.5 * sum` are double products rounded once.  tests/test_mosaic.py holds these against
the whole-array formulations of tests/test_host.py, which the existing tests pin to the host binary; the GPU tests compare the kernels with these."""
import numpy as np

f32, f64 = np.float32, np.float64
REDS = [(0, 0), (1, 0), (0, 1), (1, 1)]


def _m1(v):
    return v - 1 if v > 0 else v + 1


def _p1(v, n):
    return v + 1 if v < n - 1 else v - 1


def bayer_gr(src, rx, ry):
    """(H, W) mosaic -> (3, H, W) fp32; the element goes through a plain (float)"""
    s = np.asarray(src).astype(f32)
    H, W = s.shape
    assert W >= 2 and H >= 2, "the reference reads outside the image"
    G = np.zeros((H, W), f32)
    R, B = np.zeros((H, W), f32), np.zeros((H, W), f32)

    def is_green(y, x):
        blue_row = (y + (1 - ry)) % 2 == 0
        return blue_row, ((x + rx) % 2 == 0) if blue_row else ((x + (1 - rx)) % 2 == 0)
    with np.errstate(all="ignore"):
        for y in range(H):
            ym1, yp1 = _m1(y), _p1(y, H)
            for x in range(W):
                xm1, xp1 = _m1(x), _p1(x, W)
                if is_green(y, x)[1]:
                    G[y, x] = s[y, x]
                else:
                    t = f32(f32(f32(s[ym1, x] + s[yp1, x]) + s[y, xm1]) + s[y, xp1])
                    G[y, x] = f32(0.25 * f64(t))
        q = lambda yy, xx: f32(s[yy, xx] / G[yy, xx])
        for y in range(H):
            ym1, yp1 = _m1(y), _p1(y, H)
            for x in range(W):
                xm1, xp1 = _m1(x), _p1(x, W)
                g = f64(G[y, x])
                blue_row, green = is_green(y, x)
                if green:
                    vert = f32(g * 0.5 * f64(f32(q(ym1, x) + q(yp1, x))))
                    horz = f32(g * 0.5 * f64(f32(q(y, xm1) + q(y, xp1))))
                    R[y, x], B[y, x] = (vert, horz) if blue_row else (horz, vert)
                else:
                    d = f32(f32(f32(q(ym1, xm1) + q(ym1, xp1)) + q(yp1, xm1)) + q(yp1, xp1))
                    diag = f32(g * 0.25 * f64(d))
                    R[y, x], B[y, x] = (diag, s[y, x]) if blue_row else (s[y, x], diag)
    return np.stack([R, G, B])


def bayer_cv8u(src, rx, ry):
    """(H, W) mosaic -> (3, H, W) fp32 holding integers 0..255; W < 3 or H < 3: zeros"""
    s = np.asarray(src).astype(f32)
    H, W = s.shape
    out = np.zeros((3, H, W), f32)
    if W < 3 or H < 3:
        return out
    m = np.clip(np.rint(s.astype(f64)), 0, 255).astype(np.int64)           # lrintf: half to even; saturate
    for y in range(1, H - 1):
        red_row = (y - ry) % 2 == 0
        for x in range(1, W - 1):
            red_col = (x - rx) % 2 == 0
            c = m[y, x]
            if red_row == red_col:
                cross = (m[y - 1, x] + m[y + 1, x] + m[y, x - 1] + m[y, x + 1] + 2) >> 2
                diag = (m[y - 1, x - 1] + m[y - 1, x + 1] + m[y + 1, x - 1] + m[y + 1, x + 1] + 2) >> 2
                out[:, y, x] = (c, cross, diag) if red_row else (diag, cross, c)
            else:
                horiz, vert = (m[y, x - 1] + m[y, x + 1] + 1) >> 1, (m[y - 1, x] + m[y + 1, x] + 1) >> 1
                out[:, y, x] = (horiz, c, vert) if red_row else (vert, c, horiz)
        out[:, y, 0] = out[:, y, 1]
        out[:, y, W - 1] = out[:, y, W - 2]
    out[:, 0, :] = out[:, 1, :]
    out[:, H - 1, :] = out[:, H - 2, :]
    return out


def raw_weights(w, h, rx, ry, weight):
    """(3, h, w) fp32"""
    weight = f32(min(max(f32(weight), f32(0)), f32(3)))
    other = f32(f32(0.5) * f32(f32(3) - weight))
    W = np.zeros((3, h, w), f32)
    for y in range(h):
        for x in range(w):
            r = g = b = other
            if (y + (1 - ry)) % 2 == 0:
                green = (ry == 1 and (x + (1 - rx)) % 2 == 0) or (ry == 0 and (x + rx) % 2 == 0)
                if green:
                    g = weight
                else:
                    b = weight
            else:
                green = (ry == 0 and (x + (1 - rx)) % 2 == 0) or (ry == 1 and (x + rx) % 2 == 0)
                if green:
                    g = weight
                else:
                    r = weight
            W[:, y, x] = (r, g, b)
    return W


def demosaic(src, rx, ry, method):
    return bayer_cv8u(src, rx, ry) if method == 2 else bayer_gr(src, rx, ry)


def demosaic_crop(src, rx, ry, method, origin=(0, 0), size=None):
    """the crop the driver takes (slow_flow.cpp:533-536): the FULL mosaic demosaiced, then sliced -- borders, ring and colours are the full mosaic's"""
    H, W = np.asarray(src).shape
    x0, y0 = origin
    w, h = (W - x0, H - y0) if size is None else size
    assert 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= H
    return demosaic(src, rx, ry, method)[:, y0:y0 + h, x0:x0 + w]


def rescaled_size(w, h, scale):
    """cv::resize(Size(0, 0), fx, fy): lrint of the product in double, scale an fp32 value (the driver reads the cfg's scale as float)"""
    s = float(f32(scale))
    return int(np.rint(w * s)), int(np.rint(h * s))


def rescale_sigma(scale):
    """slow_flow.cpp:551: (float)(1 / sqrt(2 * scale)), the square root taken in double of the fp32 product (exact: a doubling)"""
    return float(f32(1.0 / np.sqrt(f64(f32(2) * f32(scale)))))
