"""dense_tracking's reduced reference image (dense_tracking.cpp:931-936) restated in numpy int64 from the definition in INTEGRATION.md 4c': the 8-bit step,
the taps of the 8-bit Gaussian blur, the separable integer blur with a replicated border and the tie rule of OpenCV's x86-64 column pass, the 2 x 2
reduction.  It shares no code with slowflow_amd/csrc/ref_image.h: the kernel (tests/test_ref_image.py), the host function (tests/test_ref_image_host.py)
and the accumulate program (tests/test_accumulate_fill_skip.py) are compared against it with ==."""
import numpy as np

SERVED = (0, 1, 3)


def taps(skip):
    """(k, c): the integer taps in 8 fractional bits and the float taps they are rounded from"""
    img_scale = float(np.float32(1.0) / np.float32(skip + 1))
    sigma = 1.0 / np.sqrt(2.0 * img_scale)
    n = int(np.rint(sigma * 6 + 1)) | 1
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    c = np.exp(-0.5 / (sigma * sigma) * x * x).astype(np.float32)
    total = c.astype(np.float64).sum()
    c = (c.astype(np.float64) * (1.0 / total)).astype(np.float32)
    k = np.rint(c.astype(np.float64) * 256).astype(np.int64)
    return k, c


def grid(w, h, skip):
    """(gw, gh), or None where OpenCV's resize would give another size than the accumulation grid"""
    img_scale = float(np.float32(1.0) / np.float32(skip + 1))
    gw, gh = w // (skip + 1), h // (skip + 1)
    if gw < 1 or gh < 1 or int(np.rint(w * img_scale)) != gw or int(np.rint(h * img_scale)) != gh:
        return None
    return gw, gh


def to_8bit(rgb, norm=1.0):
    """[3][h][w] samples as read -> int64 in 0 .. 255: times norm in fp32, to nearest with ties to even, saturated"""
    v = np.rint(np.asarray(rgb, np.float32) * np.float32(norm))
    return np.clip(v, 0, 255).astype(np.int64)


def blur(p8, skip, tie="defined"):
    """[3][h][w] int64 -> the blurred 8-bit image.  tie: "defined" (to even below 3 w & ~3 of the interleaved row, half up in the tail), "up" or "even" everywhere"""
    k, _ = taps(skip)
    n, r = len(k), len(k) // 2
    _, h, w = p8.shape
    xs = np.clip(np.arange(w)[None, :] + np.arange(n)[:, None] - r, 0, w - 1)          # [n][w]
    ys = np.clip(np.arange(h)[None, :] + np.arange(n)[:, None] - r, 0, h - 1)
    row = sum(k[i] * p8[:, :, xs[i]] for i in range(n))
    assert row.max() <= 255 * 256
    val = sum(k[i] * row[:, ys[i], :] for i in range(n))
    up = (val + 32768) >> 16
    q = val >> 16
    even = np.where((val & 65535) == 32768, q + (q & 1), up)
    if tie == "up":
        out = up
    elif tie == "even":
        out = even
    else:
        e = 3 * np.arange(w)[None, None, :] + np.arange(3)[:, None, None]
        out = np.where(e < ((3 * w) & ~3), even, up)
    return np.clip(out, 0, 255)


def reduce(b8, skip):
    """the blurred image -> [3][gh][gw]: the rounded mean of the 2 x 2 pixels at (skip + 1) g + (skip - 1) // 2 and the next, rows and columns"""
    _, h, w = b8.shape
    gw, gh = w // (skip + 1), h // (skip + 1)
    y0 = (skip + 1) * np.arange(gh) + (skip - 1) // 2
    x0 = (skip + 1) * np.arange(gw) + (skip - 1) // 2
    a = b8[:, y0][:, :, x0] + b8[:, y0][:, :, x0 + 1] + b8[:, y0 + 1][:, :, x0] + b8[:, y0 + 1][:, :, x0 + 1]
    return (a + 2) >> 2


def reference_rgb8(rgb, skip, norm=1.0, tie="defined"):
    """[3][h][w] samples as read -> the reduced 8-bit image [3][gh][gw] as uint8"""
    assert skip in SERVED
    p8 = to_8bit(rgb, norm)
    if skip == 0:
        return p8.astype(np.uint8)
    assert grid(p8.shape[2], p8.shape[1], skip) is not None
    return reduce(blur(p8, skip, tie), skip).astype(np.uint8)


def float_bound(skip):
    """how far the integer stage may lie from a float64 convolution with the float taps followed by the 2 x 2 mean, in grey levels: each pass replaces c_i
    by k_i / 256 (255 sum |k_i / 256 - c_i| per pass), the two roundings add less than one level"""
    k, c = taps(skip)
    return 255 * 2 * float(np.abs(k / 256.0 - c.astype(np.float64)).sum()) + 1


def float_reference(p8, skip):
    """the same image by a float64 convolution with the float taps (replicated border) and the 2 x 2 mean: the sanity bound's other side"""
    _, c = taps(skip)
    c = c.astype(np.float64)
    n, r = len(c), len(c) // 2
    _, h, w = p8.shape
    xs = np.clip(np.arange(w)[None, :] + np.arange(n)[:, None] - r, 0, w - 1)
    ys = np.clip(np.arange(h)[None, :] + np.arange(n)[:, None] - r, 0, h - 1)
    f = p8.astype(np.float64)
    row = sum(c[i] * f[:, :, xs[i]] for i in range(n))
    val = sum(c[i] * row[:, ys[i], :] for i in range(n))
    gw, gh = w // (skip + 1), h // (skip + 1)
    y0 = (skip + 1) * np.arange(gh) + (skip - 1) // 2
    x0 = (skip + 1) * np.arange(gw) + (skip - 1) // 2
    return (val[:, y0][:, :, x0] + val[:, y0][:, :, x0 + 1] + val[:, y0 + 1][:, :, x0] + val[:, y0 + 1][:, :, x0 + 1]) / 4


def tie_image():
    """the 10 x 6 image at skip 1 whose rows are the constants 0, 128, 192, 192, 192, 0 in all columns and channels: its blur meets exact ties"""
    rows = np.array([0, 128, 192, 192, 192, 0], np.float32)
    return np.broadcast_to(rows[None, :, None], (3, 6, 10)).copy()
