"""Plain restatements of what dense_tracking does around its EpicFlow fill-in, written from the reference's behaviour (like accum_ref.py and fuse_ref.py):
removeSmallSegments (utils/utils.cpp:169-284), the match loop (dense_tracking.cpp:1274-1289), the sample loop's float step and the trajectory scaling
(:1304-1305).  No labelling library: the region growing runs in the reference's own order, so that the GPU's order-free form is tested against it."""
import numpy as np


def remove_small_segments(F, min_segment_size=100, similarity_threshold=0.1):
    """F: int (h, w).  Returns F after removeSmallSegments: seeds in column-major scan order (u outer, v inner), a list grown over the four neighbours
    (left, right, up, down) that are not done and whose value differs from the current pixel's by at most the threshold, every pixel reached marked done,
    and the pixels of a list shorter than min_segment_size set to 0 in place"""
    h, w = F.shape
    f = [int(v) for v in F.reshape(-1)]
    done = [0] * (w * h)
    for u in range(w):
        for v in range(h):
            start = v * w + u
            if done[start]:
                continue
            seg = [start]
            curr = 0
            while curr < len(seg):
                a = seg[curr]
                cu, cv = a % w, a // w
                fa = f[a]
                for nu, nv in ((cu - 1, cv), (cu + 1, cv), (cu, cv - 1), (cu, cv + 1)):
                    if nu >= 0 and nv >= 0 and nu < w and nv < h:
                        b = nv * w + nu
                        if not done[b] and abs(fa - f[b]) <= similarity_threshold:
                            seg.append(b)
                            done[b] = 1
                curr += 1
                done[a] = 1
            if len(seg) < min_segment_size:
                for a in seg:
                    f[a] = 0
    return np.array(f, dtype=np.int32).reshape(h, w)


def consistent_regions(tracked, full, min_size=100):
    """(tracked == full) as the reference's int map (dense_tracking.cpp:1223-1226), then remove_small_segments: uint8 (h, w)"""
    return remove_small_segments((np.asarray(tracked) == full).astype(np.int32), min_size).astype(np.uint8)


def fill_samples(extent, epic_skip):
    """`for (int x = floor(0.5f * epic_skip); x < extent; x += epic_skip)`: the step is a float, and the int takes the truncated fp32 sum"""
    skip = np.float32(epic_skip)
    out = []
    x = int(np.floor(np.float32(0.5) * skip))
    while x < extent:
        out.append(x)
        x = int(np.float32(x) + skip)
    return np.array(out, dtype=np.int32)


def fill_matches(acc_u, acc_v, mask, xs, ys, divisor):
    """acc_u, acc_v: float64 (J, h, w), mask (h, w).  Returns a list of J fp32 arrays (m, 4): x, y, x + u / divisor, y + v / divisor (fp64), stored as floats"""
    out = []
    for j in range(acc_u.shape[0]):
        rows = []
        for y in ys:
            for x in xs:
                if mask[y, x] == 1:
                    rows.append((np.float32(x), np.float32(y), np.float32(np.float64(x) + acc_u[j, y, x] / np.float64(divisor)),
                                 np.float32(np.float64(y) + acc_v[j, y, x] / np.float64(divisor))))
        out.append(np.array(rows, dtype=np.float32).reshape(-1, 4))
    return out


def fill_matches_vec(acc_u, acc_v, mask, xs, ys, divisor):
    """fill_matches without its Python loops, for the sample counts of the workload: the samples in raster order (rows ys, columns xs), the same
    fp64 sum and division and the same conversion to float per element.  tests/test_second_trips.py holds it to the loop on the 70 x 45 scene"""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    yy, xx = np.repeat(ys, len(xs)), np.tile(xs, len(ys))
    sel = mask[yy, xx] == 1
    x, y = xx[sel], yy[sel]
    div = np.float64(divisor)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(acc_u.shape[0]):
            tx, ty = x.astype(np.float64) + acc_u[j, y, x] / div, y.astype(np.float64) + acc_v[j, y, x] / div
            out.append(np.stack([x.astype(np.float32), y.astype(np.float32), tx.astype(np.float32), ty.astype(np.float32)], 1).reshape(-1, 4))
    return out


def fill_trajectories(flow_x, flow_y, w, scale):
    """flow_x, flow_y: fp32 (J, h, stride).  Returns acc_u, acc_v float64 (J, h, w) = (double)(plane * (float) scale) and tracked int32 (h, w) = J"""
    with np.errstate(all="ignore"):
        au = (flow_x[:, :, :w].astype(np.float32) * np.float32(scale)).astype(np.float64)
        av = (flow_y[:, :, :w].astype(np.float32) * np.float32(scale)).astype(np.float64)
    return au, av, np.full(flow_x.shape[1:2] + (w,), flow_x.shape[0], np.int32)
