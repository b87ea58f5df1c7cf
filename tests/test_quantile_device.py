"""adaptiveFR's flow-magnitude quantile and maximum for groups of flows that already live in GPU memory (csrc/quantile.hip:
sfa_flow_magnitude_quantiles_device; slowflow_amd.device.flow_quantiles).  The selection is exact, so every comparison is `==` on both doubles of a
group (NaN, which equals nothing, is compared as NaN on both sides).  Expected values come from two places that must agree: the host path
(Context.flow_magnitude_quantile) on the same values, and a numpy restatement of adaptiveFR.cpp:645-668 that needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import slowflow_amd as sfa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H = 37, 19                                    # 703 values per field: no multiple of the 256 threads of a block


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ---- the expected values ----------------------------------------------------------------------------------------------------------------------
def np_group(flow, scale, q):
    """one group [n,2,h,w]: fp32 scale, fp32 a*a + b*b, np.sqrt in fp32, np.sort on the sign-cleared bit patterns, ranks from sfa.quantile_ranks"""
    s = np.float32(scale)
    with np.errstate(all="ignore"):
        a, b = flow[:, 0].astype(np.float32) * s, flow[:, 1].astype(np.float32) * s
        m = np.sqrt(a * a + b * b)
    assert m.dtype == np.float32
    keys = np.sort(m.ravel().view(np.uint32) & np.uint32(0x7fffffff))
    k0, k1, average = sfa.quantile_ranks(keys.size, q)
    val = lambda k: np.float64(keys[k:k + 1].view(np.float32)[0])
    quant = np.float32(0.5) * (val(k0) + val(k1)) if average else val(k0)
    return float(quant), float(val(keys.size - 1))


def group_keys(flow, scale):
    s = np.float32(scale)
    with np.errstate(all="ignore"):
        a, b = flow[:, 0] * s, flow[:, 1] * s
        return np.sqrt(a * a + b * b).ravel().view(np.uint32) & np.uint32(0x7fffffff)


def host_group(ctx, flow, scale, q):
    """the host path on the same values: planes of row stride w"""
    us = [np.ascontiguousarray(f[0]) for f in flow]
    vs = [np.ascontiguousarray(f[1]) for f in flow]
    return ctx.flow_magnitude_quantile(us, vs, flow.shape[3], scale, q)


def same_pair(got, want):
    return all(g == w or (np.isnan(g) and np.isnan(w)) for g, w in zip(got, want))


def expected(ctx, flow, scale, q, counts=None):
    """[G,n,2,h,w] -> [(quantile, max)] per group, host path and restatement agreeing"""
    out = []
    for g in range(flow.shape[0]):
        used = flow[g, :counts[g]] if counts is not None else flow[g]
        a, b = host_group(ctx, used, scale, q), np_group(used, scale, q)
        assert same_pair(a, b), (g, a, b)
        out.append(a)
    return out


def noise(seed, G, n, h=H, w=W, lo=-3.0, hi=3.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=(G, n, 2, h, w)).astype(np.float32)


def run(ctx, t, q=0.99, scale=1.0, counts=None, **kw):
    from slowflow_amd import device
    out = device.flow_quantiles(ctx, t, q, scale, counts, **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and out.is_cuda
    return [tuple(r) for r in out.cpu().numpy().tolist()]


def check(got, want):
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        assert same_pair(a, b), (g, a, b)


# ---- 1. one group equals the host path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [0.99, 0.5, 1.0])
def test_one_group_equals_the_host_path(ctx, dev, q):
    flow = noise(1, 1, 2)
    if q == 1.0:
        N = flow[0].size // 2
        assert sfa.quantile_ranks(N, q) == (N - 1, N - 1, False)               # the three wanted ranks coincide
    want = expected(ctx, flow, 2.0, q)
    check(run(ctx, torch.from_numpy(flow).to(dev), q, 2.0), want)
    got = run(ctx, torch.from_numpy(flow[0]).to(dev), q, 2.0)                   # [n,2,h,w] is one group
    assert len(got) == 1
    check(got, want)


# ---- 2. groups are independent -------------------------------------------------------------------------------------------------------------------
def test_groups_are_independent_and_unused_fields_do_not_count(ctx, dev):
    counts = [3, 1, 2]
    flow = noise(2, 3, 3)
    for g, mag in enumerate((1.0, 1e-3, 1e3)):                                  # the chosen bins differ per group
        flow[g] *= np.float32(mag)
        flow[g, counts[g]:] = np.inf
    want = expected(ctx, flow, 1.0, 0.99, counts)
    assert len({w[0] for w in want}) == 3 and all(np.isfinite(w[1]) for w in want)
    check(run(ctx, torch.from_numpy(flow).to(dev), 0.99, 1.0, counts), want)
    # without counts the +Inf fields count
    assert [g[1] for g in run(ctx, torch.from_numpy(flow).to(dev), 0.99, 1.0)] == [want[0][1], np.inf, np.inf]


# ---- 3. both branches of the rank rule -------------------------------------------------------------------------------------------------------------
def test_both_branches_of_the_rank_rule(ctx, dev):
    (wa, ha), (wb, hb) = (30, 10), (W, H)
    assert sfa.quantile_ranks(wa * ha, 0.99) == (296, 297, True) and sfa.quantile_ranks(wb * hb, 0.99) == (695, 695, False)
    for w, h in ((wa, ha), (wb, hb)):                                           # two sizes, two calls
        flow = noise(3, 1, 1, h, w)
        check(run(ctx, torch.from_numpy(flow).to(dev)), expected(ctx, flow, 1.0, 0.99))
    assert sfa.quantile_ranks(100, 0.99)[2] and not sfa.quantile_ranks(200, 0.99)[2]
    flow = noise(4, 2, 2, 4, 25)                                                # and two counts of one call
    want = expected(ctx, flow, 1.0, 0.99, [1, 2])
    check(run(ctx, torch.from_numpy(flow).to(dev), counts=[1, 2]), want)
    check(run(ctx, torch.from_numpy(flow).to(dev), counts=[2, 1]), expected(ctx, flow, 1.0, 0.99, [2, 1]))


# ---- 4. strides ---------------------------------------------------------------------------------------------------------------------------------
def test_strided_views_are_read_in_place(ctx, dev):
    flow = noise(5, 2, 3)
    want = expected(ctx, flow, 0.5, 0.99)
    t = torch.from_numpy(flow).to(dev)
    check(run(ctx, t, 0.99, 0.5), want)
    last = t.permute(0, 1, 3, 4, 2).contiguous()                                # [G,n,h,w,2] in memory
    assert last.permute(0, 1, 4, 2, 3).stride()[-1] == 2
    check(run(ctx, last.permute(0, 1, 4, 2, 3), 0.99, 0.5), want)
    padded = torch.full((2, 3, 2, H, 48), float("inf"), device=dev)             # rows padded to 48 columns
    padded[..., :W] = t
    check(run(ctx, padded[..., :W], 0.99, 0.5), want)
    big = torch.full((2, 3, 2, H + 1, W + 2), float("inf"), device=dev)         # a slice of a larger tensor
    big[:, :, :, 1:, 2:] = t
    check(run(ctx, big[:, :, :, 1:, 2:], 0.99, 0.5), want)
    check(run(ctx, t[:, :2], 0.99, 0.5), expected(ctx, flow[:, :2], 0.5, 0.99))                    # fewer fields than the tensor holds


# ---- 5. bit patterns ------------------------------------------------------------------------------------------------------------------------------
def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def test_zeros_denormals_inf_and_nan(ctx, dev):
    flow = noise(6, 1, 2)
    u = flow[0, 0, 0].ravel()
    u[:12] = f32([0x00000000, 0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x1e3ce508, 0x9e3ce508, 0x7f7fffff, 0x00800000])
    flow[0, 0, 1].ravel()[:12] = 0                                              # +0, -0, the denormals and the smallest normal alone: magnitude +0
    N = flow[0].size // 2
    keys = np.sort(group_keys(flow[0], 1.0))
    assert keys[0] == 0 and (keys > 0x7f800000).sum() == 2 and (keys == 0x7f800000).sum() == 3      # two NaN above three +Inf (3.4e38 squared overflows)
    t = torch.from_numpy(flow).to(dev)
    for q, top in ((0.5, None), ((N - 2.5) / N, "inf"), (1.0, "nan")):
        want = expected(ctx, flow, 1.0, q)
        got = run(ctx, t, q)
        check(got, want)
        assert np.isnan(got[0][1])                                              # NaN sorts above +Inf: it is the maximum
        assert top is None or (np.isinf(got[0][0]) if top == "inf" else np.isnan(got[0][0])), (q, got)


def test_a_group_of_equal_values_and_one_separated_only_by_the_last_pass(ctx, dev):
    flow = np.zeros((2, 2, 2, H, W), np.float32)
    flow[0, :, 0], flow[0, :, 1] = 3.0, -4.0                                    # every magnitude 5: one bin holds every rank in all three passes
    low = np.random.default_rng(7).integers(0, 1024, size=(2, H, W)).astype(np.uint32)
    flow[1, :, 0] = (np.uint32(0x40490000) | low).view(np.float32)              # v = 0: keys that differ in bits 9..0 only
    k = group_keys(flow[1], 1.0)
    assert (k.max() ^ k.min()) < 1024 and np.unique(k).size > 500 and np.unique(group_keys(flow[0], 1.0)).tolist() == [0x40a00000]
    t = torch.from_numpy(flow).to(dev)
    for q in (0.99, 0.5, 1.0):
        want = expected(ctx, flow, 1.0, q)
        assert want[0] == (5.0, 5.0)
        check(run(ctx, t, q), want)


# ---- 6. stream order, no host wait -----------------------------------------------------------------------------------------------------------------
def test_after_refine_pairs_on_a_side_stream(ctx, dev):
    from slowflow_amd import device
    frames = np.random.default_rng(8).uniform(0, 255, size=(2, 2, 3, 24, 32)).astype(np.float32)
    px = torch.from_numpy(frames).to(dev)
    device.refine_pairs(ctx, px)                                                # the pair job exists from here on: creating one waits, refining does not
    device.flow_quantiles(ctx, torch.zeros((1, 2, 2, 24, 32), device=dev))      # and so does the scratch
    side = torch.cuda.Stream(device=dev)
    buf = torch.zeros_like(px)
    keep = torch.empty((1, 2), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        buf.copy_(px)                                                           # the producer of the frames, on the side stream
        flows = device.refine_pairs(ctx, buf, stream=side)
        got = device.flow_quantiles(ctx, flows.view(1, 2, 2, 24, 32), 0.99, 0.25, stream=side)
        twice = got * 2                                                         # a consumer on the same stream
        again = device.flow_quantiles(ctx, flows.view(1, 2, 2, 24, 32), 0.99, 0.25, stream=side, out=keep)
    side.synchronize()
    assert again is keep and got.shape == (1, 2)
    fl = flows.cpu().numpy().reshape(1, 2, 2, 24, 32)
    want = expected(ctx, fl, 0.25, 0.99)
    assert want[0][1] > 0
    check([tuple(got.cpu().numpy()[0])], want)
    check([tuple(keep.cpu().numpy()[0])], want)
    assert np.array_equal(twice.cpu().numpy(), 2 * got.cpu().numpy())
    device.release_jobs(ctx)


# ---- 7. refusals: SFA_ERR_ARG, the argument named, nothing launched, the context still works -------------------------------------------------------
class HostArray:
    """a host array that claims to be a device array"""

    def __init__(self, a, dev):
        self.a, self.device = a, dev
        self.__cuda_array_interface__ = {"shape": a.shape, "typestr": "<f4" if a.dtype == np.float32 else "<f8", "data": (a.ctypes.data, False), "version": 3, "strides": None}


class Claimed:
    """a device tensor's memory under a shape and byte strides of the test's choosing"""

    def __init__(self, t, shape, strides):
        self.t, self.device = t, t.device
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (t.data_ptr(), False), "version": 3, "strides": tuple(4 * s for s in strides)}


@pytest.fixture(scope="module")
def valid(ctx, dev):
    flow = noise(9, 2, 2)
    return torch.from_numpy(flow).to(dev), expected(ctx, flow, 1.0, 0.99)


def refused(ctx, valid, call, *words):
    with pytest.raises(sfa.SlowflowError) as e:
        call()
    assert all(word in str(e.value) for word in words), str(e.value)
    check(run(ctx, valid[0]), valid[1])                                         # nothing was launched, and the context runs a valid call


def raw_call(ctx, G, n, counts, u, v, strides, w, h, q, out):
    from slowflow_amd import device
    ca = (C.c_int * len(counts))(*counts) if counts is not None else None
    ctx._ck(device._lib().sfa_flow_magnitude_quantiles_device(ctx.h, G, n, ca, C.c_void_p(u), C.c_void_p(v), (C.c_longlong * 4)(*strides), w, h, 1.0, q, C.c_void_p(out)),
            "sfa_flow_magnitude_quantiles_device")


def test_refusals_name_the_argument(ctx, dev, valid):
    from slowflow_amd import device
    FN = "sfa_flow_magnitude_quantiles_device"
    h, w = 4, 6
    t = torch.ones((2, 2, 2, h, w), device=dev)
    out = torch.zeros((2, 2), dtype=torch.float64, device=dev)
    dense = (2 * 2 * h * w, 2 * h * w, w, 1)
    u, v = t.data_ptr(), t.data_ptr() + 4 * h * w
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, torch.ones((65, 1, 2, 2, 2), device=dev)), FN, "-> -1", "G = 65")
    refused(ctx, valid, lambda: raw_call(ctx, 0, 2, None, u, v, dense, w, h, 0.99, out.data_ptr()), FN, "G = 0")
    refused(ctx, valid, lambda: raw_call(ctx, 2, 0, None, u, v, dense, w, h, 0.99, out.data_ptr()), FN, "n = 0")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t, counts=[2, 0]), FN, "counts[1] = 0")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t, counts=[3, 1]), FN, "counts[0] = 3")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t, counts=[1]), "counts", "1 entries for 2 groups")
    host = np.ones((2, 2, 2, h, w), np.float32)
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, host), "flow", "__cuda_array_interface__")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, HostArray(host, dev)), FN, "u_dev", "not device memory")
    refused(ctx, valid, lambda: raw_call(ctx, 2, 2, None, u, host.ctypes.data, dense, w, h, 0.99, out.data_ptr()), FN, "v_dev", "not device memory")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t, out=HostArray(np.zeros((2, 2)), dev)), FN, "out_dev", "not device memory")
    refused(ctx, valid, lambda: raw_call(ctx, 2, 2, None, u, v, dense, w, h, 0.99, 0), FN, "out_dev is null")
    far = Claimed(t, (2, 2, 2, h, w), (1 << 40, 2 * h * w, h * w, w, 1))       # the second group 2^40 elements after the first
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, far), FN, "u_dev", "beyond its allocation")
    # strides
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t[:, :, :, :1].expand(-1, -1, -1, h, -1)), FN, "strides", "row stride 0")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t[..., :1].expand(-1, -1, -1, -1, w)), FN, "strides", "column stride 0")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, Claimed(t, (2, 2, 2, h, w), (2 * 2 * h * w, 2 * h * w, h * w, -w, 1))), FN, "strides", "row stride -6")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, Claimed(t, (2, 2, 2, h, w), (2 * 2 * h * w, 2 * h * w, h * w, w, -1))), FN, "strides", "column stride -1")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t.as_strided((2, 2, 2, h, w), (2 * 2 * h * w, 2 * h * w, h * w, w - 1, 1))), FN, "strides", "share an address")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t[:, :1].expand(-1, 2, -1, -1, -1)), FN, "strides", "share an address")
    # out_dev inside the flows
    buf = torch.ones(2 * 2 * h * w, dtype=torch.float64, device=dev)
    inside = buf.view(torch.float32)[:2 * 2 * 2 * h * w].view(2, 2, 2, h, w)
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, inside, out=buf[4:8].view(2, 2)), FN, "out_dev overlaps u_dev")
    torch.cuda.synchronize()
    assert bool((buf == 1).all())                                               # nothing was written
    # more than 2^32 - 1 values in a group: refused before the view is looked at
    huge = (1, 3, 2, 40000, 40000)
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, Claimed(t, huge, (0, 2 * 40000 * 40000, 40000 * 40000, 40000, 1))), FN, "4800000000 values", "32-bit")
    # the rank rule's refusals, the group named
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t, q=0.0), FN, "group 0", "sfa_quantile_ranks", "q = 0")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t, q=1.5), FN, "group 0", "outside (0, 1]")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t, q=1e-12), FN, "group 0", "rank -1")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t[:, :, :1]), "flow", "[G,n,2,h,w]")
    refused(ctx, valid, lambda: device.flow_quantiles(ctx, t.double()), "flow", "element type")


# ---- 8. the host-pointer entry point keeps its bits around a grouped call ---------------------------------------------------------------------------
def test_the_host_path_is_unchanged_around_a_grouped_call(ctx, dev):
    flow = noise(10, 4, 2, 40, 64)
    before = [host_group(ctx, flow[g], 2.0, 0.99) for g in range(4)]
    assert before == [np_group(flow[g], 2.0, 0.99) for g in range(4)]
    t = torch.from_numpy(flow).to(dev)
    first = run(ctx, t, 0.99, 2.0)
    small = run(ctx, t[:1, :1, :, :5, :7], 0.99, 2.0)                           # a smaller call in the same scratch ...
    check(small, expected(ctx, flow[:1, :1, :, :5, :7], 2.0, 0.99))
    check(run(ctx, t, 0.99, 2.0), first)                                        # ... and the larger one again
    check(first, before)
    assert [host_group(ctx, flow[g], 2.0, 0.99) for g in range(4)] == before
