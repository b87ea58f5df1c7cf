"""dense_tracking's reduced reference image on the GPU (slowflow_amd/csrc/ref_image.hip; include/slowflow_amd.h: sfa_reference_lab_device,
sfa_reference_lab): the kernel's 8-bit image against tests/ref_image_ref.py, the numpy restatement of INTEGRATION.md 4c''s definition, and its Lab planes
against device.rgb8_to_lab of that 8-bit image (k_rgb8_to_lab: pinned exhaustively by tests/test_epic_init.py).  == on bytes and bit patterns.
The kernel's tiles are 64 x 16 grid pixels at skip 1 and 64 x 8 at skip 3: the larger shapes span two tiles and a remainder in both directions."""
import ctypes as C

import numpy as np
import pytest

import ref_image_ref as R
import slowflow_amd as sfa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


def bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def noise(n, w, h, seed, top=256):
    return np.random.default_rng(seed).integers(0, top, (n, 3, h, w)).astype(np.float32)


def check(ctx, dev, rgb, skip, norm=1.0):
    """rgb: numpy [n][3][h][w].  The 8-bit image equals the restatement, the Lab planes the pinned kernel's of that image"""
    from slowflow_amd import device
    lab, rgb8 = device.reference_lab(ctx, torch.from_numpy(rgb).to(dev), skip, norm, return_rgb8=True)
    torch.cuda.synchronize()
    want = np.stack([R.reference_rgb8(f, skip, norm) for f in rgb])
    assert rgb8.dtype == torch.uint8 and tuple(rgb8.shape) == want.shape
    assert np.array_equal(rgb8.cpu().numpy(), want)
    want_lab = device.rgb8_to_lab(ctx, torch.from_numpy(want.astype(np.float32)).to(dev), 1.0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(lab), bits(want_lab))
    only_lab = device.reference_lab(ctx, torch.from_numpy(rgb).to(dev), skip, norm)          # without the 8-bit output: the same planes
    torch.cuda.synchronize()
    assert np.array_equal(bits(only_lab), bits(lab))
    return want


@pytest.mark.parametrize("w,h,skip", [(9, 5, 1), (13, 9, 3), (140, 44, 1), (268, 76, 3)])
def test_kernel_equals_the_restatement(ctx, dev, w, h, skip):
    want = check(ctx, dev, noise(1, w, h, seed=100 * w + skip), skip)
    assert want.shape[2:] == (h // (skip + 1), w // (skip + 1)) and len(np.unique(want)) > 8                 # (blurred noise: a narrow band of greys, not a constant)


@pytest.mark.parametrize("skip", [1, 3])
def test_batch_of_three_with_strided_source_and_destination(ctx, dev, skip):
    from slowflow_amd import device
    n, w, h = 3, 76, 36
    gw, gh = sfa.reference_grid(w, h, skip)
    rgb = noise(n, w, h, seed=7 + skip)
    big = torch.full((n + 1, 3, h + 3, 2 * (w + 5)), 1e9, device=dev)
    src = big[:n, :, 1:h + 1, 2:2 * w + 2:2]                                  # images, rows and columns apart
    src.copy_(torch.from_numpy(rgb).to(dev))
    out = torch.full((n, 3, gh + 2, gw + 7), -777.0, device=dev)
    out8 = torch.full((n, 3, gh + 1, 2 * gw + 3), 201, dtype=torch.uint8, device=dev)
    device.reference_lab(ctx, src, skip, out=out[:, :, 1:gh + 1, 3:gw + 3], out_rgb8=out8[:, :, :gh, 1:2 * gw + 1:2])
    torch.cuda.synchronize()
    want = np.stack([R.reference_rgb8(f, skip) for f in rgb])
    assert np.array_equal(out8[:, :, :gh, 1:2 * gw + 1:2].cpu().numpy(), want)
    want_lab = device.rgb8_to_lab(ctx, torch.from_numpy(want.astype(np.float32)).to(dev), 1.0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out[:, :, 1:gh + 1, 3:gw + 3]), bits(want_lab))
    o = out.cpu().numpy().copy(); o[:, :, 1:gh + 1, 3:gw + 3] = -777.0
    o8 = out8.cpu().numpy().copy(); o8[:, :, :gh, 1:2 * gw + 1:2] = 201
    assert (o == -777.0).all() and (o8 == 201).all()                           # nothing outside the views was written


@pytest.mark.parametrize("skip", [1, 3])
def test_sixteen_bit_samples_with_norm(ctx, dev, skip):
    norm = float(np.float32(1.0 / 255))
    rgb = noise(1, 37, 21, seed=3, top=65536)
    rgb[0, 0, 0, :6] = [65535, 65408, 65407.5, 65152.5, 127.5, 382.5]          # 257 and 256.5 saturate; x.5 at the 8-bit step: ties to even
    rgb[0, 1, 20, 30:] = 65535
    p8 = R.to_8bit(rgb[0], norm)
    assert p8[0, 0, 0] == 255 and p8[0, 0, 1] == 255 and p8.max() == 255
    check(ctx, dev, rgb, skip, norm)


def test_tie_rule(ctx, dev):
    t = R.tie_image()
    d, up, even = (R.reference_rgb8(t, 1, tie=k) for k in ("defined", "up", "even"))
    assert (d[:, 1, 0] != up[:, 1, 0]).all()                                   # an input without ties could not tell the rules apart: this one does
    assert np.argwhere(d != even).tolist() == [[1, 1, 4], [2, 1, 4]]           # the scalar tail: 3 * 10 & ~3 = 28
    want = check(ctx, dev, t[None], 1)
    assert np.array_equal(want[0], d)


def test_skip_0_equals_rgb8_to_lab(ctx, dev):
    from slowflow_amd import device
    rgb = np.random.default_rng(5).uniform(-20, 300, (2, 3, 19, 301)).astype(np.float32)
    src = torch.from_numpy(rgb).to(dev)
    lab, rgb8 = device.reference_lab(ctx, src, 0, return_rgb8=True)
    want = device.rgb8_to_lab(ctx, src, 1.0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(lab), bits(want))
    assert np.array_equal(rgb8.cpu().numpy(), np.stack([R.reference_rgb8(f, 0) for f in rgb]))


def test_host_plane_wrapper(ctx, dev):
    from slowflow_amd import device
    rgb = noise(1, 72, 36, seed=11)[0]                                         # a size every served skip takes: 72 x 36, 36 x 18, 18 x 9
    for skip in (0, 1, 3):
        lab, rgb8 = ctx.reference_lab(rgb, skip, return_rgb8=True)
        assert np.array_equal(rgb8, R.reference_rgb8(rgb, skip))
        want = device.rgb8_to_lab(ctx, torch.from_numpy(rgb8.astype(np.float32)[None]).to(dev), 1.0)
        torch.cuda.synchronize()
        assert np.array_equal(lab.view(np.uint32), bits(want)[0])
        assert np.array_equal(ctx.reference_lab(rgb, skip).view(np.uint32), lab.view(np.uint32))


def test_refusals_name_the_argument_and_launch_nothing(ctx, dev):
    from slowflow_amd import device
    L = device._lib()
    LL4 = C.c_longlong * 4

    def call(w, h, skip, src, dst, dst8=None):
        gw, gh = max(w // max(skip + 1, 1), 1), max(h // max(skip + 1, 1), 1)
        return L.sfa_reference_lab_device(ctx.h, 1, w, h, skip, C.c_void_p(src.data_ptr()), LL4(3 * h * w, h * w, w, 1), 1.0, C.c_void_p(dst.data_ptr()),
                                          LL4(3 * gh * gw, gh * gw, gw, 1), C.c_void_p(dst8.data_ptr()) if dst8 is not None else None,
                                          LL4(3 * gh * gw, gh * gw, gw, 1) if dst8 is not None else None)

    src = torch.ones((1, 3, 16, 16), device=dev)
    dst = torch.full((1, 3, 16, 16), -777.0, device=dev)
    for w, h, skip, words in ((16, 16, 2, ("skip = 2", "not dyadic")), (16, 16, 7, ("skip = 7", "257")), (16, 16, 8, ("skip = 8",)), (16, 16, -1, ("skip = -1",)),
                              (7, 8, 1, ("w x h = 7 x 8", "4 x 4", "3 x 4")), (8, 7, 1, ("w x h = 8 x 7",))):
        assert call(w, h, skip, src, dst) == -1, (w, h, skip)
        msg = L.sfa_last_error(ctx.h).decode()
        assert "sfa_reference_lab_device" in msg and all(word in msg for word in words), msg
    with pytest.raises(sfa.SlowflowError, match="skip = 2"):
        device.reference_lab(ctx, src, 2)
    buf = torch.ones((3, 3, 16, 16), device=dev)                               # the Lab image of skip 0 over its own source; the 8-bit image over the Lab image
    with pytest.raises(sfa.SlowflowError, match="lab_dev overlaps rgb_dev"):
        device.reference_lab(ctx, buf[0:2], 0, out=buf[1:3])
    assert call(16, 16, 1, src, dst, dst8=dst) == -1 and "overlaps" in L.sfa_last_error(ctx.h).decode() and "rgb8_dev" in L.sfa_last_error(ctx.h).decode()
    assert call(16, 16, 1, src, src) == -1 and "lab_dev overlaps rgb_dev" in L.sfa_last_error(ctx.h).decode()
    with pytest.raises(sfa.SlowflowError, match="not in GPU memory|no __cuda_array_interface__"):
        device.reference_lab(ctx, torch.ones((1, 3, 8, 8)), 1)
    torch.cuda.synchronize()
    assert bool((dst == -777.0).all()) and bool((buf == 1).all()) and bool((src == 1).all())      # nothing was launched
    check(ctx, dev, noise(1, 16, 16, seed=1), 1)                               # and the context runs a valid call
