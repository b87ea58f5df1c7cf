"""The track job's per-rate exit into GPU memory (sfa_track_job_download_rate_device, sfa_track_job_download_best_device; TrackJob.download_rate_device,
download_best_device): strided and offset destinations hold exactly what download_rate / download_best copy to the host, with do_fuse 0 and 1, on T1 and
on T2 (row pitch 44 for 42 columns, skip 2); outputs left out are not written, and a sub-range of segments leaves the other segments' bytes as they were.
All comparisons are ==.  T2 gets a third segment (seed 23) so that both cases take the sub-ranges (s0, ns) = (1, 2) and (0, 1)."""
import numpy as np
import pytest

import slowflow_amd as sfa
import track_inputs as ti

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 3
SEEDS = {"T1": ti.T1.seeds[:3], "T2": ti.T2.seeds + (23,)}
ACC_FILL, ENERGY_FILL, TRACKED_FILL, BITS_FILL, BYTE_FILL = -12345.678, -9.25, -7, 0x5A5A5A5A5A5A5A5A, 0xAB     # values no result holds


@pytest.fixture(scope="module")
def ctx():
    c = sfa.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Destinations:
    """acc as a slice of a larger fp64 tensor (an extra plane in front, a row above and below, two and three columns beside: offset, padded pitch), the
    packed outputs contiguous over all N segments; everything filled with a sentinel"""

    def __init__(self, case, dev):
        gh, gw = case.gh, case.gw
        self.big = torch.full((N + 1, 2, gh + 2, gw + 5), ACC_FILL, dtype=torch.float64, device=dev)
        self.acc = self.big[1:, :, 1:1 + gh, 2:2 + gw]
        assert not self.acc.is_contiguous()
        self.tracked = torch.full((N, gh, gw), TRACKED_FILL, dtype=torch.int32, device=dev)
        self.energy = torch.full((N, gh, gw), ENERGY_FILL, dtype=torch.float64, device=dev)
        self.occ_bits = torch.full((N, gh, gw), BITS_FILL, dtype=torch.int64, device=dev)
        self.occluded = torch.full((N, gh, gw), BYTE_FILL, dtype=torch.uint8, device=dev)
        self.best = torch.full((N, gh, gw), BYTE_FILL, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def host(self):
        torch.cuda.synchronize()
        out = {k: getattr(self, k).cpu().numpy() for k in ("acc", "tracked", "energy", "occ_bits", "occluded", "best")}
        big = self.big.cpu().numpy().copy()
        big[1:, :, 1:-1, 2:-3] = ACC_FILL                                      # what lies around the view stays the sentinel
        assert np.array_equal(bits(big), bits(np.full(big.shape, ACC_FILL)))
        return out


def untouched(host, key, s):
    fill = dict(acc=ACC_FILL, tracked=TRACKED_FILL, energy=ENERGY_FILL, occ_bits=BITS_FILL, occluded=BYTE_FILL, best=BYTE_FILL)[key]
    a = host[key][s]
    return np.array_equal(bits(a), bits(np.full(a.shape, fill))) if a.dtype == np.float64 else bool((a == fill).all())


def holds(host, key, s, want):
    """segment s of a downloaded output against download_rate's dict (or download_best's array)"""
    if key == "acc":
        return np.array_equal(bits(host["acc"][s, 0]), bits(want["u"])) and np.array_equal(bits(host["acc"][s, 1]), bits(want["v"]))
    if key == "best":
        return np.array_equal(host["best"][s], want)
    if key == "energy":
        return np.array_equal(bits(host["energy"][s]), bits(want["energy"]))
    if key == "occ_bits":
        return np.array_equal(host["occ_bits"][s].view(np.uint64), want["occ_bits"])
    return np.array_equal(host[key][s], want[key])


RATE_KEYS = ("acc", "tracked", "energy", "occ_bits", "occluded")


@pytest.mark.parametrize("do_fuse", [0, 1])
@pytest.mark.parametrize("case", [ti.T1, ti.T2], ids=lambda c: c.name)
def test_rate_and_best_into_strided_destinations_equal_the_host_downloads(ctx, case, do_fuse):
    dev = torch.device("cuda", 0)
    job = sfa.TrackJob(ctx, case.params(n=N, do_fuse=do_fuse))
    for s, seed in enumerate(SEEDS[case.name]):
        seg = ti.segment(case, seed)
        for r in range(case.K):
            job.upload_flows(s, r, *seg["flows"][r])
        job.upload_frames(s, seg["frames"])
    job.run(N)
    want = [[job.download_rate(s, r) for r in range(case.K)] for s in range(N)]
    best = [job.download_best(s) for s in range(N)]
    assert any(np.isinf(w["energy"]).any() for row in want for w in row) and any(np.isfinite(w["energy"]).any() for row in want for w in row)
    assert len({tuple(b.ravel()) for b in best}) == N                          # the segments differ: an offset by one segment shows
    stream = torch.cuda.current_stream(dev)

    def download(d, r, keys, s0, ns):
        ctx.wait_stream(stream)
        if r is None:
            job.download_best_device(d.best[s0:s0 + ns], s0=s0)
        else:
            job.download_rate_device(r, s0=s0, **{k: getattr(d, k)[s0:s0 + ns] for k in keys})
        ctx.signal_stream(stream)
        return d.host()

    for r in range(case.K):
        d = Destinations(case, dev)
        host = download(d, r, RATE_KEYS, 1, 2)                                  # segments 1 and 2, every output
        for k in RATE_KEYS:
            assert untouched(host, k, 0) and holds(host, k, 1, want[1][r]) and holds(host, k, 2, want[2][r]), (r, k)
        host = download(d, r, ("acc", "energy", "occ_bits"), 0, 1)              # segment 0, tracked and occluded left out
        for k in RATE_KEYS:
            assert holds(host, k, 1, want[1][r]) and holds(host, k, 2, want[2][r]), (r, k)
            assert untouched(host, k, 0) if k in ("tracked", "occluded") else holds(host, k, 0, want[0][r]), (r, k)
        host = download(d, r, ("tracked", "occluded"), 0, 1)                    # and those two alone
        for k in RATE_KEYS:
            assert all(holds(host, k, s, want[s][r]) for s in range(N)), (r, k)
        assert untouched(host, "best", 0) and untouched(host, "best", 1) and untouched(host, "best", 2)
    d = Destinations(case, dev)
    host = download(d, None, (), 1, 2)
    assert untouched(host, "best", 0) and holds(host, "best", 1, best[1]) and holds(host, "best", 2, best[2])
    host = download(d, None, (), 0, 1)
    assert all(holds(host, "best", s, best[s]) for s in range(N))
    assert all(untouched(host, k, s) for k in RATE_KEYS for s in range(N))
    if do_fuse:
        assert all(np.array_equal(job.download_fused(s)["best"], best[s]) for s in range(N))
    job.close()
