"""sfa_fuse_hypotheses at the sizes where its kernels change path: the k_trws<4> | <8> | <16> instances and nodes that fill all K = 16 labels, grids at the
edges of the ordered sum's 512-node chunks, an anti-diagonal longer than the 256-thread workgroup, and a batch whose segments stop at different iterations.
Everything is IEEE == against tests/fuse_ref.py (test_fuse.check_equal); the restatement is first checked on the CPU at the same label counts.

Every GPU case asserts on the CPU, from fr.labels' counts or the restatement's output, that its inputs are what the case is for, before it opens the GPU."""
import numpy as np
import pytest

import fuse_ref as fr
from accum_ref import grid
from test_fuse import check_equal, ctx, same, synth, viterbi  # noqa: F401  (ctx: the module-scoped GPU context fixture)

kThreads, kChunk = 256, 512                                                     # fuse.hip: kTrwsThreads, kTrwsChunk


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# CPU: the restatement at up to 16 labels per node
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def mrf_of_counts(rng, gw, gh, counts, scale=1.0):
    """a grid MRF whose node p has counts[p] labels (0: no node)"""
    N = gw * gh
    theta = [rng.normal(0, 1, int(m)) for m in counts]
    PR, PD = [None] * N, [None] * N
    for p in range(N):
        y, x = divmod(p, gw)
        if not len(theta[p]):
            continue
        if x + 1 < gw and len(theta[p + 1]):
            PR[p] = np.abs(rng.normal(0, scale, (len(theta[p]), len(theta[p + 1]))))
        if y + 1 < gh and len(theta[p + gw]):
            PD[p] = np.abs(rng.normal(0, scale, (len(theta[p]), len(theta[p + gw]))))
    return theta, PR, PD


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("K", [9, 16])
def test_trws_scalar_equals_diagonal_form_up_to_16_labels(K, seed):
    rng = np.random.default_rng(300 + 10 * K + seed)
    gw, gh = int(rng.integers(3, 6)), int(rng.integers(2, 5))
    counts = rng.integers(0, K + 1, gw * gh)
    counts[[0, 1, gw]] = K                                                      # full nodes next to each other, right and down
    counts[gw + 1], counts[gw * gh - 1] = 0, 1                                  # no node among them; a one-label node
    assert counts.max() == K and counts.min() == 0 and len(set(counts.tolist())) > 3
    theta, PR, PD = mrf_of_counts(rng, gw, gh, counts)
    a = fr.trws_scalar(theta, PR, PD, gw, gh, 1e-5, 4)
    b = fr.trws_diag(theta, PR, PD, gw, gh, 1e-5, 4)
    assert same(a, b)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("vertical", [False, True])
def test_chains_of_up_to_16_labels_reach_the_viterbi_optimum(seed, vertical):
    rng = np.random.default_rng(400 + seed)
    n = int(rng.integers(3, 12))
    counts = rng.integers(1, 17, n)
    e = int(rng.integers(0, n - 1))
    counts[[e, e + 1]] = 16                                                     # one 16 x 16 edge
    k = int(rng.choice([k for k in range(n) if k not in (e, e + 1)]))
    counts[k] = max(9, int(counts[k]))                                          # and a node past 8 labels elsewhere
    assert ((counts[:-1] == 16) & (counts[1:] == 16)).any() and (counts > 8).sum() >= 3
    theta = [rng.normal(0, 1, int(m)) for m in counts]
    P = [rng.normal(0, 1, (len(theta[k]), len(theta[k + 1]))) for k in range(n - 1)]
    gw, gh = (1, n) if vertical else (n, 1)
    PR, PD = [None] * n, [None] * n
    for k in range(n - 1):
        (PD if vertical else PR)[k] = P[k]
    x, E, lb, its = fr.trws_diag(theta, PR, PD, gw, gh, -1.0, 2)
    assert its == 2
    opt = fr.energy_of(theta, PR, PD, gw, gh, viterbi(theta, P))
    assert E == opt
    assert lb <= opt + 1e-12
    assert same((x, E, lb, its), fr.trws_scalar(theta, PR, PD, gw, gh, -1.0, 2))


def test_spread_moves_the_slots_apart_and_draws_the_same_numbers():
    a = synth(np.random.default_rng(7), 16, 4, 16, 16, 0, 0.0)
    b = synth(np.random.default_rng(7), 16, 4, 16, 16, 0, 0.0, spread=6.0)
    assert np.array_equal(b[0][:, 0], a[0][:, 0]) and not np.array_equal(b[0][:, 1], a[0][:, 1])
    for k in range(1, 5):
        assert np.array_equal(a[k], b[k])
    for method in (0, 1):
        na = [len(l) for l in fr.labels(a[0][0], a[1][0], a[2][0], method, 0.1)]
        nb = [len(l) for l in fr.labels(b[0][0], b[1][0], b[2][0], method, 0.1)]
        assert np.median(na) < 8 and min(nb) == 16                              # unspread: the NMS break prunes; spread: every node keeps all 16


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def counts_of(want, gw, gh):
    return np.array([len(l) for l in want["lab"]]).reshape(gh, gw)


def has_neighbours(c, a, b):
    """some node where a(count) holds has a right / left / down / up neighbour where b(count) holds"""
    A, B = a(c), b(c)
    return bool((A[:, :-1] & B[:, 1:]).any() or (A[:, 1:] & B[:, :-1]).any() or (A[:-1] & B[1:]).any() or (A[1:] & B[:-1]).any())


NEED = {  # what a case's label counts c (gh, gw) must contain
    "exactly K and fewer": lambda c, K: (c == K).any() and (c < K).any(),
    "all 16": lambda c, K: K == 16 and (c == 16).all(),
    "16, over 8 and at most 8": lambda c, K: (c == 16).any() and ((c > 8) & (c < 16)).any() and (c <= 8).any() and (c > 0).all(),
    "none beside some": lambda c, K: has_neighbours(c, lambda v: v == 0, lambda v: v > 0) and (c > 4).any(),
    "none beside over 8": lambda c, K: has_neighbours(c, lambda v: v == 0, lambda v: v > 8) and has_neighbours(c, lambda v: v == 16, lambda v: v == 16),
    "16 beside 16": lambda c, K: has_neighbours(c, lambda v: v == 16, lambda v: v == 16),
    "any": lambda c, K: (c > 0).any(),
}


def run_case(request, w, h, skip, K, J, holes, method, spread, seed, need, node_holes=0.0, high_bits=False, pre=None, **kw):
    """one segment through the restatement, its preconditions (NEED[need] on the label counts, then pre(restatement's output, counts, occlusion words, energies)),
    then the GPU"""
    import slowflow_amd as sfa
    rng = np.random.default_rng(seed)
    U, V, energy, occ, weight = synth(rng, K, J, w, h, skip, holes, spread=spread)
    if node_holes:
        energy[:, :, rng.random(energy.shape[2:]) < node_holes] = np.inf       # whole nodes without any hypothesis
    if high_bits:
        occ |= rng.integers(0, 1 << 30, occ.shape, dtype=np.int64).astype(np.uint64) << np.uint64(J + 1)     # bits past t = Jets: masked off
    p = fr.Params(traj_sim_method=method, skip=skip, **kw)
    gw, gh, _, _ = grid(w, h, skip)
    want = fr.fuse(U[0], V[0], energy[0], occ[0], weight[0], p, w)
    c = counts_of(want, gw, gh)
    print("label counts 0..16:", np.bincount(c.reshape(-1), minlength=17).tolist(), "gpl", gw * gh, "iters", want["iters"])
    assert NEED[need](c, K), need
    if pre:
        pre(want, c, occ[0], energy[0])
    got = request.getfixturevalue("ctx").fuse_hypotheses(p.to_c(sfa), U, V, energy, occ, weight, w, h)
    check_equal(got, want)


# k_trws<4> | <8> | <16>: K on both sides of each boundary, with nodes that keep exactly K labels.  (K, method) on a 19 x 14 grid, skip 0.
@pytest.mark.gpu
@pytest.mark.parametrize("method", [1, 0])
@pytest.mark.parametrize("K", [4, 5, 8, 9, 16])
def test_gpu_fuse_at_the_template_boundaries(request, K, method):
    run_case(request, 19, 14, 0, K, 5, 0.15, method, 6.0, 19 * 1000 + 14 * 10 + K, "exactly K and fewer")


K16_CASES = [  # (w, h, skip, J, holes, node_holes, method, seed, need)
    (16, 16, 0, 4, 0.0, 0.0, 1, 1, "all 16"),                                   # every row of lab / theta / M filled to index 15
    (16, 16, 0, 4, 0.0, 0.0, 0, 1, "all 16"),
    (21, 13, 1, 6, 0.3, 0.0, 0, 15, "16, over 8 and at most 8"),               # ADJ, incr 2: o1 / o2 step by 2 on the weight plane
    (21, 13, 1, 6, 0.3, 0.0, 1, 15, "16, over 8 and at most 8"),
    # holes 0.9 is drawn per slot, so at most 6 of the 16 slots are present anywhere: k_trws<16> with empty and nearly empty nodes, not with full ones.
    # The two rows after it empty whole nodes instead (node_holes) and so put nodes without labels beside nodes with 16.
    (12, 11, 0, 5, 0.9, 0.0, 1, 3, "none beside some"),
    (13, 11, 0, 5, 0.0, 0.3, 1, 6, "none beside over 8"),
    (31, 23, 2, 3, 0.05, 0.2, 0, 8, "none beside over 8"),                     # the same with ADJ and incr 3
]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,skip,J,holes,node_holes,method,seed,need", K16_CASES)
def test_gpu_fuse_16_slots(request, w, h, skip, J, holes, node_holes, method, seed, need):
    run_case(request, w, h, skip, 16, J, holes, method, 6.0, seed, need, node_holes=node_holes)


# spread 6.0 keeps the NMS from ever discarding; with a small spread it discards at nodes that have already kept more than 8 labels, so the `break`
# of k_fuse_labels cuts a list past index 8 short
@pytest.mark.gpu
@pytest.mark.parametrize("method,spread", [(1, 0.05), (0, 0.2)])
def test_gpu_fuse_nms_break_after_more_than_8_kept(request, method, spread):
    def pre(want, c, occ, energy):
        present = (energy != np.inf).sum(0)
        cut = (c > 8) & (c < present)
        print("nodes whose list the break cut after more than 8 kept:", int(cut.sum()), "uncut:", int((c == present).sum()))
        assert cut.sum() >= 8 and (c == present).any()

    run_case(request, 17, 12, 0, 16, 5, 0.1, method, spread, 9, "any", pre=pre)


@pytest.mark.gpu
def test_gpu_fuse_16_slots_32_jets(request):
    """both bounds at once; the occlusion word's mask is (2 << 32) - 1: bit 32 (t = Jets) counts, the bits above it, set at random here, do not"""
    def pre(want, c, occ, energy):
        chosen = np.take_along_axis(occ, want["slot"][None].astype(np.int64), 0)[0]
        assert ((occ >> np.uint64(32)) & np.uint64(1)).any()
        assert ((want["occ"] == 0) & (chosen >> np.uint64(33) != 0)).any()       # a chosen hypothesis whose only set bits are above bit 32

    run_case(request, 6, 5, 0, 16, 32, 0.1, 1, 6.0, 4, "16 beside 16", high_bits=True, pre=pre)


# the ordered energy / bound sum stages 512 nodes at a time: one node short of a chunk, exactly one, one over, exactly two, one over two
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,gpl", [(73, 7, 511), (32, 16, 512), (27, 19, 513), (64, 16, 1024), (41, 25, 1025)])
def test_gpu_fuse_at_the_chunk_edges_of_the_ordered_sum(request, w, h, gpl):
    assert w * h == gpl and gpl in (kChunk - 1, kChunk, kChunk + 1, 2 * kChunk, 2 * kChunk + 1)

    def pre(want, c, occ, energy):
        flat = c.reshape(-1)
        assert flat[-1] > 0 and flat[kChunk - 2] > 0 and flat[min(kChunk, gpl - 1)] > 0     # the nodes at the edges contribute terms

    run_case(request, w, h, 0, 3, 4, 0.2, 1, 0.0, w * 1000 + h, "any", pre=pre)


@pytest.mark.gpu
def test_gpu_fuse_diagonal_longer_than_the_workgroup(request):
    """261 x 259: the anti-diagonals in the middle have 259 nodes, so threads 0..2 take a second trip of the stride loop in both passes.
    The restatement takes 2.8 s for the 3 iterations on one CPU core."""
    w, h = 261, 259
    gw, gh, _, _ = grid(w, h, 0)
    assert min(gw, gh) > kThreads

    def pre(want, c, occ, energy):
        d = np.add.outer(np.arange(gh), np.arange(gw))
        assert all(c[dg - x, x] > 0 for dg in (gh - 1, gw - 1) for x in (dg - (gh - 1) + kThreads, dg - (gh - 1) + kThreads + 2))
        assert max(int(((d == k) & (c > 0)).sum()) for k in range(gh - 1, gw)) > 200      # and the first trip is full of nodes
        assert want["iters"] == 3

    run_case(request, w, h, 0, 2, 2, 0.2, 1, 0.0, 5, "any", trws_max_iter=3, pre=pre)


@pytest.mark.gpu
def test_gpu_fuse_batch_of_k_trws_16_stops_unevenly(request):
    """four segments at K = 9 (k_trws<16>), three unspread and one spread: by the restatement they stop after 8, 6, 10 (= max_iter) and 9 iterations, so
    every workgroup leaves the loop on its own flag while others go on"""
    import slowflow_amd as sfa
    w, h, K, J = 23, 17, 9, 5
    segs = [synth(np.random.default_rng(seed), K, J, w, h, 0, 0.2, spread=spread) for seed, spread in ((1, 0.0), (4, 0.0), (0, 6.0), (5, 0.0))]
    U, V, energy, occ, weight = (np.concatenate([s[k] for s in segs], 0) for k in range(5))
    n = len(segs)
    p = fr.Params(trws_max_iter=10, skip=0)
    want = [fr.fuse(U[s], V[s], energy[s], occ[s], weight[s], p, w) for s in range(n)]
    iters = [o["iters"] for o in want]
    most = [max(len(l) for l in o["lab"]) for o in want]
    print("iters", iters, "largest label count per segment", most)
    assert len(set(iters)) > 1 and any(2 < i < p.trws_max_iter for i in iters)
    assert max(most) == 9 and min(most) == 9                                    # every segment has nodes past k_trws<8>'s bound
    gpu = request.getfixturevalue("ctx")
    many = gpu.fuse_hypotheses(p.to_c(sfa), U, V, energy, occ, weight, w, h)
    for s in range(n):
        one = gpu.fuse_hypotheses(p.to_c(sfa), U[s:s + 1], V[s:s + 1], energy[s:s + 1], occ[s:s + 1], weight[s:s + 1], w, h)
        for k in one:
            assert np.array_equal(many[k][s], one[k][0]), (k, s)
        check_equal(many, want[s], s)
