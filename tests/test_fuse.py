"""dense_tracking's fusion (sfa_dt_smoothness_weight, sfa_hypothesis_energies_ex, sfa_fuse_hypotheses): the float64 restatement (tests/fuse_ref.py)
against independent truths on the CPU, and the GPU kernels against the restatement with IEEE == on every output."""
import ctypes
import itertools

import numpy as np
import pytest

import fuse_ref as fr
from accum_ref import grid

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# generic MRFs for the solver checks
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def random_mrf(rng, gw, gh, kmax, holes=0.0, scale=1.0):
    theta = []
    for _ in range(gw * gh):
        m = 0 if rng.random() < holes else int(rng.integers(1, kmax + 1))
        theta.append(rng.normal(0, 1, m))
    PR, PD = [None] * (gw * gh), [None] * (gw * gh)
    for p in range(gw * gh):
        y, x = divmod(p, gw)
        if not len(theta[p]):
            continue
        if x + 1 < gw and len(theta[p + 1]):
            PR[p] = np.abs(rng.normal(0, scale, (len(theta[p]), len(theta[p + 1]))))
        if y + 1 < gh and len(theta[p + gw]):
            PD[p] = np.abs(rng.normal(0, scale, (len(theta[p]), len(theta[p + gw]))))
    return theta, PR, PD


def brute_force(theta, PR, PD, gw, gh):
    nodes = [p for p in range(gw * gh) if len(theta[p])]
    best = None
    for combo in itertools.product(*[range(len(theta[p])) for p in nodes]):
        x = [-1] * (gw * gh)
        for p, c in zip(nodes, combo):
            x[p] = c
        e = fr.energy_of(theta, PR, PD, gw, gh, x)
        if best is None or e < best:
            best = e
    return 0.0 if best is None else best


def same(a, b):
    la, Ea, Ba, ia = a
    lb, Eb, Bb, ib = b
    return np.array_equal(np.asarray(la), np.asarray(lb)) and Ea == Eb and Ba == Bb and ia == ib


@pytest.mark.parametrize("seed", range(12))
def test_trws_scalar_equals_diagonal_form(seed):
    rng = np.random.default_rng(seed)
    gw, gh = int(rng.integers(1, 7)), int(rng.integers(1, 7))
    theta, PR, PD = random_mrf(rng, gw, gh, int(rng.integers(1, 5)), holes=0.2 * (seed % 3))
    a = fr.trws_scalar(theta, PR, PD, gw, gh, 1e-5, 6)
    b = fr.trws_diag(theta, PR, PD, gw, gh, 1e-5, 6)
    assert same(a, b)


@pytest.mark.parametrize("seed", range(30))
def test_trws_against_brute_force(seed):
    rng = np.random.default_rng(100 + seed)
    gw, gh = int(rng.integers(1, 4)), int(rng.integers(1, 4))
    theta, PR, PD = random_mrf(rng, gw, gh, 3, holes=0.25 if seed % 2 else 0.0, scale=2.0)
    x, E, lb, its = fr.trws_diag(theta, PR, PD, gw, gh, 1e-5, 10)
    assert E == fr.energy_of(theta, PR, PD, gw, gh, x)
    opt = brute_force(theta, PR, PD, gw, gh)
    assert lb <= opt + 1e-12 and opt <= E
    assert 1 <= its <= 10


def viterbi(theta, P):
    """chain: theta[k] arrays, P[k] the (len k, len k+1) edge costs.  The optimal labelling."""
    cost = theta[0].copy()
    back = []
    for k in range(1, len(theta)):
        c = cost[:, None] + P[k - 1]
        back.append(np.argmin(c, 0))
        cost = c.min(0) + theta[k]
    x = [int(np.argmin(cost))]
    for b in back[::-1]:
        x.append(int(b[x[-1]]))
    return x[::-1]


@pytest.mark.parametrize("seed", range(8))
@pytest.mark.parametrize("vertical", [False, True])
def test_chains_reach_the_viterbi_optimum_after_two_iterations(seed, vertical):
    rng = np.random.default_rng(200 + seed)
    n = int(rng.integers(2, 12))
    theta = [rng.normal(0, 1, int(rng.integers(1, 5))) for _ in range(n)]
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


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# synthetic hypotheses
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def synth(rng, K, J, w, h, skip=1, holes=0.2, n=1, spread=0.0):
    """n segments: U, V (n, K, J, gh, gw), energy (n, K, gh, gw), occ (n, K, gh, gw), weight (n, h, w).  Slots near a copy of slot 0 (NMS active);
    spread adds spread * k to slot k's u, which moves the slots apart so that the NMS keeps them (same random draws with and without it)."""
    gw, gh, _, _ = grid(w, h, skip)
    base = np.cumsum(rng.normal(0, 1, (n, 1, J, gh, gw)), 2)
    scale = rng.choice([1e-3, 0.05, 1.0], (n, K, 1, gh, gw))
    U = base + np.cumsum(rng.normal(0, 1, (n, K, J, gh, gw)), 2) * scale
    if spread:
        U = U + spread * np.arange(K).reshape(1, K, 1, 1, 1)
    V = base[..., ::-1, :] + np.cumsum(rng.normal(0, 1, (n, K, J, gh, gw)), 2) * scale
    energy = rng.uniform(0, 50, (n, K, gh, gw)).astype(F32).astype(np.float64)
    energy[rng.random(energy.shape) < holes] = np.inf
    occ = (rng.integers(0, 1 << 62, (n, K, gh, gw), dtype=np.int64).astype(np.uint64) & np.uint64((1 << (J + 1)) - 2))
    occ[rng.random(occ.shape) < 0.5] = 0
    weight = rng.uniform(0.01, 0.5, (n, h, w)).astype(F32)
    return U, V, energy, occ, weight


def test_no_pairwise_terms_gives_argmin_unary():
    rng = np.random.default_rng(3)
    U, V, energy, occ, weight = synth(rng, 4, 5, 12, 9, holes=0.3)
    p = fr.Params(acc_beta=0.0, acc_spatial_occ=0.0, traj_sim_thres=-1.0)
    out = fr.fuse(U[0], V[0], energy[0], occ[0], weight[0], p, 12)
    e = energy[0]
    for y, x in np.ndindex(out["slot"].shape):
        col = e[:, y, x]
        want = -1 if np.all(col == np.inf) else int(np.argmin(col))
        assert out["slot"][y, x] == want


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# hand-worked cases, one per quirk: each fails with its quirk switched off
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def one_pixel(flows, energies, J):
    K = len(flows)
    U = np.zeros((K, J, 1, 1))
    V = np.zeros((K, J, 1, 1))
    for k, f in enumerate(flows):
        U[k, :, 0, 0] = f
    return U, V, np.array(energies, np.float64).reshape(K, 1, 1)


@pytest.mark.parametrize("off", [(), ("nms_break",)])
def test_nms_break_drops_everything_after_the_first_discard(off):
    # sorted: slot 0 (1.0), slot 1 (2.0, 0.01 from slot 0: discarded), slot 2 (3.0, far): the break drops slot 2 as well
    U, V, e = one_pixel([[1, 1], [1.01, 1.0], [5, 5]], [1.0, 2.0, 3.0], 2)
    lab = fr.labels(U, V, e, 1, 0.1, off)
    assert (lab[0] == [0]) == (off == ())
    if off:
        assert lab[0] == [0, 2]


@pytest.mark.parametrize("off", [(), ("float_score",)])
def test_ties_of_the_float_score_go_to_the_lower_slot(off):
    # slot 0: 1 + 2^-40, slot 1: 1.0 -- equal as floats (score() is a float); the two are close, so NMS keeps only the first of the sort
    U, V, e = one_pixel([[1, 1], [1.0, 1.0]], [1.0 + 2.0 ** -40, 1.0], 2)
    lab = fr.labels(U, V, e, 1, 0.1, off)
    assert (lab[0] == [0]) == (off == ())


@pytest.mark.parametrize("off", [(), ("img_norm_keys",)])
def test_smoothness_weight_reads_img_norm_keys_with_defaults(off):
    cfg = {"slow_flow_img_norm_avg_1": "120.5", "slow_flow_img_norm_std_1": "60.25"}
    avg, std = fr.program_norm(cfg, off)
    assert ((avg, std) == ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])) == (off == ())
    assert fr.program_norm({"img_norm_avg_2": "3", "img_norm_std_3": "2"}) == ([0.0, 3.0, 0.0], [1.0, 1.0, 2.0])


@pytest.mark.parametrize("off", [(), ("acc_unnormalised",)])
def test_acc_distance_is_not_normalised_adj_is(off):
    a = np.array([[1.0, 2.0, 3.0]])
    z = np.zeros((1, 3))
    # ACC: |1|/1 + |2|/2 + |3|/3 = 3;  ADJ: (1 + 1 + 1) / 3 = 1
    assert fr.distance(a, z, z, z, 0, off)[0] == 1.0
    assert (fr.distance(a, z, z, z, 1, off)[0] == 3.0) == (off == ())


@pytest.mark.parametrize("off", [(), ("occ_jets_plus_1",)])
def test_smooth_occ_counts_jets_plus_one_frames(off):
    # Jets 2: the hypotheses differ only in occluded(2), the last frame
    p = fr.Params(acc_beta=0.0, acc_spatial_occ=10.0)
    z = np.zeros((1, 2))
    P = fr.pair_cost(z, z, np.array([4], np.uint64), z, z, np.array([0], np.uint64), F32(0.25), F32(0.25), 2, p, off)
    assert (P[0] == 5.0) == (off == ())


@pytest.mark.parametrize("off", [(), ("fp32_weight_sum",)])
def test_weight_sum_is_fp32(off):
    p = fr.Params(acc_beta=0.0, acc_spatial_occ=1.0)
    z = np.zeros((1, 2))
    P = fr.pair_cost(z, z, np.array([2], np.uint64), z, z, np.array([0], np.uint64), F32(1.0), F32(2.0 ** -30), 2, p, off)
    assert (P[0] == 1.0) == (off == ())                                     # 1 + 2^-30 rounds to 1 in fp32


@pytest.mark.parametrize("off", [(), ("float_dist",)])
def test_distance_is_rounded_to_float(off):
    p = fr.Params(acc_beta=1.0, acc_spatial_occ=0.0)
    a, z = np.array([[0.1, 0.1]]), np.zeros((1, 2))
    d = fr.distance(a, z, z, z, 1)[0]                                       # 0.1 + 0.05
    P = fr.pair_cost(a, z, np.array([0], np.uint64), z, z, np.array([0], np.uint64), F32(0.5), F32(0.5), 2, p, off)
    assert (P[0] == float(F32(d))) == (off == ())


def test_expf_restatement_matches_libm():
    libm = ctypes.CDLL("libm.so.6")
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    x = np.random.default_rng(0).uniform(-12, 0, 4000).astype(F32)
    ours = fr.expf(x)
    ref = np.array([libm.expf(float(v)) for v in x], F32)
    ulp = np.abs(ours.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1 and (ulp > 0).mean() < 1e-3


def test_smoothness_weight_restatement_against_the_oracle(oracle):
    rng = np.random.default_rng(5)
    w, h, stride = 37, 23, 40
    im = np.zeros((3, h, stride), F32)
    im[:, :, :w] = rng.uniform(0, 255, (3, h, w)).astype(F32)
    a = fr.smoothness_weight(oracle, im, w)
    b = oracle.dpsis_weight(im, w)[:, :w]
    ulp = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1                                                   # the oracle calls this machine's libm expf


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import slowflow_amd as sfa
    c = sfa.Context(0)
    yield c
    c.close()


def check_equal(got, want, s=0):
    for k in ("slot", "u", "v", "occ"):
        assert np.array_equal(got[k][s], want[k]), k
    assert got["energy"][s] == want["energy"]
    assert got["bound"][s] == want["bound"]
    assert got["iters"][s] == want["iters"]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,hbit,stats", [(64, 48, 0, False), (37, 23, 0, True), (128, 20, 1, True)])
def test_gpu_smoothness_weight(ctx, oracle, w, h, hbit, stats):
    rng = np.random.default_rng(w + h)
    stride = (w + 3) // 4 * 4
    im = np.zeros((3, h, stride), F32)
    im[:, :, :w] = rng.normal(0, 1, (3, h, w)).astype(F32)
    avg, std = ((120.5, 110.25, 90.0), (60.0, 55.5, 40.0)) if stats else ((0, 0, 0), (1, 1, 1))
    if hbit:
        avg = tuple(256 * a for a in avg)
        std = tuple(256 * s for s in std)
    got = ctx.smoothness_weight(im, w, avg, std, hbit)
    want = fr.smoothness_weight(oracle, im, w, avg, std, hbit)
    assert got.shape == (h, w) and np.array_equal(got, want)


CASES = [  # (w, h, skip, K, J, holes, method)
    (1, 1, 0, 1, 1, 0.0, 1), (1, 1, 0, 3, 4, 0.3, 1), (9, 1, 0, 2, 3, 0.2, 1), (1, 11, 0, 3, 5, 0.2, 0), (7, 5, 0, 4, 8, 0.0, 1), (13, 9, 1, 5, 16, 0.3, 0),
    (17, 12, 0, 8, 32, 0.25, 1), (10, 10, 0, 6, 7, 0.9, 1), (21, 15, 2, 7, 12, 0.1, 1), (512, 218, 0, 3, 6, 0.1, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,skip,K,J,holes,method", CASES)
def test_gpu_fuse_equals_restatement(ctx, w, h, skip, K, J, holes, method):
    import slowflow_amd as sfa  # noqa: F401
    rng = np.random.default_rng(w * 1000 + h * 10 + K)
    U, V, energy, occ, weight = synth(rng, K, J, w, h, skip, holes)
    p = fr.Params(traj_sim_method=method, skip=skip)
    got = ctx.fuse_hypotheses(p.to_c(sfa), U, V, energy, occ, weight, w, h)
    want = fr.fuse(U[0], V[0], energy[0], occ[0], weight[0], p, w)
    check_equal(got, want)


@pytest.mark.gpu
def test_gpu_fuse_batch_equals_single_calls(ctx):
    import slowflow_amd as sfa
    rng = np.random.default_rng(11)
    w, h, K, J = 23, 14, 4, 6
    U, V, energy, occ, weight = synth(rng, K, J, w, h, 0, 0.2, n=5)
    p = fr.Params(trws_max_iter=7, skip=0).to_c(sfa)
    many = ctx.fuse_hypotheses(p, U, V, energy, occ, weight, w, h)
    for s in range(5):
        one = ctx.fuse_hypotheses(p, U[s:s + 1], V[s:s + 1], energy[s:s + 1], occ[s:s + 1], weight[s:s + 1], w, h)
        for k in one:
            assert np.array_equal(many[k][s], one[k][0]), k
    want = fr.fuse(U[2], V[2], energy[2], occ[2], weight[2], fr.Params(trws_max_iter=7, skip=0), w)
    check_equal(many, want, 2)


@pytest.mark.gpu
def test_gpu_fuse_refusals(ctx):
    import slowflow_amd as sfa
    rng = np.random.default_rng(1)
    U, V, energy, occ, weight = synth(rng, 2, 3, 8, 6)
    for kw in (dict(traj_sim_method=2), dict(trws_max_iter=0)):
        with pytest.raises(sfa.SlowflowError):
            ctx.fuse_hypotheses(sfa.fuse_params(**kw), U, V, energy, occ, weight, 8, 6)
    U, V, energy, occ, weight = synth(rng, 17, 3, 8, 6)
    with pytest.raises(sfa.SlowflowError):
        ctx.fuse_hypotheses(sfa.fuse_params(), U, V, energy, occ, weight, 8, 6)
    U, V, energy, occ, weight = synth(rng, 2, 33, 8, 6)
    with pytest.raises(sfa.SlowflowError):
        ctx.fuse_hypotheses(sfa.fuse_params(), U, V, energy, occ, weight, 8, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("r_Jets,Jets", [(4, 4), (8, 4), (2, 4)])
def test_gpu_energies_ex_returns_the_adapted_flows(ctx, r_Jets, Jets):
    import slowflow_amd as sfa
    from energy_ref import adapt_table
    rng = np.random.default_rng(r_Jets * 10 + Jets)
    w, h, n = 24, 16, 2
    stride = w
    gw, gh, _, _ = grid(w, h, 1)
    acc_u, acc_v = rng.normal(0, 2, (n, r_Jets, gh, gw)), rng.normal(0, 2, (n, r_Jets, gh, gw))
    tracked = np.where(rng.random((n, gh, gw)) < 0.7, r_Jets, 1).astype(np.int32)
    frames = rng.uniform(-1, 1, (n, Jets + 1, 3, h, stride)).astype(F32)
    p = sfa.energy_params()
    e0, o0 = ctx.hypothesis_energies(p, r_Jets, acc_u, acc_v, tracked, frames, w)
    e1, o1, au, av = ctx.hypothesis_energies(p, r_Jets, acc_u, acc_v, tracked, frames, w, adapted=True)
    assert np.array_equal(e0, e1) and np.array_equal(o0, o1)
    up, skip, off, offm1 = adapt_table(r_Jets, Jets)
    for t in range(Jets):
        if up:
            wu, wv = acc_u[:, off[t]], acc_v[:, off[t]]
        else:
            lu = acc_u[:, offm1[t]].astype(F32).astype(np.float64) if t > 0 else 0.0
            lv = acc_v[:, offm1[t]].astype(F32).astype(np.float64) if t > 0 else 0.0
            wu = lu + float(skip) * (acc_u[:, off[t]] - lu)
            wv = lv + float(skip) * (acc_v[:, off[t]] - lv)
        have = tracked == r_Jets
        assert np.array_equal(au[:, t], np.where(have, wu, 0.0)) and np.array_equal(av[:, t], np.where(have, wv, 0.0))
