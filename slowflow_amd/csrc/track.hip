// track.hip -- the resident track job: dense_tracking's three stages (accumulate.hip, energy.hip, fuse.hip) chained on the device for up to n start_jets of K
// rates.  The job owns every plane between the inputs and the fused flow; sfa_track_job_run enqueues
//     frame derivatives and records -> accumulation (all steps) per rate -> energies and adapted flows per rate, best / occluded -> smoothness weight
//     -> labels -> pairwise -> TRW-S -> output
// on the context's stream through the stages' device-level functions (sfa_internal.h) and returns: TRW-S's stopping rule lives inside k_trws, so nothing in
// the chain needs a host decision, and no stage boundary crosses the host.  The flows are brought into the kernels' layout when they are uploaded (host
// planes: a copy and the stage wrappers' kernels; device memory: the pack kernels below; occlusion images likewise), so a run reads only what the job holds.
// Segment s of a run comes out with the bits of the staged calls on that segment alone: the same kernels over the same planes, blockIdx.y = s.
// The device entry points describe their arguments as views and leave every check of them to check_view / check_disjoint (api.hip on dev_view.h).
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "sfa_device.h"

#pragma clang fp contract(off)

static_assert(sizeof(sfa_track_params) == 832, "sfa_track_params: the layout slowflow_amd/__init__.py mirrors");

namespace sfa {

constexpr int kTrThreads = 256;
constexpr int kTrMaxN = 64, kTrMaxK = 16, kTrMaxJets = 32;

// fp32 flows in device memory, element (segment, step, u|v, row, column) at src + the 64-bit element strides st -> float2 planes [seg][np][h][w] (the layout
// k_accumulate and k_hyp_serial gather from).  One element per thread: two 4-byte loads, one 8-byte store.
__global__ void __launch_bounds__(kTrThreads) k_track_pack_flow(const float *__restrict__ src, long long s_seg, long long s_step, long long s_c, long long s_row,
                                                                long long s_col, int w, int h, int np, float2 *__restrict__ out, size_t total) {
    const size_t i = (size_t)blockIdx.x * kTrThreads + threadIdx.x;
    if (i >= total) return;
    const size_t pl = (size_t)w * h, k = i / pl, p = i % pl;
    const float *b = src + (long long)(k / np) * s_seg + (long long)(k % np) * s_step + (long long)(p / w) * s_row + (long long)(p % w) * s_col;
    out[i] = make_float2(b[0], b[s_c]);
}

// the same source, one segment: the crop (x0, y0, cw, ch) of its np fields as packed float planes su[k], sv[k] -- what k_jet_resample reads
__global__ void __launch_bounds__(kTrThreads) k_track_pack_planes(const float *__restrict__ src, long long s_step, long long s_c, long long s_row, long long s_col,
                                                                  int x0, int y0, int cw, int ch, float *__restrict__ su, float *__restrict__ sv, size_t total) {
    const size_t i = (size_t)blockIdx.x * kTrThreads + threadIdx.x;
    if (i >= total) return;
    const size_t spl = (size_t)cw * ch, k = i / spl, p = i % spl;
    const float *b = src + (long long)k * s_step + (long long)(y0 + p / cw) * s_row + (long long)(x0 + p % cw) * s_col;
    su[i] = b[0];
    sv[i] = b[s_c];
}

// the driver's grey image of an occlusion label (occlusion_image, host/slow_flow.cpp; reference variational_mt.cpp:277-279): (x + 1) / 2 * 255 in fp32 without
// contraction, nearbyint (halves to even), then std::min(255.0f, .) and std::max(0.0f, .) as written there: NaN -> 255, -Inf -> 0, +Inf -> 255
__device__ __forceinline__ unsigned char occ_byte(float x) {
    const float v = (x + 1) * 0.5f * 255.0f, q = nearbyintf(v);
    const float lo = q < 255.0f ? q : 255.0f;                                   // std::min(255.0f, q)
    return (unsigned char)(0.0f < lo ? lo : 0.0f);                              // std::max(0.0f, lo)
}
__device__ __forceinline__ unsigned char occ_byte(unsigned char x) { return x; }   // the raw image as the occlusion files hold it

// occlusion images of one segment in device memory, element (step, row, column) at src + the strides, raw bytes or fp32 labels -> packed bytes [np][sh][sw],
// the planes k_jet_occ_decode reads.  One element per thread.
template <class T>
__global__ void __launch_bounds__(kTrThreads) k_track_pack_occ(const T *__restrict__ src, long long s_step, long long s_row, long long s_col, int sw, int sh,
                                                               unsigned char *__restrict__ out, size_t total) {
    const size_t i = (size_t)blockIdx.x * kTrThreads + threadIdx.x;
    if (i >= total) return;
    const size_t spl = (size_t)sw * sh, k = i / spl, p = i % spl;
    out[i] = occ_byte(src[(long long)k * s_step + (long long)(p / sw) * s_row + (long long)(p % sw) * s_col]);
}

// fp32 frames, element (segment, frame, channel, row, column) at src + st -> packed planes [seg][nfr][3][h][w], the planes k_energy_records reads
__global__ void __launch_bounds__(kTrThreads) k_track_pack_frames(const float *__restrict__ src, long long s_seg, long long s_fr, long long s_c, long long s_row,
                                                                  long long s_col, int w, int h, int nfr, float *__restrict__ out, size_t total) {
    const size_t i = (size_t)blockIdx.x * kTrThreads + threadIdx.x;
    if (i >= total) return;
    const size_t pl = (size_t)w * h, k = i / pl, p = i % pl;                    // k = (seg * nfr + frame) * 3 + channel
    const size_t fr = k / 3;
    out[i] = src[(long long)(fr / nfr) * s_seg + (long long)(fr % nfr) * s_fr + (long long)(k % 3) * s_c + (long long)(p / w) * s_row + (long long)(p % w) * s_col];
}

// per grid pixel of segment blockIdx.y: best = the rate of the lowest fp32 energy, ties to the lower rate, 255 for none; occluded[k] = popcount of rate k's bits
// (the host loop of the accumulate program).  E, O: [n][K][gpl]; best: [n][gpl]; occluded: [K][cap][gpl]
// On a fill job E and O hold S = 2 K slots per segment and rate k sits in slot k * step, step = 2 (a plain job: S = K, step = 1)
__global__ void __launch_bounds__(kTrThreads) k_track_best(const double *__restrict__ E, const unsigned long long *__restrict__ O, int K, int S, int step, int gpl, int cap,
                                                           unsigned char *__restrict__ best, unsigned char *__restrict__ occluded) {
    const int i = blockIdx.x * kTrThreads + threadIdx.x;
    if (i >= gpl) return;
    const int s = blockIdx.y;
    float be = __int_as_float(0x7f800000);
    int b = 255;
    for (int k = 0; k < K; k++) {
        const size_t o = ((size_t)s * S + (size_t)k * step) * gpl + i;
        const float e = (float)E[o];                                            // an fp32 sum stored in a double: exact
        if (e < be) { be = e; b = k; }                                          // strict: ties keep the lower rate
        occluded[((size_t)k * cap + s) * gpl + i] = (unsigned char)__popcll(O[o]);
    }
    best[(size_t)s * gpl + i] = (unsigned char)b;
}

// the fused results of segments s0 .. into the caller's device memory: flow (segment, u|v, row, column) at st, packed slots, occlusions and (energy, bound,
// iterations) per segment
__global__ void __launch_bounds__(kTrThreads) k_track_unpack(const double *__restrict__ fu, const double *__restrict__ fv, const int *__restrict__ slot,
                                                             const unsigned char *__restrict__ occ, const double *__restrict__ seg_energy,
                                                             const double *__restrict__ seg_bound, const int *__restrict__ seg_iters, int gw, int gpl,
                                                             double *__restrict__ flow, long long t_seg, long long t_c, long long t_row, long long t_col,
                                                             int *__restrict__ slot_out, unsigned char *__restrict__ occ_out, double *__restrict__ stats) {
    const int i = blockIdx.x * kTrThreads + threadIdx.x;
    if (i >= gpl) return;
    const int s = blockIdx.y;
    const size_t si = (size_t)s * gpl + i;
    double *f = flow + (long long)s * t_seg + (long long)(i / gw) * t_row + (long long)(i % gw) * t_col;
    f[0] = fu[si];
    f[t_c] = fv[si];
    if (slot_out) slot_out[si] = slot[si];
    if (occ_out) occ_out[si] = occ[si];
    if (stats && i == 0) { stats[3 * s] = seg_energy[s]; stats[3 * s + 1] = seg_bound[s]; stats[3 * s + 2] = (double)seg_iters[s]; }
}

// rate results of segments s0 .. into the caller's device memory: the last accumulated step (segment, u|v, row, column) at st, and packed tracked, energy,
// occlusion word and one byte plane (a rate's occluded, or best); every output or null.  The sources come offset to segment s0, one segment a_seg, g_seg,
// e_seg, b_seg elements after the other
__global__ void __launch_bounds__(kTrThreads) k_track_unpack_rate(const double *__restrict__ au, const double *__restrict__ av, size_t a_seg,
                                                                  const int *__restrict__ tracked, size_t g_seg, const double *__restrict__ E,
                                                                  const unsigned long long *__restrict__ O, size_t e_seg, const unsigned char *__restrict__ bytes,
                                                                  size_t b_seg, int gw, int gpl, double *__restrict__ acc, long long t_seg, long long t_c,
                                                                  long long t_row, long long t_col, int *__restrict__ tracked_out, double *__restrict__ energy_out,
                                                                  unsigned long long *__restrict__ occ_bits_out, unsigned char *__restrict__ bytes_out) {
    const int i = blockIdx.x * kTrThreads + threadIdx.x;
    if (i >= gpl) return;
    const size_t s = blockIdx.y, si = s * gpl + i;
    if (acc) {
        double *f = acc + (long long)s * t_seg + (long long)(i / gw) * t_row + (long long)(i % gw) * t_col;
        f[0] = au[s * a_seg + i];
        f[t_c] = av[s * a_seg + i];
    }
    if (tracked_out) tracked_out[si] = tracked[s * g_seg + i];
    if (energy_out) energy_out[si] = E[s * e_seg + i];
    if (occ_bits_out) occ_bits_out[si] = O[s * e_seg + i];
    if (bytes_out) bytes_out[si] = bytes[s * b_seg + i];
}

inline unsigned blocks_of(size_t total) { return (unsigned)((total + kTrThreads - 1) / kTrThreads); }

}  // namespace sfa

using namespace sfa;

// Everything below is launch orchestration: argument checks, layout arithmetic, copies and launches, a few microseconds per call beside milliseconds of
// kernels.  It is compiled for size, so that the release build stays under the share of the full build tests/test_abi.py holds it to.
#pragma clang attribute push(__attribute__((minsize)), apply_to = function)

// Every plane of the job inside one allocation; this struct is the only statement of the list (sfa_track_job_bytes walks it without a device)
struct TrackPlanes {
    struct Rate { size_t fw, bw, mask, acc_u, acc_v, tracked; } rate[kTrMaxK];
    size_t occluded, stage, occ_stage, frames, der, rec, wU, wV, wocc, jc, oc, ep, E, O, best;
    size_t aU, aV, weight, nl, lab, theta, P, M, xcur, xbest, slot, fu, fv, out_occ, seg_energy, seg_bound, seg_iters;
    // a fill job only: the saliency's workspace of one start_jet (15 planes at the device pitch), sal [n][plp], edges (as uploaded) and run_cost (the map
    // as the calls so far left it) [n][cpl], cost [n][rJmax][cpl], full [K][n], the regions' T, P, S [n][gpl] and mask, kept and count [n], the sample
    // positions, block_count, matches [n][rJmax][nx ny][4], fx, fy [n][rJmax][gpl], inf [gpl] doubles of +Inf; per rate the fill-in's trajectories [n][rJ][gpl] and tracked [n][gpl]
    size_t lab_stage, sal, edges, run_cost, cost, full, cT, cP, cS, mask, kept, count, xs, ys, block_count, matches, fx, fy, inf;
    struct Fill { size_t u, v, tracked; } fill[kTrMaxK];
    size_t total;
};

// what a fill job derives from its parameters besides the planes: the sample positions, the longest rate, the planes' strides
struct FillGeo { std::unique_ptr<int[]> xs, ys; int nx = 0, ny = 0, rJmax = 0, pitch = 0; size_t cpl = 0, plp = 0; };

struct sfa_track_job {
    sfa_ctx *ctx = nullptr;
    sfa_track_params p;
    int gw = 0, gh = 0;
    bool identity[kTrMaxK] = {};
    EnergyPlan plan[kTrMaxK];
    TrackPlanes at;
    DevMem mem;
    hipEvent_t ev[10] = {};             // [9]: after the smoothness weight, before the fusion's clears
    bool timed = false, timed_fuse = false;
    bool fill = false;                  // made by sfa_track_job_create_fill
    sfa_track_fill_params fp{};
    FillGeo fg;
    std::unique_ptr<int[]> full, stats; // [K][n] r_Jets[r]; [K][n][3] kept_pixels, matches, filled of the last run
    std::unique_ptr<double[]> inf;      // [gpl] +Inf, the source of at.inf
    // the interpolation's images of one rate, n * rJmax entries each: EpicChainDev's arrays, their counts, start_jets and steps, rc and status
    std::unique_ptr<const float *[]> c_in;   // cost, matches, sal
    std::unique_ptr<float *[]> c_out;        // fx, fy
    std::unique_ptr<int[]> c_int;            // nm, start_jet, step, rc, status, then kept and count [n]
    int chain_runs[2] = {};             // the last run's interpolation sub-batches over all rates: completed, cut short and run again
    hipEvent_t fev[kTrMaxK][5] = {};    // per rate: before the regions, after the matches, the edge costs, the chain, the trajectories
    hipEvent_t ev_energy = nullptr;     // a fill job: after the last rate's fill-in, where the energies begin
    int slots() const { return fill ? 2 * p.K : p.K; }
    int step() const { return fill ? 2 : 1; }
    template <class T> T *ptr(size_t off) const { return reinterpret_cast<T *>(static_cast<char *>(mem.p) + off); }
};

// the argument checks of create and bytes (no device): everything the three stages refuse, by the name of the argument
static int track_check(sfa_ctx *ctx, const char *fn, const sfa_track_params *p, int *gw, int *gh, bool *identity, EnergyPlan *plan) {
    if (!p) REFUSE("%s: params is null", fn);
    if (p->n < 1 || p->n > kTrMaxN) REFUSE("%s: n = %d (1 <= n <= %d start_jets)", fn, p->n, kTrMaxN);
    if (p->K < 1 || p->K > kTrMaxK) REFUSE("%s: K = %d (1 <= K <= %d rates)", fn, p->K, kTrMaxK);
    if (p->Jets < 1 || p->Jets > kTrMaxJets) REFUSE("%s: Jets = %d (1 <= Jets <= %d)", fn, p->Jets, kTrMaxJets);
    if (p->w < 1) REFUSE("%s: w = %d", fn, p->w);
    if (p->h < 4) REFUSE("%s: h = %d; the reference's vertical 5-tap derivative needs h >= 4", fn, p->h);
    if (p->min_fps_idx < 0 || p->min_fps_idx >= p->K) REFUSE("%s: min_fps_idx = %d names none of the %d rates", fn, p->min_fps_idx, p->K);
    for (int r = 0; r < p->K; r++)
        if (p->r_Jets[r] < 1) REFUSE("%s: r_Jets[%d] = %d", fn, r, p->r_Jets[r]);
    if (p->r_Jets[p->min_fps_idx] != p->Jets)
        REFUSE("%s: r_Jets[%d] = %d, not Jets = %d: rate min_fps_idx's flows are the Jets steps the energies read", fn, p->min_fps_idx, p->r_Jets[p->min_fps_idx], p->Jets);
    if (p->do_fuse) {
        if (p->fuse.traj_sim_method != 0 && p->fuse.traj_sim_method != 1)
            REFUSE("%s: fuse.traj_sim_method %d (0 ADJ, 1 ACC; 2 FINAL reads flow_y[Jets], past the array)", fn, p->fuse.traj_sim_method);
        if (p->fuse.trws_max_iter < 1) REFUSE("%s: fuse.trws_max_iter %d < 1", fn, p->fuse.trws_max_iter);
    }
    if (sfa_accumulate_grid(p->w, p->h, p->skip, gw, gh) != SFA_OK) REFUSE("%s: skip: %s", fn, sfa_last_error(nullptr));
    if (((size_t)*gw * *gh * p->K * p->K + kTrThreads - 1) / kTrThreads > 0x7fffffffull) REFUSE("%s: grid too large", fn);
    for (int r = 0; r < p->K; r++) {
        char name[96];
        snprintf(name, sizeof name, "%s: source[%d]", fn, r);
        const sfa_jet_source &s = p->source[r];
        SFA_TRY(jet_source_check(ctx, name, &s, p->w, p->h, &identity[r]));
        if (p->use_occlusions && (s.x0 != 0 || s.y0 != 0 || s.cw != s.sw || s.ch != s.sh))
            REFUSE("%s: source: cropped occlusions are not supported (the reference's crop() reads the 8-bit Mat through at<Vec2d>)", name);
        sfa_energy_params ep = p->energy;
        ep.skip = p->skip;
        ep.weight = p->weight[r];
        SFA_TRY(energy_plan(ctx, &ep, p->r_Jets[r], p->Jets, p->w, p->h, &plan[r]));
    }
    return SFA_OK;
}

// the checks of a fill job beyond track_check's, by the name of the argument, and what the layout needs of it
static int fill_check(sfa_ctx *ctx, const char *fn, const sfa_track_params *p, const sfa_track_fill_params *f, int gw, int gh, FillGeo *g) {
    if (!f) REFUSE("%s: fill is null", fn);
    if (p->K > kTrMaxK / 2) REFUSE("%s: K = %d (a fill job fuses 2 K slots: at most %d rates)", fn, p->K, kTrMaxK / 2);
    if (f->epic.nn < 1) REFUSE("%s: epic.nn = %d (at least one neighbour)", fn, f->epic.nn);
    if (f->epic.pref_nn < 0) REFUSE("%s: epic.pref_nn = %d (0: no consistency filter, else its neighbours)", fn, f->epic.pref_nn);
    if (f->epic.method != 0 && f->epic.method != 1) REFUSE("%s: epic.method = %d (0: locally-weighted affine, 1: Nadaraya-Watson)", fn, f->epic.method);
    if (!std::isfinite(f->epic_skip) || f->epic_skip < 1) REFUSE("%s: epic_skip = %g (finite, at least 1)", fn, (double)f->epic_skip);
    if (f->min_size < 1) REFUSE("%s: min_size = %d (>= 1)", fn, f->min_size);
    if (f->epic.saliency_th != 0 && (gw <= 8 || gh <= 8))
        REFUSE("%s: gw x gh = %d x %d with epic.saliency_th != 0 (the saliency's Gaussian of sigma 1.0 needs more than 8 columns and rows)", fn, gw, gh);
    SFA_TRY(epic_nn_check_sizes(ctx, fn, gw, gh));
    if (((size_t)gw * gh * 4 * p->K * p->K + kTrThreads - 1) / kTrThreads > 0x7fffffffull) REFUSE("%s: grid too large for 2 K slots", fn);
    g->xs.reset(new int[gw]()); g->ys.reset(new int[gh]());
    if (sfa_fill_samples(gw, f->epic_skip, g->xs.get(), &g->nx) != SFA_OK || sfa_fill_samples(gh, f->epic_skip, g->ys.get(), &g->ny) != SFA_OK)
        REFUSE("%s: epic_skip: %s", fn, sfa_last_error(nullptr));
    g->rJmax = 0;
    for (int r = 0; r < p->K; r++) g->rJmax = std::max(g->rJmax, p->r_Jets[r]);
    g->pitch = dev_pitch(gw);
    g->plp = (size_t)g->pitch * gh;
    g->cpl = ((size_t)gw * gh + 3) / 4 * 4;
    return SFA_OK;
}

static void track_layout(const sfa_track_params &p, int gw, int gh, const bool *identity, int NN, const sfa_track_fill_params *fill, const FillGeo *fg,
                         TrackPlanes *out) {
    TrackPlanes &a = *out;
    size_t top = 0;
    auto take = [&](size_t bytes) { const size_t o = top; top += (bytes + 255) / 256 * 256; return o; };
    const size_t n = p.n, K = p.K, J = p.Jets, pl = (size_t)p.w * p.h, gpl = (size_t)gw * gh;
    const size_t S = fill ? 2 * K : K;                                          // the fusion's slots
    size_t stage = 0, occ_stage = 0;
    for (int r = 0; r < p.K; r++) {
        const size_t rJ = p.r_Jets[r], tap = identity[r] ? 8 : 16, spl = identity[r] ? pl : (size_t)p.source[r].cw * p.source[r].ch;
        a.rate[r].fw = take(n * rJ * pl * tap);
        a.rate[r].bw = take(n * rJ * pl * tap);
        a.rate[r].mask = p.use_occlusions ? take(n * rJ * pl) : 0;
        a.rate[r].acc_u = take(n * rJ * gpl * 8);
        a.rate[r].acc_v = take(n * rJ * gpl * 8);
        a.rate[r].tracked = take(n * gpl * 4);
        stage = std::max(stage, 2 * rJ * spl * 4);                              // one segment's u and v planes of one direction
        occ_stage = std::max(occ_stage, rJ * (size_t)p.source[r].sw * p.source[r].sh);
    }
    a.occluded = take(K * n * gpl);                                             // [K][n][gpl]
    a.stage = take(stage);
    a.occ_stage = p.use_occlusions ? take(occ_stage) : 0;
    a.frames = take(n * (J + 1) * 3 * pl * 4);
    a.der = take(n * (J + 1) * 6 * pl * 4);
    a.rec = take(n * (J + 1) * pl * 48);
    a.wU = take(n * J * gpl * 8); a.wV = take(n * J * gpl * 8); a.wocc = take(n * gpl * 8);
    a.jc = take(n * gpl * 4); a.oc = take(n * gpl * 4); a.ep = take(n * gpl * NN * 8);
    a.E = take(n * S * gpl * 8); a.O = take(n * S * gpl * 8); a.best = take(n * gpl);
    if (p.do_fuse) {
        a.aU = take(n * S * J * gpl * 8); a.aV = take(n * S * J * gpl * 8); a.weight = take(n * pl * 4);
        a.nl = take(n * gpl); a.lab = take(n * gpl * 16); a.theta = take(n * gpl * 16 * 8); a.P = take(n * 2 * gpl * S * S * 8);
        a.M = take(n * gpl * 4 * 16 * 8); a.xcur = take(n * gpl); a.xbest = take(n * gpl);
        a.slot = take(n * gpl * 4); a.fu = take(n * gpl * 8); a.fv = take(n * gpl * 8); a.out_occ = take(n * gpl);
        a.seg_energy = take(n * 8); a.seg_bound = take(n * 8); a.seg_iters = take(n * 4);
    }
    if (fill) {
        const size_t rJm = fg->rJmax, samples = (size_t)fg->nx * fg->ny;
        a.lab_stage = fill->epic.saliency_th != 0 ? take((size_t)kEpicSaliencyPlanes * fg->plp * 4) : 0;
        a.sal = fill->epic.saliency_th != 0 ? take(n * fg->plp * 4) : 0;
        a.edges = take(n * fg->cpl * 4); a.run_cost = take(n * fg->cpl * 4); a.cost = take(n * rJm * fg->cpl * 4);
        a.full = take(K * n * 4);
        a.cT = take(n * gpl * 4); a.cP = take(n * gpl * 4); a.cS = take(n * gpl * 4); a.mask = take(n * gpl); a.kept = take(n * 4); a.count = take(n * 4);
        a.xs = take((size_t)gw * 4); a.ys = take((size_t)gh * 4);
        a.block_count = take(n * std::max<size_t>(fill_matches_blocks(fg->nx, fg->ny), 1) * 4);
        a.matches = take(n * rJm * std::max<size_t>(samples, 1) * 16);
        a.fx = take(n * rJm * gpl * 4); a.fy = take(n * rJm * gpl * 4); a.inf = take(gpl * 8);
        for (int r = 0; r < p.K; r++) {
            a.fill[r].u = take(n * p.r_Jets[r] * gpl * 8); a.fill[r].v = take(n * p.r_Jets[r] * gpl * 8); a.fill[r].tracked = take(n * gpl * 4);
        }
    }
    a.total = top;
}

void sfa_track_params_default(sfa_track_params *p) {
    if (!p) return;
    *p = sfa_track_params{};
    p->n = 1; p->K = 1; p->Jets = 1; p->do_fuse = 1;
    p->epsilon = 1.0;                    // acc_consistency_threshold
    p->skip = 1;                         // acc_skip_pixel
    p->discard = 1;                      // acc_discard_inconsistent
    sfa_energy_params_default(&p->energy);
    sfa_fuse_params_default(&p->fuse);
    p->coef = 5.0f;                      // computeSmoothnessWeight's call (dense_tracking.cpp:969-981)
    for (int k = 0; k < 3; k++) p->std_dev[k] = 1.0f;
    for (int r = 0; r < kTrMaxK; r++) { p->r_Jets[r] = 1; p->weight[r] = (float)r; }   // weight_jet_estimation[r] = r where none is given
}

void sfa_track_fill_params_default(sfa_track_fill_params *fill) {
    if (!fill) return;
    *fill = sfa_track_fill_params{};
    fill->epic_skip = 2.0f;                                                     // acc_epic_skip (:651)
    fill->min_size = 100;                                                       // removeSmallSegments(r_consistent, 0.1, 100) (:1265)
    // epic_params_default (epic.cpp:127-136), then dense_tracking.cpp:652-656
    fill->epic.method = 0; fill->epic.saliency_th = 0.045f; fill->epic.pref_nn = 25; fill->epic.pref_th = 5.0f; fill->epic.nn = 160;
    fill->epic.coef_kernel = 1.1f; fill->epic.euc = 0.001f;
}

// one-line forms of the stream calls the fill-in makes many of
static int copy_on(sfa_ctx *ctx, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    SFA_HIP(ctx, hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
    return SFA_OK;
}
static int zero_on(sfa_ctx *ctx, void *dst, size_t bytes) {
    SFA_HIP(ctx, hipMemsetAsync(dst, 0, bytes, ctx->stream));
    return SFA_OK;
}
static int mark(sfa_ctx *ctx, hipEvent_t e) {
    SFA_HIP(ctx, hipEventRecord(e, ctx->stream));
    return SFA_OK;
}

// fill: null for a plain job
static int track_bytes(const char *fn, const sfa_track_params *p, const sfa_track_fill_params *fill, bool with_fill, size_t *bytes) {
    sfa_ctx *ctx = nullptr;
    if (!bytes) REFUSE("%s: bytes is null", fn);
    int gw, gh;
    bool identity[kTrMaxK];
    EnergyPlan plan[kTrMaxK];
    SFA_TRY(track_check(ctx, fn, p, &gw, &gh, identity, plan));
    FillGeo fg;
    if (with_fill) SFA_TRY(fill_check(ctx, fn, p, fill, gw, gh, &fg));
    TrackPlanes at{};
    track_layout(*p, gw, gh, identity, plan[0].NN, with_fill ? fill : nullptr, &fg, &at);
    *bytes = at.total;
    return SFA_OK;
}

int sfa_track_job_bytes(const sfa_track_params *p, size_t *bytes) { return track_bytes(__func__, p, nullptr, false, bytes); }
int sfa_track_job_bytes_fill(const sfa_track_params *p, const sfa_track_fill_params *fill, size_t *bytes) { return track_bytes(__func__, p, fill, true, bytes); }

static int track_create(sfa_ctx *ctx, const char *fn, const sfa_track_params *p, const sfa_track_fill_params *fill, bool with_fill, sfa_track_job **out) {
    if (!ctx || !out) REFUSE("%s: ctx or job is null", fn);
    *out = nullptr;
    sfa_track_job *j = new sfa_track_job;
    struct Guard { sfa_track_job *j; ~Guard() { if (j) sfa_track_job_destroy(j); } } guard{j};
    j->ctx = ctx;
    SFA_TRY(track_check(ctx, fn, p, &j->gw, &j->gh, j->identity, j->plan));
    if (with_fill) {
        SFA_TRY(fill_check(ctx, fn, p, fill, j->gw, j->gh, &j->fg));
        j->fill = true;
        j->fp = *fill;
    }
    j->p = *p;
    j->p.energy.skip = j->p.fuse.skip = p->skip;
    track_layout(j->p, j->gw, j->gh, j->identity, j->plan[0].NN, with_fill ? &j->fp : nullptr, &j->fg, &j->at);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(j->mem.alloc(ctx, j->at.total));
    SFA_HIP(ctx, hipMemsetAsync(j->mem.p, 0, j->at.total, ctx->stream));        // a run before an upload reads zeros, not another job's planes
    for (auto &e : j->ev) SFA_HIP(ctx, hipEventCreate(&e));
    if (with_fill) {
        for (int r = 0; r < p->K; r++)
            for (auto &e : j->fev[r]) SFA_HIP(ctx, hipEventCreate(&e));
        SFA_HIP(ctx, hipEventCreate(&j->ev_energy));
        const size_t rates = (size_t)p->K * p->n, images = (size_t)p->n * j->fg.rJmax, gpl = (size_t)j->gw * j->gh;
        j->full.reset(new int[rates]);
        for (size_t k = 0; k < rates; k++) j->full[k] = p->r_Jets[k / p->n];
        j->stats.reset(new int[3 * rates]());
        j->c_in.reset(new const float *[3 * images]()); j->c_out.reset(new float *[2 * images]()); j->c_int.reset(new int[5 * images + 2 * (size_t)p->n]());
        j->inf.reset(new double[gpl]);
        for (size_t k = 0; k < gpl; k++) j->inf[k] = (double)__builtin_inff();
        SFA_TRY(copy_on(ctx, j->ptr<double>(j->at.inf), j->inf.get(), gpl * 8, hipMemcpyHostToDevice));
        // (the host arrays live as long as the job, and the wait below is before anything can change them)
        SFA_TRY(copy_on(ctx, j->ptr<int>(j->at.full), j->full.get(), rates * 4, hipMemcpyHostToDevice));
        SFA_TRY(copy_on(ctx, j->ptr<int>(j->at.xs), j->fg.xs.get(), (size_t)j->gw * 4, hipMemcpyHostToDevice));
        SFA_TRY(copy_on(ctx, j->ptr<int>(j->at.ys), j->fg.ys.get(), (size_t)j->gh * 4, hipMemcpyHostToDevice));
        SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    guard.j = nullptr;
    *out = j;
    return SFA_OK;
}

int sfa_track_job_create(sfa_ctx *ctx, const sfa_track_params *p, sfa_track_job **out) { return track_create(ctx, __func__, p, nullptr, false, out); }
int sfa_track_job_create_fill(sfa_ctx *ctx, const sfa_track_params *p, const sfa_track_fill_params *fill, sfa_track_job **out) {
    return track_create(ctx, __func__, p, fill, true, out);
}

void sfa_track_job_destroy(sfa_track_job *job) {
    if (!job) return;
    if (job->ctx && job->ctx->stream) (void)hipStreamSynchronize(job->ctx->stream);
    for (auto &e : job->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &rate : job->fev)
        for (auto &e : rate)
            if (e) (void)hipEventDestroy(e);
    if (job->ev_energy) (void)hipEventDestroy(job->ev_energy);
    delete job;
}

#define TRACK_JOB(job) \
    if (!(job)) return sfa::set_error(nullptr, SFA_ERR_ARG, "%s: job is null", __func__); \
    sfa_ctx *ctx = (job)->ctx; \
    const sfa_track_params &p = (job)->p; \
    const size_t pl = (size_t)p.w * p.h, gpl = (size_t)(job)->gw * (job)->gh; \
    (void)pl; (void)gpl

static int track_range(sfa_ctx *ctx, const char *fn, const sfa_track_params &p, int s0, int ns, int r) {
    if (s0 < 0 || ns < 1 || (long)s0 + ns > p.n) {
        if (ns == 1) REFUSE("%s: s = %d lies outside the job's %d start_jets", fn, s0, p.n);
        REFUSE("%s: s0 = %d, ns = %d lie outside the job's %d start_jets", fn, s0, ns, p.n);
    }
    if (r < 0 || r >= p.K) REFUSE("%s: r = %d names none of the job's %d rates", fn, r, p.K);
    return SFA_OK;
}

int sfa_track_job_upload_flows(sfa_track_job *job, int s, int r, const float *const *fwd_u, const float *const *fwd_v, const float *const *bwd_u,
                               const float *const *bwd_v, const unsigned char *const *occ) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, r));
    if (!(fwd_u && fwd_v && bwd_u && bwd_v)) REFUSE("%s: null flow array", __func__);
    if (p.use_occlusions && !occ) REFUSE("%s: occ is null on a job with use_occlusions", __func__);
    const int rJ = p.r_Jets[r];
    for (int k = 0; k < rJ; k++)
        if (!fwd_u[k] || !fwd_v[k] || !bwd_u[k] || !bwd_v[k] || (p.use_occlusions && !occ[k])) REFUSE("%s: null plane %d", __func__, k);
    const sfa_jet_source &src = p.source[r];
    const bool identity = job->identity[r];
    const size_t tap = identity ? 8 : 16, seg = (size_t)s * rJ * pl;
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    float *stage = job->ptr<float>(job->at.stage);
    for (int dir = 0; dir < 2; dir++) {
        const float *const *U = dir ? bwd_u : fwd_u, *const *V = dir ? bwd_v : fwd_v;
        char *dst = job->ptr<char>(dir ? job->at.rate[r].bw : job->at.rate[r].fw) + seg * tap;
        if (!identity) {
            SFA_TRY(jet_resample_flows(ctx, src, (size_t)rJ, U, V, p.w, p.h, stage, reinterpret_cast<double2 *>(dst), nullptr, nullptr));
            continue;
        }
        float *su = stage, *sv = stage + (size_t)rJ * pl;
        for (int k = 0; k < rJ; k++) {                                          // the valid columns of each plane, packed, then interleaved
            SFA_HIP(ctx, hipMemcpy2DAsync(su + k * pl, (size_t)p.w * 4, U[k], (size_t)src.stride * 4, (size_t)p.w * 4, p.h, hipMemcpyHostToDevice, ctx->stream));
            SFA_HIP(ctx, hipMemcpy2DAsync(sv + k * pl, (size_t)p.w * 4, V[k], (size_t)src.stride * 4, (size_t)p.w * 4, p.h, hipMemcpyHostToDevice, ctx->stream));
        }
        launch_interleave(ctx, su, sv, reinterpret_cast<float2 *>(dst), (size_t)rJ * pl);
        SFA_HIP(ctx, hipGetLastError());
    }
    if (p.use_occlusions)
        SFA_TRY(jet_decode_occlusions(ctx, src, (size_t)rJ, occ, p.w, p.h, job->ptr<unsigned char>(job->at.occ_stage),
                                      job->ptr<unsigned char>(job->at.rate[r].mask) + seg));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));                            // the caller's planes are free again
    return SFA_OK;
}

int sfa_track_job_upload_frames(sfa_track_job *job, int s, const float *const *frames, int stride) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, 0));
    if (!frames) REFUSE("%s: frames is null", __func__);
    if (stride < p.w) REFUSE("%s: stride = %d < w = %d", __func__, stride, p.w);
    for (int k = 0; k <= p.Jets; k++)
        if (!frames[k]) REFUSE("%s: null frame %d", __func__, k);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    float *dst = job->ptr<float>(job->at.frames) + (size_t)s * (p.Jets + 1) * 3 * pl;
    for (int k = 0; k <= p.Jets; k++)
        for (int c = 0; c < 3; c++)
            SFA_HIP(ctx, hipMemcpy2DAsync(dst + ((size_t)k * 3 + c) * pl, (size_t)p.w * 4, frames[k] + (size_t)c * p.h * stride, (size_t)stride * 4, (size_t)p.w * 4,
                                          p.h, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

int sfa_track_job_upload_flows_device(sfa_track_job *job, int s0, int ns, int r, const float *fwd_dev, const float *bwd_dev, const long long strides[5]) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s0, ns, r));
    const sfa_jet_source &src = p.source[r];
    const int rJ = p.r_Jets[r];
    SFA_TRY(check_view(ctx, __func__, View{"fwd_dev", fwd_dev, sizeof(float), 5, {ns, rJ, 2, src.sh, src.sw}, strides}));
    SFA_TRY(check_view(ctx, __func__, View{"bwd_dev", bwd_dev, sizeof(float), 5, {ns, rJ, 2, src.sh, src.sw}, strides}));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const bool identity = job->identity[r];
    const size_t tap = identity ? 8 : 16, seg = (size_t)rJ * pl;
    for (int dir = 0; dir < 2; dir++) {
        const float *from = dir ? bwd_dev : fwd_dev;
        char *dst = job->ptr<char>(dir ? job->at.rate[r].bw : job->at.rate[r].fw) + (size_t)s0 * seg * tap;
        if (identity) {
            const size_t total = (size_t)ns * seg;
            hipLaunchKernelGGL(k_track_pack_flow, dim3(blocks_of(total)), dim3(kTrThreads), 0, ctx->stream, from, strides[0], strides[1], strides[2], strides[3],
                               strides[4], p.w, p.h, rJ, reinterpret_cast<float2 *>(dst), total);
            SFA_HIP(ctx, hipGetLastError());
            continue;
        }
        const size_t spl = (size_t)src.cw * src.ch, total = (size_t)rJ * spl;   // segment by segment through the one-segment stage, in stream order
        float *su = job->ptr<float>(job->at.stage), *sv = su + total;
        for (int s = 0; s < ns; s++) {
            hipLaunchKernelGGL(k_track_pack_planes, dim3(blocks_of(total)), dim3(kTrThreads), 0, ctx->stream, from + (long long)s * strides[0], strides[1], strides[2],
                               strides[3], strides[4], src.x0, src.y0, src.cw, src.ch, su, sv, total);
            SFA_HIP(ctx, hipGetLastError());
            SFA_TRY(launch_jet_resample(ctx, src, (size_t)rJ, su, sv, p.w, p.h, reinterpret_cast<double2 *>(dst + (size_t)s * seg * tap)));
        }
    }
    return SFA_OK;
}

int sfa_track_job_upload_occlusions_device(sfa_track_job *job, int s0, int ns, int r, const void *occ_dev, int dtype, const long long strides[4]) {
    TRACK_JOB(job);
    if (!p.use_occlusions) REFUSE("%s: the job was created without use_occlusions: it holds no occlusion masks", __func__);
    SFA_TRY(track_range(ctx, __func__, p, s0, ns, r));
    if (dtype != SFA_DEV_F32 && dtype != SFA_DEV_U8)
        REFUSE("%s: dtype %d is %s (fp32 0: the labels sfa_job_download_device leaves; u8 1: the raw images)", __func__, dtype,
               dtype == SFA_DEV_U16 ? "u16, which occlusion images do not come in" : "no element type");
    const sfa_jet_source &src = p.source[r];
    const int rJ = p.r_Jets[r];
    SFA_TRY(check_view(ctx, __func__, View{"occ_dev", occ_dev, dtype == SFA_DEV_F32 ? sizeof(float) : 1, 4, {ns, rJ, src.sh, src.sw}, strides}));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const size_t total = (size_t)rJ * src.sw * src.sh;                          // segment by segment through the one-segment stage, in stream order
    unsigned char *stage = job->ptr<unsigned char>(job->at.occ_stage), *mask = job->ptr<unsigned char>(job->at.rate[r].mask) + (size_t)s0 * rJ * pl;
    for (int s = 0; s < ns; s++) {
        if (dtype == SFA_DEV_F32)
            hipLaunchKernelGGL(k_track_pack_occ<float>, dim3(blocks_of(total)), dim3(kTrThreads), 0, ctx->stream,
                               static_cast<const float *>(occ_dev) + (long long)s * strides[0], strides[1], strides[2], strides[3], src.sw, src.sh, stage, total);
        else
            hipLaunchKernelGGL(k_track_pack_occ<unsigned char>, dim3(blocks_of(total)), dim3(kTrThreads), 0, ctx->stream,
                               static_cast<const unsigned char *>(occ_dev) + (long long)s * strides[0], strides[1], strides[2], strides[3], src.sw, src.sh, stage, total);
        SFA_HIP(ctx, hipGetLastError());
        SFA_TRY(launch_jet_occ_decode(ctx, src, (size_t)rJ, stage, p.w, p.h, mask + (size_t)s * rJ * pl));
    }
    return SFA_OK;
}

int sfa_track_job_upload_frames_device(sfa_track_job *job, int s0, int ns, const float *frames_dev, const long long strides[5]) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s0, ns, 0));
    SFA_TRY(check_view(ctx, __func__, View{"frames_dev", frames_dev, sizeof(float), 5, {ns, p.Jets + 1, 3, p.h, p.w}, strides}));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const size_t total = (size_t)ns * (p.Jets + 1) * 3 * pl;
    hipLaunchKernelGGL(k_track_pack_frames, dim3(blocks_of(total)), dim3(kTrThreads), 0, ctx->stream, frames_dev, strides[0], strides[1], strides[2], strides[3],
                       strides[4], p.w, p.h, p.Jets + 1, job->ptr<float>(job->at.frames) + (size_t)s0 * (p.Jets + 1) * 3 * pl, total);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

// The fill-in of every rate of segments 0 .. ns-1, between the accumulation and the energies (the header's description).  It leaves the trajectories in the
// rates' fill planes and {kept_pixels, matches, filled} in job->stats
static int track_run_fill(sfa_track_job *job, int ns) {
    TRACK_JOB(job);
    const TrackPlanes &at = job->at;
    const FillGeo &g = job->fg;
    const sfa_track_fill_params &fp = job->fp;
    hipStream_t st = ctx->stream;
    const int gw = job->gw, gh = job->gh, n = p.n;
    const size_t samples = (size_t)g.nx * g.ny;
    float *run_cost = job->ptr<float>(at.run_cost), *cost = job->ptr<float>(at.cost), *matches = job->ptr<float>(at.matches);
    float *fx = job->ptr<float>(at.fx), *fy = job->ptr<float>(at.fy);
    // the running maps start from the maps as uploaded: a run leaves them advanced by all its calls
    SFA_TRY(copy_on(ctx, run_cost, job->ptr<float>(at.edges), (size_t)ns * g.cpl * 4, hipMemcpyDeviceToDevice));
    const size_t images = (size_t)n * g.rJmax;
    const float **c_cost = job->c_in.get(), **c_matches = c_cost + images, **c_sal = c_matches + images;
    float **c_fx = job->c_out.get(), **c_fy = c_fx + images;
    int *c_nm = job->c_int.get(), *seg_of = c_nm + images, *step_of = seg_of + images, *rc = step_of + images, *status = rc + images, *kept = status + images,
        *count = kept + n;
    job->chain_runs[0] = job->chain_runs[1] = 0;
    for (int r = 0; r < p.K; r++) {
        const int rJ = p.r_Jets[r];
        hipEvent_t *ev = job->fev[r];
        int *stats = job->stats.get() + (size_t)r * n * 3;
        const double *acc_u = job->ptr<double>(at.rate[r].acc_u), *acc_v = job->ptr<double>(at.rate[r].acc_v);
        // ---- r_consistent after removeSmallSegments, the matches of every step; the one host read this stage adds
        SFA_TRY(mark(ctx, ev[0]));
        SFA_TRY(consistent_regions_device(ctx, ns, gw, gh, job->ptr<int>(at.rate[r].tracked), job->ptr<int>(at.full) + (size_t)r * n, fp.min_size, job->ptr<int>(at.cT),
                                          job->ptr<int>(at.cP), job->ptr<int>(at.cS), job->ptr<unsigned char>(at.mask), job->ptr<int>(at.kept)));
        if (samples)
            SFA_TRY(fill_matches_device(ctx, ns, rJ, gw, gh, acc_u, acc_v, job->ptr<unsigned char>(at.mask), job->ptr<int>(at.xs), g.nx, job->ptr<int>(at.ys), g.ny,
                                        p.skip + 1, job->ptr<int>(at.block_count), matches, job->ptr<int>(at.count)));
        SFA_TRY(copy_on(ctx, kept, job->ptr<int>(at.kept), (size_t)ns * 4, hipMemcpyDeviceToHost));
        if (samples) SFA_TRY(copy_on(ctx, count, job->ptr<int>(at.count), (size_t)ns * 4, hipMemcpyDeviceToHost));
        SFA_TRY(mark(ctx, ev[1]));
        SFA_HIP(ctx, hipStreamSynchronize(st));
        if (!samples) std::fill(count, count + ns, 0);                 // no sample on the grid: no match
        // ---- the edge costs of the rate's steps, for every segment: the calls count whether or not a rate is filled
        SFA_TRY(epic_edge_costs_device(ctx, ns, rJ, g.cpl, (int)gpl, fp.epic.euc, run_cost, cost));
        SFA_TRY(mark(ctx, ev[2]));
        // ---- the interpolation of the images of every segment with a match, segment-major
        int m = 0;
        for (int s = 0; s < ns; s++) {
            stats[3 * s] = kept[s]; stats[3 * s + 1] = count[s]; stats[3 * s + 2] = count[s] > 0;
            for (int j = 0; j < rJ && count[s] > 0; j++, m++) {
                const size_t k = (size_t)s * rJ + j;
                c_cost[m] = cost + k * g.cpl; c_matches[m] = matches + k * samples * 4; c_nm[m] = count[s];
                c_sal[m] = fp.epic.saliency_th != 0 ? job->ptr<float>(at.sal) + (size_t)s * g.plp : nullptr;
                c_fx[m] = fx + k * gpl; c_fy[m] = fy + k * gpl;
                seg_of[m] = s; step_of[m] = j;
            }
        }
        if (m) {
            const EpicChainDev io{c_cost, c_matches, c_nm, c_sal, c_fx, c_fy};
            SFA_TRY(epic_chain_device(ctx, "sfa_track_job_run", m, gw, gh, &fp.epic, io, rc, nullptr, fp.workspace_bytes, status));
            for (int k = 0; k < 2; k++) job->chain_runs[k] += ctx->epic_chain_runs[k];
            for (int k = 0; k < m; k++) {
                if (status[k])
                    REFUSE("sfa_track_job_run: the fill-in image of start_jet %d, rate %d, step %d (%d matches) does not fit the interpolation's workspace even alone",
                           seg_of[k], r, step_of[k], c_nm[k]);
                if (rc[k] > 0) stats[3 * seg_of[k] + 2] = 0;                     // a step without a usable match: no fill-in hypothesis for the rate
            }
        }
        SFA_TRY(mark(ctx, ev[3]));
        // ---- the planes as trajectories; a segment that is not filled gets zeros (its slot is emptied after the energies)
        for (int s = 0; s < ns; s++) {
            if (stats[3 * s + 2]) continue;
            SFA_TRY(zero_on(ctx, fx + (size_t)s * rJ * gpl, (size_t)rJ * gpl * 4));
            SFA_TRY(zero_on(ctx, fy + (size_t)s * rJ * gpl, (size_t)rJ * gpl * 4));
        }
        SFA_TRY(fill_trajectories_device(ctx, ns, rJ, gw, gh, gw, fx, fy, p.skip + 1, job->ptr<double>(at.fill[r].u), job->ptr<double>(at.fill[r].v),
                                         job->ptr<int>(at.fill[r].tracked)));
        SFA_TRY(mark(ctx, ev[4]));
    }
    SFA_TRY(mark(ctx, job->ev_energy));
    return SFA_OK;
}

int sfa_track_job_run(sfa_track_job *job, int ns) {
    TRACK_JOB(job);
    if (ns < 1 || ns > p.n) REFUSE("%s: ns = %d (1 <= ns <= n = %d, the job's start_jets)", __func__, ns, p.n);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const TrackPlanes &at = job->at;
    const int K = p.K, J = p.Jets, mf = p.min_fps_idx;
    hipEvent_t *ev = job->ev;
    SFA_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    energy_records_device(ctx, (size_t)ns * (J + 1), p.w, p.h, job->ptr<float>(at.frames), job->ptr<float>(at.der), job->ptr<void>(at.rec));
    SFA_HIP(ctx, hipGetLastError());
    SFA_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    for (int r = 0; r < K; r++)
        SFA_TRY(accumulate_device(ctx, ns, p.r_Jets[r], p.w, p.h, job->gw, job->gh, p.skip, job->identity[r], job->ptr<void>(at.rate[r].fw),
                                  job->ptr<void>(at.rate[r].bw), p.use_occlusions ? job->ptr<unsigned char>(at.rate[r].mask) : nullptr, p.epsilon, p.discard, 1,
                                  job->ptr<double>(at.rate[r].acc_u), job->ptr<double>(at.rate[r].acc_v), job->ptr<int>(at.rate[r].tracked)));
    SFA_HIP(ctx, hipEventRecord(ev[2], ctx->stream));
    if (job->fill) SFA_TRY(track_run_fill(job, ns));
    const int S = job->slots(), step = job->step();                            // rate r's accumulated hypothesis is slot r * step, its fill-in the next
    EnergyWork wk;
    wk.U = job->ptr<double>(at.wU); wk.V = job->ptr<double>(at.wV); wk.occ = job->ptr<unsigned long long>(at.wocc);
    wk.jc = job->ptr<float>(at.jc); wk.oc = job->ptr<float>(at.oc); wk.ep = job->ptr<double>(at.ep);
    double *E = job->ptr<double>(at.E);
    unsigned long long *O = job->ptr<unsigned long long>(at.O);
    for (int r = 0; r < K; r++) {
        const bool flows = r >= mf;                                             // a rate before acc_min_fps sees empty flow Mats (:786, :1148-1151)
        SFA_TRY(energies_device(ctx, job->plan[r], ns, job->ptr<double>(at.rate[r].acc_u), job->ptr<double>(at.rate[r].acc_v), job->ptr<int>(at.rate[r].tracked),
                                job->ptr<void>(at.rec), job->identity[mf], flows ? job->ptr<void>(at.rate[mf].fw) : nullptr,
                                flows ? job->ptr<void>(at.rate[mf].bw) : nullptr, wk, E + (size_t)r * step * gpl, O + (size_t)r * step * gpl, (size_t)S * gpl,
                                p.do_fuse ? job->ptr<double>(at.aU) + (size_t)r * step * J * gpl : nullptr,
                                p.do_fuse ? job->ptr<double>(at.aV) + (size_t)r * step * J * gpl : nullptr, (size_t)S * J * gpl));
        if (!job->fill) continue;
        const size_t slot = 2 * (size_t)r + 1;                                  // the fill-in: the rate's plan and weight, the same flows
        double *aU = p.do_fuse ? job->ptr<double>(at.aU) + slot * J * gpl : nullptr, *aV = p.do_fuse ? job->ptr<double>(at.aV) + slot * J * gpl : nullptr;
        SFA_TRY(energies_device(ctx, job->plan[r], ns, job->ptr<double>(at.fill[r].u), job->ptr<double>(at.fill[r].v), job->ptr<int>(at.fill[r].tracked),
                                job->ptr<void>(at.rec), job->identity[mf], flows ? job->ptr<void>(at.rate[mf].fw) : nullptr,
                                flows ? job->ptr<void>(at.rate[mf].bw) : nullptr, wk, E + slot * gpl, O + slot * gpl, (size_t)S * gpl, aU, aV, (size_t)S * J * gpl));
        for (int s = 0; s < ns; s++) {
            if (job->stats[((size_t)r * p.n + s) * 3 + 2]) continue;
            const size_t so = (size_t)s * S * gpl, sa = (size_t)s * S * J * gpl;
            // the slot of a hypothesis that does not exist: energy +Inf, occlusion word 0, adapted flows 0
            SFA_TRY(copy_on(ctx, E + slot * gpl + so, job->ptr<double>(at.inf), gpl * 8, hipMemcpyDeviceToDevice));
            SFA_TRY(zero_on(ctx, O + slot * gpl + so, gpl * 8));
            if (aU) SFA_TRY(zero_on(ctx, aU + sa, (size_t)J * gpl * 8));
            if (aV) SFA_TRY(zero_on(ctx, aV + sa, (size_t)J * gpl * 8));
        }
    }
    const dim3 pix(blocks_of(gpl), (unsigned)ns);
    hipLaunchKernelGGL(k_track_best, pix, dim3(kTrThreads), 0, ctx->stream, E, O, K, S, step, (int)gpl, p.n, job->ptr<unsigned char>(at.best),
                       job->ptr<unsigned char>(at.occluded));
    SFA_HIP(ctx, hipGetLastError());
    SFA_HIP(ctx, hipEventRecord(ev[3], ctx->stream));
    job->timed = true;
    job->timed_fuse = false;
    if (!p.do_fuse) return SFA_OK;
    // computeSmoothnessWeight of every segment's normalised frame 0 (sfa_dt_smoothness_weight's kernel) on the packed planes
    Geo g{p.w, p.h, p.w, (long)pl, (long)pl, ns, WMask::first(ns), nullptr};
    launch_dpsis(ctx, g, job->ptr<float>(at.weight), job->ptr<float>(at.frames), (long)((size_t)(J + 1) * 3 * pl), p.coef, p.avg, p.std_dev, p.hbit);
    SFA_HIP(ctx, hipGetLastError());
    SFA_HIP(ctx, hipEventRecord(ev[9], ctx->stream));
    FuseWork f;
    f.U = job->ptr<double>(at.aU); f.V = job->ptr<double>(at.aV); f.energy = E; f.occ = O; f.weight = job->ptr<float>(at.weight);
    f.nl = job->ptr<unsigned char>(at.nl); f.lab = job->ptr<unsigned char>(at.lab); f.theta = job->ptr<double>(at.theta); f.P = job->ptr<double>(at.P);
    f.M = job->ptr<double>(at.M); f.xcur = job->ptr<unsigned char>(at.xcur); f.xbest = job->ptr<unsigned char>(at.xbest);
    f.slot = job->ptr<int>(at.slot); f.fu = job->ptr<double>(at.fu); f.fv = job->ptr<double>(at.fv); f.out_occ = job->ptr<unsigned char>(at.out_occ);
    f.seg_energy = job->ptr<double>(at.seg_energy); f.seg_bound = job->ptr<double>(at.seg_bound); f.seg_iters = job->ptr<int>(at.seg_iters);
    SFA_TRY(fuse_device(ctx, &p.fuse, ns, S, J, p.w, p.h, job->gw, job->gh, f, ev + 4));
    job->timed_fuse = true;
    return SFA_OK;
}

int sfa_track_job_download_rate(sfa_track_job *job, int s, int r, double *acc_u_last, double *acc_v_last, int *tracked, double *energy,
                                unsigned long long *occ_bits, unsigned char *occluded) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, r));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const TrackPlanes::Rate &a = job->at.rate[r];
    const size_t last = ((size_t)s * p.r_Jets[r] + (p.r_Jets[r] - 1)) * gpl, sk = ((size_t)s * job->slots() + (size_t)r * job->step()) * gpl;
    auto get = [&](void *dst, const void *src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess; };
    SFA_HIP(ctx, get(acc_u_last, job->ptr<double>(a.acc_u) + last, gpl * 8));
    SFA_HIP(ctx, get(acc_v_last, job->ptr<double>(a.acc_v) + last, gpl * 8));
    SFA_HIP(ctx, get(tracked, job->ptr<int>(a.tracked) + (size_t)s * gpl, gpl * 4));
    SFA_HIP(ctx, get(energy, job->ptr<double>(job->at.E) + sk, gpl * 8));
    SFA_HIP(ctx, get(occ_bits, job->ptr<unsigned long long>(job->at.O) + sk, gpl * 8));
    SFA_HIP(ctx, get(occluded, job->ptr<unsigned char>(job->at.occluded) + ((size_t)r * p.n + s) * gpl, gpl));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

int sfa_track_job_download_fused(sfa_track_job *job, int s, int *slot, double *flow_u, double *flow_v, unsigned char *occ, unsigned char *best, double *energy,
                                 double *bound, int *iters) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, 0));
    if (!p.do_fuse) REFUSE("%s: the job was created with do_fuse = 0: it holds no fused result", __func__);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const TrackPlanes &at = job->at;
    const size_t o = (size_t)s * gpl;
    auto get = [&](void *dst, const void *src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess; };
    SFA_HIP(ctx, get(slot, job->ptr<int>(at.slot) + o, gpl * 4));
    SFA_HIP(ctx, get(flow_u, job->ptr<double>(at.fu) + o, gpl * 8));
    SFA_HIP(ctx, get(flow_v, job->ptr<double>(at.fv) + o, gpl * 8));
    SFA_HIP(ctx, get(occ, job->ptr<unsigned char>(at.out_occ) + o, gpl));
    SFA_HIP(ctx, get(best, job->ptr<unsigned char>(at.best) + o, gpl));
    SFA_HIP(ctx, get(energy, job->ptr<double>(at.seg_energy) + s, 8));
    SFA_HIP(ctx, get(bound, job->ptr<double>(at.seg_bound) + s, 8));
    SFA_HIP(ctx, get(iters, job->ptr<int>(at.seg_iters) + s, 4));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

int sfa_track_job_download_best(sfa_track_job *job, int s, unsigned char *best) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, 0));
    if (!best) REFUSE("%s: best is null", __func__);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_HIP(ctx, hipMemcpyAsync(best, job->ptr<unsigned char>(job->at.best) + (size_t)s * gpl, gpl, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

int sfa_ctx_free_bytes(sfa_ctx *ctx, size_t *free_bytes) {
    if (!ctx || !free_bytes) REFUSE("%s: null argument", __func__);
    size_t total = 0;
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_HIP(ctx, hipMemGetInfo(free_bytes, &total));
    return SFA_OK;
}

int sfa_track_job_download_device(sfa_track_job *job, int s0, int ns, double *flow_dev, const long long strides[4], int *slot_dev, unsigned char *occ_dev,
                                  double *stats_dev) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s0, ns, 0));
    if (!p.do_fuse) REFUSE("%s: the job was created with do_fuse = 0: it holds no fused result", __func__);
    // the fp64 flow at the caller's strides; slot, occlusions and statistics (each optional) dense
    const long long plane[2] = {(long long)gpl, 1}, triple[2] = {3, 1};
    const View flow{"flow_dev", flow_dev, sizeof(double), 4, {ns, 2, job->gh, job->gw}, strides}, slot{"slot_dev", slot_dev, sizeof(int), 2, {ns, (int)gpl}, plane},
        occ{"occ_dev", occ_dev, 1, 2, {ns, (int)gpl}, plane}, stats{"stats_dev", stats_dev, sizeof(double), 2, {ns, 3}, triple};
    SFA_TRY(check_view(ctx, __func__, flow));
    if (!strides_nest(strides, flow.n, 4)) REFUSE("%s: the strides of flow_dev (%lld, %lld, %lld, %lld) let two elements of [%d][2][%d][%d] share an address", __func__,
                                                 strides[0], strides[1], strides[2], strides[3], ns, job->gh, job->gw);
    for (const View *v : {&slot, &occ, &stats})
        if (v->p) SFA_TRY(check_view(ctx, __func__, *v));
    SFA_TRY(check_disjoint(ctx, __func__, {flow, slot, occ, stats}));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const TrackPlanes &at = job->at;
    const size_t o = (size_t)s0 * gpl;
    hipLaunchKernelGGL(k_track_unpack, dim3(blocks_of(gpl), (unsigned)ns), dim3(kTrThreads), 0, ctx->stream, job->ptr<double>(at.fu) + o, job->ptr<double>(at.fv) + o,
                       job->ptr<int>(at.slot) + o, job->ptr<unsigned char>(at.out_occ) + o, job->ptr<double>(at.seg_energy) + s0, job->ptr<double>(at.seg_bound) + s0,
                       job->ptr<int>(at.seg_iters) + s0, job->gw, (int)gpl, flow_dev, strides[0], strides[1], strides[2], strides[3], slot_dev, occ_dev, stats_dev);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

// what the two per-rate exits share: the views of the destinations, and k_track_unpack_rate over segments s0 .. (bytes: rate r's occluded, or best)
static int track_unpack_rate(sfa_track_job *job, const char *fn, int s0, int ns, int r, double *acc_dev, const long long *strides, int *tracked_dev,
                             double *energy_dev, unsigned long long *occ_bits_dev, unsigned char *bytes_dev, const char *bytes_name, bool best) {
    TRACK_JOB(job);
    const long long plane[2] = {(long long)gpl, 1};
    const View acc{"acc_dev", acc_dev, sizeof(double), 4, {ns, 2, job->gh, job->gw}, strides}, tracked{"tracked_dev", tracked_dev, sizeof(int), 2, {ns, (int)gpl}, plane},
        energy{"energy_dev", energy_dev, sizeof(double), 2, {ns, (int)gpl}, plane}, bits{"occ_bits_dev", occ_bits_dev, 8, 2, {ns, (int)gpl}, plane},
        bytes{bytes_name, bytes_dev, 1, 2, {ns, (int)gpl}, plane};
    if (acc_dev) {
        SFA_TRY(check_view(ctx, fn, acc));
        if (!strides_nest(strides, acc.n, 4)) REFUSE("%s: the strides of acc_dev (%lld, %lld, %lld, %lld) let two elements of [%d][2][%d][%d] share an address", fn,
                                                    strides[0], strides[1], strides[2], strides[3], ns, job->gh, job->gw);
    }
    for (const View *v : {&tracked, &energy, &bits, &bytes})
        if (v->p) SFA_TRY(check_view(ctx, fn, *v));
    if (!acc_dev && !tracked_dev && !energy_dev && !occ_bits_dev && !bytes_dev) return SFA_OK;
    SFA_TRY(check_disjoint(ctx, fn, {acc, tracked, energy, bits, bytes}));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const TrackPlanes &at = job->at;
    const TrackPlanes::Rate &a = at.rate[r];
    const size_t rJ = p.r_Jets[r], last = ((size_t)s0 * rJ + (rJ - 1)) * gpl, sk = ((size_t)s0 * job->slots() + (size_t)r * job->step()) * gpl;
    const unsigned char *from = best ? job->ptr<unsigned char>(at.best) + (size_t)s0 * gpl : job->ptr<unsigned char>(at.occluded) + ((size_t)r * p.n + s0) * gpl;
    const long long none[4] = {0, 0, 0, 0}, *st = acc_dev ? strides : none;
    hipLaunchKernelGGL(k_track_unpack_rate, dim3(blocks_of(gpl), (unsigned)ns), dim3(kTrThreads), 0, ctx->stream, job->ptr<double>(a.acc_u) + last,
                       job->ptr<double>(a.acc_v) + last, rJ * gpl, job->ptr<int>(a.tracked) + (size_t)s0 * gpl, gpl, job->ptr<double>(at.E) + sk,
                       job->ptr<unsigned long long>(at.O) + sk, (size_t)job->slots() * gpl, from, gpl, job->gw, (int)gpl, acc_dev, st[0], st[1], st[2], st[3], tracked_dev,
                       energy_dev, occ_bits_dev, bytes_dev);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_track_job_download_rate_device(sfa_track_job *job, int s0, int ns, int r, double *acc_dev, const long long strides[4], int *tracked_dev, double *energy_dev,
                                       unsigned long long *occ_bits_dev, unsigned char *occluded_dev) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s0, ns, r));
    return track_unpack_rate(job, __func__, s0, ns, r, acc_dev, strides, tracked_dev, energy_dev, occ_bits_dev, occluded_dev, "occluded_dev", false);
}

int sfa_track_job_download_best_device(sfa_track_job *job, int s0, int ns, unsigned char *best_dev) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s0, ns, 0));
    if (!best_dev) REFUSE("%s: best_dev is null", __func__);
    return track_unpack_rate(job, __func__, s0, ns, 0, nullptr, nullptr, nullptr, nullptr, nullptr, best_dev, "best_dev", true);
}

int sfa_track_job_stage_ms(sfa_track_job *job, float ms[8]) {
    TRACK_JOB(job);
    if (!ms) REFUSE("%s: ms is null", __func__);
    if (!job->timed) REFUSE("%s: the job has not run", __func__);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 8; i++) ms[i] = 0;
    const int last = job->timed_fuse ? 8 : 3;
    for (int i = 0; i < last; i++)                                              // ms[3]: the weight kernel alone, without the fusion's clears behind it
        SFA_HIP(ctx, hipEventElapsedTime(&ms[i], i == 2 && job->fill ? job->ev_energy : job->ev[i], job->ev[i == 3 ? 9 : i + 1]));
    return SFA_OK;
}

// ---- a fill job's own entry points ------------------------------------------------------------------------------------------------------------------------
#define FILL_JOB(job) \
    TRACK_JOB(job); \
    if (!(job)->fill) REFUSE("%s: the job was not created by sfa_track_job_create_fill: it holds no fill-in", __func__); \
    const FillGeo &g = (job)->fg; \
    const bool saliency = (job)->fp.epic.saliency_th != 0; \
    (void)g; (void)saliency

// the saliency of the Lab image in the workspace's first three planes -> segment s's plane
static int track_saliency(sfa_track_job *job, int s) {
    sfa_ctx *ctx = job->ctx;
    const FillGeo &g = job->fg;
    float *stage = job->ptr<float>(job->at.lab_stage);
    const Geo geo{job->gw, job->gh, g.pitch, (long)g.plp, (long)(kEpicSaliencyPlanes * g.plp), 1, WMask::first(1), nullptr};
    epic_saliency_device(ctx, geo, stage, 0.8f, 1.0f);                          // epic()'s saliency(im, 0.8f, 1.0f)
    SFA_HIP(ctx, hipGetLastError());
    SFA_TRY(copy_on(ctx, job->ptr<float>(job->at.sal) + (size_t)s * g.plp, stage + (size_t)kEpicSaliencyOut * g.plp, g.plp * 4, hipMemcpyDeviceToDevice));
    return SFA_OK;
}

int sfa_track_job_upload_fill(sfa_track_job *job, int s, const float *lab, int lab_stride, const float *edges) {
    FILL_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, 0));
    if (!edges) REFUSE("%s: edges is null", __func__);
    if (saliency && !lab) REFUSE("%s: lab is null (epic.saliency_th != 0: the saliency filter reads the Lab image)", __func__);
    if (saliency && lab_stride < job->gw) REFUSE("%s: lab_stride = %d < gw = %d", __func__, lab_stride, job->gw);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    if (saliency) {
        for (int c = 0; c < 3; c++)
            SFA_TRY(upload_plane(ctx, job->ptr<float>(job->at.lab_stage) + (size_t)c * g.plp, g.pitch, lab + (size_t)c * job->gh * lab_stride, lab_stride, job->gw, job->gh));
        SFA_TRY(track_saliency(job, s));
    }
    SFA_TRY(copy_on(ctx, job->ptr<float>(job->at.edges) + (size_t)s * g.cpl, edges, gpl * 4, hipMemcpyHostToDevice));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));                            // the caller's planes are free again
    return SFA_OK;
}

int sfa_track_job_upload_fill_device(sfa_track_job *job, int s0, int ns, const float *lab_dev, const long long lab_strides[4], const float *edges_dev,
                                     const long long edge_strides[3]) {
    FILL_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s0, ns, 0));
    if (saliency) SFA_TRY(check_view(ctx, __func__, View{"lab_dev", lab_dev, sizeof(float), 4, {ns, 3, job->gh, job->gw}, lab_strides}));
    SFA_TRY(check_view(ctx, __func__, View{"edges_dev", edges_dev, sizeof(float), 3, {ns, job->gh, job->gw}, edge_strides}));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    for (int s = 0; saliency && s < ns; s++) {                                  // segment by segment through the one workspace, in stream order
        // packed by the frames' kernel (one frame of three channels) into planes the saliency only uses as scratch, then row by row to the device pitch
        const size_t total = 3 * gpl;
        float *stage = job->ptr<float>(job->at.lab_stage), *packed = stage + 3 * g.plp;
        hipLaunchKernelGGL(k_track_pack_frames, dim3(blocks_of(total)), dim3(kTrThreads), 0, ctx->stream, lab_dev + (long long)s * lab_strides[0], 0ll, 0ll, lab_strides[1],
                           lab_strides[2], lab_strides[3], job->gw, job->gh, 1, packed, total);
        SFA_HIP(ctx, hipGetLastError());
        for (int c = 0; c < 3; c++)
            SFA_HIP(ctx, hipMemcpy2DAsync(stage + (size_t)c * g.plp, (size_t)g.pitch * 4, packed + (size_t)c * gpl, (size_t)job->gw * 4, (size_t)job->gw * 4, job->gh,
                                          hipMemcpyDeviceToDevice, ctx->stream));
        SFA_TRY(track_saliency(job, s0 + s));
    }
    for (int s = 0; s < ns; s++) {                                              // the frames' kernel again: one frame, its first channel alone
        hipLaunchKernelGGL(k_track_pack_frames, dim3(blocks_of(gpl)), dim3(kTrThreads), 0, ctx->stream, edges_dev + (long long)s * edge_strides[0], 0ll, 0ll, 0ll,
                           edge_strides[1], edge_strides[2], job->gw, job->gh, 1, job->ptr<float>(job->at.edges) + (size_t)(s0 + s) * g.cpl, gpl);
        SFA_HIP(ctx, hipGetLastError());
    }
    return SFA_OK;
}

int sfa_track_job_download_fill(sfa_track_job *job, int s, int r, double *fill_u, double *fill_v, double *energy, unsigned long long *occ_bits, int *stats) {
    FILL_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, r));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const size_t rJ = p.r_Jets[r], sk = ((size_t)s * job->slots() + 2 * (size_t)r + 1) * gpl;
    auto get = [&](void *dst, const void *src, size_t bytes) { return dst ? copy_on(ctx, dst, src, bytes, hipMemcpyDeviceToHost) : (int)SFA_OK; };
    SFA_TRY(get(fill_u, job->ptr<double>(job->at.fill[r].u) + (size_t)s * rJ * gpl, rJ * gpl * 8));
    SFA_TRY(get(fill_v, job->ptr<double>(job->at.fill[r].v) + (size_t)s * rJ * gpl, rJ * gpl * 8));
    SFA_TRY(get(energy, job->ptr<double>(job->at.E) + sk, gpl * 8));
    SFA_TRY(get(occ_bits, job->ptr<unsigned long long>(job->at.O) + sk, gpl * 8));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stats)
        for (int k = 0; k < 3; k++) stats[k] = job->stats[((size_t)r * p.n + s) * 3 + k];
    return SFA_OK;
}

int sfa_track_job_fill_info(sfa_track_job *job, int info[2]) {
    FILL_JOB(job);
    if (!info) REFUSE("%s: info is null", __func__);
    if (!job->timed) REFUSE("%s: the job has not run", __func__);
    info[0] = job->chain_runs[0]; info[1] = job->chain_runs[1];
    return SFA_OK;
}

int sfa_track_job_fill_ms(sfa_track_job *job, float ms[4]) {
    FILL_JOB(job);
    if (!ms) REFUSE("%s: ms is null", __func__);
    if (!job->timed) REFUSE("%s: the job has not run", __func__);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 4; i++) ms[i] = 0;
    for (int r = 0; r < p.K; r++)
        for (int i = 0; i < 4; i++) {
            float v = 0;
            SFA_HIP(ctx, hipEventElapsedTime(&v, job->fev[r][i], job->fev[r][i + 1]));
            ms[i] += v;
        }
    return SFA_OK;
}

#pragma clang attribute pop
