// track.hip -- the resident track job: dense_tracking's three stages (accumulate.hip, energy.hip, fuse.hip) chained on the device for up to n start_jets of K
// rates.  The job owns every plane between the inputs and the fused flow; sfa_track_job_run enqueues
//     frame derivatives and records -> accumulation (all steps) per rate -> energies and adapted flows per rate, best / occluded -> smoothness weight
//     -> labels -> pairwise -> TRW-S -> output
// on the context's stream through the stages' device-level functions (sfa_internal.h) and returns: TRW-S's stopping rule lives inside k_trws, so nothing in
// the chain needs a host decision, and no stage boundary crosses the host.  The flows are brought into the kernels' layout when they are uploaded (host
// planes: stage_io.hip's uploads, the stage wrappers' own; device memory: the pack kernels below; occlusion images likewise), so a run reads only what the job holds.
// Segment s of a run comes out with the bits of the staged calls on that segment alone: the same kernels over the same planes, blockIdx.y = s.
// The device entry points describe their arguments as views and leave every check of them to check_view / check_disjoint (api.hip on dev_view.h).
// The job and its plane table are track_job.h's; what a fill job adds between the accumulation and the energies is track_fill.hip.
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

#include "sfa_device.h"
#include "track_job.h"

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

static_assert(kTrMaxK == kTrackMaxRates && kTrThreads == kTrackThreads, "track_job.h restates the two for track_fill.hip");

// Everything below is launch orchestration: argument checks, layout arithmetic, copies and launches, a few microseconds per call beside milliseconds of
// kernels.  It is compiled for size, so that the release build stays under the share of the full build tests/test_abi.py holds it to.
#pragma clang attribute push(__attribute__((minsize)), apply_to = function)

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
        if (p->fuse.pin_first != 0) REFUSE("%s: fuse.pin_first %d: the job's one fusion sorts every slot (call sfa_fuse_params_default first)", fn, p->fuse.pin_first);
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

// the planes in TrackPlanes' order, counted in elements; fill, fg: null for a plain job
static void track_layout(const sfa_track_params &p, int gw, int gh, const bool *identity, int NN, const sfa_track_fill_params *fill, const FillGeo *fg,
                         const sfa_track_alt_params *alt, TrackPlanes *out) {
    TrackPlanes &a = *out;
    a = TrackPlanes{};                                                          // a plane the job does not have stays at offset 0
    PlaneCursor c;
    const size_t n = p.n, K = p.K, J = p.Jets, pl = (size_t)p.w * p.h, gpl = (size_t)gw * gh;
    const size_t S = fill ? 2 * K : K;                                          // the fusion's slots
    size_t stage = 0, occ_stage = 0;
    for (int r = 0; r < p.K; r++) {
        TrackPlanes::Rate &t = a.rate[r];
        const size_t rJ = p.r_Jets[r], tap = identity[r] ? sizeof(float2) : sizeof(double2), spl = identity[r] ? pl : (size_t)p.source[r].cw * p.source[r].ch;
        c.take(t.fw, n * rJ * pl * tap); c.take(t.bw, n * rJ * pl * tap);
        if (p.use_occlusions) c.take(t.mask, n * rJ * pl);
        c.take(t.acc_u, n * rJ * gpl); c.take(t.acc_v, n * rJ * gpl); c.take(t.tracked, n * gpl);
        stage = std::max(stage, 2 * rJ * spl);                                  // one segment's u and v planes of one direction
        occ_stage = std::max(occ_stage, rJ * (size_t)p.source[r].sw * p.source[r].sh);
    }
    c.take(a.occluded, K * n * gpl);                                            // [K][n][gpl]
    c.take(a.stage, stage);
    if (p.use_occlusions) c.take(a.occ_stage, occ_stage);
    c.take(a.frames, n * (J + 1) * 3 * pl); c.take(a.der, n * (J + 1) * 6 * pl); c.take(a.rec, n * (J + 1) * pl * 48);
    c.take(a.wU, n * J * gpl); c.take(a.wV, n * J * gpl); c.take(a.wocc, n * gpl);
    c.take(a.jc, n * gpl); c.take(a.oc, n * gpl); c.take(a.ep, n * gpl * NN);
    c.take(a.E, n * S * gpl); c.take(a.O, n * S * gpl); c.take(a.best, n * gpl);
    if (p.do_fuse) {
        c.take(a.aU, n * S * J * gpl); c.take(a.aV, n * S * J * gpl); c.take(a.weight, n * pl);
        c.take(a.nl, n * gpl); c.take(a.lab, n * gpl * 16); c.take(a.theta, n * gpl * 16); c.take(a.P, n * 2 * gpl * S * S);
        c.take(a.M, n * gpl * 4 * 16); c.take(a.xcur, n * gpl); c.take(a.xbest, n * gpl);
        c.take(a.slot, n * gpl); c.take(a.fu, n * gpl); c.take(a.fv, n * gpl); c.take(a.out_occ, n * gpl);
        c.take(a.seg_energy, n); c.take(a.seg_bound, n); c.take(a.seg_iters, n);
    }
    if (fill) fill_layout(c, p, gw, gh, *fill, *fg, &a);
    if (alt) alt_layout(c, p, gw, gh, *alt, &a);
    a.total = c.top;
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

// with_fill: the call is a fill job's, and a null fill is refused under its name
int sfa::track_bytes(const char *fn, const sfa_track_params *p, const sfa_track_fill_params *fill, bool with_fill, const sfa_track_alt_params *alt, bool with_alt,
                     size_t *bytes) {
    sfa_ctx *ctx = nullptr;
    if (!bytes) REFUSE("%s: bytes is null", fn);
    int gw, gh;
    bool identity[kTrMaxK];
    EnergyPlan plan[kTrMaxK];
    SFA_TRY(track_check(ctx, fn, p, &gw, &gh, identity, plan));
    FillGeo fg;
    if (with_fill) SFA_TRY(fill_check(ctx, fn, p, fill, gw, gh, &fg));
    if (with_alt) SFA_TRY(alt_check(ctx, fn, p, alt, with_fill, gw, gh, nullptr));
    TrackPlanes at;
    track_layout(*p, gw, gh, identity, plan[0].NN, with_fill ? fill : nullptr, &fg, with_alt ? alt : nullptr, &at);
    *bytes = at.total;
    return SFA_OK;
}

int sfa_track_job_bytes(const sfa_track_params *p, size_t *bytes) { return track_bytes(__func__, p, nullptr, false, nullptr, false, bytes); }
int sfa_track_job_bytes_fill(const sfa_track_params *p, const sfa_track_fill_params *fill, size_t *bytes) {
    return track_bytes(__func__, p, fill, true, nullptr, false, bytes);
}

int sfa::track_create(sfa_ctx *ctx, const char *fn, const sfa_track_params *p, const sfa_track_fill_params *fill, bool with_fill, const sfa_track_alt_params *alt,
                      bool with_alt, sfa_track_job **out) {
    if (!ctx || !out) REFUSE("%s: ctx or job is null", fn);
    *out = nullptr;
    sfa_track_job *j = new sfa_track_job;
    struct Guard { sfa_track_job *j; ~Guard() { if (j) sfa_track_job_destroy(j); } } guard{j};
    j->ctx = ctx;
    SFA_TRY(track_check(ctx, fn, p, &j->gw, &j->gh, j->identity, j->plan));
    if (with_fill) {
        j->fill.reset(new TrackFill);
        SFA_TRY(fill_check(ctx, fn, p, fill, j->gw, j->gh, &j->fill->g));
        j->fill->fp = *fill;
    }
    if (with_alt) {
        j->alt.reset(new TrackAlt);
        SFA_TRY(alt_check(ctx, fn, p, alt, with_fill, j->gw, j->gh, j->alt.get()));
    }
    j->p = *p;
    j->p.energy.skip = j->p.fuse.skip = p->skip;
    track_layout(j->p, j->gw, j->gh, j->identity, j->plan[0].NN, with_fill ? &j->fill->fp : nullptr, with_fill ? &j->fill->g : nullptr,
                 with_alt ? &j->alt->ap : nullptr, &j->at);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(j->mem.alloc(ctx, j->at.total));
    SFA_TRY(zero_on(ctx, j->mem.p, j->at.total));                               // a run before an upload reads zeros, not another job's planes
    for (auto &e : j->ev) SFA_HIP(ctx, hipEventCreate(&e));
    if (with_fill) SFA_TRY(track_fill_create(j));
    guard.j = nullptr;
    *out = j;
    return SFA_OK;
}

int sfa_track_job_create(sfa_ctx *ctx, const sfa_track_params *p, sfa_track_job **out) { return track_create(ctx, __func__, p, nullptr, false, nullptr, false, out); }
int sfa_track_job_create_fill(sfa_ctx *ctx, const sfa_track_params *p, const sfa_track_fill_params *fill, sfa_track_job **out) {
    return track_create(ctx, __func__, p, fill, true, nullptr, false, out);
}

void sfa_track_job_destroy(sfa_track_job *job) {
    if (!job) return;
    if (job->ctx && job->ctx->stream) (void)hipStreamSynchronize(job->ctx->stream);
    for (auto &e : job->ev)
        if (e) (void)hipEventDestroy(e);
    delete job;                                                                 // a fill job's events go with its TrackFill
}

int sfa::track_range(sfa_ctx *ctx, const char *fn, const sfa_track_params &p, int s0, int ns, int r) {
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
    const TrackPlanes::Rate &a = job->at.rate[r];
    const bool identity = job->identity[r];
    const size_t tap = identity ? sizeof(float2) : sizeof(double2), seg = (size_t)s * rJ * pl;
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    float *stage = job->ptr(job->at.stage);
    SFA_TRY(upload_flow_pairs(ctx, src, identity, (size_t)rJ, fwd_u, fwd_v, p.w, p.h, stage, job->ptr(a.fw) + seg * tap, nullptr, nullptr));
    SFA_TRY(upload_flow_pairs(ctx, src, identity, (size_t)rJ, bwd_u, bwd_v, p.w, p.h, stage, job->ptr(a.bw) + seg * tap, nullptr, nullptr));
    if (p.use_occlusions) SFA_TRY(jet_decode_occlusions(ctx, src, (size_t)rJ, occ, p.w, p.h, job->ptr(job->at.occ_stage), job->ptr(a.mask) + seg));
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
    SFA_TRY(upload_frames(ctx, (size_t)p.Jets + 1, frames, stride, p.w, p.h, job->ptr(job->at.frames) + (size_t)s * (p.Jets + 1) * 3 * pl));
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
    const size_t tap = identity ? sizeof(float2) : sizeof(double2), seg = (size_t)rJ * pl;
    for (int dir = 0; dir < 2; dir++) {
        const float *from = dir ? bwd_dev : fwd_dev;
        char *dst = job->ptr(dir ? job->at.rate[r].bw : job->at.rate[r].fw) + (size_t)s0 * seg * tap;
        if (identity) {
            const size_t total = (size_t)ns * seg;
            hipLaunchKernelGGL(k_track_pack_flow, dim3(blocks_of(total)), dim3(kTrThreads), 0, ctx->stream, from, strides[0], strides[1], strides[2], strides[3],
                               strides[4], p.w, p.h, rJ, reinterpret_cast<float2 *>(dst), total);
            SFA_HIP(ctx, hipGetLastError());
            continue;
        }
        const size_t spl = (size_t)src.cw * src.ch, total = (size_t)rJ * spl;   // segment by segment through the one-segment stage, in stream order
        float *su = job->ptr(job->at.stage), *sv = su + total;
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
    unsigned char *stage = job->ptr(job->at.occ_stage), *mask = job->ptr(job->at.rate[r].mask) + (size_t)s0 * rJ * pl;
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
                       strides[4], p.w, p.h, p.Jets + 1, job->ptr(job->at.frames) + (size_t)s0 * (p.Jets + 1) * 3 * pl, total);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

// k_track_pack_frames reads element ((segment, frame), channel, row, column): with one frame and no more than three planes, segment and frame are 0 for every
// element, their strides are never multiplied by anything else, and the kernel packs the nc channel planes of one image
int sfa::pack_strided_planes(sfa_ctx *ctx, const float *src, long long s_c, long long s_row, long long s_col, int w, int h, int nc, float *out) {
    const size_t total = (size_t)nc * w * h;
    hipLaunchKernelGGL(k_track_pack_frames, dim3(blocks_of(total)), dim3(kTrThreads), 0, ctx->stream, src, 0ll, 0ll, s_c, s_row, s_col, w, h, 1, out, total);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

// ---- the stages of a run: each enqueues its part on the context's stream and records the event behind it ----------------------------------------------------
static int run_records(sfa_track_job *job, int ns) {
    TRACK_JOB(job);
    const TrackPlanes &at = job->at;
    energy_records_device(ctx, (size_t)ns * (p.Jets + 1), p.w, p.h, job->ptr(at.frames), job->ptr(at.der), job->ptr(at.rec));
    SFA_HIP(ctx, hipGetLastError());
    return mark(ctx, job->ev[kEvRecords]);
}

static int run_accumulation(sfa_track_job *job, int ns) {
    TRACK_JOB(job);
    for (int r = 0; r < p.K; r++) {
        const TrackPlanes::Rate &a = job->at.rate[r];
        SFA_TRY(accumulate_device(ctx, ns, p.r_Jets[r], p.w, p.h, job->gw, job->gh, p.skip, job->identity[r], job->ptr(a.fw), job->ptr(a.bw),
                                  p.use_occlusions ? job->ptr(a.mask) : nullptr, p.epsilon, p.discard, 1, job->ptr(a.acc_u), job->ptr(a.acc_v), job->ptr(a.tracked)));
    }
    return mark(ctx, job->ev[kEvAccumulated]);
}

EnergyWork sfa::energy_work(const sfa_track_job *job) {
    const TrackPlanes &at = job->at;
    return EnergyWork{job->ptr(at.wU), job->ptr(at.wV), job->ptr(at.wocc), job->ptr(at.jc), job->ptr(at.oc), job->ptr(at.ep)};
}

// The energies, occlusion words and adapted flows of one hypothesis of rate r -- the trajectories u, v [ns][r_Jets[r]][gpl] and tracked -- into slot `slot` of
// the fusion's planes: the rate's plan and weight, and rate min_fps_idx's flows
static int slot_energies(sfa_track_job *job, int ns, int r, Plane<double> u, Plane<double> v, Plane<int> tracked, size_t slot) {
    TRACK_JOB(job);
    const TrackPlanes &at = job->at;
    const TrackPlanes::Rate &mf = at.rate[p.min_fps_idx];
    const size_t S = job->slots(), J = p.Jets;
    const bool flows = r >= p.min_fps_idx;                                      // a rate before acc_min_fps sees empty flow Mats (:786, :1148-1151)
    return energies_device(ctx, job->plan[r], ns, job->ptr(u), job->ptr(v), job->ptr(tracked), job->ptr(at.rec), job->identity[p.min_fps_idx],
                           flows ? job->ptr(mf.fw) : nullptr, flows ? job->ptr(mf.bw) : nullptr, energy_work(job), job->ptr(at.E) + slot * gpl,
                           job->ptr(at.O) + slot * gpl, S * gpl, p.do_fuse ? job->ptr(at.aU) + slot * J * gpl : nullptr,
                           p.do_fuse ? job->ptr(at.aV) + slot * J * gpl : nullptr, S * J * gpl);
}

// segment s's slot of a hypothesis that does not exist: energy +Inf, occlusion word 0, adapted flows 0
static int empty_slot(sfa_track_job *job, int s, size_t slot) {
    TRACK_JOB(job);
    const TrackPlanes &at = job->at;
    const size_t J = p.Jets, o = ((size_t)s * job->slots() + slot) * gpl;
    SFA_TRY(copy_on(ctx, job->ptr(at.E) + o, job->ptr(at.inf), gpl * sizeof(double), hipMemcpyDeviceToDevice));
    SFA_TRY(zero_on(ctx, job->ptr(at.O) + o, gpl * sizeof(unsigned long long)));
    if (!p.do_fuse) return SFA_OK;
    SFA_TRY(zero_on(ctx, job->ptr(at.aU) + o * J, J * gpl * sizeof(double)));
    return zero_on(ctx, job->ptr(at.aV) + o * J, J * gpl * sizeof(double));
}

// rate r's accumulated hypothesis is slot r * step; on a fill job its fill-in is the next, emptied for the segments the last fill-in left unfilled
static int run_energies(sfa_track_job *job, int ns) {
    const sfa_track_params &p = job->p;
    for (int r = 0; r < p.K; r++) {
        const TrackPlanes::Rate &a = job->at.rate[r];
        const TrackPlanes::Fill &f = job->at.fill[r];
        const size_t slot = (size_t)r * job->step();
        SFA_TRY(slot_energies(job, ns, r, a.acc_u, a.acc_v, a.tracked, slot));
        if (!job->fill) continue;
        SFA_TRY(slot_energies(job, ns, r, f.u, f.v, f.tracked, slot + 1));
        for (int s = 0; s < ns; s++)
            if (!job->fill->stats[((size_t)r * p.n + s) * 3 + 2]) SFA_TRY(empty_slot(job, s, slot + 1));
    }
    return SFA_OK;
}

static int run_best(sfa_track_job *job, int ns) {
    TRACK_JOB(job);
    const TrackPlanes &at = job->at;
    hipLaunchKernelGGL(k_track_best, dim3(blocks_of(gpl), (unsigned)ns), dim3(kTrThreads), 0, ctx->stream, job->ptr(at.E), job->ptr(at.O), p.K, job->slots(), job->step(),
                       (int)gpl, p.n, job->ptr(at.best), job->ptr(at.occluded));
    SFA_HIP(ctx, hipGetLastError());
    return mark(ctx, job->ev[kEvBest]);
}

// computeSmoothnessWeight of every segment's normalised frame 0 (sfa_dt_smoothness_weight's kernel) on the packed planes
static int run_weight(sfa_track_job *job, int ns) {
    TRACK_JOB(job);
    Geo g{p.w, p.h, p.w, (long)pl, (long)pl, ns, WMask::first(ns), nullptr};
    launch_dpsis(ctx, g, job->ptr(job->at.weight), job->ptr(job->at.frames), (long)((size_t)(p.Jets + 1) * 3 * pl), p.coef, p.avg, p.std_dev, p.hbit);
    SFA_HIP(ctx, hipGetLastError());
    return mark(ctx, job->ev[kEvWeight]);
}

FuseWork sfa::fuse_work(const sfa_track_job *job) {
    const TrackPlanes &at = job->at;
    FuseWork f;
    f.U = job->ptr(at.aU); f.V = job->ptr(at.aV); f.energy = job->ptr(at.E); f.occ = job->ptr(at.O); f.weight = job->ptr(at.weight);
    f.nl = job->ptr(at.nl); f.lab = job->ptr(at.lab); f.theta = job->ptr(at.theta); f.P = job->ptr(at.P);
    f.M = job->ptr(at.M); f.xcur = job->ptr(at.xcur); f.xbest = job->ptr(at.xbest);
    f.slot = job->ptr(at.slot); f.fu = job->ptr(at.fu); f.fv = job->ptr(at.fv); f.out_occ = job->ptr(at.out_occ);
    f.seg_energy = job->ptr(at.seg_energy); f.seg_bound = job->ptr(at.seg_bound); f.seg_iters = job->ptr(at.seg_iters);
    return f;
}

// labels -> pairwise -> TRW-S -> output; fuse_device records kEvFuse .. kEvFuseEnd around the four
static int run_fusion(sfa_track_job *job, int ns) {
    TRACK_JOB(job);
    return fuse_device(ctx, &p.fuse, ns, job->slots(), p.Jets, p.w, p.h, job->gw, job->gh, fuse_work(job), job->ev + kEvFuse);
}

int sfa_track_job_run(sfa_track_job *job, int ns) {
    TRACK_JOB(job);
    if (ns < 1 || ns > p.n) REFUSE("%s: ns = %d (1 <= ns <= n = %d, the job's start_jets)", __func__, ns, p.n);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(mark(ctx, job->ev[kEvStart]));
    SFA_TRY(run_records(job, ns));
    SFA_TRY(run_accumulation(job, ns));
    if (job->fill) SFA_TRY(track_run_fill(job, ns));
    SFA_TRY(run_energies(job, ns));
    SFA_TRY(run_best(job, ns));
    job->timed = true;
    job->timed_fuse = false;
    if (!p.do_fuse) return SFA_OK;
    SFA_TRY(run_weight(job, ns));
    SFA_TRY(job->alt ? track_run_alternation(job, ns) : run_fusion(job, ns));   // a job that alternates fuses once per round
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
    SFA_TRY(download(ctx, acc_u_last, job->ptr(a.acc_u) + last, gpl * 8));
    SFA_TRY(download(ctx, acc_v_last, job->ptr(a.acc_v) + last, gpl * 8));
    SFA_TRY(download(ctx, tracked, job->ptr(a.tracked) + (size_t)s * gpl, gpl * 4));
    SFA_TRY(download(ctx, energy, job->ptr(job->at.E) + sk, gpl * 8));
    SFA_TRY(download(ctx, occ_bits, job->ptr(job->at.O) + sk, gpl * 8));
    SFA_TRY(download(ctx, occluded, job->ptr(job->at.occluded) + ((size_t)r * p.n + s) * gpl, gpl));
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
    SFA_TRY(download(ctx, slot, job->ptr(at.slot) + o, gpl * 4));
    SFA_TRY(download(ctx, flow_u, job->ptr(at.fu) + o, gpl * 8));
    SFA_TRY(download(ctx, flow_v, job->ptr(at.fv) + o, gpl * 8));
    SFA_TRY(download(ctx, occ, job->ptr(at.out_occ) + o, gpl));
    SFA_TRY(download(ctx, best, job->ptr(at.best) + o, gpl));
    SFA_TRY(download(ctx, energy, job->ptr(at.seg_energy) + s, 8));
    SFA_TRY(download(ctx, bound, job->ptr(at.seg_bound) + s, 8));
    SFA_TRY(download(ctx, iters, job->ptr(at.seg_iters) + s, 4));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

int sfa_track_job_download_best(sfa_track_job *job, int s, unsigned char *best) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, 0));
    if (!best) REFUSE("%s: best is null", __func__);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(download(ctx, best, job->ptr(job->at.best) + (size_t)s * gpl, gpl));
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
    hipLaunchKernelGGL(k_track_unpack, dim3(blocks_of(gpl), (unsigned)ns), dim3(kTrThreads), 0, ctx->stream, job->ptr(at.fu) + o, job->ptr(at.fv) + o,
                       job->ptr(at.slot) + o, job->ptr(at.out_occ) + o, job->ptr(at.seg_energy) + s0, job->ptr(at.seg_bound) + s0, job->ptr(at.seg_iters) + s0, job->gw,
                       (int)gpl, flow_dev, strides[0], strides[1], strides[2], strides[3], slot_dev, occ_dev, stats_dev);
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
    const unsigned char *from = best ? job->ptr(at.best) + (size_t)s0 * gpl : job->ptr(at.occluded) + ((size_t)r * p.n + s0) * gpl;
    const long long none[4] = {0, 0, 0, 0}, *st = acc_dev ? strides : none;
    hipLaunchKernelGGL(k_track_unpack_rate, dim3(blocks_of(gpl), (unsigned)ns), dim3(kTrThreads), 0, ctx->stream, job->ptr(a.acc_u) + last, job->ptr(a.acc_v) + last,
                       rJ * gpl, job->ptr(a.tracked) + (size_t)s0 * gpl, gpl, job->ptr(at.E) + sk, job->ptr(at.O) + sk, (size_t)job->slots() * gpl, from, gpl, job->gw,
                       (int)gpl, acc_dev, st[0], st[1], st[2], st[3], tracked_dev, energy_dev, occ_bits_dev, bytes_dev);
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
    const hipEvent_t *e = job->ev;
    const hipEvent_t span[8][2] = {
        {e[kEvStart], e[kEvRecords]},                                           // derivatives and records
        {e[kEvRecords], e[kEvAccumulated]},                                     // accumulation
        {job->fill ? job->fill->ev_energy : e[kEvAccumulated], e[kEvBest]},     // energies, best / occluded: on a fill job from where its fill-in ends
        {e[kEvBest], e[kEvWeight]},                                             // the weight kernel alone, without the fusion's clears behind it
        {e[kEvFuse], e[kEvFuse + 1]}, {e[kEvFuse + 1], e[kEvFuse + 2]}, {e[kEvFuse + 2], e[kEvFuse + 3]}, {e[kEvFuse + 3], e[kEvFuseEnd]},
    };
    for (int i = 0; i < 8; i++) ms[i] = 0;
    const int last = job->timed_fuse ? 8 : 3;
    for (int i = 0; i < last; i++) SFA_HIP(ctx, hipEventElapsedTime(&ms[i], span[i][0], span[i][1]));
    return SFA_OK;
}

#pragma clang attribute pop
