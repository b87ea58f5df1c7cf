// sfa_internal.h -- internal declarations of libslowflow_amd (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/slowflow_amd.h"
#include "dev_view.h"

#pragma clang fp contract(off)   // the reference is strict fp32 without FMA contraction (CMakeLists.txt:6)

namespace sfa {

// Windows a lockstep job can hold.  Which of them take part in a launch is a bit set of kMaskWords 64-bit words (WMask): what the host knows (Geo::active) AND what the
// device knows (the windows that have not met the outer threshold yet: sfa_ctx::d_amask, Geo::amask).  Round 5 widened the set from one word to two.
constexpr int kMaskWords = 2;
constexpr int kMaxBatch = 64 * kMaskWords;
struct WMask {
    unsigned long long w[kMaskWords];
    __host__ __device__ bool test(int b) const { return (w[b >> 6] >> (b & 63)) & 1ull; }
    __host__ __device__ void clear(int b) { w[b >> 6] &= ~(1ull << (b & 63)); }
    __host__ __device__ void set(int b) { w[b >> 6] |= 1ull << (b & 63); }
    __host__ __device__ bool any() const { unsigned long long o = 0; for (int i = 0; i < kMaskWords; i++) o |= w[i]; return o != 0; }
    __host__ __device__ bool operator==(const WMask &o) const { bool e = true; for (int i = 0; i < kMaskWords; i++) e = e && w[i] == o.w[i]; return e; }
    __host__ __device__ bool operator!=(const WMask &o) const { return !(*this == o); }
    __host__ __device__ WMask operator&(const WMask &o) const { WMask r; for (int i = 0; i < kMaskWords; i++) r.w[i] = w[i] & o.w[i]; return r; }
    __host__ __device__ WMask andnot(const WMask &o) const { WMask r; for (int i = 0; i < kMaskWords; i++) r.w[i] = w[i] & ~o.w[i]; return r; }
    int count() const { int n = 0; for (int i = 0; i < kMaskWords; i++) n += __builtin_popcountll(w[i]); return n; }
    static WMask none() { WMask r; for (int i = 0; i < kMaskWords; i++) r.w[i] = 0; return r; }
    static WMask first(int nb) {                                   // windows 0 .. nb - 1
        WMask r;
        for (int i = 0; i < kMaskWords; i++) r.w[i] = nb >= 64 * (i + 1) ? ~0ull : nb <= 64 * i ? 0ull : (1ull << (nb - 64 * i)) - 1;
        return r;
    }
    static WMask one(int b) { WMask r = none(); r.w[b >> 6] = 1ull << (b & 63); return r; }
};
constexpr int kMaxTerms = 4 * SFA_MAX_REF;
// What ctx->d_last holds (ONE definition for job.hip and kernels.hip -- ADVICE r5: the layout was repeated by hand in four places): the norms of every window's
// last outer iteration, the windows' finished-block counters of k_update_outer_x, the windows k_outer_threshold could not decide, the exact norms of
// launch_exact_norms.  The pinned mirror ctx->h_red is at least this large (the exact norms are read back into ITS `exact` member, never into pageable memory).
struct LastBlock {
    double last[2 * kMaxBatch];
    unsigned done[kMaxBatch];
    unsigned long long unsure[kMaskWords];
    float exact[2 * kMaxBatch];
};
// How close to a break threshold (relative) the fp64 tree sum of a change norm may come before the decision is taken on the reference's own fp32 running sum
// (k_exact_break / launch_exact_norms).  The reference adds ceil(w / 4) * h block sums to ONE fp32 accumulator (variational_mt.cpp:412-425); each addition rounds
// by at most 2^-24 of the running sum, and the errors need not cancel -- block sums below half an ulp of the accumulator (a converged background behind a few
// moving pixels) are dropped one after the other, always downwards -- so the two sums can differ by up to blocks * 2^-24 of their value: 6.7e-3 at 1024 x 436,
// 6.3e-2 at 2048 x 2048.  Outside that band both decide alike by construction; inside it the reference's arithmetic is repeated.  (Rounds 4-5 used a constant
// 1e-3, the size of the typical difference, not of the bound: ADVICE r5.)
__host__ __device__ inline double break_band(int w, int h) {
    const double bound = (double)((w + 3) / 4) * (double)h * (1.0 / 16777216.0);
    return bound > 1e-3 ? bound : 1e-3;
}

// device-side outer break (job.hip: struct OuterBreak): the host reads the mask of kMaskLag iterations ago from a ring of kMaskRing pinned words
constexpr int kMaskLag = 2, kMaskRing = 4;
static_assert(kMaskLag < kMaskRing, "a ring slot is rewritten kMaskRing iterations after it was read kMaskLag iterations late");

// ---------------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------------
struct DevBlock { void *p; size_t bytes; };

}  // namespace sfa

struct sfa_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // scratch for reductions / flags
    double *d_red = nullptr;      // device, kRedDoubles doubles
    double *h_red = nullptr;      // pinned host mirror
    // thresholds on the device (variational_mt.cpp:436): the windows still iterating, the norms of each window's last iteration, and a ring of pinned
    // copies of the mask (one per outer iteration in flight) with the events that say a copy has landed
    unsigned long long *d_amask = nullptr;         // kMaskWords words
    sfa::LastBlock *d_last = nullptr;              // norms of each window's last iteration + the small device-side state of the break decisions (sfa::LastBlock)
    sfa::WMask *h_amask = nullptr;                      // kMaskRing pinned masks
    hipEvent_t ev_mask[sfa::kMaskRing] = {};
    unsigned *d_err = nullptr;    // device error/timeout word
    // profiling of the SOR solve kernel
    bool profile = false;
    std::vector<hipEvent_t> ev;   // pairs
    size_t ev_used = 0;
    double sor_bytes = 0;         // algorithmic bytes of the bracketed launches
    std::vector<hipEvent_t> ev2;  // pairs around the data-term assembly kernel (k_assemble_images)
    size_t ev2_used = 0;
    double asm_pixel_terms = 0;   // pixels x data terms of the bracketed assembly launches
    char sor_kernel[160] = {0};   // the solver kernel (shape) of the last solve launched
    void *rb_tmp = nullptr;       // labelled red-black mode: scratch (du, dv) pair the tile visits ping-pong with, grown on demand
    size_t rb_tmp_bytes = 0;
    void *q_tmp = nullptr;        // sfa_flow_magnitude_quantiles_device (quantile.hip): group records, histograms and keys, kept from call to call, grown on demand
    size_t q_tmp_bytes = 0;
    float epic_ms[5] = {};        // sfa_epic_nearest_seeds_batch (epic_nn.hip): the last call's kernel time by group (sfa_epic_nn_stage_ms)
    int epic_search = 0;          // sfa_ctx_set_epic_search: SFA_EPIC_SEARCH_DENSE (the default) or SFA_EPIC_SEARCH_COMPACT (epic_nn.hip, epic_nn_plan.h)
    long long epic_info[4] = {};  // sfa_epic_nn_search_info: slices, images searched dense, images searched sparse, the largest slice workspace of the last stage
    float epic_fit_ms[2] = {};    // sfa_epic_interpolate_batch (epic_fit.hip): the last call's fit and apply kernel time (sfa_epic_fit_stage_ms)
    float epic_batch_ms[8] = {};  // sfa_epic_batch (epic_batch.hip): the last call's kernel time by stage (sfa_epic_batch_stage_ms)
    int epic_chain_runs[2] = {};  // the last chain's sub-batches: those that ran to their end, those that were cut short and run again with fewer images
    hipEvent_t t0 = nullptr, t1 = nullptr;
    hipEvent_t ev_wait = nullptr, ev_signal = nullptr;   // sfa_ctx_wait_stream / sfa_ctx_signal_stream: recorded on the caller's / the context's stream
    // the reference's per-iteration "avg change" lines (variational_mt.cpp:404-405, 431-432): sfa_ctx_set_verbose; costs a host round trip per iteration
    bool verbose_changes = false;
    // default-ctx bookkeeping
    int cu_count = 256;
};

namespace sfa {

constexpr int kRedDoubles = 1 << 20;   // 2*kMaxBatch result words + per-block partials: 2 x windows x ceil(w / 64) x 16 row blocks (sfa_job_create checks the size)

int set_error(sfa_ctx *ctx, int code, const char *fmt, ...);
extern thread_local std::string g_thread_err;

// ---------------------------------------------------------------------------------------------------
// Cross-check and what-if paths of the library (the unfused pipeline, other solver shapes, the cut's knobs ...).  ONE record per process, filled once: from the
// environment ONLY when SFA_DEBUG=1 is set at the first sfa_ctx_create -- without it no variable of a caller's environment can change which kernels the drop-in
// library runs --, afterwards only through the test hook sfa_debug_set() (include/slowflow_amd.h).  api.hip holds the table of names.
// ---------------------------------------------------------------------------------------------------
struct Switches {
    enum Id {
        SOR_CHAIN, SOR_BAND, SOR_F, SOR_CH, SOR_LEAD, CHAIN_LDS, RB_TILE, WARP_ALLJ, NO_WARP_SMOOTH, ASSEMBLE_GENERIC, EXACT_DIV, ASM_XCD, NO_DIRECT_OPERANDS,
        NO_UV_ALIAS, DEBUG_ACTIVE, UNFUSED, SHARE_SOR, PYRAMID_UNFUSED, CUT_DISCHARGE, CUT_INNER, CUT_SUPER, CUT_TAIL_INNER, CUT_PER, CUT_TAIL_PER, CUT_TAIL_SUPER,
        CUT_DEBUG, CUT_NO_TAIL, CUT_TAIL, NO_EXACT_BREAK, PAIR_UNFUSED, EPIC_FIT_PLAIN, EPIC_NN_SET, EPIC_NN_SLICE, N
    };
    bool given[N] = {};
    int value[N] = {};
};
// code of the full build only
#ifdef SFA_RELEASE
#define SFA_FULL(...)
#else
#define SFA_FULL(...) __VA_ARGS__
#endif
#ifdef SFA_RELEASE
// RELEASE BUILD (make -C slowflow_amd/csrc release -> build_release/libslowflow_amd.so): no switch exists -- every cross-check / what-if branch
// is dead code the compiler removes, the environment is never read (not even behind SFA_DEBUG=1), sfa_debug_set refuses by name, and only the solver shapes the
// library picks by default are compiled (sor_chain.hip: 2,2,2,2,2,2,3 / 1 x 5 with either lag pair; sor.hip: the task kernel as the one fallback for sweep counts
// no chain shape divides).  Same C-ABI, same results as the full build's defaults; the tests run the full build.
constexpr bool sw_given(Switches::Id) { return false; }
constexpr int sw_int(Switches::Id, int dflt) { return dflt; }
#else
extern Switches g_switches;
inline bool sw_given(Switches::Id i) { return g_switches.given[i]; }                                   // what `getenv(name) != nullptr` used to say
inline int sw_int(Switches::Id i, int dflt) { return g_switches.given[i] ? g_switches.value[i] : dflt; }   // `getenv(name) ? atoi(getenv(name)) : dflt`
#endif

#define SFA_HIP(ctx, call)                                                                         \
    do {                                                                                           \
        hipError_t _e = (call);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return sfa::set_error((ctx), SFA_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

#define SFA_TRY(expr)            \
    do {                         \
        int _rc = (expr);        \
        if (_rc != SFA_OK) return _rc; \
    } while (0)

// argument checks of the entry points: refuse with "<function>: <msg>" on the context `ctx` of the scope (a helper names its caller in `fn`)
#define CHECK_ARGS_FN(fn, cond, msg) do { if (!(cond)) return sfa::set_error(ctx, SFA_ERR_ARG, "%s: %s", fn, msg); } while (0)
#define CHECK_ARGS(cond, msg) CHECK_ARGS_FN(__func__, cond, msg)
// the same with a message of the caller's own making (the device seam, the mosaic entry points: a refusal names the argument)
#define REFUSE(...) return sfa::set_error(ctx, SFA_ERR_ARG, __VA_ARGS__)

inline int round_up(int a, int m) { return (a + m - 1) / m * m; }
inline int host_stride(int w) { return ((w + 3) / 4) * 4; }     // image.c:25
#ifndef SFA_PITCH_ODD
#define SFA_PITCH_ODD 0
#endif
// device rows are 256-B aligned.  SFA_PITCH_ODD (what-if, round 6): an ODD number of 256-byte units per row, so that the rows of a tile and the planes of an image set
// (a whole number of rows apart) do not all fall on addresses that agree modulo 4 KB (1024-column frames: rows 4 096 bytes apart)
inline int dev_pitch(int w) { const int p = round_up(w, 64); return (SFA_PITCH_ODD && ((p / 64) & 1) == 0) ? p + 64 : p; }

// RAII device allocation
struct DevMem {
    void *p = nullptr;
    size_t bytes = 0;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { release(); }
    int alloc(sfa_ctx *ctx, size_t n);
    void release();
    float *f() const { return static_cast<float *>(p); }
};

// host <-> device plane copies (valid columns only unless full_stride)
int upload_plane(sfa_ctx *ctx, float *dev, int pitch, const float *host, int stride, int w, int h);
int download_plane(sfa_ctx *ctx, float *host, int stride, const float *dev, int pitch, int w, int h);

// jets of another size than the tracking frames (jet_resample.hip).  All three enqueue on the context's stream and return without waiting.
// *identity: no crop, the target's size, rescale 1 -- such a source is not resampled by accumulate.hip and energy.hip.  fn names the entry point.
int jet_source_check(sfa_ctx *ctx, const char *fn, const sfa_jet_source *src, int w, int h, bool *identity);
// np fields u[k], v[k] -> out: np double2 planes of w x h (.x = u, .y = v).  stage: 2 * np * cw * ch floats, free again once the stream has passed.
// before, after: null, or events recorded around the kernel (after the uploads)
int jet_resample_flows(sfa_ctx *ctx, const sfa_jet_source &src, size_t np, const float *const *u, const float *const *v, int w, int h, float *stage, double2 *out,
                       hipEvent_t before, hipEvent_t after);
// np raw occlusion images -> out: np packed w x h masks (0 = occluded).  stage: np * sw * sh bytes
int jet_decode_occlusions(sfa_ctx *ctx, const sfa_jet_source &src, size_t np, const unsigned char *const *occ, int w, int h, unsigned char *stage, unsigned char *out);
// jet_resample_flows' kernel alone: su, sv are np packed cw x ch planes already in device memory
int launch_jet_resample(sfa_ctx *ctx, const sfa_jet_source &src, size_t np, const float *su, const float *sv, int w, int h, double2 *out);
// jet_decode_occlusions' kernel alone: stage holds np packed sw x sh images already in device memory
int launch_jet_occ_decode(sfa_ctx *ctx, const sfa_jet_source &src, size_t np, const unsigned char *stage, int w, int h, unsigned char *out);

// ---- stage_io.hip: the host side of dense_tracking's stages, shared by the sfa_* stage wrappers and the track job.  Everything enqueues on the context's
// stream and returns without waiting --------------------------------------------------------------------------------------------------------------------
// n float planes u, v -> n float2 planes (total n elements)
void launch_interleave(sfa_ctx *ctx, const float *u, const float *v, float2 *out, size_t n);
#pragma GCC visibility push(hidden)   // nothing from here to the pop is part of the library's interface
// one-line forms of the stream calls; download: a result to the host, or nothing where the caller passes no dst
int copy_on(sfa_ctx *ctx, void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
int zero_on(sfa_ctx *ctx, void *dst, size_t bytes);
int mark(sfa_ctx *ctx, hipEvent_t e);
int download(sfa_ctx *ctx, void *dst, const void *src, size_t bytes);
// h rows of `row` bytes, the rows dpitch and spitch bytes apart
int copy_rows_on(sfa_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t row, size_t h, hipMemcpyKind kind);
// event i of a device-level function's `ev`, where the caller gave events
inline int mark_if(sfa_ctx *ctx, hipEvent_t *ev, int i) { return ev ? mark(ctx, ev[i]) : (int)SFA_OK; }
// nf host frames [3][h][stride] -> dst: [nf][3][h][w] packed; np host byte planes [h][stride] (decoded masks, raw occlusion images) -> dst: [np][h][w] packed
int upload_frames(sfa_ctx *ctx, size_t nf, const float *const *frames, int stride, int w, int h, float *dst);
int upload_masks(sfa_ctx *ctx, size_t np, const unsigned char *const *masks, int stride, int w, int h, unsigned char *dst);
// np host fields u[k], v[k] of one direction, as src describes them -> np planes of pairs at dst.  identity: the valid columns packed into stage (u, then v
// np * w * h floats further) and interleaved to float2; else jet_resample_flows to double2, stage and events as there
int upload_flow_pairs(sfa_ctx *ctx, const sfa_jet_source &src, bool identity, size_t np, const float *const *u, const float *const *v, int w, int h, float *stage,
                      void *dst, hipEvent_t before, hipEvent_t after);
// up to six events around a stage's kernels, made only where the caller asks for the times (e[i] stays null otherwise); read: ms[i] = e[i] to e[i + 1]
struct StageEvents {
    hipEvent_t e[6] = {};
    int make(sfa_ctx *ctx, int n) {
        for (int i = 0; i < n; i++) SFA_HIP(ctx, hipEventCreate(&e[i]));
        return SFA_OK;
    }
    int mark(sfa_ctx *ctx, int i) { return e[i] ? sfa::mark(ctx, e[i]) : (int)SFA_OK; }   // where made
    int read(sfa_ctx *ctx, int n, float *ms) {
        for (int i = 0; i + 1 < n; i++) SFA_HIP(ctx, hipEventElapsedTime(&ms[i], e[i], e[i + 1]));
        return SFA_OK;
    }
    ~StageEvents() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};
#pragma GCC visibility pop

// ---- dense_tracking's three stages at device level (accumulate.hip, energy.hip, fuse.hip): device pointers and a caller-owned workspace in, launches on the
// context's stream out; no allocation, no copy, no wait.  The sfa_* entry points wrap them (allocate, upload through stage_io.hip, call, download, wait), the
// track job (track.hip, track_fill.hip, track_alt.hip) chains them -------------------------------------------------------------------------------------------
// k_accumulate over n segments of FF steps.  fwd, bwd: [n][FF] planes of float2 (identity) or double2; masks: [n][FF] decoded masks or null;
// acc_u, acc_v: [n][S][gpl], S = FF (all_steps) or 1; tracked: [n][gpl]
int accumulate_device(sfa_ctx *ctx, int n, int FF, int w, int h, int gw, int gh, int skip, bool identity, const void *fwd, const void *bwd,
                      const unsigned char *masks, double epsilon, int discard, int all_steps, double *acc_u, double *acc_v, int *tracked);
// What the energy kernels of one (r_Jets, Jets) need besides their planes: adaptFPS's index table, the keys in the kernels' types, the grid and addBCGC's window
struct AdaptTab {
    int off[32], offm1[32];              // kEnMaxJets entries
    float skip;                          // (1.0f * F) / nF, a float
    int up;                              // skip >= 1
};
struct EnergyArgs {
    double acc_jc, acc_cv, acc_bc, acc_gc, acc_occ, acc_temporal_occ;   // the parameters' double types in addJC / addBCGC / addOC
    float thr, fb_thr;                   // setOcclusions' float thresholds
    int penalty;                         // 0 quadratic, 1 modified L1, else Lorentzian (:665-675)
    double eps_sq;                       // (double)(e * e), e the float the penalty's constructor takes
    float weight;                        // weight_jet_estimation[r], a float (:489)
};
struct EnergyPlan { AdaptTab tab; EnergyArgs a; int rJ, J, w, h, gw, gh, incr, start, r, NN; size_t lds; };
// the grid and adaptFPS's indices, each checked against the r_Jets flows it reads; refuses as sfa_hypothesis_energies does
int energy_plan(sfa_ctx *ctx, const sfa_energy_params *p, int r_Jets, int Jets, int w, int h, EnergyPlan *out);
// nf frames [nf][3][pl] packed fp32 -> dx, dy (der: 6 nf pl floats of scratch) -> rec: [nf][pl] records of 48 bytes
void energy_records_device(sfa_ctx *ctx, size_t nf, int w, int h, const float *frames, float *der, void *rec);
// the scratch of energies_device for n segments: U, V [n][gpl][J], occ [n][gpl], jc, oc [n][gpl], ep [n][gpl][NN]
struct EnergyWork { double *U, *V; unsigned long long *occ; float *jc, *oc; double *ep; };
// k_hyp_serial, k_hyp_bcgc, k_hyp_sum (and k_hyp_adapted where adapted_u is given) over n segments.  acc_u, acc_v: [n][r_Jets][gpl]; tracked: [n][gpl]; rec:
// [n][J + 1][pl] records; fwd, bwd: [n][J] planes of float2 (identity) / double2, or null.  Segment s's energy and occlusion word go to energy / occ_out +
// s * out_seg, its adapted flows [J][gpl] to adapted_u / adapted_v + s * adapted_seg (elements): the fusion's [n][K][gpl] and [n][K][J][gpl] take slot k at
// base + k * gpl (k * J * gpl) with out_seg = K * gpl (adapted_seg = K * J * gpl)
int energies_device(sfa_ctx *ctx, const EnergyPlan &pl, int n, const double *acc_u, const double *acc_v, const int *tracked, const void *rec, bool identity,
                    const void *fwd, const void *bwd, const EnergyWork &wk, double *energy, unsigned long long *occ_out, size_t out_seg, double *adapted_u,
                    double *adapted_v, size_t adapted_seg);
// energies_device's last launch alone (k_hyp_adapted), for a caller that provides the adapted planes after the other kernels are enqueued
int energies_adapted_device(sfa_ctx *ctx, const EnergyPlan &pl, int n, const int *tracked, const EnergyWork &wk, double *adapted_u, double *adapted_v, size_t adapted_seg);
#pragma GCC visibility push(hidden)
// What the energy kernels read, for the entry points that bring it from the host (sfa_hypothesis_energies*, sfa_rescore_proposals; the track job keeps
// the same planes in its own allocation): n segments' frames [n][J + 1][3][pl], derivatives and records, both directions' [n][J] planes of pairs with
// their stage where flow_src is given (null: no flows; is_identity: what jet_source_check said of it), and energies_device's scratch for work_n segments
struct EnergyMem {
    DevMem frames, der, rec, fwd, bwd, stage, U, V, occ, jc, oc, ep;            // fwd.p, bwd.p stay null without flows: what energies_device takes then
    int segments = 0; bool flows = false, identity = true; sfa_jet_source src{};   // as alloc was called
    int alloc(sfa_ctx *ctx, const EnergyPlan &e, int n, int work_n, const sfa_jet_source *flow_src, bool is_identity);
    // the frames at `stride`, energy_records_device, and the four flow arrays where alloc had a flow_src (their planes are allocated here); does not wait
    int upload(sfa_ctx *ctx, const EnergyPlan &e, const float *const *host_frames, int stride, const float *const *fwd_u, const float *const *fwd_v,
               const float *const *bwd_u, const float *const *bwd_v);
    EnergyWork work() const { return EnergyWork{static_cast<double *>(U.p), static_cast<double *>(V.p), static_cast<unsigned long long *>(occ.p), jc.f(), oc.f(), static_cast<double *>(ep.p)}; }
};
// What the two refuse alike in the caller's name: flow arrays given in part, a null frame among the nf or a null flow plane among the nj (with_index: the
// text names the plane's index).  *flows: the arrays are given
int energy_planes_check(sfa_ctx *ctx, const char *fn, bool with_index, size_t nf, const float *const *frames, size_t nj, const float *const *fwd_u,
                        const float *const *fwd_v, const float *const *bwd_u, const float *const *bwd_v, bool *flows);
#pragma GCC visibility pop
// The fusion's planes for n segments: inputs U, V [n][K][J][gpl], energy, occ [n][K][gpl], weight [n][h][w]; scratch nl [n][gpl], lab [n][gpl][16], theta
// [n][gpl][16], P [n][2][gpl][K K], M [n][gpl][4][16], xcur, xbest [n][gpl]; outputs slot, fu, fv, out_occ [n][gpl], seg_energy, seg_bound, seg_iters [n]
struct FuseWork {
    const double *U, *V, *energy; const unsigned long long *occ; const float *weight;
    unsigned char *nl, *lab; double *theta, *P, *M; unsigned char *xcur, *xbest;
    int *slot; double *fu, *fv; unsigned char *out_occ; double *seg_energy, *seg_bound; int *seg_iters;
};
// zeroes the messages and labellings of the n segments, then k_fuse_labels, k_fuse_pairwise, k_trws, k_fuse_output.  ev: null or 5 events recorded around the four
int fuse_device(sfa_ctx *ctx, const sfa_fuse_params *p, int n, int K, int Jets, int w, int h, int gw, int gh, const FuseWork &f, hipEvent_t *ev);

// ---- the alternation's steps at device level (neigh.hip), in the same form.  A list plane set: U, V [n][16][J][gpl], energy, occ, origin [n][16][gpl]
struct NeighPlanes { double *U, *V, *energy; unsigned long long *occ; unsigned char *origin; };
// scratch: flags, srcpos [n][gpl], total [n][2], map [n][16][gpl]
struct NeighWork { unsigned char *flags, *srcpos; int *total; int *map; };
// what the proposals' entry point and a job refuse alike, by the key's name
int neigh_check(sfa_ctx *ctx, const char *fn, const sfa_neigh_params *p, int gw, int gh, int round);
// k_neigh_prune, k_neigh_gather: in -> out by sel [n][gpl]; map: [n][16][gpl] scratch.  ev: null, or 3 (the proposals: 4) events recorded around the kernels
int neigh_prune_device(sfa_ctx *ctx, int n, int Jets, int gw, int gh, int keep, const int *sel, const NeighPlanes &in, const NeighPlanes &out, int *map,
                       hipEvent_t *ev);
// k_neigh_flags, k_neigh_propose, k_neigh_gather: in -> out; wk.map is left as the propose kernel wrote it (bit 30: accepted in this call)
int neigh_propose_device(sfa_ctx *ctx, const sfa_neigh_params *p, int n, int Jets, int gw, int gh, int round, const unsigned *seq_start,
                         const unsigned char *consistent, const NeighPlanes &in, const NeighPlanes &out, const NeighWork &wk,
                         hipEvent_t *ev);

// the weight a proposal's energy ends with, by the slot it was born in
struct NeighWeights { float w[16]; };
// The accepted proposals of a round scored at their new place: per segment and position of todo [n][16] (host), energies_device on the list's flow planes
// (plan: r_Jets = Jets, weight 0; tracked [n][16][gpl]: Jets where the position was filled in this round) into E, O [gpl], then k_neigh_rescored into the
// list's energy and occ.  rec: [n][J + 1][pl] records; fwd, bwd: [n][J] planes of pairs or null; wk: the scratch of ONE segment
int neigh_rescore_device(sfa_ctx *ctx, const EnergyPlan &plan, int n, const int *tracked, const unsigned char *todo, const void *rec, bool identity, const void *fwd,
                         const void *bwd, const EnergyWork &wk, double *E, unsigned long long *O, const NeighWeights &wt, const NeighPlanes &lists);

// ---- the steps around dense_tracking's EpicFlow fill-in at device level (fill.hip), in the same form: device pointers in, launches on the context's
// stream out; no allocation, no copy, no wait.  The sfa_consistent_regions / sfa_fill_matches / sfa_fill_trajectories entry points wrap them -------------
// tracked: [n][h][w], full: [n] (device); scratch T, P, S: [n][h][w] ints each; mask: [n][h][w] bytes, kept: [n]
int consistent_regions_device(sfa_ctx *ctx, int n, int w, int h, const int *tracked, const int *full, int min_size, int *T, int *P, int *S, unsigned char *mask,
                              int *kept);
// the entries of fill_matches_device's block_count per map
size_t fill_matches_blocks(int nx, int ny);
// acc_u, acc_v: [n][J][h][w]; mask: [n][h][w]; xs: [nx], ys: [ny] (device, on the map); block_count: [n][fill_matches_blocks(nx, ny)] scratch; matches:
// [n][J][nx ny][4], of which map m's first count[m] rows of every step are written; count: [n]
int fill_matches_device(sfa_ctx *ctx, int n, int J, int w, int h, const double *acc_u, const double *acc_v, const unsigned char *mask, const int *xs, int nx,
                        const int *ys, int ny, int divisor, int *block_count, float *matches, int *count);
// flow_x, flow_y: [n J][h][stride]; acc_u, acc_v: [n][J][h][w]; tracked: [n][h][w]
int fill_trajectories_device(sfa_ctx *ctx, int n, int J, int w, int h, int stride, const float *flow_x, const float *flow_y, int scale, double *acc_u,
                             double *acc_v, int *tracked);

// ---- EpicFlow's interpolation at device level (epic_nn.hip, epic_fit.hip, epic_filter.hip), in the same form: device pointers in, launches on the context's
// stream out.  The sfa_epic_nearest_seeds_batch / sfa_epic_interpolate_batch entry points wrap them, sfa_epic_batch (epic_batch.hip) chains them ----------
// One image of the nearest-seeds stage.  cost: w * h; seeds: 2 ns ints; out: lab w * h, index and dist ns * nn
struct EpicNnIo { const float *cost; const int *seeds; int ns, nn; int *lab; int *index; float *dist; };
// The stage for m images.  It keeps its two host reads of counts (border pairs; edges and the largest degree), which size what cannot be bounded beforehand,
// and allocates that itself, within `budget` bytes: *done leading images fit and are computed (0: not even the first), the rest are untouched.  Returns
// after waiting for the stream.  estimate (or null): raised to the largest need of an image seen -- the whole search in the default mode, one workgroup's
// in the compact mode (ctx->epic_search), where the search runs in slices that share a workspace; ms[5]: the kernel time by group, added to; info (or
// null): the four numbers of sfa_epic_nn_search_info, added to (the workspace: raised to)
int epic_nn_device(sfa_ctx *ctx, const char *fn, int m, int w, int h, const EpicNnIo *io, size_t budget, int *done, size_t *estimate, float ms[5], long long info[4]);
// what epic_nn_device allocates for an image at least: everything known beforehand (the default mode: `done` among it)
size_t epic_nn_need0(const sfa_ctx *ctx, int w, int h, int ns, int nn);
int epic_nn_check_sizes(sfa_ctx *ctx, const char *fn, int w, int h);
// the domain of a host cost map, w * h floats: +0 ... +Inf, -0.0 taken as +0.  A NaN or a cost below 0 is refused in the name of `fn`, the map named by `what`
// (a printf format that takes `image`) and the pixel by its coordinates
int epic_check_costs(sfa_ctx *ctx, const char *fn, const char *what, int image, const float *cost, int w, int h) __attribute__((format(printf, 3, 0)));
// One image of the fit and its application.  seeds, vects: ns; index, weight: ns * nn; lab, fx, fy: w * h packed (apply only); model: 6 ns (LA) or 2 ns (NW)
struct EpicFitImg {
    const int2 *seeds; const float2 *vects; const int *index; const float *weight; const int *lab;
    float *model, *fx, *fy; int ns, nn;
};
// k_epic_fit (method 0 LA, 1 NW) and k_epic_apply over the m records d_imgs (device memory); ns_max: the largest ns among them
void epic_fit_device(sfa_ctx *ctx, int method, int m, int ns_max, const EpicFitImg *d_imgs);
void epic_apply_device(sfa_ctx *ctx, int method, int m, int w, int h, const EpicFitImg *d_imgs);
// One image of the steps between the stages (epic_filter.hip).  in, out: match lists (x1 y1 x2 y2) of capacity nm; count: the matches of `in`; flag: nm
// bytes; block_off: ceil(nm / 256) ints; kept: one int (device); sal: the saliency plane at `pitch`; index, dist: the lists the weights are applied to
struct EpicFilterImg {
    float4 *in, *out; int count; unsigned char *flag; int *block_off; int *kept;
    const float *sal; int2 *seeds; float2 *vects; const float *est; float *dist; int nn;
};
// each runs one grid over the m records d_imgs; count_max: the largest count among them
void epic_clamp_device(sfa_ctx *ctx, int m, int count_max, int w, int h, const EpicFilterImg *d_imgs);
void epic_saliency_flags_device(sfa_ctx *ctx, int m, int count_max, int w, int h, int pitch, float th, const EpicFilterImg *d_imgs);
void epic_consistency_flags_device(sfa_ctx *ctx, int m, int count_max, float th2, const EpicFilterImg *d_imgs);
void epic_compact_device(sfa_ctx *ctx, int m, int count_max, const EpicFilterImg *d_imgs);        // flag -> out, kept
void epic_seeds_vects_device(sfa_ctx *ctx, int m, int count_max, const EpicFilterImg *d_imgs);    // of `in`
void epic_weights_device(sfa_ctx *ctx, int m, size_t list_max, float coef, const EpicFilterImg *d_imgs);    // (kernels.hip: beside expf_glibc)
// image.c:729-791 for g.nb images.  planes: kEpicSaliencyPlanes planes per image at g (es = kEpicSaliencyPlanes * pl), of which the first three hold the
// Lab image and are overwritten; the result is plane kEpicSaliencyOut of every image
struct Geo;
constexpr int kEpicSaliencyPlanes = 15, kEpicSaliencyOut = 9;
void epic_saliency_device(sfa_ctx *ctx, const Geo &g, float *planes, float sigma_image, float sigma_matrix);
// k_ef_edge_costs (epic_filter.hip): run [ns][cpl], the edge maps as the epic() calls so far left them, advanced by rJ additions of euc; cost [ns][rJ][cpl], the
// map each of the rJ calls reads.  cpl: a multiple of 4, at least gpl; both bases 16-byte aligned
int epic_edge_costs_device(sfa_ctx *ctx, int ns, int rJ, size_t cpl, int gpl, float euc, float *run, float *cost);
// sfa_epic_batch's chain (epic_batch.hip) for n images whose inputs are in device memory already.  cost[i]: w * h packed, euc added, read in place;
// matches[i]: nm[i] rows of x1 y1 x2 y2, copied before the chain touches them; sal[i]: the image's saliency plane at dev_pitch(w) (read where
// p->saliency_th != 0; images may share one); fx[i], fy[i]: w * h packed, written by copies on the stream once image i's sub-batch has finished.  rc,
// counts, status and workspace_bytes as sfa_epic_batch has them; sub-batches, their re-runs and the compact search likewise.  Waits for the stream
struct EpicChainDev { const float *const *cost; const float *const *matches; const int *nm; const float *const *sal; float *const *fx; float *const *fy; };
int epic_chain_device(sfa_ctx *ctx, const char *fn, int n, int w, int h, const sfa_epic_params *p, const EpicChainDev &io, int *rc, int (*counts)[3],
                      size_t workspace_bytes, int *status);

// ---------------------------------------------------------------------------------------------------
// kernel launchers (kernels.hip).  All planes are device pointers of batch element 0; element b lives
// `es` floats further (es = 0 for a single element).  `nb` = batch size, `active` = bit mask of the
// elements that still iterate (threshold breaks).
// ---------------------------------------------------------------------------------------------------
// pl = pitch*h.  A window b takes part in a launch when bit b is set in `active` (what the host knows) AND in *amask (what the device knows: the windows
// that have not met the outer threshold yet, sfa_ctx::d_amask; null = no device-side mask)
struct Geo { int w, h, pitch; long pl; long es; int nb; WMask active; const unsigned long long *amask; };

struct PenaltyDev { int id; float eps, trunc; };
inline PenaltyDev pen(const sfa_penalty &p) { return PenaltyDev{p.id, p.eps, p.trunc}; }

// several warps (factor != 0) of one flow field in one pass; offsets are arena offsets of element 0 like Term::i1_off, mask_off < 0: no mask
struct WarpJob { long src_off, dst_off, mask_off; int factor; };
struct WarpJobs { WarpJob job[4 * SFA_MAX_REF]; int n; };
void launch_warp_jobs(sfa_ctx *c, const Geo &g, const WarpJobs &J, float *base, const float *wx, const float *wy);
bool launch_warp_smooth(sfa_ctx *c, const Geo &g, const WarpJobs &J, float *base, const float *wx, const float *wy, int method, float *sh, float *sv,
                        const float *dpsis, float alpha, PenaltyDev reg);   // the warps + compute_smoothness of the same flow in one pass; false: not this combination
void launch_warp(sfa_ctx *c, const Geo &g, float *dst3, float *mask, const float *src3, const float *wx, const float *wy, int factor,
                 long src_es /* batch stride of src3 (frames) */);
void launch_deriv_stack(sfa_ctx *c, const Geo &g, float *out24, const float *I1, const float *I2, long es1, long es2);
void launch_convolve(sfa_ctx *c, const Geo &g, float *dst, const float *src, int order, int horiz, int nplanes);
void launch_dpsis(sfa_ctx *c, const Geo &g, float *dst, const float *im3, long im_es, float coef, const float avg[3], const float stdv[3], int hbit);
void launch_smoothness(sfa_ctx *c, const Geo &g, int method, float *sh, float *sv, const float *uu, const float *vv, const float *dpsis,
                       float alpha, PenaltyDev reg);
void launch_sub_laplacian(sfa_ctx *c, const Geo &g, float *dst, const float *src, const float *wh, const float *wv);
void launch_mask_weight(sfa_ctx *c, const Geo &g, float *masks, const float *occ, float data_norm, int ref, int one_direction);
void launch_fill(sfa_ctx *c, float *p, size_t n, float v);
void launch_division_chain(sfa_ctx *c, const float *a, const float *b, float *q_chain, float *q_exact, unsigned char *admitted, size_t n);
void launch_fill_planes(sfa_ctx *c, const Geo &g, float *p, int nplanes, float v);
void launch_zero_planes(sfa_ctx *c, const Geo &g, float *p, int nplanes);
// updates *c->d_amask and c->d_last.  dfa, dfb (or null): the per-pixel |differences| of the two norms as the update left them -- windows whose norm lies within
// 1e-3 of the threshold are then decided by the reference's own fp32 running sums (k_exact_break)
void launch_outer_threshold(sfa_ctx *c, const Geo &g, const double *red, float thres, const float *dfa = nullptr, const float *dfb = nullptr);
void launch_set_mask(sfa_ctx *c, const WMask &v);

// Where a kernel other than k_sor_prepare leaves the solver's operands (diagonal-major planes of a SorWorkspace)
struct SorOperandOut {
    float4 *sa = nullptr, *sb = nullptr; unsigned long long *x = nullptr; unsigned *flags = nullptr;
    long ent = 0; int RP = 0, G = 0, ntasks = 0, nb = 0;
};
struct Term {
    long stack_off; long mask_off; float hd, hg, s; int is_ref;
    // fused form (launch_assemble_images): the image pair the derivative stack is taken of, arena offsets like mask_off;
    // backward: the mask is weighted with the backward (slot < ref) or forward occlusion factor
    long i1_off, i2_off; int backward;
};
struct AssembleArgs {
    Term t[kMaxTerms];
    int n;
    int dt_norm;
    PenaltyDev color, grad;
    // channel weights: NULL => ones.  chw planes live OUTSIDE the element arena stride logic: chw_es batch stride
    const float *chw; long chw_pl; long chw_es; int chw_pitch; int chw_stride0; int lstride;
    int accumulate;      // 1: add to existing a11.. (stage API), 0: start from zero
    int do_laplacian;    // apply sub_laplacian(b1,uu), (b2,vv) at the end
    // fused form only: occlusion / direction weighting of the masks (variational_mt.cpp:293-320) applied on the fly
    float data_norm; int one_direction;
    // fused form only: if op.sa is set, the 2x2 blocks are inverted and the operands written diagonal-major for the solver
    // (what k_sor_prepare does from the planes); a11 .. b2 are then not written at all
    SorOperandOut op;
    int zero_duv;        // fused form: du = dv = 0 (first inner iteration, variational_mt.cpp:323-324): the planes are not read
    int chain_ok = 0;    // fused form, set by the launcher: the scalars admit the shared-reciprocal divisions (kernels.hip: recip_of / div_by)
};
void launch_assemble(sfa_ctx *c, const Geo &g, const AssembleArgs &a, const float *base /*element arena of batch 0*/, float *a11, float *a12,
                     float *a22, float *b1, float *b2, const float *du, const float *dv, const float *uu, const float *vv, const float *sh, const float *sv);

// The same system from the warped image pairs directly: derivative stacks formed in LDS tiles, never stored
// (get_derivatives' 8 filters + :293-320 mask weights + :336-365 in one pass).  occ: occlusion plane.
int launch_assemble_images(sfa_ctx *c, const Geo &g, const AssembleArgs &a, const float *base, float *a11, float *a12, float *a22, float *b1, float *b2,
                            const float *du, const float *dv, const float *uu, const float *vv, const float *sh, const float *sv, const float *occ);

// two-frame refinement (variational.c / variational_aux.c)
void launch_smoothness_2f(sfa_ctx *c, const Geo &g, float *sh, float *sv, const float *uu, const float *vv, const float *dpsis, float half_alpha);
void launch_data_2f(sfa_ctx *c, const Geo &g, const float *D, const float *mask, const float *du, const float *dv, float *a11, float *a12, float *a22, float *b1,
                    float *b2, const float *wx, const float *wy, const float *sh, const float *sv, float hd, float hg);
// launch_deriv_stack(I1, I2) + launch_data_2f in one kernel: the stack stays in LDS and registers (k_data_2f_fused); every plane at g.es
void launch_data_2f_fused(sfa_ctx *c, const Geo &g, const float *I1, const float *I2, const float *mask, const float *du, const float *dv, float *a11, float *a12,
                          float *a22, float *b1, float *b2, const float *wx, const float *wy, const float *sh, const float *sv, float hd, float hg);

// ---- occlusion.hip: optimizeOcc (variational_aux_mt.cpp:758-887) ----------------------------------------------------
struct OccSlot {
    long s1_off, s2_off;     // image pair of the slot's successive-frames stack (arena offsets, like Term::i1_off)
    long r1_off, r2_off;     // image pair of its reference-frame stack (variational_mt.cpp:139-144)
    long mask_off;           // raw warp mask
    float rho, omega;        // rho[idx], omega[idx], idx = max(ref-s-1, s-ref)  (:814)
    int label;               // 0: slot in the future (s >= ref), 1: in the past  (:829-837)
};
struct OccArgs { OccSlot slot[2 * SFA_MAX_REF]; int nslots; float hd, hg, penalty; PenaltyDev color, grad; };
void launch_occ_costs(sfa_ctx *c, const Geo &g, const OccArgs &a, const float *base, float *d0, float *d1, long d_es /* window stride of d0,d1 */);
constexpr int kCutWorkPlanes = 13;
// exact two-label cut of sum D_l(p) + alpha * [l_p != l_q] over 4-neighbours; occ = 2*l - 1.  d0, d1, work: planes packed [nb][pl]
int run_grid_cut(sfa_ctx *c, const Geo &g, float *occ, long occ_es, const float *d0, const float *d1, float *work, float alpha);

// du/dv -> uu,vv, zero padding, L1 change norms (variational_mt.cpp:371-402); red = per-element 2 doubles (sum|old_du-du|, sum|old_dv-dv|)
void launch_update_inner(sfa_ctx *c, const Geo &g, float *uu, float *vv, const float *wx, const float *wy, const float *du, const float *dv,
                         const float *old_du, const float *old_dv, double *red /* [nb][2] */, float *dfa = nullptr, float *dfb = nullptr);   // dfa, dfb: the per-pixel terms (launch_exact_norms)
// the same with du,dv taken from a solver workspace's x plane (diagonal-major); old_du == nullptr: zeros; du_out == nullptr:
// du,dv are not stored
void launch_update_inner_x(sfa_ctx *c, const Geo &g, float *uu, float *vv, const float *wx, const float *wy, const SorOperandOut &x, const float *old_du,
                           const float *old_dv, float *du_out, float *dv_out, double *red, float *dfa = nullptr, float *dfb = nullptr);
// the norms of the windows `which` as the reference forms them (fp32 running sums over blocks of four pixels in raster order, the fp32 division) from the per-pixel terms an
// update left in dfa, dfb: out[2 b], out[2 b + 1] (device)
void launch_exact_norms(sfa_ctx *c, const Geo &g, const float *dfa, const float *dfb, const WMask &which, float *out);
// flow update of the LAST inner iteration straight from the x plane, fused with the outer update below (uu, vv, wx, wy all written)
void launch_update_outer_x(sfa_ctx *c, const Geo &g, float *uu, float *vv, float *wx, float *wy, const SorOperandOut &x, double *red, float *dfa = nullptr,
                           float *dfb = nullptr);   // dfa, dfb: where to leave the per-pixel |differences| (launch_outer_threshold)
// sum|uu-wx|, sum|vv-wy|; wx<-uu, wy<-vv (variational_mt.cpp:412-429)
void launch_update_outer(sfa_ctx *c, const Geo &g, float *wx, float *wy, const float *uu, const float *vv, double *red, float *dfa = nullptr, float *dfb = nullptr);
void launch_copy_planes(sfa_ctx *c, const Geo &g, float *dst, const float *src, int nplanes, long dst_es, long src_es);
void launch_scale_plane(sfa_ctx *c, const Geo &g, float *p, float s);

// pyramid (kernels.hip)
// the widest Gaussian the blur kernels carry: cv::GaussianBlur's 33 taps (sigma * 8 + 1 rounds to at most 33), the range sfa_gaussian_blur documents.  Every
// host buffer of taps has kMaxBlurTaps entries and is filled by cv_gauss_taps alone, which writes no more
constexpr int kMaxBlurRadius = 16, kMaxBlurTaps = 2 * kMaxBlurRadius + 1;
// SFA_ERR_ARG (nothing copied, nothing launched) for a radius beyond kMaxBlurRadius
int launch_gauss_blur(sfa_ctx *c, const Geo &g, float *dst, float *tmp, const float *src, int nplanes, const float *taps, int radius);
void launch_resize(sfa_ctx *c, float *dst, int dw, int dh, int dpitch, long dpl, long des, const float *src, int sw, int sh, int spitch, long spl, long ses,
                   int nplanes, int nb, float post_scale);
void launch_resize_flow(sfa_ctx *c, float *dstx, float *dsty, int dw, int dh, int dpitch, long des, const float *srcx, const float *srcy, int sw, int sh, int spitch,
                        long ses, int nb, float post_x, float post_y);   // both planes of a flow field, k_resize's arithmetic
void launch_resize_scaled(sfa_ctx *c, float *dst, int dw, int dh, int dpitch, long dpl, long des, const float *src, int sw, int sh, int spitch, long spl,
                          long ses, int nplanes, int nb, float post_scale, double scale_x, double scale_y);
struct PyrInfo { int fused, td, lds; };   // what a pyramid step ran: k_pyr_down (1) with its tile height and LDS bytes, or the two kernels (0, 0, 0)
bool launch_pyr_down(sfa_ctx *c, float *dst, int dw, int dh, int dpitch, long dpl, long des, const float *src, int sw, int sh, int spitch, long spl, long ses,
                     int nplanes, int nb, const float *taps, int radius, PyrInfo *info = nullptr);   // blur + resize fused; false: footprint too large or radius > 8, use the two kernels
// one pyramid step, fused where launch_pyr_down accepts, else blur + resize through tmp (6 source planes per window, ses apart): kernels.hip
int pyramid_step(sfa_ctx *c, float *dst, int dw, int dh, int dpitch, long dpl, long des, const float *src, int sw, int sh, int spitch, long spl, long ses, int nplanes,
                 int nb, const float *taps, int radius, float *tmp, PyrInfo *info = nullptr);
void launch_presmooth(sfa_ctx *c, const Geo &g, float *dst, float *tmp, const float *src, int nplanes, float sigma);
void launch_normalize_sums(sfa_ctx *c, const Geo &g, const float *frames3, double *red /* [3][2] */);
void launch_normalize_apply(sfa_ctx *c, const Geo &g, float *frames3, const double avg[3], const double stdv[3]);
// cv::getGaussianKernel's taps for cv::GaussianBlur(Size(0,0), sigma) on CV_32F (api.hip) into k[kMaxBlurTaps]; returns the radius, or -1 (k untouched) when
// sigma is not a positive number or the kernel has more than kMaxBlurTaps taps.  Hidden: job.hip's use adds no export
__attribute__((visibility("hidden"))) int cv_gauss_taps(float sigma, float k[kMaxBlurTaps]);

// ---- device_io.hip: the device seam (sfa_job_upload_device ...): conversions and moves only ---------------------------------------------
// A strided source of colour frames in device memory: element (window, frame, channel, row, column) at p + the strides, in elements of dtype (sfa_dev_dtype)
struct PackSrc { const void *p; int dtype; long long sw, sf, sc, sr, sx; };
// dst = plane 0 of frame 0 of the first window; window i lies dst_es floats further, frame f 3 pl, channel c pl.  Columns >= w are not written.
void launch_pack_frames(sfa_ctx *c, float *dst, long dst_es, long pl, int pitch, int w, int h, int nwin, int F, const PackSrc &s);
// dst = u plane of the first window (v one pl further, the next window dst_es); src null: zeros.  st = element strides of (window, u|v, row, column)
void launch_pack_flow(sfa_ctx *c, float *dst, long dst_es, long pl, int pitch, int w, int h, int nwin, const float *src, const long long st[4]);
// the planes wx, wy (and occ, or null) of nwin windows src_es floats apart -> flow (st[4]) and occ_dst (ost[3] = window, row, column)
void launch_unpack_planes(sfa_ctx *c, const float *wx, const float *wy, const float *occ, long src_es, int pitch, int w, int h, int nwin, float *flow,
                          const long long st[4], float *occ_dst, const long long ost[3]);

// ---- mosaic.hip: raw Bayer ingest (sfa_demosaic_device, sfa_sequence_upload_mosaic*, sfa_job_set_raw_weights) -----------------------------
// n one-channel mosaics of W x H elements of dtype in device memory, element (frame, row, column) at p + the strides; the crop starts at (x0, y0)
struct MosaicSrc { const void *p; int dtype; long long sf, sr, sx; int W, H, x0, y0; };
// n fp32 RGB frames of w x h (the crop's size), element (frame, channel, row, column) at p + the strides
struct MosaicDst { float *p; long long sf, sc, sr, sx; int w, h; };
// method 0: bayer2rgbGR, 2: the 8-bit OpenCV conversion; one launch per 32768 frames
void launch_demosaic(sfa_ctx *c, const MosaicSrc &src, const MosaicDst &dst, int n, int method, int red_x, int red_y);
// rawWeighting into the weight planes of nwin windows: chw = plane 0 of the first, planes pl apart, windows es apart, rows of `stride` floats at pitch cp
void launch_raw_weights(sfa_ctx *c, float *chw, long es, long pl, int cp, int stride, int w, int h, int nwin, int red_x, int red_y, float weight);

// ---------------------------------------------------------------------------------------------------
// SOR (sor.hip)
// ---------------------------------------------------------------------------------------------------
struct SorWorkspace {
    sfa_ctx *ctx = nullptr;
    int w = 0, h = 0, K = 0, nb = 0;
    int NB = 0, NG = 0, RP = 0, ND = 0, G = 0, NS = 0, NCH = 0, ntasks = 0, F = 0, CHK = 0;
    int nwords = 0;               // progress words per window (one per task, each on a 128-byte line of its own)
    long ent = 0;                 // entries per element (ND*RP)
    int band = 0, Wp = 0, EP = 0;   // band kernel: fused sweeps per wave (0 = task kernel), edge row pitch / left pad
    int chain = 0;                  // sor_chain.hip shape id (0 = the band / task kernels); then NG = groups per band, NCH = chunks per stage, NS = barrier intervals
    long edge_job = 0;
    DevMem sa, sb, x, flags, order, edge;
    int configure(sfa_ctx *ctx, int w, int h, int K, int nb);   // (re)allocates for this shape
};
// planes: row-major device planes of element 0 (+es).  inv_out: write the inverted blocks back to a11/a12/a22
// the same in two halves for a producer that writes the operands itself (launch_assemble_images with a.op set)
int sor_operand_target(sfa_ctx *c, SorWorkspace &ws, const Geo &g, int K, SorOperandOut *out);
// du == nullptr: leave the result in the workspace's x plane (read it with launch_update_inner_x)
int sor_run_prepared(sfa_ctx *c, SorWorkspace &ws, const Geo &g, float *du, float *dv, int K, float omega);
// labelled mode slow_flow_sor_order red_black (a different algorithm; sor.hip): K two-colour sweeps on row-major planes, blocks inverted in place
int sor_rb_run(sfa_ctx *c, const Geo &g, float *du, float *dv, float *a11, float *a12, float *a22, const float *b1, const float *b2, const float *sh,
               const float *sv, int K, float omega);
int sor_run(sfa_ctx *c, SorWorkspace &ws, const Geo &g, float *du, float *dv, float *a11, float *a12, float *a22, const float *b1, const float *b2,
            const float *sh, const float *sv, int K, float omega, bool inv_out);

// ---- the device seam's argument checks, shared by every entry point that takes device memory (job.hip, two_frame.hip, track.hip, track_fill.hip, quantile.hip, api.hip).
// The arithmetic -- View, the sign and extent rule, strides_nest, byte ranges and their overlap -- is dev_view.h's, host code a CPU test compiles; what asks
// the HIP runtime is api.hip's.  Each refuses with SFA_ERR_ARG and a message that names `fn` and the argument; nothing is launched on a refusal ------------
// a view: refuses a null pointer or null strides, then what view_extent refuses, then what check_device_pointer does
__attribute__((visibility("hidden"))) int check_view(sfa_ctx *ctx, const char *fn, const View &v, long long min_inner = 1);
// no two of the checked views share a byte (a null pointer is skipped); why: what an overlap would break, or null
__attribute__((visibility("hidden"))) int check_disjoint(sfa_ctx *ctx, const char *fn, std::initializer_list<View> views, const char *why = nullptr);
// the frames of `nwin` windows (or pairs) of F frames each, or a sequence's n frames as one window of n: the layout's element type, and its view
int check_frames_source(sfa_ctx *ctx, const char *fn, const void *frames_dev, const sfa_dev_layout *l, long long win_stride, int nwin, int F, int w, int h);
// p is device memory of the context's GPU, and element `last` (of `elem` bytes) lies inside its allocation
int check_device_pointer(sfa_ctx *ctx, const char *fn, const char *arg, const void *p, long long last, size_t elem);
// download destinations: flow [n][2][h][w] at `strides`, occlusions [n][h][w] at `occ_strides` (or null): checked views, and freedom from overlap
int check_download_destination(sfa_ctx *ctx, const char *fn, int n, int w, int h, float *flow_dev, const long long strides[4], float *occ_dev,
                               const long long occ_strides[3]);
// elements [b0, b0 + n) of a batch of nb (`what`: "windows", "pairs")
int check_batch_range(sfa_ctx *ctx, const char *fn, const char *what, int b0, int n, int nb);
// the demosaicing method and the red site's parities of the raw-ingest entry points (and of sfa_job_set_raw_weights: method 0)
__attribute__((visibility("hidden"))) int check_mosaic_method(sfa_ctx *ctx, const char *fn, int method, int red_x, int red_y);

}  // namespace sfa

namespace sfa {
// ---- epic_init.hip: EpicFlow's initialisation on resident data (sfa_rgb8_to_lab_device, sfa_sequence_lab, sfa_epic_job_*, sfa_job_set_flow_epic) -------
// n fp32 images of w x h, element (image, channel, row, column) at p + the strides: rgb8_to_lab (host/epic.cpp:19-28) of every pixel, csrc/lab_math.h.
// Columns >= w of the destination are not written
struct LabSrc { const float *p; long long sn, sc, sr, sx; };
struct LabDst { float *p; long long sn, sc, sr, sx; };
void launch_rgb8_to_lab(sfa_ctx *c, const LabSrc &src, const LabDst &dst, int n, int w, int h, float norm);
// epic_to_initial_flow (host/slow_flow.cpp:530-546) for nwin windows: the packed sw x sh fields src_u (v: src_v; the next window src_es floats further)
// -> dst (u plane of the first window, v one pl further, the next window dst_es) of w x h at `pitch`.  Sizes equal: one fp32 multiplication by mul_u /
// mul_v (image_mul_scalar); else k_resize itself (sfa_resize_linear's kernel) with that multiplication as its post_scale.  Columns >= w are not written
void launch_epic_initial_flow(sfa_ctx *c, float *dst, long dst_es, long pl, int pitch, int w, int h, int nwin, const float *src_u, const float *src_v, long src_es,
                              int sw, int sh, float mul_u, float mul_v);

// ---- ref_image.hip: dense_tracking's reduced reference image (sfa_reference_lab_device, sfa_track_job_upload_fill_reference*) ---------------------------
// n 8-bit images, element (image, channel, row, column) at p + the strides; p null: not wanted
struct Rgb8Dst { unsigned char *p; long long sn, sc, sr, sx; };
// what the stage refuses of a size and a skip, in the name of `fn`: a skip that is not served (csrc/ref_image.h), an empty grid, a size OpenCV's resize
// rounds to another grid.  *gw, *gh: the accumulation grid
__attribute__((visibility("hidden"))) int reference_check(sfa_ctx *ctx, const char *fn, int w, int h, int skip, int *gw, int *gh);
// n frames of w x h as read -> their Lab images (and 8-bit RGB images) on the grid of a size and skip reference_check passed.  skip 0: k_rgb8_to_lab
__attribute__((visibility("hidden"))) void launch_reference_lab(sfa_ctx *c, int n, int w, int h, int skip, const LabSrc &src, float norm, const LabDst &dst,
                                                                const Rgb8Dst &rgb8);

}  // namespace sfa

// ---- sfa_epic_job: the inputs and fields of epic() for n images of one size, resident (epic_init.hip) ----
struct sfa_epic_job {
    sfa_ctx *ctx = nullptr;
    sfa_epic_params p;
    int w = 0, h = 0, n = 0, pitch = 0;
    size_t npix = 0, pl = 0;                // w * h (the chain's packed planes); pitch * h (the saliency's)
    bool saliency = false;
    sfa::DevMem cost;                       // n packed planes, euc added
    sfa::DevMem flow;                       // n x (u, v) packed planes
    sfa::DevMem sal;                        // n saliency planes at the device pitch (saliency_th != 0)
    sfa::DevMem stage;                      // the saliency's work planes for stage_images images; their first three take the Lab image
    int stage_images = 0;
    std::vector<std::unique_ptr<sfa::DevMem>> matches;   // per image: nm rows of x1 y1 x2 y2
    std::vector<int> nm;                    // -1: no matches given yet
    std::vector<char> have_cost, have_lab;
    std::vector<int> rc;                    // the last run's epic() value per image: 0 a field, 1 zeros (no match left); -1: none (not run, or flagged)
    float *u(int i) const { return flow.f() + (size_t)i * 2 * npix; }
    float *v(int i) const { return u(i) + npix; }
};

// ---- sfa_pair_job: n frame pairs of one size in HBM for the two-frame refinement (two_frame.hip: the one launch sequence, the resident jobs, the host calls) ----
// Pair b owns the planes [b * NPL, (b + 1) * NPL) of one allocation; this enum is the only statement of the plane list.  IM1 and IM2 lie next to each other
// (launch_pack_frames fills them as frames 0 and 1 of a window), so do WX and WY (launch_pack_flow, launch_unpack_planes).
struct sfa_pair_job {
    enum { WX, WY, UU, VV, DU, DV, SH, SV, A11, A12, A22, B1, B2, MASK, DPS, IM1, IM2 = IM1 + 3, WIM2 = IM2 + 3, NPL = WIM2 + 3 };
    sfa_ctx *ctx = nullptr;
    int w = 0, h = 0, n = 0, pitch = 0;
    long pl = 0, es = 0;
    sfa_params_2frame p;
    bool stored_stack = false;       // the data term reads a stored derivative stack (the host calls): 24 planes per pair, behind the n x NPL planes of `mem`
    sfa::DevMem mem;
    sfa::DevMem stack;               // SFA_PAIR_UNFUSED=1 on a job without a stored stack: 24 planes per pair, allocated by the first such run
    sfa::SorWorkspace ws;
    float *plane(int b, int i) const { return mem.f() + b * es + (long)i * pl; }
    sfa::Geo geo() const { return sfa::Geo{w, h, pitch, pl, es, n, sfa::WMask::first(n), nullptr}; }
};

// ---- sfa_sequence: n colour frames of one size resident in HBM (api.hip: the entry points; job.hip: sfa_job_upload_resident copies windows out of one) ----
struct sfa_sequence {
    sfa_ctx *ctx = nullptr;
    int w = 0, h = 0, n = 0, pitch = 0;
    long pl = 0;
    sfa::DevMem mem;                        // n x 3 planes at the device pitch
    sfa::DevMem sums;                       // n x 6 doubles: per frame and channel sum(I), sum(I*I)
    // sfa_sequence_upload_mosaic: the caller's mosaic goes through a pinned copy into mos_dev, the demosaicing kernel's source; ev_mos says the copy out of
    // the pinned buffer has been made (the device buffer is reused in stream order)
    void *mos_stage = nullptr;
    size_t mos_stage_bytes = 0;
    hipEvent_t ev_mos = nullptr;
    sfa::DevMem mos_dev;
    sfa::DevMem rescale_tmp;                // sfa_sequence_rescale into this sequence: the blurred frames of a chunk and the row pass's scratch
    float *frame(int f) const { return mem.f() + (long)f * 3 * pl; }
    sfa::Geo geo() const { return sfa::Geo{w, h, pitch, pl, 0, 1, sfa::WMask::first(1), nullptr}; }
};
