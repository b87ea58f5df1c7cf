// epic_batch.hip -- sfa_epic_batch: epic() (host/epic.cpp, epic_flow_extended/epic.cpp:147-235) for a batch of images of one size as ONE chain on the GPU.
// Matches, Lab images and cost maps go up, the two flow planes (and the survivor counts) come down; everything between stays in device memory:
//   clamp -> [saliency (epic_saliency_device) -> saliency filter -> compaction] -> [seeds and vectors -> nearest seeds with min(pref_nn + 1, count) neighbours
//   (epic_nn_device) -> kernel weights -> Nadaraya-Watson estimate (epic_fit_device) -> consistency filter -> compaction] -> seeds and vectors -> nearest
//   seeds with min(nn, count) -> kernel weights -> fit -> apply
// The neighbour count is carried per image (EpicNnIo::nn, EpicFitImg::nn), so images with different counts share every launch.  The host reads what it must:
// the survivors of each compaction (they size the next stage's grids and decide who drops out), and the two counts the nearest-seeds stage reads itself.
// Sub-batches: consecutive images whose known needs fit the budget.  When the nearest-seeds stage finds that not all of a sub-batch fits after all, the
// sub-batch is run again from its start with the images that did fit (nothing of a sub-batch is written before it has finished, and no result depends on the
// cut); an image that does not fit alone is flagged.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "sfa_device.h"
#include "sfa_internal.h"

// This file holds no kernel: sizing, records, copies and launches around the stages' own launch functions.  Compiled for size (see track.hip).
#pragma clang attribute push(__attribute__((minsize)), apply_to = function)

namespace sfa {
namespace {

constexpr int kMaxSubBatch = 4096;                                   // images per launch (the grids' second dimension)
constexpr int kEfThreads = 256;                                      // epic_filter.hip's block: the compaction's block_off has one entry per block

inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }
struct Bump {
    char *base = nullptr; size_t used = 0;
    template <class T> T *take(size_t count) { T *r = reinterpret_cast<T *>(base + used); used += al(count * sizeof(T)); return r; }
};

// kernel time by stage: pairs of events, read once the stream has been waited for
struct StageTimer {
    struct Span { int slot; hipEvent_t a, b; };
    std::vector<Span> spans;
    hipStream_t st;
    explicit StageTimer(hipStream_t s) : st(s) {}
    ~StageTimer() { for (Span &s : spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); } }
    void begin(int slot) {
        Span s{slot, nullptr, nullptr};
        if (hipEventCreate(&s.a) != hipSuccess || hipEventCreate(&s.b) != hipSuccess) return;
        (void)hipEventRecord(s.a, st);
        spans.push_back(s);
    }
    void end() { if (!spans.empty()) (void)hipEventRecord(spans.back().b, st); }
    void collect(float ms[8]) {                                      // after a wait
        for (Span &s : spans) {
            float v = 0.f;
            if (hipEventElapsedTime(&v, s.a, s.b) == hipSuccess) ms[s.slot] += v;
            (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b);
        }
        spans.clear();
    }
};

// what one image of a sub-batch owns in device memory for the whole chain
struct Item {
    int i;                                                           // its place in the caller's arrays
    float *cost, *fx, *fy, *model, *dist;
    int *lab, *index, *block_off, *kept;
    float4 *list[2];                                                 // the match list in play and the one a compaction writes
    int2 *seeds; float2 *vects; unsigned char *flag;
    int count, cnt[3];
};

struct Sizes { int w, h, pitch; size_t npix, pl; bool saliency, sal_own; };       // sal_own: the chain computes the saliency planes itself (and holds them)

int nn_max_of(const sfa_epic_params &p, int nm) { return std::max(p.pref_nn ? std::min(p.pref_nn + 1, nm) : 1, std::min(p.nn, nm)); }

size_t persistent_bytes(const Sizes &z, const sfa_epic_params &p, int nm) {
    const size_t list = (size_t)nm * nn_max_of(p, nm);
    return al(sizeof(EpicFilterImg)) + al(sizeof(EpicFitImg)) + 4 * al(z.npix * 4) + 2 * al((size_t)nm * 16) + 2 * al((size_t)nm * 8) + 2 * al(list * 4) +
           al((size_t)nm * 24) + al((size_t)nm) + al(((size_t)nm + kEfThreads - 1) / kEfThreads * 4) + al(4);
}
size_t saliency_bytes(const Sizes &z) { return z.sal_own ? al((size_t)kEpicSaliencyPlanes * z.pl * 4) : 0; }

struct Call {
    sfa_ctx *ctx; const char *fn; Sizes z; const sfa_epic_params *p;
    const float *const *lab; int lab_stride; const float *const *cost; const float *const *matches; const int *nm;
    float *const *flow_x, *const *flow_y; int flow_stride; int *rc; int (*counts)[3]; float *const *kept_matches;
    size_t budget; size_t estimate;                                  // of the nearest-seeds stage's own part, per image
    long long info[4];                                               // sfa_epic_nn_search_info of the sub-batch's last search
    // dev: cost, matches, flow_x and flow_y point into device memory (packed w x h planes, nm rows) and sal[i] is image i's saliency plane at the device
    // pitch, computed by the caller; lab is not read.  The costs are read in place and the matches copied, so a sub-batch that is run again finds both as
    // they were; the flows are left in the caller's planes by copies on the stream
    bool dev; const float *const *sal;
};

// The chain for the images `which` (all with matches).  *fit: how many of them, from the first, the sub-batch can hold (== which.size(): done and written)
int run_sub_batch(Call &c, const std::vector<int> &which, int *fit) {
    sfa_ctx *ctx = c.ctx;
    const Sizes &z = c.z;
    const sfa_epic_params &p = *c.p;
    hipStream_t st = ctx->stream;
    const int m = (int)which.size();
    *fit = 0;
    for (long long &v : c.info) v = 0;
    size_t bytes = 0;
    for (int i : which) bytes += persistent_bytes(z, p, c.nm[i]);
    DevMem mem, sal_mem;
    SFA_TRY(mem.alloc(ctx, bytes));
    Bump b{static_cast<char *>(mem.p)};
    EpicFilterImg *d_filter = b.take<EpicFilterImg>(m);
    EpicFitImg *d_fit = b.take<EpicFitImg>(m);
    b.used = m * (al(sizeof(EpicFilterImg)) + al(sizeof(EpicFitImg)));                 // (the records are counted per image)
    std::vector<Item> items(m);
    for (int k = 0; k < m; k++) {
        Item &t = items[k];
        const int nm = c.nm[which[k]];
        const size_t list = (size_t)nm * nn_max_of(p, nm);
        t.i = which[k];
        t.cost = b.take<float>(z.npix); t.lab = b.take<int>(z.npix); t.fx = b.take<float>(z.npix); t.fy = b.take<float>(z.npix);
        t.list[0] = b.take<float4>(nm); t.list[1] = b.take<float4>(nm);
        t.seeds = b.take<int2>(nm); t.vects = b.take<float2>(nm);
        t.index = b.take<int>(list); t.dist = b.take<float>(list);
        t.model = b.take<float>((size_t)nm * 6);
        t.flag = b.take<unsigned char>(nm);
        t.block_off = b.take<int>(((size_t)nm + kEfThreads - 1) / kEfThreads);
        t.kept = b.take<int>(1);
        t.count = nm; t.cnt[0] = t.cnt[1] = t.cnt[2] = nm;
        if (c.dev) t.cost = const_cast<float *>(c.cost[t.i]);                              // (read only: EpicNnIo::cost)
        else SFA_HIP(ctx, hipMemcpyAsync(t.cost, c.cost[t.i], z.npix * 4, hipMemcpyHostToDevice, st));
        SFA_HIP(ctx, hipMemcpyAsync(t.list[0], c.matches[t.i], (size_t)nm * 16, c.dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    StageTimer timer(st);
    float *ms = ctx->epic_batch_ms;
    // the records of the images `live` (positions in items), with the saliency plane and the neighbour count of the stage
    std::vector<EpicFilterImg> frec;
    float *sal_planes = nullptr;
    auto put_filter = [&](const std::vector<int> &live, bool sal, int nn_cap) {
        frec.assign(live.size(), EpicFilterImg{});
        for (size_t k = 0; k < live.size(); k++) {
            const Item &t = items[live[k]];
            EpicFilterImg &r = frec[k];
            r.in = t.list[0]; r.out = t.list[1]; r.count = t.count; r.flag = t.flag; r.block_off = t.block_off; r.kept = t.kept;
            r.sal = !sal ? nullptr : c.dev ? c.sal[t.i] : sal_planes + (size_t)live[k] * kEpicSaliencyPlanes * z.pl + (size_t)kEpicSaliencyOut * z.pl;
            r.seeds = t.seeds; r.vects = t.vects; r.est = t.model; r.dist = t.dist; r.nn = std::min(nn_cap, t.count);
        }
        return hipMemcpyAsync(d_filter, frec.data(), frec.size() * sizeof(EpicFilterImg), hipMemcpyHostToDevice, st);
    };
    auto count_max_of = [&](const std::vector<int> &live) { int v = 0; for (int k : live) v = std::max(v, items[k].count); return v; };
    // the survivors of a compaction: kept -> count, the lists change places
    std::vector<int> kept_host(m);
    auto read_kept = [&](const std::vector<int> &live, int slot) {
        for (int k : live) SFA_HIP(ctx, hipMemcpyAsync(&kept_host[k], items[k].kept, 4, hipMemcpyDeviceToHost, st));
        SFA_TRY(sfa_ctx_sync(ctx));
        timer.collect(ms);
        for (int k : live) {
            Item &t = items[k];
            t.count = kept_host[k];
            std::swap(t.list[0], t.list[1]);
            for (int s = slot; s < 3; s++) t.cnt[s] = t.count;
        }
        return (int)SFA_OK;
    };
    auto still_live = [&](const std::vector<int> &live) { std::vector<int> r; for (int k : live) if (items[k].count > 0) r.push_back(k); return r; };
    // nearest seeds, kernel weights and the fit of `method` for the images `live`, each with min(nn_cap, count) neighbours
    std::vector<EpicFitImg> fitrec;
    auto search_and_fit = [&](const std::vector<int> &live, int nn_cap, int method, int slot_nn, int slot_w, int slot_fit, int *done, long long *info) {
        const int L = (int)live.size(), cm = count_max_of(live);
        SFA_HIP(ctx, put_filter(live, false, nn_cap));
        timer.begin(1);
        epic_seeds_vects_device(ctx, L, cm, d_filter);
        timer.end();
        std::vector<EpicNnIo> io(L);
        size_t list_max = 0;
        for (int k = 0; k < L; k++) {
            const Item &t = items[live[k]];
            io[k] = EpicNnIo{t.cost, reinterpret_cast<const int *>(t.seeds), t.count, std::min(nn_cap, t.count), t.lab, t.index, t.dist};
            list_max = std::max(list_max, (size_t)io[k].ns * io[k].nn);
        }
        float nn_ms[5] = {};
        SFA_TRY(epic_nn_device(ctx, c.fn, L, z.w, z.h, io.data(), c.budget - bytes, done, &c.estimate, nn_ms, info));
        for (float v : nn_ms) ms[slot_nn] += v;
        timer.collect(ms);
        if (*done < L) return (int)SFA_OK;
        fitrec.assign(L, EpicFitImg{});
        for (int k = 0; k < L; k++) {
            const Item &t = items[live[k]];
            fitrec[k] = EpicFitImg{t.seeds, t.vects, t.index, t.dist, t.lab, t.model, t.fx, t.fy, t.count, io[k].nn};
        }
        SFA_HIP(ctx, hipMemcpyAsync(d_fit, fitrec.data(), (size_t)L * sizeof(EpicFitImg), hipMemcpyHostToDevice, st));
        timer.begin(slot_w);
        epic_weights_device(ctx, L, list_max, p.coef_kernel, d_filter);
        if (slot_fit != slot_w) { timer.end(); timer.begin(slot_fit); }
        epic_fit_device(ctx, method, L, cm, d_fit);
        timer.end();
        return (int)SFA_OK;
    };

    std::vector<int> live(m);
    for (int k = 0; k < m; k++) live[k] = k;
    // ---- clamp, saliency filter --------------------------------------------------------------------------------------------------------------------------
    if (z.sal_own) {
        SFA_TRY(sal_mem.alloc(ctx, (size_t)m * saliency_bytes(z)));
        sal_planes = sal_mem.f();
        for (int k = 0; k < m; k++)
            for (int ch = 0; ch < 3; ch++) {
                SFA_TRY(upload_plane(ctx, sal_planes + ((size_t)k * kEpicSaliencyPlanes + ch) * z.pl, z.pitch, c.lab[items[k].i] + (size_t)ch * z.h * c.lab_stride,
                                     c.lab_stride, z.w, z.h));
            }
    }
    SFA_HIP(ctx, put_filter(live, z.saliency, 1));
    timer.begin(1);
    epic_clamp_device(ctx, m, count_max_of(live), z.w, z.h, d_filter);
    timer.end();
    if (z.saliency) {
        if (z.sal_own) {
            const Geo g{z.w, z.h, z.pitch, (long)z.pl, (long)(kEpicSaliencyPlanes * z.pl), m, WMask::first(std::min(m, kMaxBatch)), nullptr};
            timer.begin(0);
            epic_saliency_device(ctx, g, sal_planes, 0.8f, 1.0f);
            timer.end();
        }
        timer.begin(1);
        epic_saliency_flags_device(ctx, m, count_max_of(live), z.w, z.h, z.pitch, p.saliency_th, d_filter);
        epic_compact_device(ctx, m, count_max_of(live), d_filter);
        timer.end();
        SFA_TRY(read_kept(live, 1));
        sal_mem.release();
        live = still_live(live);
    }
    // ---- consistency filter -------------------------------------------------------------------------------------------------------------------------------
    int done = 0;
    auto partial = [&](int done_live) {                              // the leading images of the sub-batch up to the first live one that did not fit
        *fit = done_live < (int)live.size() ? live[done_live] : m;
        return (int)SFA_OK;
    };
    if (p.pref_nn && !live.empty()) {
        SFA_TRY(search_and_fit(live, p.pref_nn + 1, 1, 2, 3, 3, &done, nullptr));
        if (done < (int)live.size()) return partial(done);
        timer.begin(1);
        epic_consistency_flags_device(ctx, (int)live.size(), count_max_of(live), p.pref_th * p.pref_th, d_filter);
        epic_compact_device(ctx, (int)live.size(), count_max_of(live), d_filter);
        timer.end();
        SFA_TRY(read_kept(live, 2));
        live = still_live(live);
    }
    // ---- interpolation ---------------------------------------------------------------------------------------------------------------------------------------
    if (!live.empty()) {
        SFA_TRY(search_and_fit(live, p.nn, p.method, 4, 5, 6, &done, c.info));
        if (done < (int)live.size()) return partial(done);
        timer.begin(7);
        epic_apply_device(ctx, p.method, (int)live.size(), z.w, z.h, d_fit);
        timer.end();
        SFA_HIP(ctx, hipGetLastError());
        for (int k : live) {
            const Item &t = items[k];
            if (c.dev) {
                SFA_HIP(ctx, hipMemcpyAsync(c.flow_x[t.i], t.fx, z.npix * 4, hipMemcpyDeviceToDevice, st));
                SFA_HIP(ctx, hipMemcpyAsync(c.flow_y[t.i], t.fy, z.npix * 4, hipMemcpyDeviceToDevice, st));
                continue;
            }
            SFA_TRY(download_plane(ctx, c.flow_x[t.i], c.flow_stride, t.fx, z.w, z.w, z.h));      // the valid columns only
            SFA_TRY(download_plane(ctx, c.flow_y[t.i], c.flow_stride, t.fy, z.w, z.w, z.h));
            if (c.kept_matches) SFA_HIP(ctx, hipMemcpyAsync(c.kept_matches[t.i], t.list[0], (size_t)t.count * 16, hipMemcpyDeviceToHost, st));
        }
        SFA_TRY(sfa_ctx_sync(ctx));
        timer.collect(ms);
    }
    for (const Item &t : items) {
        c.rc[t.i] = t.count > 0 ? 0 : 1;
        if (c.counts)
            for (int s = 0; s < 3; s++) c.counts[t.i][s] = t.cnt[s];
    }
    *fit = m;
    return SFA_OK;
}

// the sub-batches of a call over its n images, in order
int run_chain(Call &c, int n, int *status) {
    sfa_ctx *ctx = c.ctx;
    for (float &v : ctx->epic_batch_ms) v = 0.f;
    for (long long &v : ctx->epic_info) v = 0;
    ctx->epic_chain_runs[0] = ctx->epic_chain_runs[1] = 0;
    // what an image needs at least: what it owns for the whole chain, and beside that the larger of the saliency's planes and the search's known part
    auto need0 = [&](int i) {
        return persistent_bytes(c.z, *c.p, c.nm[i]) + std::max(saliency_bytes(c.z), std::max(epic_nn_need0(ctx, c.z.w, c.z.h, c.nm[i], nn_max_of(*c.p, c.nm[i])), c.estimate));
    };
    for (int i = 0; i < n; i++) status[i] = 0;
    int first = 0, cap = kMaxSubBatch;                               // cap: what the sub-batch before this attempt showed to fit
    while (first < n) {
        if (c.nm[first] == 0) {                                        // no match: epic() returns 1 before it computes anything
            c.rc[first] = 1;
            if (c.counts) c.counts[first][0] = c.counts[first][1] = c.counts[first][2] = 0;
            first++;
            continue;
        }
        std::vector<int> which;
        int next = first;
        for (size_t used = 0; next < n && (int)which.size() < cap; next++) {
            if (c.nm[next] == 0) break;                                // (handled above, in order)
            used += need0(next);
            if (used > c.budget) break;
            which.push_back(next);
        }
        if (which.empty()) {
            if (persistent_bytes(c.z, *c.p, c.nm[first]) + std::max(saliency_bytes(c.z), epic_nn_need0(ctx, c.z.w, c.z.h, c.nm[first], nn_max_of(*c.p, c.nm[first]))) > c.budget) {
                status[first++] = 1;                                 // not even alone: flagged, its outputs untouched
                cap = kMaxSubBatch;
                continue;
            }
            which.push_back(first);                                  // (the estimate is another image's: this one may still fit)
        }
        int fit = 0;
        SFA_TRY(run_sub_batch(c, which, &fit));
        if (fit == (int)which.size()) {                              // (a sub-batch that is run again counts once)
            for (int k = 0; k < 3; k++) ctx->epic_info[k] += c.info[k];
            ctx->epic_info[3] = std::max(ctx->epic_info[3], c.info[3]);
            first = which.back() + 1; cap = kMaxSubBatch;
            ctx->epic_chain_runs[0]++;
            continue;
        }
        if (which.size() == 1) { status[first++] = 1; cap = kMaxSubBatch; continue; }
        cap = std::max(fit, 1);                                      // again, with the images that fit
        ctx->epic_chain_runs[1]++;
    }
    return SFA_OK;
}

}  // namespace

int epic_chain_device(sfa_ctx *ctx, const char *fn, int n, int w, int h, const sfa_epic_params *p, const EpicChainDev &io, int *rc, int (*counts)[3],
                      size_t workspace_bytes, int *status) {
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    size_t budget = workspace_bytes;
    if (!budget) {                                                   // half of what the GPU has free now
        size_t free_b = 0, total_b = 0;
        SFA_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
        budget = free_b / 2;
    }
    Call c{ctx, fn, Sizes{w, h, dev_pitch(w), (size_t)w * h, (size_t)dev_pitch(w) * h, p->saliency_th != 0, false}, p, nullptr, 0, io.cost, io.matches, io.nm,
           io.fx, io.fy, w, rc, counts, nullptr, budget, 0, {}, true, io.sal};
    return run_chain(c, n, status);
}

}  // namespace sfa

using namespace sfa;

int sfa_epic_batch(sfa_ctx *ctx, int n, int w, int h, const sfa_epic_params *p, const float *const *lab, int lab_stride, const float *const *cost,
                   const float *const *matches, const int *nm, float *const *flow_x, float *const *flow_y, int flow_stride, int *rc, int (*counts)[3],
                   float *const *kept_matches, size_t workspace_bytes, int *status) {
    const char *fn = __func__;
    if (!ctx) return set_error(nullptr, SFA_ERR_ARG, "%s: ctx is null", fn);
    if (n < 1) REFUSE("%s: n = %d (at least one image)", fn, n);
    if (w < 1 || h < 1) REFUSE("%s: w x h = %d x %d (both at least 1)", fn, w, h);
    if (!p || !cost || !matches || !nm || !flow_x || !flow_y || !rc || !status) {
        REFUSE("%s: %s is null", fn, !p ? "p" : !cost ? "cost" : !matches ? "matches" : !nm ? "nm" : !flow_x ? "flow_x" : !flow_y ? "flow_y" : !rc ? "rc" : "status");
    }
    if (p->nn < 1) REFUSE("%s: nn = %d (at least one neighbour)", fn, p->nn);
    if (p->pref_nn < 0) REFUSE("%s: pref_nn = %d (0: no consistency filter, else its neighbours)", fn, p->pref_nn);
    if (p->method != 0 && p->method != 1) REFUSE("%s: method = %d (0: locally-weighted affine, 1: Nadaraya-Watson)", fn, p->method);
    if (flow_stride < w) REFUSE("%s: flow_stride = %d (at least w = %d)", fn, flow_stride, w);
    const bool saliency = p->saliency_th != 0;
    if (saliency && !lab) REFUSE("%s: lab is null (the saliency filter reads the Lab images)", fn);
    if (saliency && lab_stride < w) REFUSE("%s: lab_stride = %d (at least w = %d)", fn, lab_stride, w);
    if (saliency && (w <= 8 || h <= 8)) REFUSE("%s: w x h = %d x %d (the saliency's Gaussian of sigma 1.0 needs more than 8 columns and rows)", fn, w, h);
    SFA_TRY(epic_nn_check_sizes(ctx, fn, w, h));
    for (int i = 0; i < n; i++) {
        if (nm[i] < 0) REFUSE("%s: nm[%d] = %d (a count of matches)", fn, i, nm[i]);
        if (!cost[i] || !flow_x[i] || !flow_y[i] || (nm[i] && !matches[i]) || (saliency && !lab[i]) || (kept_matches && !kept_matches[i])) {
            REFUSE("%s: %s[%d] is null", fn, !cost[i] ? "cost" : !flow_x[i] ? "flow_x" : !flow_y[i] ? "flow_y" : (nm[i] && !matches[i]) ? "matches" : (saliency && !lab[i]) ? "lab" : "kept_matches", i);
        }
        const long long list = (long long)nm[i] * std::min(std::max(p->nn, p->pref_nn + 1), std::max(nm[i], 1));
        if (list > INT_MAX) REFUSE("%s: nm[%d] * nn = %lld entries (the kernels index the lists with 32 bits)", fn, i, list);
        for (size_t k = 0; k < (size_t)4 * nm[i]; k++) {
            if (!std::isfinite(matches[i][k])) REFUSE("%s: matches[%d]: match %zu holds a coordinate that is not finite", fn, i, k / 4);
        }
        SFA_TRY(epic_check_costs(ctx, fn, "cost[%d]", i, cost[i], w, h));
    }
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    size_t budget = workspace_bytes;
    if (!budget) {                                                   // half of what the GPU has free now
        size_t free_b = 0, total_b = 0;
        SFA_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
        budget = free_b / 2;
    }
    Call c{ctx, fn, Sizes{w, h, dev_pitch(w), (size_t)w * h, (size_t)dev_pitch(w) * h, saliency, saliency}, p, lab, lab_stride, cost, matches, nm,
           flow_x, flow_y, flow_stride, rc, counts, kept_matches, budget, 0, {}, false, nullptr};
    return run_chain(c, n, status);
}

int sfa_epic_saliency_batch(sfa_ctx *ctx, int n, int w, int h, const float *const *lab, int stride, float sigma_image, float sigma_matrix, float *const *out) {
    const char *fn = __func__;
    if (!ctx) return set_error(nullptr, SFA_ERR_ARG, "%s: ctx is null", fn);
    if (n < 1 || n > kMaxSubBatch) REFUSE("%s: n = %d (1 .. %d images)", fn, n, kMaxSubBatch);
    if (w < 1 || h < 1 || stride < w) REFUSE("%s: w x h = %d x %d, stride = %d (both at least 1, stride at least w)", fn, w, h, stride);
    if (!lab || !out) REFUSE("%s: %s is null", fn, !lab ? "lab" : "out");
    for (float sigma : {sigma_image, sigma_matrix}) {
        if (!(sigma > 0)) REFUSE("%s: sigma = %g (positive)", fn, (double)sigma);
        const int order = std::max(1, (int)floor(3 * sigma) + 1);
        if (order > 16 || w <= 2 * order || h <= 2 * order) REFUSE("%s: w x h = %d x %d is smaller than the filter of sigma %g (more than %d columns and rows)", fn, w, h, (double)sigma, 2 * order);
    }
    if (h < 2) REFUSE("%s: h = %d (the vertical derivative needs two rows)", fn, h);
    for (int i = 0; i < n; i++)
        if (!lab[i] || !out[i]) REFUSE("%s: %s[%d] is null", fn, !lab[i] ? "lab" : "out", i);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const int pitch = dev_pitch(w);
    const size_t pl = (size_t)pitch * h;
    DevMem mem;
    SFA_TRY(mem.alloc(ctx, (size_t)n * kEpicSaliencyPlanes * pl * 4));
    for (int i = 0; i < n; i++)
        for (int ch = 0; ch < 3; ch++) SFA_TRY(upload_plane(ctx, mem.f() + ((size_t)i * kEpicSaliencyPlanes + ch) * pl, pitch, lab[i] + (size_t)ch * h * stride, stride, w, h));
    const Geo g{w, h, pitch, (long)pl, (long)(kEpicSaliencyPlanes * pl), n, WMask::first(std::min(n, kMaxBatch)), nullptr};
    epic_saliency_device(ctx, g, mem.f(), sigma_image, sigma_matrix);
    SFA_HIP(ctx, hipGetLastError());
    for (int i = 0; i < n; i++) SFA_TRY(download_plane(ctx, out[i], stride, mem.f() + ((size_t)i * kEpicSaliencyPlanes + kEpicSaliencyOut) * pl, pitch, w, h));
    SFA_TRY(sfa_ctx_sync(ctx));
    for (int i = 0; i < n; i++)
        for (int y = 0; y < h; y++)
            for (int x = w; x < stride; x++) out[i][(size_t)y * stride + x] = 0.0f;       // image_erase
    return SFA_OK;
}

int sfa_epic_batch_stage_ms(sfa_ctx *ctx, float ms[8]) {
    if (!ctx || !ms) return set_error(ctx, SFA_ERR_ARG, "%s: %s is null", __func__, !ctx ? "ctx" : "ms");
    for (int k = 0; k < 8; k++) ms[k] = ctx->epic_batch_ms[k];
    return SFA_OK;
}

#pragma clang attribute pop
