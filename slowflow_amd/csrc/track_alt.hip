// track_alt.hip -- what a track job that alternates (sfa_track_job_create_alternate) adds to the resident job of track.hip: dense_tracking's loop
// `for p_it < acc_alternate` (dense_tracking.cpp:1381-1903) in place of the one fusion.  Per round
//     prune by the last fusion's selection (p > 0) -> neighbour proposals -> rescoring of the accepted ones -> fusion (position 0 pinned, p > 0)
// on two sets of hypothesis lists the stages read and write in turn, every step the device-level function of its stage call (neigh.hip, fuse.hip,
// energy.hip; sfa_internal.h), all enqueued on the context's stream: no host read between the rounds.  The kernels here only move values: the job's
// slots into lists, the consistent mask, which positions a round filled, the per-round figures, the chosen hypothesis' origin.
#include "track_job.h"

namespace sfa {

constexpr int kAltK = 16, kAltThreads = kTrackThreads, kAltNew = 1 << 30;       // neigh.hip's kNeighK and kNeighNew

struct AltTracked { const int *t[kTrackMaxRates]; int rJ[kTrackMaxRates]; int K; };

// position k of segment blockIdx.y: slot k's energy, occlusion word and origin k where k < S, absent beyond; U, V are copied row-wise by the host code.
// k == 0 also writes consistent: some rate's accumulated hypothesis is tracked over its whole length (:1224)
__global__ void __launch_bounds__(kAltThreads) k_alt_lists(const double *__restrict__ E, const unsigned long long *__restrict__ O, int S, int gpl, int n_stride,
                                                           AltTracked tr, double *__restrict__ energy, unsigned long long *__restrict__ occ,
                                                           unsigned char *__restrict__ origin, unsigned char *__restrict__ consistent) {
    const int p = blockIdx.x * kAltThreads + threadIdx.x;
    if (p >= gpl) return;
    const int s = blockIdx.y / kAltK, k = blockIdx.y % kAltK;
    const size_t o = ((size_t)s * kAltK + k) * gpl + p, i = ((size_t)s * S + k) * gpl + p;
    energy[o] = k < S ? E[i] : __longlong_as_double(0x7ff0000000000000ll);
    occ[o] = k < S ? O[i] : 0ull;
    origin[o] = (unsigned char)(k < S ? k : 0);
    if (k == 0) {
        bool c = false;
        for (int r = 0; r < tr.K; r++) c = c || tr.t[r][(size_t)s * gpl + p] == tr.rJ[r];
        consistent[(size_t)s * gpl + p] = c;
    }
    (void)n_stride;
}

// trk = Jets where the round filled the position (bit 30 of the proposals' map), else 0; the segment's count of such positions is added to accepted[s]
__global__ void __launch_bounds__(kAltThreads) k_alt_filled(const int *__restrict__ map, int J, int gpl, int *__restrict__ trk, int *__restrict__ accepted) {
    const int p = blockIdx.x * kAltThreads + threadIdx.x;
    const int s = blockIdx.y / kAltK;
    bool is_new = false;
    if (p < gpl) {
        const size_t o = (size_t)blockIdx.y * gpl + p;
        const int m = map[o];
        is_new = m >= 0 && (m & kAltNew);
        trk[o] = is_new ? J : 0;
    }
    const int c = __popcll(__ballot(is_new));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(accepted + s, c);
}

// the round's node count per segment, and the chosen hypothesis' origin (255: no node)
__global__ void __launch_bounds__(kAltThreads) k_alt_chosen(const int *__restrict__ slot, const unsigned char *__restrict__ origin, int gpl, int *__restrict__ nodes,
                                                            unsigned char *__restrict__ chosen) {
    const int p = blockIdx.x * kAltThreads + threadIdx.x;
    const int s = blockIdx.y;
    bool node = false;
    if (p < gpl) {
        const int k = slot[(size_t)s * gpl + p];
        node = k >= 0;
        chosen[(size_t)s * gpl + p] = node ? origin[((size_t)s * kAltK + k) * gpl + p] : (unsigned char)255;
    }
    const int c = __popcll(__ballot(node));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(nodes + s, c);
}

}  // namespace sfa

#pragma clang attribute push(__attribute__((minsize)), apply_to = function)

using namespace sfa;

void sfa_track_alt_params_default(sfa_track_alt_params *a) {
    if (!a) return;
    *a = sfa_track_alt_params{};
    a->rounds = 5;                                                              // acc_alternate (setDefault)
    sfa_neigh_params_default(&a->neigh);
}

int sfa::alt_check(sfa_ctx *ctx, const char *fn, const sfa_track_params *p, const sfa_track_alt_params *alt, bool with_fill, int gw, int gh, TrackAlt *out) {
    if (!alt) REFUSE("%s: alt is null", fn);
    if (alt->rounds < 1) REFUSE("%s: rounds (acc_alternate) = %d < 1", fn, alt->rounds);
    if (!p->do_fuse) REFUSE("%s: do_fuse = 0: a job that alternates fuses in every round", fn);
    sfa_track_alt_params ap = *alt;
    ap.neigh.slots = with_fill ? 2 * p->K : p->K;
    ap.neigh.traj_sim_method = p->fuse.traj_sim_method;
    ap.neigh.traj_sim_thres = p->fuse.traj_sim_thres;
    SFA_TRY(neigh_check(ctx, fn, &ap.neigh, gw, gh, 0));
    if (ap.rounds > 1) SFA_TRY(neigh_check(ctx, fn, &ap.neigh, gw, gh, 1));
    if (!out) return SFA_OK;
    out->ap = ap;
    sfa_energy_params ep = p->energy;
    ep.skip = p->skip;
    ep.weight = 0.0f;                                                           // the rate's weight is added by the origin (k_neigh_rescored)
    return energy_plan(ctx, &ep, p->Jets, p->Jets, p->w, p->h, &out->plan);
}

void sfa::alt_layout(PlaneCursor &c, const sfa_track_params &p, int gw, int gh, const sfa_track_alt_params &alt, TrackPlanes *out) {
    TrackPlanes::Alt &a = out->alt;
    const size_t n = p.n, J = p.Jets, gpl = (size_t)gw * gh, R = alt.rounds;
    for (int i = 0; i < 2; i++) {
        c.take(a.U[i], n * kAltK * J * gpl); c.take(a.V[i], n * kAltK * J * gpl); c.take(a.energy[i], n * kAltK * gpl); c.take(a.occ[i], n * kAltK * gpl);
        c.take(a.origin[i], n * kAltK * gpl);
    }
    c.take(a.flags, n * gpl); c.take(a.srcpos, n * gpl); c.take(a.consistent, n * gpl); c.take(a.chosen, n * gpl);
    c.take(a.total, n * 2); c.take(a.map, n * kAltK * gpl); c.take(a.trk, n * kAltK * gpl); c.take(a.seq, n); c.take(a.E1, gpl); c.take(a.O1, gpl);
    c.take(a.P16, n * 2 * gpl * kAltK * kAltK); c.take(a.r_energy, R * n); c.take(a.r_bound, R * n); c.take(a.r_iters, R * n); c.take(a.r_nodes, R * n);
    c.take(a.r_accepted, R * n);
}

int sfa_track_job_bytes_alternate(const sfa_track_params *p, const sfa_track_fill_params *fill, const sfa_track_alt_params *alt, size_t *bytes) {
    return track_bytes(__func__, p, fill, fill != nullptr, alt, true, bytes);
}

int sfa_track_job_create_alternate(sfa_ctx *ctx, const sfa_track_params *p, const sfa_track_fill_params *fill, const sfa_track_alt_params *alt, sfa_track_job **job) {
    return track_create(ctx, __func__, p, fill, fill != nullptr, alt, true, job);
}

int sfa_track_job_set_sequence_starts(sfa_track_job *job, const unsigned *sequence_start) {
    TRACK_JOB(job);
    if (!job->alt) REFUSE("%s: the job does not alternate (sfa_track_job_create_alternate)", __func__);
    if (!sequence_start) REFUSE("%s: sequence_start is null", __func__);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(copy_on(ctx, job->ptr(job->at.alt.seq), sequence_start, (size_t)p.n * sizeof(unsigned), hipMemcpyHostToDevice));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));                            // the caller's array is free on return
    return SFA_OK;
}

static NeighPlanes alt_lists(const sfa_track_job *job, int i) {
    const TrackPlanes::Alt &a = job->at.alt;
    return NeighPlanes{job->ptr(a.U[i]), job->ptr(a.V[i]), job->ptr(a.energy[i]), job->ptr(a.occ[i]), job->ptr(a.origin[i])};
}

int sfa::track_run_alternation(sfa_track_job *job, int ns) {
    TRACK_JOB(job);
    const TrackPlanes &at = job->at;
    const TrackPlanes::Alt &a = at.alt;
    TrackAlt &alt = *job->alt;
    const sfa_neigh_params &np = alt.ap.neigh;
    const int S = job->slots(), J = p.Jets, R = alt.ap.rounds, gw = job->gw, gh = job->gh;
    const dim3 pix((unsigned)((gpl + kAltThreads - 1) / kAltThreads), (unsigned)ns), pos(pix.x, (unsigned)(ns * kAltK));
    // ---- the job's slots as lists: set 0
    int cur = 0;
    NeighPlanes L = alt_lists(job, 0);
    SFA_TRY(zero_on(ctx, L.U, (size_t)ns * kAltK * J * gpl * 8));
    SFA_TRY(zero_on(ctx, L.V, (size_t)ns * kAltK * J * gpl * 8));
    SFA_TRY(copy_rows_on(ctx, L.U, (size_t)kAltK * J * gpl * 8, job->ptr(at.aU), (size_t)S * J * gpl * 8, (size_t)S * J * gpl * 8, ns, hipMemcpyDeviceToDevice));
    SFA_TRY(copy_rows_on(ctx, L.V, (size_t)kAltK * J * gpl * 8, job->ptr(at.aV), (size_t)S * J * gpl * 8, (size_t)S * J * gpl * 8, ns, hipMemcpyDeviceToDevice));
    AltTracked tr{};
    tr.K = p.K;
    for (int r = 0; r < p.K; r++) { tr.t[r] = job->ptr(at.rate[r].tracked); tr.rJ[r] = p.r_Jets[r]; }
    hipLaunchKernelGGL(k_alt_lists, pos, dim3(kAltThreads), 0, ctx->stream, job->ptr(at.E), job->ptr(at.O), S, (int)gpl, 0, tr, L.energy, L.occ, L.origin,
                       job->ptr(a.consistent));
    SFA_HIP(ctx, hipGetLastError());
    SFA_TRY(zero_on(ctx, job->ptr(a.r_nodes), (size_t)R * p.n * 4));
    SFA_TRY(zero_on(ctx, job->ptr(a.r_accepted), (size_t)R * p.n * 4));
    // ---- what every round uses
    const NeighWork wk{job->ptr(a.flags), job->ptr(a.srcpos), job->ptr(a.total), job->ptr(a.map)};
    NeighWeights wt{};
    for (int k = 0; k < S; k++) wt.w[k] = p.weight[k / job->step()];
    const TrackPlanes::Rate &mf = at.rate[p.min_fps_idx];
    unsigned char todo[64 * kAltK];                                             // kTrMaxN start_jets: every position a list may reach
    sfa_fuse_params fp = p.fuse;
    FuseWork fw = fuse_work(job);
    fw.P = job->ptr(a.P16);
    for (int r = 0; r < R; r++) {
        if (r > 0) {
            SFA_TRY(neigh_prune_device(ctx, ns, J, gw, gh, np.perturb_keep, job->ptr(at.slot), alt_lists(job, cur), alt_lists(job, cur ^ 1), wk.map, nullptr));
            cur ^= 1;
        }
        SFA_TRY(neigh_propose_device(ctx, &np, ns, J, gw, gh, r, job->ptr(a.seq), job->ptr(a.consistent), alt_lists(job, cur), alt_lists(job, cur ^ 1), wk, nullptr));
        cur ^= 1;
        hipLaunchKernelGGL(k_alt_filled, pos, dim3(kAltThreads), 0, ctx->stream, wk.map, J, (int)gpl, job->ptr(a.trk), job->ptr(a.r_accepted) + (size_t)r * p.n);
        SFA_HIP(ctx, hipGetLastError());
        const int reach = (r == 0 ? S : np.perturb_keep + 1) + 2 * np.neigh_hyp;  // <= 16 (alt_check)
        for (int s = 0; s < ns; s++)
            for (int k = 0; k < kAltK; k++) todo[s * kAltK + k] = k < reach;
        L = alt_lists(job, cur);
        SFA_TRY(neigh_rescore_device(ctx, alt.plan, ns, job->ptr(a.trk), todo, job->ptr(at.rec), job->identity[p.min_fps_idx], job->ptr(mf.fw), job->ptr(mf.bw),
                                     energy_work(job), job->ptr(a.E1), job->ptr(a.O1), wt, L));
        fp.pin_first = r > 0;
        fw.U = L.U; fw.V = L.V; fw.energy = L.energy; fw.occ = L.occ;
        SFA_TRY(fuse_device(ctx, &fp, ns, kAltK, J, p.w, p.h, gw, gh, fw, job->ev + kEvFuse));
        SFA_TRY(copy_on(ctx, job->ptr(a.r_energy) + (size_t)r * p.n, fw.seg_energy, (size_t)ns * 8, hipMemcpyDeviceToDevice));
        SFA_TRY(copy_on(ctx, job->ptr(a.r_bound) + (size_t)r * p.n, fw.seg_bound, (size_t)ns * 8, hipMemcpyDeviceToDevice));
        SFA_TRY(copy_on(ctx, job->ptr(a.r_iters) + (size_t)r * p.n, fw.seg_iters, (size_t)ns * 4, hipMemcpyDeviceToDevice));
        hipLaunchKernelGGL(k_alt_chosen, pix, dim3(kAltThreads), 0, ctx->stream, fw.slot, L.origin, (int)gpl, job->ptr(a.r_nodes) + (size_t)r * p.n, job->ptr(a.chosen));
        SFA_HIP(ctx, hipGetLastError());
    }
    alt.cur = cur;
    return SFA_OK;
}

int sfa_track_job_download_alternation(sfa_track_job *job, int s, unsigned char *origin, double *energy, double *bound, int *iters, int *nodes, int *accepted) {
    TRACK_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, 0));
    if (!job->alt) REFUSE("%s: the job does not alternate (sfa_track_job_create_alternate)", __func__);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const TrackPlanes::Alt &a = job->at.alt;
    SFA_TRY(download(ctx, origin, job->ptr(a.chosen) + (size_t)s * gpl, gpl));
    for (int r = 0; r < job->alt->ap.rounds; r++) {
        const size_t o = (size_t)r * p.n + s;
        SFA_TRY(download(ctx, energy ? energy + r : nullptr, job->ptr(a.r_energy) + o, 8));
        SFA_TRY(download(ctx, bound ? bound + r : nullptr, job->ptr(a.r_bound) + o, 8));
        SFA_TRY(download(ctx, iters ? iters + r : nullptr, job->ptr(a.r_iters) + o, 4));
        SFA_TRY(download(ctx, nodes ? nodes + r : nullptr, job->ptr(a.r_nodes) + o, 4));
        SFA_TRY(download(ctx, accepted ? accepted + r : nullptr, job->ptr(a.r_accepted) + o, 4));
    }
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

#pragma clang attribute pop
