// track_fill.hip -- what a track job that fills in (sfa_track_job_create_fill) adds to the resident job of track.hip: the checks and planes of the fill-in, the
// stage between the accumulation and the energies that makes a second hypothesis per rate
//     consistent regions and matches (one host read of their counts) -> edge costs -> EpicFlow interpolation of every step's image -> trajectories
// and the fill job's own entry points.  This file holds no kernel: the steps are the device-level functions of fill.hip, epic_filter.hip and epic_batch.hip
// (sfa_internal.h) on the job's planes (track_job.h).  Compiled for size (see track.hip).
#include <algorithm>
#include <cmath>

#include "track_job.h"

#pragma clang attribute push(__attribute__((minsize)), apply_to = function)

using namespace sfa;

void sfa_track_fill_params_default(sfa_track_fill_params *fill) {
    if (!fill) return;
    *fill = sfa_track_fill_params{};
    fill->epic_skip = 2.0f;                                                     // acc_epic_skip (:651)
    fill->min_size = 100;                                                       // removeSmallSegments(r_consistent, 0.1, 100) (:1265)
    // epic_params_default (epic.cpp:127-136), then dense_tracking.cpp:652-656
    fill->epic.method = 0; fill->epic.saliency_th = 0.045f; fill->epic.pref_nn = 25; fill->epic.pref_th = 5.0f; fill->epic.nn = 160;
    fill->epic.coef_kernel = 1.1f; fill->epic.euc = 0.001f;
}

int sfa::fill_check(sfa_ctx *ctx, const char *fn, const sfa_track_params *p, const sfa_track_fill_params *f, int gw, int gh, FillGeo *g) {
    if (!f) REFUSE("%s: fill is null", fn);
    if (p->K > kTrackMaxRates / 2) REFUSE("%s: K = %d (a fill job fuses 2 K slots: at most %d rates)", fn, p->K, kTrackMaxRates / 2);
    if (f->epic.nn < 1) REFUSE("%s: epic.nn = %d (at least one neighbour)", fn, f->epic.nn);
    if (f->epic.pref_nn < 0) REFUSE("%s: epic.pref_nn = %d (0: no consistency filter, else its neighbours)", fn, f->epic.pref_nn);
    if (f->epic.method != 0 && f->epic.method != 1) REFUSE("%s: epic.method = %d (0: locally-weighted affine, 1: Nadaraya-Watson)", fn, f->epic.method);
    if (!std::isfinite(f->epic_skip) || f->epic_skip < 1) REFUSE("%s: epic_skip = %g (finite, at least 1)", fn, (double)f->epic_skip);
    if (f->min_size < 1) REFUSE("%s: min_size = %d (>= 1)", fn, f->min_size);
    if (f->epic.saliency_th != 0 && (gw <= 8 || gh <= 8))
        REFUSE("%s: gw x gh = %d x %d with epic.saliency_th != 0 (the saliency's Gaussian of sigma 1.0 needs more than 8 columns and rows)", fn, gw, gh);
    SFA_TRY(epic_nn_check_sizes(ctx, fn, gw, gh));
    if (((size_t)gw * gh * 4 * p->K * p->K + kTrackThreads - 1) / kTrackThreads > 0x7fffffffull) REFUSE("%s: grid too large for 2 K slots", fn);
    g->xs.alloc(gw); g->ys.alloc(gh);
    if (sfa_fill_samples(gw, f->epic_skip, g->xs.get(), &g->nx) != SFA_OK || sfa_fill_samples(gh, f->epic_skip, g->ys.get(), &g->ny) != SFA_OK)
        REFUSE("%s: epic_skip: %s", fn, sfa_last_error(nullptr));
    g->rJmax = 0;
    for (int r = 0; r < p->K; r++) g->rJmax = std::max(g->rJmax, p->r_Jets[r]);
    g->pitch = dev_pitch(gw);
    g->plp = (size_t)g->pitch * gh;
    g->cpl = ((size_t)gw * gh + 3) / 4 * 4;
    return SFA_OK;
}

void sfa::fill_layout(PlaneCursor &c, const sfa_track_params &p, int gw, int gh, const sfa_track_fill_params &fill, const FillGeo &g, TrackPlanes *out) {
    TrackPlanes &a = *out;
    const size_t n = p.n, K = p.K, gpl = (size_t)gw * gh, rJm = g.rJmax, samples = (size_t)g.nx * g.ny;
    if (fill.epic.saliency_th != 0) { c.take(a.lab_stage, kEpicSaliencyPlanes * g.plp); c.take(a.sal, n * g.plp); }
    c.take(a.edges, n * g.cpl); c.take(a.run_cost, n * g.cpl); c.take(a.cost, n * rJm * g.cpl);
    c.take(a.full, K * n);
    c.take(a.cT, n * gpl); c.take(a.cP, n * gpl); c.take(a.cS, n * gpl); c.take(a.mask, n * gpl); c.take(a.kept, n); c.take(a.count, n);
    c.take(a.xs, gw); c.take(a.ys, gh);
    c.take(a.block_count, n * std::max<size_t>(fill_matches_blocks(g.nx, g.ny), 1));
    c.take(a.matches, n * rJm * std::max<size_t>(samples, 1) * 4);
    c.take(a.fx, n * rJm * gpl); c.take(a.fy, n * rJm * gpl); c.take(a.inf, gpl);
    for (int r = 0; r < p.K; r++) {
        const size_t rJ = p.r_Jets[r];
        c.take(a.fill[r].u, n * rJ * gpl); c.take(a.fill[r].v, n * rJ * gpl); c.take(a.fill[r].tracked, n * gpl);
    }
}

int sfa::track_fill_create(sfa_track_job *job) {
    TRACK_JOB(job);
    const TrackPlanes &at = job->at;
    TrackFill &f = *job->fill;
    for (int r = 0; r < p.K; r++)
        for (auto &e : f.ev[r]) SFA_HIP(ctx, hipEventCreate(&e));
    SFA_HIP(ctx, hipEventCreate(&f.ev_energy));
    const size_t n = p.n, rates = (size_t)p.K * n, images = n * f.g.rJmax;
    f.full.alloc(rates);
    for (size_t k = 0; k < rates; k++) f.full[k] = p.r_Jets[k / n];
    f.stats.alloc(3 * rates);
    f.cost.alloc(images); f.matches.alloc(images); f.sal.alloc(images); f.fx.alloc(images); f.fy.alloc(images);
    f.nm.alloc(images); f.seg_of.alloc(images); f.step_of.alloc(images); f.rc.alloc(images); f.status.alloc(images);
    f.kept.alloc(n); f.count.alloc(n);
    f.inf.alloc(gpl);
    for (size_t k = 0; k < gpl; k++) f.inf[k] = (double)__builtin_inff();
    // (the host arrays live as long as the job, and the wait below is before anything can change them)
    SFA_TRY(copy_on(ctx, job->ptr(at.inf), f.inf.get(), gpl * sizeof(double), hipMemcpyHostToDevice));
    SFA_TRY(copy_on(ctx, job->ptr(at.full), f.full.get(), rates * sizeof(int), hipMemcpyHostToDevice));
    SFA_TRY(copy_on(ctx, job->ptr(at.xs), f.g.xs.get(), (size_t)job->gw * sizeof(int), hipMemcpyHostToDevice));
    SFA_TRY(copy_on(ctx, job->ptr(at.ys), f.g.ys.get(), (size_t)job->gh * sizeof(int), hipMemcpyHostToDevice));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

TrackFill::~TrackFill() {
    for (auto &rate : ev)
        for (auto &e : rate)
            if (e) (void)hipEventDestroy(e);
    if (ev_energy) (void)hipEventDestroy(ev_energy);
}

// ---- the fill-in of one rate, in four phases.  Each ends with its mark ---------------------------------------------------------------------------------------
// r_consistent after removeSmallSegments and the matches of every step; then the one host read this stage adds: kept and count of every segment
static int fill_regions_and_matches(sfa_track_job *job, int ns, int r) {
    TRACK_JOB(job);
    const TrackPlanes &at = job->at;
    TrackFill &f = *job->fill;
    const FillGeo &g = f.g;
    const bool samples = g.nx && g.ny;
    SFA_TRY(mark(ctx, f.ev[r][kFevBegin]));
    SFA_TRY(consistent_regions_device(ctx, ns, job->gw, job->gh, job->ptr(at.rate[r].tracked), job->ptr(at.full) + (size_t)r * p.n, f.fp.min_size, job->ptr(at.cT),
                                      job->ptr(at.cP), job->ptr(at.cS), job->ptr(at.mask), job->ptr(at.kept)));
    if (samples)
        SFA_TRY(fill_matches_device(ctx, ns, p.r_Jets[r], job->gw, job->gh, job->ptr(at.rate[r].acc_u), job->ptr(at.rate[r].acc_v), job->ptr(at.mask), job->ptr(at.xs),
                                    g.nx, job->ptr(at.ys), g.ny, p.skip + 1, job->ptr(at.block_count), job->ptr(at.matches), job->ptr(at.count)));
    SFA_TRY(download(ctx, f.kept.get(), job->ptr(at.kept), (size_t)ns * sizeof(int)));
    if (samples) SFA_TRY(download(ctx, f.count.get(), job->ptr(at.count), (size_t)ns * sizeof(int)));
    SFA_TRY(mark(ctx, f.ev[r][kFevMatched]));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!samples) std::fill(f.count.get(), f.count.get() + ns, 0);             // no sample on the grid: no match
    return SFA_OK;
}

// the edge costs of the rate's steps, for every segment: the calls count whether or not a rate is filled
static int fill_edge_costs(sfa_track_job *job, int ns, int r) {
    TRACK_JOB(job);
    const TrackFill &f = *job->fill;
    SFA_TRY(epic_edge_costs_device(ctx, ns, p.r_Jets[r], f.g.cpl, (int)gpl, f.fp.epic.euc, job->ptr(job->at.run_cost), job->ptr(job->at.cost)));
    return mark(ctx, f.ev[r][kFevCosts]);
}

// the interpolation of the images of every segment with a match, segment-major; stats: the rate's [n][3]
static int fill_interpolate(sfa_track_job *job, int ns, int r, int *stats) {
    TRACK_JOB(job);
    const TrackPlanes &at = job->at;
    TrackFill &f = *job->fill;
    const FillGeo &g = f.g;
    const int rJ = p.r_Jets[r];
    const size_t samples = (size_t)g.nx * g.ny;
    int m = 0;
    for (int s = 0; s < ns; s++) {
        stats[3 * s] = f.kept[s]; stats[3 * s + 1] = f.count[s]; stats[3 * s + 2] = f.count[s] > 0;
        for (int j = 0; j < rJ && f.count[s] > 0; j++, m++) {
            const size_t k = (size_t)s * rJ + j;
            f.cost[m] = job->ptr(at.cost) + k * g.cpl; f.matches[m] = job->ptr(at.matches) + k * samples * 4; f.nm[m] = f.count[s];
            f.sal[m] = f.fp.epic.saliency_th != 0 ? job->ptr(at.sal) + (size_t)s * g.plp : nullptr;
            f.fx[m] = job->ptr(at.fx) + k * gpl; f.fy[m] = job->ptr(at.fy) + k * gpl;
            f.seg_of[m] = s; f.step_of[m] = j;
        }
    }
    if (m) {
        const EpicChainDev io{f.cost.get(), f.matches.get(), f.nm.get(), f.sal.get(), f.fx.get(), f.fy.get()};
        SFA_TRY(epic_chain_device(ctx, "sfa_track_job_run", m, job->gw, job->gh, &f.fp.epic, io, f.rc.get(), nullptr, f.fp.workspace_bytes, f.status.get()));
        for (int k = 0; k < 2; k++) f.chain_runs[k] += ctx->epic_chain_runs[k];
        for (int k = 0; k < m; k++) {
            if (f.status[k])
                REFUSE("sfa_track_job_run: the fill-in image of start_jet %d, rate %d, step %d (%d matches) does not fit the interpolation's workspace even alone",
                       f.seg_of[k], r, f.step_of[k], f.nm[k]);
            if (f.rc[k] > 0) stats[3 * f.seg_of[k] + 2] = 0;                    // a step without a usable match: no fill-in hypothesis for the rate
        }
    }
    return mark(ctx, f.ev[r][kFevChain]);
}

// the planes as trajectories; a segment that is not filled gets zeros (its slot is emptied after the energies)
static int fill_trajectories(sfa_track_job *job, int ns, int r, const int *stats) {
    TRACK_JOB(job);
    const TrackPlanes &at = job->at;
    const size_t seg = (size_t)p.r_Jets[r] * gpl;
    for (int s = 0; s < ns; s++) {
        if (stats[3 * s + 2]) continue;
        SFA_TRY(zero_on(ctx, job->ptr(at.fx) + s * seg, seg * sizeof(float)));
        SFA_TRY(zero_on(ctx, job->ptr(at.fy) + s * seg, seg * sizeof(float)));
    }
    SFA_TRY(fill_trajectories_device(ctx, ns, p.r_Jets[r], job->gw, job->gh, job->gw, job->ptr(at.fx), job->ptr(at.fy), p.skip + 1, job->ptr(at.fill[r].u),
                                     job->ptr(at.fill[r].v), job->ptr(at.fill[r].tracked)));
    return mark(ctx, job->fill->ev[r][kFevTrajectories]);
}

int sfa::track_run_fill(sfa_track_job *job, int ns) {
    TRACK_JOB(job);
    TrackFill &f = *job->fill;
    // the running maps start from the maps as uploaded: a run leaves them advanced by all its calls
    SFA_TRY(copy_on(ctx, job->ptr(job->at.run_cost), job->ptr(job->at.edges), (size_t)ns * f.g.cpl * sizeof(float), hipMemcpyDeviceToDevice));
    f.chain_runs[0] = f.chain_runs[1] = 0;
    for (int r = 0; r < p.K; r++) {
        int *stats = f.stats.get() + (size_t)r * p.n * 3;
        SFA_TRY(fill_regions_and_matches(job, ns, r));
        SFA_TRY(fill_edge_costs(job, ns, r));
        SFA_TRY(fill_interpolate(job, ns, r, stats));
        SFA_TRY(fill_trajectories(job, ns, r, stats));
    }
    return mark(ctx, f.ev_energy);
}

// ---- a fill job's own entry points ------------------------------------------------------------------------------------------------------------------------
#define FILL_JOB(job) \
    TRACK_JOB(job); \
    if (!(job)->fill) REFUSE("%s: the job was not created by sfa_track_job_create_fill: it holds no fill-in", __func__); \
    const FillGeo &g = (job)->fill->g; \
    const bool saliency = (job)->fill->fp.epic.saliency_th != 0; \
    (void)g; (void)saliency

// the saliency of the Lab image in the workspace's first three planes -> segment s's plane
static int track_saliency(sfa_track_job *job, int s) {
    sfa_ctx *ctx = job->ctx;
    const FillGeo &g = job->fill->g;
    float *stage = job->ptr(job->at.lab_stage);
    const Geo geo{job->gw, job->gh, g.pitch, (long)g.plp, (long)(kEpicSaliencyPlanes * g.plp), 1, WMask::first(1), nullptr};
    epic_saliency_device(ctx, geo, stage, 0.8f, 1.0f);                          // epic()'s saliency(im, 0.8f, 1.0f)
    SFA_HIP(ctx, hipGetLastError());
    return copy_on(ctx, job->ptr(job->at.sal) + (size_t)s * g.plp, stage + (size_t)kEpicSaliencyOut * g.plp, g.plp * sizeof(float), hipMemcpyDeviceToDevice);
}

int sfa_track_job_upload_fill(sfa_track_job *job, int s, const float *lab, int lab_stride, const float *edges) {
    FILL_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, 0));
    if (!edges) REFUSE("%s: edges is null", __func__);
    if (saliency && !lab) REFUSE("%s: lab is null (epic.saliency_th != 0: the saliency filter reads the Lab image)", __func__);
    if (saliency && lab_stride < job->gw) REFUSE("%s: lab_stride = %d < gw = %d", __func__, lab_stride, job->gw);
    SFA_TRY(epic_check_costs(ctx, __func__, "edges of start_jet %d", s, edges, job->gw, job->gh));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    if (saliency) {
        for (int c = 0; c < 3; c++)
            SFA_TRY(upload_plane(ctx, job->ptr(job->at.lab_stage) + (size_t)c * g.plp, g.pitch, lab + (size_t)c * job->gh * lab_stride, lab_stride, job->gw, job->gh));
        SFA_TRY(track_saliency(job, s));
    }
    SFA_TRY(copy_on(ctx, job->ptr(job->at.edges) + (size_t)s * g.cpl, edges, gpl * sizeof(float), hipMemcpyHostToDevice));
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
        // packed into planes the saliency only uses as scratch, then row by row to the device pitch
        float *stage = job->ptr(job->at.lab_stage), *packed = stage + 3 * g.plp;
        SFA_TRY(pack_strided_planes(ctx, lab_dev + (long long)s * lab_strides[0], lab_strides[1], lab_strides[2], lab_strides[3], job->gw, job->gh, 3, packed));
        for (int c = 0; c < 3; c++)
            SFA_TRY(copy_rows_on(ctx, stage + (size_t)c * g.plp, (size_t)g.pitch * 4, packed + (size_t)c * gpl, (size_t)job->gw * 4, (size_t)job->gw * 4, job->gh,
                                 hipMemcpyDeviceToDevice));
        SFA_TRY(track_saliency(job, s0 + s));
    }
    // the edge planes stay on the device, so their domain (+0 ... +Inf, -0.0 for +0: sfa_track_job_upload_fill refuses the rest) is the caller's to guarantee
    for (int s = 0; s < ns; s++)
        SFA_TRY(pack_strided_planes(ctx, edges_dev + (long long)s * edge_strides[0], 0, edge_strides[1], edge_strides[2], job->gw, job->gh, 1,
                                    job->ptr(job->at.edges) + (size_t)(s0 + s) * g.cpl));
    return SFA_OK;
}

// frame 0 of one start_jet, in device memory at the frames' size, -> its Lab image on the grid in the saliency's workspace -> segment s's saliency
static int track_reference_saliency(sfa_track_job *job, int s, const LabSrc &src, float norm) {
    const FillGeo &g = job->fill->g;
    launch_reference_lab(job->ctx, 1, job->p.w, job->p.h, job->p.skip, src, norm, LabDst{job->ptr(job->at.lab_stage), 0, (long long)g.plp, g.pitch, 1},
                         Rgb8Dst{nullptr, 0, 0, 0, 0});
    SFA_HIP(job->ctx, hipGetLastError());
    return track_saliency(job, s);
}

int sfa_track_job_upload_fill_reference(sfa_track_job *job, int s, const float *rgb, int stride, float norm, const float *edges) {
    FILL_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, 0));
    if (!edges) REFUSE("%s: edges is null", __func__);
    if (saliency && !rgb) REFUSE("%s: rgb is null (epic.saliency_th != 0: the saliency filter reads the Lab image)", __func__);
    if (saliency && stride < p.w) REFUSE("%s: stride = %d < w = %d", __func__, stride, p.w);
    if (!(norm == norm)) REFUSE("%s: norm is NaN", __func__);
    int gw = 0, gh = 0;
    SFA_TRY(reference_check(ctx, __func__, p.w, p.h, p.skip, &gw, &gh));
    SFA_TRY(epic_check_costs(ctx, __func__, "edges of start_jet %d", s, edges, job->gw, job->gh));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    if (saliency) {
        DevMem &stage = job->fill->ref_stage;                                   // the frame as read: made by the first call, gone with the job
        if (!stage.p) SFA_TRY(stage.alloc(ctx, 3 * pl * sizeof(float)));
        for (int c = 0; c < 3; c++) SFA_TRY(upload_plane(ctx, stage.f() + c * pl, p.w, rgb + (size_t)c * p.h * stride, stride, p.w, p.h));
        SFA_TRY(track_reference_saliency(job, s, LabSrc{stage.f(), 0, (long long)pl, p.w, 1}, norm));
    }
    SFA_TRY(copy_on(ctx, job->ptr(job->at.edges) + (size_t)s * g.cpl, edges, gpl * sizeof(float), hipMemcpyHostToDevice));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));                            // the caller's planes are free again
    return SFA_OK;
}

int sfa_track_job_upload_fill_reference_device(sfa_track_job *job, int s0, int ns, const float *rgb_dev, const long long strides[4], float norm,
                                               const float *edges_dev, const long long edge_strides[3]) {
    FILL_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s0, ns, 0));
    if (!(norm == norm)) REFUSE("%s: norm is NaN", __func__);
    int gw = 0, gh = 0;
    SFA_TRY(reference_check(ctx, __func__, p.w, p.h, p.skip, &gw, &gh));
    if (saliency) SFA_TRY(check_view(ctx, __func__, View{"rgb_dev", rgb_dev, sizeof(float), 4, {ns, 3, p.h, p.w}, strides}, 0));
    SFA_TRY(check_view(ctx, __func__, View{"edges_dev", edges_dev, sizeof(float), 3, {ns, job->gh, job->gw}, edge_strides}));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    for (int s = 0; saliency && s < ns; s++)                                    // segment by segment through the one workspace, in stream order
        SFA_TRY(track_reference_saliency(job, s0 + s, LabSrc{rgb_dev + (long long)s * strides[0], 0, strides[1], strides[2], strides[3]}, norm));
    // (the edge planes' domain is the caller's to guarantee, as in sfa_track_job_upload_fill_device)
    for (int s = 0; s < ns; s++)
        SFA_TRY(pack_strided_planes(ctx, edges_dev + (long long)s * edge_strides[0], 0, edge_strides[1], edge_strides[2], job->gw, job->gh, 1,
                                    job->ptr(job->at.edges) + (size_t)(s0 + s) * g.cpl));
    return SFA_OK;
}

int sfa_track_job_download_fill(sfa_track_job *job, int s, int r, double *fill_u, double *fill_v, double *energy, unsigned long long *occ_bits, int *stats) {
    FILL_JOB(job);
    SFA_TRY(track_range(ctx, __func__, p, s, 1, r));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const size_t seg = (size_t)p.r_Jets[r] * gpl, sk = ((size_t)s * job->slots() + 2 * (size_t)r + 1) * gpl;
    SFA_TRY(download(ctx, fill_u, job->ptr(job->at.fill[r].u) + s * seg, seg * sizeof(double)));
    SFA_TRY(download(ctx, fill_v, job->ptr(job->at.fill[r].v) + s * seg, seg * sizeof(double)));
    SFA_TRY(download(ctx, energy, job->ptr(job->at.E) + sk, gpl * sizeof(double)));
    SFA_TRY(download(ctx, occ_bits, job->ptr(job->at.O) + sk, gpl * sizeof(unsigned long long)));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stats)
        for (int k = 0; k < 3; k++) stats[k] = job->fill->stats[((size_t)r * p.n + s) * 3 + k];
    return SFA_OK;
}

int sfa_track_job_fill_info(sfa_track_job *job, int info[2]) {
    FILL_JOB(job);
    if (!info) REFUSE("%s: info is null", __func__);
    if (!job->timed) REFUSE("%s: the job has not run", __func__);
    info[0] = job->fill->chain_runs[0]; info[1] = job->fill->chain_runs[1];
    return SFA_OK;
}

int sfa_track_job_fill_ms(sfa_track_job *job, float ms[4]) {
    FILL_JOB(job);
    if (!ms) REFUSE("%s: ms is null", __func__);
    if (!job->timed) REFUSE("%s: the job has not run", __func__);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // regions and matches, edge costs, interpolation, trajectories: each summed over the rates
    static const FillEvent span[4][2] = {{kFevBegin, kFevMatched}, {kFevMatched, kFevCosts}, {kFevCosts, kFevChain}, {kFevChain, kFevTrajectories}};
    for (int i = 0; i < 4; i++) ms[i] = 0;
    for (int r = 0; r < p.K; r++)
        for (int i = 0; i < 4; i++) {
            float v = 0;
            SFA_HIP(ctx, hipEventElapsedTime(&v, job->fill->ev[r][span[i][0]], job->fill->ev[r][span[i][1]]));
            ms[i] += v;
        }
    return SFA_OK;
}

#pragma clang attribute pop
