// epic_init.hip -- EpicFlow's initialisation on resident data (include/slowflow_amd.h: sfa_rgb8_to_lab_device, sfa_sequence_lab, sfa_epic_job_*; the
// kernel behind sfa_job_set_flow_epic, whose entry point is job.hip's): what stood between frames in GPU memory and sfa_epic_batch's chain on one side,
// and between the chain's field and a job's initial flow on the other.
//   k_rgb8_to_lab            rgb8_to_lab (host/epic.cpp:19-28, 57-73) per pixel: csrc/lab_math.h, the function tests/host/test_lab_math.cpp walks over its
//                            whole domain on the CPU.  fp64 arithmetic on a few values per pixel; the kernel runs once per reference frame
//   k_epic_cost_pack         a strided cost map -> the chain's packed plane, euc added once in fp32 (epic.cpp:155-163)
//   k_epic_flow_mul          epic_to_initial_flow (host/slow_flow.cpp:530-546) for fields of the job's size: image_mul_scalar's product; other sizes go
//                            through k_resize (kernels.hip) with that product as its post_scale
//   k_epic_flow_unpack       the packed fields -> the caller's strided tensor
// The job keeps packed w x h planes for the chain (epic_chain_device reads and writes those) and planes at the device pitch for the saliency.
#include <algorithm>
#include <climits>
#include <cmath>

#include "lab_math.h"
#include "sfa_internal.h"

namespace sfa {
namespace {

constexpr int kEiThreads = 256;                                      // one row segment per block: consecutive lanes, consecutive columns
constexpr int kMaxEpicJobImages = 4096;                              // epic_batch.hip: images per launch
constexpr int kStageImages = 8;                                      // Lab images whose saliency is formed at once: bounds the work planes to 8 x 15

inline dim3 row_grid(int w, int h, int planes) { return dim3((w + kEiThreads - 1) / kEiThreads, h, planes); }

__global__ void __launch_bounds__(kEiThreads) k_rgb8_to_lab(LabSrc s, LabDst d, int w, float norm) {
    const int x = blockIdx.x * kEiThreads + threadIdx.x, y = blockIdx.y, i = blockIdx.z;
    if (x >= w) return;
    const float *p = s.p + (long long)i * s.sn + (long long)y * s.sr + (long long)x * s.sx;
    float L, a, b;
    lab::rgb8_to_lab_pixel(p[0], p[s.sc], p[2 * s.sc], norm, &L, &a, &b);
    float *q = d.p + (long long)i * d.sn + (long long)y * d.sr + (long long)x * d.sx;
    q[0] = L; q[d.sc] = a; q[2 * d.sc] = b;
}

// image blockIdx.z: dst packed w x h, dst_es apart; src at (image, row, column) strides.  In place (src == dst, the same strides) is fine: one element per thread
__global__ void __launch_bounds__(kEiThreads) k_epic_cost_pack(float *dst, long dst_es, const float *src, long long sn, long long sr, long long sx, int w, float euc) {
    const int x = blockIdx.x * kEiThreads + threadIdx.x, y = blockIdx.y, i = blockIdx.z;
    if (x >= w) return;
    float v = src[(long long)i * sn + (long long)y * sr + (long long)x * sx];
    if (euc != 0.0f) v += euc;                                       // `if (params->euc) c += params->euc`
    dst[(long)i * dst_es + (long)y * w + x] = v;
}

// fields of the job's own size: plane blockIdx.z & 1 of window blockIdx.z >> 1 times mul_u / mul_v, one fp32 multiplication (image_mul_scalar, :545-546)
__global__ void __launch_bounds__(kEiThreads) k_epic_flow_mul(float *__restrict__ dst, long dst_es, long pl, int pitch, int w, const float *__restrict__ src_u,
                                                             const float *__restrict__ src_v, long src_es, float mul_u, float mul_v) {
    const int x = blockIdx.x * kEiThreads + threadIdx.x, y = blockIdx.y, p = blockIdx.z & 1, wi = blockIdx.z >> 1;
    if (x >= w) return;
    dst[(long)wi * dst_es + (long)p * pl + (size_t)y * pitch + x] = (p ? src_v : src_u)[(long)wi * src_es + (size_t)y * w + x] * (p ? mul_v : mul_u);
}

__global__ void __launch_bounds__(kEiThreads) k_epic_flow_unpack(float *dst, long long sn, long long sp, long long sr, long long sx, const float *src, long src_es, long npix,
                                                                int w) {
    const int x = blockIdx.x * kEiThreads + threadIdx.x, y = blockIdx.y, p = blockIdx.z & 1, i = blockIdx.z >> 1;
    if (x >= w) return;
    dst[(long long)i * sn + (long long)p * sp + (long long)y * sr + (long long)x * sx] = src[(long)i * src_es + (long)p * npix + (long)y * w + x];
}

// what follows holds no kernel: checks, copies and launches.  Compiled for size (see track.hip)
#pragma clang attribute push(__attribute__((minsize)), apply_to = function)

// images [i0, i0 + n) of an epic job
int job_images(sfa_ctx *ctx, const char *fn, const sfa_epic_job *j, int i0, int n) { return check_batch_range(ctx, fn, "images", i0, n, j->n); }

int check_match_count(sfa_ctx *ctx, const char *fn, const sfa_epic_job *j, int nm) {
    if (nm < 0) REFUSE("%s: nm = %d (a count of matches)", fn, nm);
    const long long list = (long long)nm * std::min(std::max(j->p.nn, j->p.pref_nn + 1), std::max(nm, 1));
    if (list > INT_MAX) REFUSE("%s: nm * nn = %lld entries (the kernels index the lists with 32 bits)", fn, list);
    return SFA_OK;
}

// image i's match list from `src` (host or device memory, by `kind`)
int set_matches(sfa_epic_job *j, int i, const float *src, int nm, hipMemcpyKind kind) {
    sfa_ctx *ctx = j->ctx;
    if (nm) {
        if (!j->matches[i]) j->matches[i].reset(new DevMem());
        if ((size_t)nm * 16 > j->matches[i]->bytes) {                // (the stream may still read the smaller list)
            SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
            SFA_TRY(j->matches[i]->alloc(ctx, (size_t)nm * 16));
        }
        SFA_TRY(copy_on(ctx, j->matches[i]->p, src, (size_t)nm * 16, kind));
    }
    j->nm[i] = nm;
    j->rc[i] = -1;
    return SFA_OK;
}

// the saliency of the m Lab images in the work planes' first three planes each -> the planes of images [i0, i0 + m)
int saliency_of_stage(sfa_epic_job *j, int i0, int m) {
    sfa_ctx *ctx = j->ctx;
    const Geo g{j->w, j->h, j->pitch, (long)j->pl, (long)(kEpicSaliencyPlanes * j->pl), m, WMask::first(m), nullptr};
    epic_saliency_device(ctx, g, j->stage.f(), 0.8f, 1.0f);          // epic()'s saliency(im, 0.8f, 1.0f)
    SFA_HIP(ctx, hipGetLastError());
    for (int k = 0; k < m; k++) {
        SFA_TRY(copy_on(ctx, j->sal.f() + (size_t)(i0 + k) * j->pl, j->stage.f() + ((size_t)k * kEpicSaliencyPlanes + kEpicSaliencyOut) * j->pl, j->pl * sizeof(float),
                        hipMemcpyDeviceToDevice));
        j->have_lab[i0 + k] = 1;
        j->rc[i0 + k] = -1;
    }
    return SFA_OK;
}

}  // namespace

void launch_rgb8_to_lab(sfa_ctx *c, const LabSrc &src, const LabDst &dst, int n, int w, int h, float norm) {
    const int chunk = 32768;                                         // images in the grid's z, rows in its y (the callers hold h below 65536)
    for (int i = 0; i < n; i += chunk) {
        const LabSrc s{src.p + (long long)i * src.sn, src.sn, src.sc, src.sr, src.sx};
        const LabDst d{dst.p + (long long)i * dst.sn, dst.sn, dst.sc, dst.sr, dst.sx};
        hipLaunchKernelGGL(k_rgb8_to_lab, row_grid(w, h, std::min(chunk, n - i)), dim3(kEiThreads), 0, c->stream, s, d, w, norm);
    }
}

void launch_epic_initial_flow(sfa_ctx *c, float *dst, long dst_es, long pl, int pitch, int w, int h, int nwin, const float *src_u, const float *src_v, long src_es,
                              int sw, int sh, float mul_u, float mul_v) {
    if (sw == w && sh == h) {
        hipLaunchKernelGGL(k_epic_flow_mul, row_grid(w, h, 2 * nwin), dim3(kEiThreads), 0, c->stream, dst, dst_es, pl, pitch, w, src_u, src_v, src_es, mul_u, mul_v);
        return;
    }
    // sfa_resize_linear's kernel with its own multiplication behind it (k_resize's post_scale: the same single fp32 product), a plane at a time: the packed
    // field is a source of pitch sw
    launch_resize(c, dst, w, h, pitch, pl, dst_es, src_u, sw, sh, sw, 0, src_es, 1, nwin, mul_u);
    launch_resize(c, dst + pl, w, h, pitch, pl, dst_es, src_v, sw, sh, sw, 0, src_es, 1, nwin, mul_v);
}

}  // namespace sfa

using namespace sfa;

extern "C" {

int sfa_rgb8_to_lab_device(sfa_ctx *ctx, int n, int w, int h, const float *rgb_dev, const long long rgb_strides[4], float norm, float *lab_dev,
                           const long long lab_strides[4]) {
    CHECK_ARGS(ctx, "ctx is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    if (n < 1) REFUSE("%s: n = %d images", __func__, n);
    if (w < 1 || h < 1 || h > 65535) REFUSE("%s: w x h = %d x %d (both at least 1, h at most 65535: a row per block)", __func__, w, h);
    if (!(norm == norm)) REFUSE("%s: norm is NaN", __func__);
    const View from{"rgb_dev", rgb_dev, sizeof(float), 4, {n, 3, h, w}, rgb_strides}, to{"lab_dev", lab_dev, sizeof(float), 4, {n, 3, h, w}, lab_strides};
    SFA_TRY(check_view(ctx, __func__, from, 0));
    SFA_TRY(check_view(ctx, __func__, to));
    if (!strides_nest(lab_strides, to.n, 4)) REFUSE("%s: lab_strides let images, channels or rows of lab_dev share memory (or interleave them in a way the check cannot clear)", __func__);
    SFA_TRY(check_disjoint(ctx, __func__, {to, from}, "a block may write a pixel's Lab values before another has read its samples"));
    launch_rgb8_to_lab(ctx, LabSrc{rgb_dev, rgb_strides[0], rgb_strides[1], rgb_strides[2], rgb_strides[3]},
                       LabDst{lab_dev, lab_strides[0], lab_strides[1], lab_strides[2], lab_strides[3]}, n, w, h, norm);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_sequence_lab(sfa_sequence *dq, int f_dst, sfa_sequence *sq, int f_src, int n, float norm) {
    sfa_ctx *ctx = dq ? dq->ctx : (sq ? sq->ctx : nullptr);
    CHECK_ARGS(dq, "dst_seq is null");
    CHECK_ARGS(sq, "src_seq is null");
    if (sq->ctx != ctx) REFUSE("%s: src_seq lives on another context than dst_seq: one stream orders the frames before their Lab images", __func__);
    if (dq->w != sq->w || dq->h != sq->h) REFUSE("%s: dst_seq is %d x %d, src_seq %d x %d: the Lab image has its frame's size", __func__, dq->w, dq->h, sq->w, sq->h);
    if (!(norm == norm)) REFUSE("%s: norm is NaN", __func__);
    if (n < 1 || f_src < 0 || (long)f_src + n > sq->n) REFUSE("%s: frames f_src = %d, n = %d lie outside src_seq of %d", __func__, f_src, n, sq->n);
    if (f_dst < 0 || (long)f_dst + n > dq->n) REFUSE("%s: frames f_dst = %d, n = %d lie outside dst_seq of %d", __func__, f_dst, n, dq->n);
    if (sq == dq && f_dst < f_src + n && f_src < f_dst + n) REFUSE("%s: dst_seq is src_seq and the frames [%d, %d) overlap [%d, %d)", __func__, f_dst, f_dst + n, f_src, f_src + n);
    if (sq->h > 65535) REFUSE("%s: h = %d (at most 65535: a row per block)", __func__, sq->h);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    launch_rgb8_to_lab(ctx, LabSrc{sq->frame(f_src), 3 * (long long)sq->pl, sq->pl, sq->pitch, 1}, LabDst{dq->frame(f_dst), 3 * (long long)dq->pl, dq->pl, dq->pitch, 1}, n,
                       sq->w, sq->h, norm);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_epic_job_create(sfa_ctx *ctx, const sfa_epic_params *p, int w, int h, int n, sfa_epic_job **out) {
    const char *fn = __func__;
    if (!ctx) return set_error(nullptr, SFA_ERR_ARG, "%s: ctx is null", fn);
    if (!p || !out) REFUSE("%s: %s is null", fn, !p ? "params" : "out");
    *out = nullptr;
    if (n < 1 || n > kMaxEpicJobImages) REFUSE("%s: n = %d (1 .. %d images)", fn, n, kMaxEpicJobImages);
    if (w < 1 || h < 1 || h > 65535) REFUSE("%s: w x h = %d x %d (both at least 1, h at most 65535: a row per block)", fn, w, h);
    if (p->nn < 1) REFUSE("%s: nn = %d (at least one neighbour)", fn, p->nn);
    if (p->pref_nn < 0) REFUSE("%s: pref_nn = %d (0: no consistency filter, else its neighbours)", fn, p->pref_nn);
    if (p->method != 0 && p->method != 1) REFUSE("%s: method = %d (0: locally-weighted affine, 1: Nadaraya-Watson)", fn, p->method);
    if (!(p->euc >= 0)) REFUSE("%s: euc = %g (the costs stay in +0 ... +Inf)", fn, (double)p->euc);
    const bool saliency = p->saliency_th != 0;
    if (saliency && (w <= 8 || h <= 8)) REFUSE("%s: w x h = %d x %d (the saliency's Gaussian of sigma 1.0 needs more than 8 columns and rows)", fn, w, h);
    SFA_TRY(epic_nn_check_sizes(ctx, fn, w, h));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<sfa_epic_job> j(new sfa_epic_job());
    j->ctx = ctx; j->p = *p; j->w = w; j->h = h; j->n = n; j->pitch = dev_pitch(w);
    j->npix = (size_t)w * h; j->pl = (size_t)j->pitch * h; j->saliency = saliency;
    SFA_TRY(j->cost.alloc(ctx, (size_t)n * j->npix * sizeof(float)));
    SFA_TRY(j->flow.alloc(ctx, (size_t)n * 2 * j->npix * sizeof(float)));
    SFA_HIP(ctx, hipMemsetAsync(j->flow.p, 0, (size_t)n * 2 * j->npix * sizeof(float), ctx->stream));
    if (saliency) {
        j->stage_images = std::min(n, kStageImages);
        SFA_TRY(j->sal.alloc(ctx, (size_t)n * j->pl * sizeof(float)));
        SFA_TRY(j->stage.alloc(ctx, (size_t)j->stage_images * kEpicSaliencyPlanes * j->pl * sizeof(float)));
        SFA_HIP(ctx, hipMemsetAsync(j->stage.p, 0, j->stage.bytes, ctx->stream));      // (the padding columns: never written, read by no result)
    }
    j->matches.resize(n);
    j->nm.assign(n, -1);
    j->have_cost.assign(n, 0); j->have_lab.assign(n, 0);
    j->rc.assign(n, -1);
    *out = j.release();
    return SFA_OK;
}

void sfa_epic_job_destroy(sfa_epic_job *j) {
    if (!j) return;
    (void)hipSetDevice(j->ctx->device);
    (void)hipStreamSynchronize(j->ctx->stream);
    delete j;
}

int sfa_epic_job_upload(sfa_epic_job *j, int i, const float *matches, int nm, const float *edges) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_TRY(job_images(ctx, __func__, j, i, 1));
    SFA_TRY(check_match_count(ctx, __func__, j, nm));
    if (nm && !matches) REFUSE("%s: matches is null", __func__);
    if (!edges) REFUSE("%s: edges is null", __func__);
    for (size_t k = 0; k < (size_t)4 * nm; k++)
        if (!std::isfinite(matches[k])) REFUSE("%s: matches: match %zu holds a coordinate that is not finite", __func__, k / 4);
    SFA_TRY(epic_check_costs(ctx, __func__, "edges of image %d", i, edges, j->w, j->h));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    float *cost = j->cost.f() + (size_t)i * j->npix;
    SFA_TRY(copy_on(ctx, cost, edges, j->npix * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_epic_cost_pack, row_grid(j->w, j->h, 1), dim3(kEiThreads), 0, ctx->stream, cost, 0L, cost, 0LL, (long long)j->w, 1LL, j->w, j->p.euc);
    SFA_HIP(ctx, hipGetLastError());
    j->have_cost[i] = 1;
    SFA_TRY(set_matches(j, i, matches, nm, hipMemcpyHostToDevice));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));                 // host buffers may go away after the call
    return SFA_OK;
}

int sfa_epic_job_set_matches_device(sfa_epic_job *j, int i, const float *matches_dev, int nm) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(job_images(ctx, __func__, j, i, 1));
    SFA_TRY(check_match_count(ctx, __func__, j, nm));
    if (nm) {
        const long long st[2] = {4, 1};
        SFA_TRY(check_view(ctx, __func__, View{"matches_dev", matches_dev, sizeof(float), 2, {nm, 4}, st}));
    }
    return set_matches(j, i, matches_dev, nm, hipMemcpyDeviceToDevice);
}

int sfa_epic_job_set_lab(sfa_epic_job *j, int i0, int n, const sfa_sequence *q, const int *frame_index) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_TRY(job_images(ctx, __func__, j, i0, n));
    if (!q || !frame_index) REFUSE("%s: %s is null", __func__, !q ? "lab_seq" : "frame_index");
    if (q->ctx->device != ctx->device) REFUSE("%s: lab_seq lives on GPU %d, the job on GPU %d", __func__, q->ctx->device, ctx->device);
    if (q->w != j->w || q->h != j->h) REFUSE("%s: lab_seq is %d x %d, the job's images %d x %d", __func__, q->w, q->h, j->w, j->h);
    for (int k = 0; k < n; k++)
        if (frame_index[k] < 0 || frame_index[k] >= q->n) REFUSE("%s: frame_index[%d] = %d lies outside lab_seq of %d", __func__, k, frame_index[k], q->n);
    if (!j->saliency) return SFA_OK;                                 // epic() reads the image for its saliency only
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    for (int k0 = 0; k0 < n; k0 += j->stage_images) {
        const int m = std::min(j->stage_images, n - k0);
        for (int k = 0; k < m; k++)                                  // (a sequence's planes have the job's pitch: whole planes)
            SFA_TRY(copy_on(ctx, j->stage.f() + (size_t)k * kEpicSaliencyPlanes * j->pl, q->frame(frame_index[k0 + k]), 3 * j->pl * sizeof(float), hipMemcpyDeviceToDevice));
        SFA_TRY(saliency_of_stage(j, i0 + k0, m));
    }
    return SFA_OK;
}

int sfa_epic_job_upload_device(sfa_epic_job *j, int i0, int n, const float *lab_dev, const long long lab_strides[4], const float *cost_dev, const long long cost_strides[3],
                               int cost_has_euc) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(job_images(ctx, __func__, j, i0, n));
    if (!lab_dev && !cost_dev) REFUSE("%s: lab_dev and cost_dev are both null", __func__);
    if (j->h > 65535) REFUSE("%s: h = %d (at most 65535: a row per block)", __func__, j->h);
    if (lab_dev) SFA_TRY(check_view(ctx, __func__, View{"lab_dev", lab_dev, sizeof(float), 4, {n, 3, j->h, j->w}, lab_strides}, 0));
    if (cost_dev) SFA_TRY(check_view(ctx, __func__, View{"cost_dev", cost_dev, sizeof(float), 3, {n, j->h, j->w}, cost_strides}, 0));
    if (cost_dev) {
        for (int k0 = 0; k0 < n; k0 += 32768)
            hipLaunchKernelGGL(k_epic_cost_pack, row_grid(j->w, j->h, std::min(32768, n - k0)), dim3(kEiThreads), 0, ctx->stream, j->cost.f() + (size_t)(i0 + k0) * j->npix,
                               (long)j->npix, cost_dev + (long long)k0 * cost_strides[0], cost_strides[0], cost_strides[1], cost_strides[2], j->w, cost_has_euc ? 0.0f : j->p.euc);
        SFA_HIP(ctx, hipGetLastError());
        for (int k = 0; k < n; k++) { j->have_cost[i0 + k] = 1; j->rc[i0 + k] = -1; }
    }
    if (lab_dev && j->saliency) {
        for (int k0 = 0; k0 < n; k0 += j->stage_images) {
            const int m = std::min(j->stage_images, n - k0);
            const PackSrc src{lab_dev + (long long)k0 * lab_strides[0], SFA_DEV_F32, lab_strides[0], 0, lab_strides[1], lab_strides[2], lab_strides[3]};
            launch_pack_frames(ctx, j->stage.f(), (long)(kEpicSaliencyPlanes * j->pl), (long)j->pl, j->pitch, j->w, j->h, m, 1, src);
            SFA_HIP(ctx, hipGetLastError());
            SFA_TRY(saliency_of_stage(j, i0 + k0, m));
        }
    }
    return SFA_OK;
}

int sfa_epic_job_run(sfa_epic_job *j, int n, int *rc, int (*counts)[3], size_t workspace_bytes, int *status) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_TRY(job_images(ctx, __func__, j, 0, n));
    if (!rc || !status) REFUSE("%s: %s is null", __func__, !rc ? "rc" : "status");
    for (int i = 0; i < n; i++) {
        if (j->nm[i] < 0) REFUSE("%s: image %d has no matches yet (sfa_epic_job_upload, sfa_epic_job_set_matches_device)", __func__, i);
        if (!j->have_cost[i]) REFUSE("%s: image %d has no cost map yet (sfa_epic_job_upload, sfa_epic_job_upload_device)", __func__, i);
        if (j->saliency && !j->have_lab[i]) REFUSE("%s: image %d has no Lab image yet (saliency_th != 0: sfa_epic_job_set_lab, sfa_epic_job_upload_device)", __func__, i);
    }
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<const float *> cost(n), matches(n), sal(n);
    std::vector<float *> fx(n), fy(n);
    for (int i = 0; i < n; i++) {
        cost[i] = j->cost.f() + (size_t)i * j->npix;
        matches[i] = j->nm[i] ? j->matches[i]->f() : nullptr;
        sal[i] = j->saliency ? j->sal.f() + (size_t)i * j->pl : nullptr;
        fx[i] = j->u(i); fy[i] = j->v(i);
        j->rc[i] = -1;
    }
    const EpicChainDev io{cost.data(), matches.data(), j->nm.data(), sal.data(), fx.data(), fy.data()};
    SFA_TRY(epic_chain_device(ctx, __func__, n, j->w, j->h, &j->p, io, rc, counts, workspace_bytes, status));
    for (int i = 0; i < n; i++) {
        if (status[i]) continue;
        if (rc[i] > 0) SFA_HIP(ctx, hipMemsetAsync(j->u(i), 0, 2 * j->npix * sizeof(float), ctx->stream));   // no match (left): the window starts from zero
        j->rc[i] = rc[i];
    }
    return SFA_OK;
}

int sfa_epic_job_upload_flow(sfa_epic_job *j, int i, const float *fx, const float *fy, int stride) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_TRY(job_images(ctx, __func__, j, i, 1));
    if (!fx || !fy) REFUSE("%s: %s is null", __func__, !fx ? "fx" : "fy");
    if (stride < j->w) REFUSE("%s: stride = %d (at least w = %d)", __func__, stride, j->w);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(upload_plane(ctx, j->u(i), j->w, fx, stride, j->w, j->h));
    SFA_TRY(upload_plane(ctx, j->v(i), j->w, fy, stride, j->w, j->h));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));                 // host buffers may go away after the call
    j->rc[i] = 0;
    return SFA_OK;
}

int sfa_epic_job_download(sfa_epic_job *j, int i, float *fx, float *fy, int stride) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_TRY(job_images(ctx, __func__, j, i, 1));
    if (!fx || !fy) REFUSE("%s: %s is null", __func__, !fx ? "fx" : "fy");
    if (stride < j->w) REFUSE("%s: stride = %d (at least w = %d)", __func__, stride, j->w);
    if (j->rc[i] < 0) REFUSE("%s: image %d holds no field (not run since its inputs changed, or flagged by the run)", __func__, i);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(download_plane(ctx, fx, stride, j->u(i), j->w, j->w, j->h));
    SFA_TRY(download_plane(ctx, fy, stride, j->v(i), j->w, j->w, j->h));
    return sfa_ctx_sync(ctx);
}

int sfa_epic_job_download_device(sfa_epic_job *j, int i0, int n, float *flow_dev, const long long strides[4]) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(job_images(ctx, __func__, j, i0, n));
    if (j->h > 65535) REFUSE("%s: h = %d (at most 65535: a row per block)", __func__, j->h);
    for (int k = 0; k < n; k++)
        if (j->rc[i0 + k] < 0) REFUSE("%s: image %d holds no field (not run since its inputs changed, or flagged by the run)", __func__, i0 + k);
    const View to{"flow_dev", flow_dev, sizeof(float), 4, {n, 2, j->h, j->w}, strides};
    SFA_TRY(check_view(ctx, __func__, to));
    if (!strides_nest(strides, to.n, 4)) REFUSE("%s: strides let images, planes or rows of flow_dev share memory (or interleave them in a way the check cannot clear)", __func__);
    for (int k0 = 0; k0 < n; k0 += 16384)
        hipLaunchKernelGGL(k_epic_flow_unpack, row_grid(j->w, j->h, 2 * std::min(16384, n - k0)), dim3(kEiThreads), 0, ctx->stream, flow_dev + (long long)k0 * strides[0],
                           strides[0], strides[1], strides[2], strides[3], j->u(i0 + k0), (long)(2 * j->npix), (long)j->npix, j->w);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

}  // extern "C"

#pragma clang attribute pop
