// two_frame.hip -- the original two-frame refinement (variational.c:19-143) behind the C-ABI of include/slowflow_amd.h: sfa_variational_2frame and its
// batch on host planes, the resident pair jobs (struct sfa_pair_job: sfa_internal.h) with their device seam, and the variational() shim.  ONE launch
// sequence (enqueue_two_frame) serves all of them; the kernels are those of kernels.hip, sor*.hip and device_io.hip.
#include <memory>
#include <mutex>

#include "sfa_internal.h"

#pragma clang fp contract(off)

using namespace sfa;
typedef sfa_pair_job J;

// n pairs of w x h as one pair job, for the entry point `fn`
static int check_pair_shape(sfa_ctx *ctx, const char *fn, int w, int h, int n) {
    CHECK_ARGS_FN(fn, w >= 2 && h >= 5, "bad arguments (h >= 5, w >= 2)");
    CHECK_ARGS_FN(fn, n >= 1 && n <= kMaxBatch, "n out of range (1 .. 128 pairs)");
    // launch_update_inner leaves its per-block partials -- 2 x n x ceil(w / 64) x 16 doubles -- behind the result words of ctx->d_red, as in sfa_job_create
    CHECK_ARGS_FN(fn, 2L * kMaxBatch + 2L * n * ((w + 63) / 64) * 16 <= kRedDoubles, "n x width beyond the change norms' scratch (sfa_internal.h: kRedDoubles)");
    return SFA_OK;
}

// A job of a checked shape: one allocation and one memset.  stored_stack: the derivative stacks of the n pairs lie behind their n x NPL planes.  The solver
// workspace is shaped here, so that enqueue_two_frame only enqueues: the two-frame path has no break decision, nothing needs the host.
static int pair_job_new(sfa_ctx *ctx, const sfa_params_2frame *pp, int w, int h, int n, bool stored_stack, std::unique_ptr<J> &j) {
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    j.reset(new J());
    j->ctx = ctx; j->w = w; j->h = h; j->n = n; j->pitch = dev_pitch(w); j->stored_stack = stored_stack;
    j->pl = (long)j->pitch * h; j->es = J::NPL * j->pl;
    if (pp) j->p = *pp; else sfa_params_2frame_default(&j->p);
    const size_t bytes = (size_t)n * j->es * (stored_stack ? 2 : 1) * sizeof(float);
    SFA_TRY(j->mem.alloc(ctx, bytes));
    SFA_HIP(ctx, hipMemsetAsync(j->mem.p, 0, bytes, ctx->stream));
    if (j->p.niter_solver >= 1) SFA_TRY(j->ws.configure(ctx, w, h, j->p.niter_solver, n));     // (waits for the stream once, here and not in the first run)
    return SFA_OK;
}

// host planes <-> pair b; the copies are enqueued, the caller waits
static int pair_upload(J *j, int b, const float *wx, const float *wy, int stride, const float *im1, const float *im2) {
    SFA_TRY(upload_plane(j->ctx, j->plane(b, J::WX), j->pitch, wx, stride, j->w, j->h));
    SFA_TRY(upload_plane(j->ctx, j->plane(b, J::WY), j->pitch, wy, stride, j->w, j->h));
    for (int k = 0; k < 3; k++) {
        SFA_TRY(upload_plane(j->ctx, j->plane(b, J::IM1 + k), j->pitch, im1 + (size_t)k * stride * j->h, stride, j->w, j->h));
        SFA_TRY(upload_plane(j->ctx, j->plane(b, J::IM2 + k), j->pitch, im2 + (size_t)k * stride * j->h, stride, j->w, j->h));
    }
    return SFA_OK;
}
static int pair_download(J *j, int b, float *wx, float *wy, int stride) {
    SFA_TRY(download_plane(j->ctx, wx, stride, j->plane(b, J::WX), j->pitch, j->w, j->h));
    return download_plane(j->ctx, wy, stride, j->plane(b, J::WY), j->pitch, j->w, j->h);
}

// variational() (variational.c:19-84) for the n pairs of a job at once.  Pair b owns the planes [b * NPL, (b + 1) * NPL), so every launcher reaches it `es`
// further along (grid z = pair; launch_dpsis: im_es, launch_warp: src_es, launch_deriv_stack: es1, es2, launch_copy_planes: dst_es, src_es, the others
// g.es; sor_run: a workspace of g.nb systems).  Same per-pixel arithmetic, no cross-pair reduction that feeds back: pair b is bit-identical to the same
// pair in a job of its own.  The data term comes from a stored stack (launch_deriv_stack + launch_data_2f: the host calls, and any job under
// SFA_PAIR_UNFUSED=1) or from the image pair directly (k_data_2f_fused, same arithmetic: kernels.hip data_2f_pixel); the tests hold the two to each other.
static int enqueue_two_frame(J *j) {
    sfa_ctx *ctx = j->ctx;
    const sfa_params_2frame &p = j->p;
    const float half_alpha = 0.5f * p.alpha, hg = p.gamma * 0.5f / 3.0f, hd = p.delta * 0.5f / 3.0f;   // variational.c:113-115
    const long es = j->es;
    const Geo g = j->geo();
    auto P = [&](int i) { return j->plane(0, i); };
    // pair b's stack lies J::NPL planes after pair b - 1's, as every plane of the job does (launch_data_2f knows one batch stride): 24 = 8 derivatives x 3 channels
    static_assert(J::NPL == 24, "the stack shares the job's pair stride");
    float *stack = j->stored_stack ? j->plane(j->n, 0) : nullptr;
    if (!stack && sw_int(Switches::PAIR_UNFUSED, 0) != 0) {           // cross-check of a resident job (the release build: constant false)
        SFA_TRY(j->stack.alloc(ctx, (size_t)j->n * es * sizeof(float)));
        stack = j->stack.f();
    }
    const float zero3[3] = {0, 0, 0}, one3[3] = {1, 1, 1};
    launch_dpsis(ctx, g, P(J::DPS), P(J::IM1), es, 5.0f, zero3, one3, 0);                                // :35
    for (int outer = 0; outer < p.niter_outer; outer++) {
        launch_warp(ctx, g, P(J::WIM2), P(J::MASK), P(J::IM2), P(J::WX), P(J::WY), 1, es);               // :41
        if (stack) launch_deriv_stack(ctx, g, stack, P(J::WIM2), P(J::IM1), es, es);                     // :43 (mean of both, dt = im2 - im1)
        launch_zero_planes(ctx, g, P(J::DU), 2);                                                         // :45-46
        launch_copy_planes(ctx, g, P(J::UU), P(J::WX), 2, es, es);                                       // :48-49
        for (int inner = 0; inner < p.niter_inner; inner++) {
            launch_smoothness_2f(ctx, g, P(J::SH), P(J::SV), P(J::UU), P(J::VV), P(J::DPS), half_alpha);   // :54
            if (stack)
                launch_data_2f(ctx, g, stack, P(J::MASK), P(J::DU), P(J::DV), P(J::A11), P(J::A12), P(J::A22), P(J::B1), P(J::B2), P(J::WX), P(J::WY), P(J::SH),
                               P(J::SV), hd, hg);                                                        // :55-57
            else
                launch_data_2f_fused(ctx, g, P(J::WIM2), P(J::IM1), P(J::MASK), P(J::DU), P(J::DV), P(J::A11), P(J::A12), P(J::A22), P(J::B1), P(J::B2), P(J::WX),
                                     P(J::WY), P(J::SH), P(J::SV), hd, hg);                              // :43 + :55-57
            SFA_TRY(sor_run(ctx, j->ws, g, P(J::DU), P(J::DV), P(J::A11), P(J::A12), P(J::A22), P(J::B1), P(J::B2), P(J::SH), P(J::SV), p.niter_solver, p.sor_omega,
                            false));                                                                     // :59
            // uu = wx + du, vv = wy + dv (:62-67); the change norms of the shared kernel land in ctx->d_red and are not used here
            launch_update_inner(ctx, g, P(J::UU), P(J::VV), P(J::WX), P(J::WY), P(J::DU), P(J::DV), P(J::DU), P(J::DV), ctx->d_red);
        }
        launch_copy_planes(ctx, g, P(J::WX), P(J::UU), 2, es, es);                                       // :70-71
    }
    return SFA_OK;
}

extern "C" {

void sfa_params_2frame_default(sfa_params_2frame *p) {                                   // variational.c:86-98
    if (!p) return;
    p->alpha = 1.0f; p->gamma = 0.71f; p->delta = 0.0f; p->sigma = 1.00f;
    p->niter_outer = 5; p->niter_inner = 1; p->niter_solver = 30; p->sor_omega = 1.9f;
}

// ---- host planes: a pair job that lives for the call, its data term from the stored stack (k_deriv_stack + k_data_2f: what the pin tests on
// tests/golden/ref_two_frame.npz hold bit for bit to the compiled reference) ------------------------------------------------------------------
int sfa_variational_2frame_batch(sfa_ctx *ctx, int n, float *const *wx, float *const *wy, int w, int h, int stride, const float *const *im1,
                                 const float *const *im2, const sfa_params_2frame *pp) {
    CHECK_ARGS(ctx && wx && wy && im1 && im2 && stride >= w, "bad arguments (h >= 5, w >= 2)");
    SFA_TRY(check_pair_shape(ctx, __func__, w, h, n));
    for (int i = 0; i < n; i++) CHECK_ARGS(wx[i] && wy[i] && im1[i] && im2[i], "null plane");
    std::unique_ptr<J> j;
    SFA_TRY(pair_job_new(ctx, pp, w, h, n, true, j));
    for (int i = 0; i < n; i++) SFA_TRY(pair_upload(j.get(), i, wx[i], wy[i], stride, im1[i], im2[i]));
    SFA_TRY(enqueue_two_frame(j.get()));
    SFA_TRY(sfa_ctx_sync(ctx));                              // a solver that gave up: nothing is copied back
    for (int i = 0; i < n; i++) SFA_TRY(pair_download(j.get(), i, wx[i], wy[i], stride));
    return sfa_ctx_sync(ctx);
}

int sfa_variational_2frame(sfa_ctx *ctx, float *wx, float *wy, int w, int h, int stride, const float *im1, const float *im2, const sfa_params_2frame *pp) {
    CHECK_ARGS(ctx && wx && wy && im1 && im2 && w >= 2 && h >= 5 && stride >= w, "bad arguments (h >= 5, w >= 2)");
    return sfa_variational_2frame_batch(ctx, 1, &wx, &wy, w, h, stride, &im1, &im2, pp);
}

void variational(sfa_image *wx, sfa_image *wy, const sfa_color_image *im1, const sfa_color_image *im2, sfa_params_2frame *params) {
    static std::mutex mu;
    static sfa_ctx *def = nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!def && sfa_ctx_create(0, &def) != SFA_OK) {
        fprintf(stderr, "error in variational(): %s\n", sfa_last_error(nullptr));
        exit(1);
    }
    const bool ok = wx && wy && im1 && im2 && wx->data && wy->data && im1->c1 && im2->c1 && wy->width == wx->width && wy->height == wx->height &&
                    wy->stride == wx->stride && im1->width == wx->width && im1->height == wx->height && im1->stride == wx->stride &&
                    im2->width == wx->width && im2->height == wx->height && im2->stride == wx->stride &&
                    im1->c2 == im1->c1 + (size_t)im1->stride * im1->height && im2->c2 == im2->c1 + (size_t)im2->stride * im2->height;
    if (!ok || sfa_variational_2frame(def, wx->data, wy->data, wx->width, wx->height, wx->stride, im1->c1, im2->c1, params) != SFA_OK) {
        fprintf(stderr, "error in variational(): %s\n", ok ? sfa_last_error(def) : "images must share one geometry (color_image_new layout)");
        exit(1);
    }
}

// ---- resident pair jobs: n pairs that stay in HBM, 24 planes per pair, no stack (k_data_2f_fused) -------------------------------------------
int sfa_pair_job_create(sfa_ctx *ctx, const sfa_params_2frame *pp, int w, int h, int n, sfa_pair_job **out) {
    CHECK_ARGS(ctx && out, "ctx or out is null");
    SFA_TRY(check_pair_shape(ctx, __func__, w, h, n));
    std::unique_ptr<J> j;
    SFA_TRY(pair_job_new(ctx, pp, w, h, n, false, j));
    *out = j.release();
    return SFA_OK;
}
void sfa_pair_job_destroy(sfa_pair_job *j) {
    if (!j) return;
    (void)hipSetDevice(j->ctx->device);
    (void)hipStreamSynchronize(j->ctx->stream);
    delete j;
}
int sfa_pair_job_upload(sfa_pair_job *j, int b, const float *wx, const float *wy, int stride, const float *im1, const float *im2) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    CHECK_ARGS(b >= 0 && b < j->n, "b outside the job");
    CHECK_ARGS(wx && wy && im1 && im2, "null plane");
    CHECK_ARGS(stride >= j->w, "stride below the width");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(pair_upload(j, b, wx, wy, stride, im1, im2));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the copies read the caller's pageable memory (like sfa_job_upload)
    return SFA_OK;
}
int sfa_pair_job_run(sfa_pair_job *j) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(enqueue_two_frame(j));
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}
int sfa_pair_job_download(sfa_pair_job *j, int b, float *wx, float *wy, int stride) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    CHECK_ARGS(b >= 0 && b < j->n, "b outside the job");
    CHECK_ARGS(wx && wy, "null plane");
    CHECK_ARGS(stride >= j->w, "stride below the width");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(pair_download(j, b, wx, wy, stride));
    return sfa_ctx_sync(ctx);
}
int sfa_pair_job_download_system(sfa_pair_job *j, int b, float *a11, float *a12, float *a22, float *b1, float *b2, int stride) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    CHECK_ARGS(b >= 0 && b < j->n, "b outside the job");
    CHECK_ARGS(a11 && a12 && a22 && b1 && b2, "null plane");
    CHECK_ARGS(stride >= j->w, "stride below the width");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    float *dst[5] = {a11, a12, a22, b1, b2};
    for (int i = 0; i < 5; i++) SFA_TRY(download_plane(ctx, dst[i], stride, j->plane(b, J::A11 + i), j->pitch, j->w, j->h));
    return sfa_ctx_sync(ctx);
}

// ---- the jobs' device seam.  A pair is a window of two frames for k_pack_frames (IM1, IM2 lie next to each other in the job), its flow the planes WX, WY
// for k_pack_flow and k_unpack_planes: no kernel of its own, and sfa_job_*_device's checks.  One launch per call, nothing waits. ------------------
int sfa_pair_job_upload_device(sfa_pair_job *j, int b0, int n, const void *frames_dev, const sfa_dev_layout *l) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(check_batch_range(ctx, __func__, "pairs", b0, n, j->n));
    SFA_TRY(check_frames_source(ctx, __func__, frames_dev, l, l ? l->window : 0, n, 2, j->w, j->h));
    const PackSrc src{frames_dev, l->dtype, l->window, l->frame, l->channel, l->row, l->column};
    launch_pack_frames(ctx, j->plane(b0, J::IM1), j->es, j->pl, j->pitch, j->w, j->h, n, 2, src);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}
int sfa_pair_job_set_flow_device(sfa_pair_job *j, int b0, int n, const float *flow_dev, const long long strides[4]) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(check_batch_range(ctx, __func__, "pairs", b0, n, j->n));
    if (flow_dev) {
        SFA_TRY(check_view(ctx, __func__, View{"flow_dev", flow_dev, sizeof(float), 4, {n, 2, j->h, j->w}, strides}));
    }
    launch_pack_flow(ctx, j->plane(b0, J::WX), j->es, j->pl, j->pitch, j->w, j->h, n, flow_dev, strides);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}
int sfa_pair_job_download_device(sfa_pair_job *j, int b0, int n, float *flow_dev, const long long strides[4]) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(check_batch_range(ctx, __func__, "pairs", b0, n, j->n));
    SFA_TRY(check_download_destination(ctx, __func__, n, j->w, j->h, flow_dev, strides, nullptr, nullptr));
    launch_unpack_planes(ctx, j->plane(b0, J::WX), j->plane(b0, J::WY), nullptr, j->es, j->pitch, j->w, j->h, n, flow_dev, strides, nullptr, nullptr);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

}  // extern "C"
