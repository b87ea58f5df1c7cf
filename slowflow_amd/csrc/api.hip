// api.hip -- the C-ABI of include/slowflow_amd.h but for the jobs (job.hip: the multi-frame job; two_frame.hip: the pair jobs): context, debug switches and
// profiling hooks, the single-operator entry points with their host<->HBM staging, the SOR batch, the resident sequence, the raw Bayer ingest, and the argument checks
// of every entry point that takes device memory (check_view, check_disjoint ...: the arithmetic is dev_view.h's, what asks the HIP runtime is here).  All compute is in kernels.hip / sor*.hip / mosaic.hip; there is no CPU path.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>

#include "sfa_internal.h"

#pragma clang fp contract(off)

namespace sfa {

thread_local std::string g_thread_err;

// ---- the process-wide switch record (sfa_internal.h) ----------------------------------------------------------------
#ifndef SFA_RELEASE
Switches g_switches;
static const char *const kSwitchNames[Switches::N] = {
    "SFA_SOR_CHAIN", "SFA_SOR_BAND", "SFA_SOR_F", "SFA_SOR_CH", "SFA_SOR_LEAD", "SFA_CHAIN_LDS", "SFA_RB_TILE", "SFA_WARP_ALLJ", "SFA_NO_WARP_SMOOTH",
    "SFA_ASSEMBLE_GENERIC", "SFA_EXACT_DIV", "SFA_ASM_XCD", "SFA_NO_DIRECT_OPERANDS", "SFA_NO_UV_ALIAS", "SFA_DEBUG_ACTIVE", "SFA_UNFUSED", "SFA_SHARE_SOR",
    "SFA_PYRAMID_UNFUSED", "SFA_CUT_DISCHARGE", "SFA_CUT_INNER", "SFA_CUT_SUPER", "SFA_CUT_TAIL_INNER", "SFA_CUT_PER", "SFA_CUT_TAIL_PER", "SFA_CUT_TAIL_SUPER",
    "SFA_CUT_DEBUG", "SFA_CUT_NO_TAIL", "SFA_CUT_TAIL", "SFA_NO_EXACT_BREAK", "SFA_PAIR_UNFUSED", "SFA_EPIC_FIT_PLAIN", "SFA_EPIC_NN_SET", "SFA_EPIC_NN_SLICE"};
static int set_switch(const char *name, const char *value) {
    for (int i = 0; i < Switches::N; i++)
        if (!strcmp(name, kSwitchNames[i])) {
            g_switches.given[i] = value != nullptr;
            g_switches.value[i] = value ? atoi(value) : 0;
            if (i == Switches::EPIC_NN_SET && value) g_switches.value[i] = !strcmp(value, "sparse") ? 1 : !strcmp(value, "dense") ? 0 : -1;      // (else: no form forced)
            return SFA_OK;
        }
    return SFA_ERR_ARG;
}
// the environment is looked at ONCE per process and only behind SFA_DEBUG=1 (tools/ and the A/B scripts set it)
static void switches_from_environment() {
    static std::once_flag once;
    std::call_once(once, [] {
        const char *d = getenv("SFA_DEBUG");
        if (!d || atoi(d) == 0) return;
        for (int i = 0; i < Switches::N; i++)
            if (const char *e = getenv(kSwitchNames[i])) (void)set_switch(kSwitchNames[i], e);
    });
}
#else
static void switches_from_environment() {}      // (release build: there are no switches, sfa_internal.h)
#endif

int set_error(sfa_ctx *ctx, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_thread_err = buf;
    if (ctx) ctx->err = buf;
    return code;
}

int DevMem::alloc(sfa_ctx *ctx, size_t n) {
    if (n <= bytes && p) return SFA_OK;
    release();
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) { p = nullptr; return set_error(ctx, SFA_ERR_HIP, "hipMalloc(%zu) failed: %s", n, hipGetErrorString(e)); }
    bytes = n;
    return SFA_OK;
}
void DevMem::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
}

int upload_plane(sfa_ctx *ctx, float *dev, int pitch, const float *host, int stride, int w, int h) {
    SFA_HIP(ctx, hipMemcpy2DAsync(dev, (size_t)pitch * 4, host, (size_t)stride * 4, (size_t)w * 4, h, hipMemcpyHostToDevice, ctx->stream));
    return SFA_OK;
}
int download_plane(sfa_ctx *ctx, float *host, int stride, const float *dev, int pitch, int w, int h) {
    SFA_HIP(ctx, hipMemcpy2DAsync(host, (size_t)stride * 4, dev, (size_t)pitch * 4, (size_t)w * 4, h, hipMemcpyDeviceToHost, ctx->stream));
    return SFA_OK;
}

static int check_device_error(sfa_ctx *c) {
    unsigned e = 0;
    SFA_HIP(c, hipMemcpyAsync(&e, c->d_err, sizeof e, hipMemcpyDeviceToHost, c->stream));
    SFA_HIP(c, hipStreamSynchronize(c->stream));
    if (e) {
        (void)hipMemsetAsync(c->d_err, 0, sizeof(unsigned), c->stream);
        return set_error(c, SFA_ERR_TIMEOUT, "SOR pipeline: a bounded in-kernel wait gave up (code %u)", e);
    }
    return SFA_OK;
}

// cv::getGaussianKernel(ksize, sigma, CV_32F) with ksize = cvRound(sigma*8+1)|1 (cv::GaussianBlur, Size(0,0), CV_32F)
int cv_gauss_taps(float sigma, float k[kMaxBlurTaps]) {
    if (!(sigma > 0) || !((double)sigma * 4 * 2 + 1 < 2 * kMaxBlurTaps)) return -1;     // (NaN, inf and what lrint could not hold end here)
    const int ksize = ((int)lrint((double)sigma * 4 * 2 + 1)) | 1;
    if (ksize > kMaxBlurTaps) return -1;
    const double scale2X = -0.5 / ((double)sigma * sigma);
    double sum = 0;
    for (int i = 0; i < ksize; i++) {
        const double x = i - (ksize - 1) * 0.5;
        k[i] = (float)exp(scale2X * x * x);
        sum += k[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < ksize; i++) k[i] = (float)(k[i] * sum);
    return ksize / 2;
}

}  // namespace sfa

using namespace sfa;

extern "C" {

int sfa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sfa_ctx_create(int device, sfa_ctx **out) {
    if (!out) return set_error(nullptr, SFA_ERR_ARG, "sfa_ctx_create: out is null");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_error(nullptr, SFA_ERR_NO_DEVICE, "no HIP device available: slowflow_amd has no CPU fallback");
    if (device < 0 || device >= n) return set_error(nullptr, SFA_ERR_ARG, "device %d out of range (%d devices)", device, n);
    switches_from_environment();
    std::unique_ptr<sfa_ctx> c(new sfa_ctx());
    c->device = device;
    SFA_HIP(c.get(), hipSetDevice(device));
    SFA_HIP(c.get(), hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    SFA_HIP(c.get(), hipMalloc((void **)&c->d_red, kRedDoubles * sizeof(double)));
    SFA_HIP(c.get(), hipHostMalloc((void **)&c->h_red, sizeof(LastBlock) + 64, hipHostMallocDefault));
    SFA_HIP(c.get(), hipMalloc((void **)&c->d_amask, 64));
    SFA_HIP(c.get(), hipMalloc((void **)&c->d_last, sizeof(LastBlock)));
    SFA_HIP(c.get(), hipMemset(c->d_last, 0, sizeof(LastBlock)));
    SFA_HIP(c.get(), hipHostMalloc((void **)&c->h_amask, kMaskRing * sizeof(WMask), hipHostMallocDefault));
    for (auto &e : c->ev_mask) SFA_HIP(c.get(), hipEventCreateWithFlags(&e, hipEventDisableTiming));
    SFA_HIP(c.get(), hipMalloc((void **)&c->d_err, 64));
    SFA_HIP(c.get(), hipMemset(c->d_err, 0, 64));
    SFA_HIP(c.get(), hipEventCreate(&c->t0));
    SFA_HIP(c.get(), hipEventCreate(&c->t1));
    SFA_HIP(c.get(), hipEventCreateWithFlags(&c->ev_wait, hipEventDisableTiming));
    SFA_HIP(c.get(), hipEventCreateWithFlags(&c->ev_signal, hipEventDisableTiming));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->cu_count = prop.multiProcessorCount;
    *out = c.release();
    return SFA_OK;
}

void sfa_ctx_destroy(sfa_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto e : c->ev) (void)hipEventDestroy(e);
    for (auto e : c->ev2) (void)hipEventDestroy(e);
    if (c->t0) (void)hipEventDestroy(c->t0);
    if (c->t1) (void)hipEventDestroy(c->t1);
    if (c->ev_wait) (void)hipEventDestroy(c->ev_wait);
    if (c->ev_signal) (void)hipEventDestroy(c->ev_signal);
    if (c->d_red) (void)hipFree(c->d_red);
    if (c->h_red) (void)hipHostFree(c->h_red);
    if (c->d_err) (void)hipFree(c->d_err);
    if (c->d_amask) (void)hipFree(c->d_amask);
    if (c->d_last) (void)hipFree(c->d_last);
    if (c->h_amask) (void)hipHostFree(c->h_amask);
    for (auto e : c->ev_mask) if (e) (void)hipEventDestroy(e);
    if (c->rb_tmp) (void)hipFree(c->rb_tmp);
    if (c->q_tmp) (void)hipFree(c->q_tmp);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *sfa_last_error(const sfa_ctx *c) { return c ? c->err.c_str() : g_thread_err.c_str(); }

int sfa_ctx_sync(sfa_ctx *c) {
    if (!c) return set_error(nullptr, SFA_ERR_ARG, "null context");
    SFA_HIP(c, hipSetDevice(c->device));
    return check_device_error(c);
}

void sfa_params_default(sfa_params *p) {           // slow_flow.cpp:64-128
    memset(p, 0, sizeof *p);
    p->S = 2; p->one_direction = 0; p->smoothing = 1; p->dataterm_norm = 1;
    p->niter_alter = 10; p->niter_outer = 10; p->niter_inner = 1; p->niter_solver = 30;
    p->thres_outer = 1e-5f; p->thres_inner = 1e-5f; p->sor_omega = 1.9f;
    p->alpha = 4.0f; p->gamma = 6.0f; p->delta = 1.0f;
    p->robust_color = sfa_penalty{1, 0.001f, 0.5f};
    p->robust_grad = p->robust_color; p->robust_reg = p->robust_color;
    for (int a = 0; a < SFA_MAX_REF; a++) { p->rho[a] = 1; p->omega[a] = 1; }       // variational_mt.cpp:561-568: "1.0" where the cfg names nothing ...
    p->omega[0] = 0; p->omega[1] = 2;                                               // ... and slow_flow.cpp:96-99 for the first two
    p->hbit = 1;
    for (int k = 0; k < 3; k++) { p->norm_avg[k] = 0; p->norm_std[k] = 1; }
    p->occlusion_reasoning = 1; p->layers = 1; p->p_scale = 0.9f; p->presmooth_sigma = 0;
    p->sor_order = 0;                                                                  // the reference's raster order
    p->occlusion_penalty = 0.1f; p->occlusion_alpha = 0.1f; p->niter_graphc = 10;     // slow_flow.cpp:117-118 (the class itself falls back to 1.0 / 0.5, variational_mt.cpp:189-190)
}

// ---- profiling / timing -----------------------------------------------------------------------------
int sfa_profile_enable(sfa_ctx *c, int on) {
    if (!c) return SFA_ERR_ARG;
    SFA_HIP(c, hipSetDevice(c->device));
    c->profile = on != 0;
    c->ev_used = 0;
    c->sor_bytes = 0;
    c->ev2_used = 0;
    c->asm_pixel_terms = 0;
    if (on && c->ev.empty()) {
        c->ev.resize(4096);
        for (auto &e : c->ev) SFA_HIP(c, hipEventCreate(&e));
        c->ev2.resize(4096);
        for (auto &e : c->ev2) SFA_HIP(c, hipEventCreate(&e));
    }
    return SFA_OK;
}
int sfa_profile_read_kernels(sfa_ctx *c, int *n_asm, double *asm_ms_total, double *asm_pixel_terms, char *sor_kernel, int sor_kernel_len) {
    if (!c) return SFA_ERR_ARG;
    SFA_HIP(c, hipStreamSynchronize(c->stream));
    double tot = 0;
    for (size_t i = 0; i + 1 < c->ev2_used; i += 2) {
        float ms = 0;
        SFA_HIP(c, hipEventElapsedTime(&ms, c->ev2[i], c->ev2[i + 1]));
        tot += ms;
    }
    if (n_asm) *n_asm = (int)(c->ev2_used / 2);
    if (asm_ms_total) *asm_ms_total = tot;
    if (asm_pixel_terms) *asm_pixel_terms = c->asm_pixel_terms;
    if (sor_kernel && sor_kernel_len > 0) snprintf(sor_kernel, (size_t)sor_kernel_len, "%s", c->sor_kernel);
    c->ev2_used = 0;
    c->asm_pixel_terms = 0;
    return SFA_OK;
}
int sfa_profile_read(sfa_ctx *c, int *n, double *ms_total, double *bytes_total) {
    if (!c) return SFA_ERR_ARG;
    SFA_HIP(c, hipStreamSynchronize(c->stream));
    double tot = 0;
    for (size_t i = 0; i + 1 < c->ev_used; i += 2) {
        float ms = 0;
        SFA_HIP(c, hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
        tot += ms;
    }
    if (n) *n = (int)(c->ev_used / 2);
    if (ms_total) *ms_total = tot;
    if (bytes_total) *bytes_total = c->sor_bytes;
    c->ev_used = 0;
    c->sor_bytes = 0;
    return SFA_OK;
}
int sfa_debug_set(const char *name, const char *value) {
    if (!name) return set_error(nullptr, SFA_ERR_ARG, "sfa_debug_set: null name");
#ifdef SFA_RELEASE
    (void)value;
    return set_error(nullptr, SFA_ERR_ARG, "sfa_debug_set('%s'): this is the release build of the library -- it has no cross-check / what-if paths (build the full library: make -C slowflow_amd/csrc)", name);
#else
    switches_from_environment();                    // so that a later first sfa_ctx_create cannot overwrite what is set here
    if (set_switch(name, value) != SFA_OK) return set_error(nullptr, SFA_ERR_ARG, "sfa_debug_set: unknown switch '%s'", name);
    return SFA_OK;
#endif
}
int sfa_ctx_set_epic_search(sfa_ctx *ctx, int mode) {
    if (!ctx) return set_error(nullptr, SFA_ERR_ARG, "%s: ctx is null", __func__);
    if (mode != SFA_EPIC_SEARCH_DENSE && mode != SFA_EPIC_SEARCH_COMPACT) REFUSE("%s: mode = %d (SFA_EPIC_SEARCH_DENSE = 0 or SFA_EPIC_SEARCH_COMPACT = 1)", __func__, mode);
    ctx->epic_search = mode;
    return SFA_OK;
}
int sfa_ctx_set_verbose(sfa_ctx *c, int on) {
    if (!c) return SFA_ERR_ARG;
    c->verbose_changes = on != 0;
    return SFA_OK;
}
int sfa_ctx_set_wait_bound(sfa_ctx *c, unsigned spins) {
    if (!c) return SFA_ERR_ARG;
    SFA_HIP(c, hipSetDevice(c->device));
    SFA_HIP(c, hipMemcpyAsync(c->d_err + 1, &spins, sizeof spins, hipMemcpyHostToDevice, c->stream));
    SFA_HIP(c, hipStreamSynchronize(c->stream));
    return SFA_OK;
}
int sfa_timer_start(sfa_ctx *c) {
    if (!c) return SFA_ERR_ARG;
    SFA_HIP(c, hipEventRecord(c->t0, c->stream));
    return SFA_OK;
}
int sfa_timer_stop(sfa_ctx *c, float *ms) {
    if (!c) return SFA_ERR_ARG;
    SFA_HIP(c, hipEventRecord(c->t1, c->stream));
    SFA_HIP(c, hipEventSynchronize(c->t1));
    float v = 0;
    SFA_HIP(c, hipEventElapsedTime(&v, c->t0, c->t1));
    if (ms) *ms = v;
    return SFA_OK;
}

// ---- stage entry points on host planes ------------------------------------------------------------------
struct Staging {
    sfa_ctx *c;
    DevMem mem;
    int w, h, pitch; long pl;
    float *plane(int i) { return mem.f() + (long)i * pl; }
    int init(sfa_ctx *ctx, int w_, int h_, int nplanes) {
        c = ctx; w = w_; h = h_; pitch = dev_pitch(w_); pl = (long)pitch * h_;
        SFA_HIP(c, hipSetDevice(c->device));
        SFA_TRY(mem.alloc(c, (size_t)nplanes * pl * sizeof(float)));
        SFA_HIP(c, hipMemsetAsync(mem.p, 0, (size_t)nplanes * pl * sizeof(float), c->stream));
        return SFA_OK;
    }
    Geo geo() const { return Geo{w, h, pitch, pl, 0, 1, WMask::first(1), nullptr}; }
    int up(int i, const float *host, int stride, int n = 1) {
        for (int k = 0; k < n; k++) SFA_TRY(upload_plane(c, plane(i + k), pitch, host + (size_t)k * stride * h, stride, w, h));
        return SFA_OK;
    }
    int down(float *host, int stride, int i, int n = 1) {
        for (int k = 0; k < n; k++) SFA_TRY(download_plane(c, host + (size_t)k * stride * h, stride, plane(i + k), pitch, w, h));
        return SFA_OK;
    }
};

int sfa_image_warp(sfa_ctx *ctx, float *dst3, float *mask, const float *src3, const float *wx, const float *wy, int w, int h, int stride, int factor) {
    CHECK_ARGS(ctx && dst3 && src3 && wx && wy && w > 0 && h > 0 && stride >= w, "bad arguments");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, 9));
    SFA_TRY(s.up(0, src3, stride, 3)); SFA_TRY(s.up(3, wx, stride)); SFA_TRY(s.up(4, wy, stride));
    if (mask) SFA_TRY(s.up(8, mask, stride));
    launch_warp(ctx, s.geo(), s.plane(5), mask ? s.plane(8) : nullptr, s.plane(0), s.plane(3), s.plane(4), factor, 0);
    SFA_TRY(s.down(dst3, stride, 5, 3));
    if (mask) SFA_TRY(s.down(mask, stride, 8));
    return sfa_ctx_sync(ctx);
}

int sfa_derivative_stack(sfa_ctx *ctx, float *out8x3, const float *I1, const float *I2, int w, int h, int stride) {
    CHECK_ARGS(ctx && out8x3 && I1 && I2 && w > 0 && h >= 4 && stride >= w, "bad arguments (h >= 4 needed by the 5-tap vertical filter, image.c:443)");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, 30));
    SFA_TRY(s.up(24, I1, stride, 3)); SFA_TRY(s.up(27, I2, stride, 3));
    launch_deriv_stack(ctx, s.geo(), s.plane(0), s.plane(24), s.plane(27), 0, 0);
    SFA_TRY(s.down(out8x3, stride, 0, 24));
    return sfa_ctx_sync(ctx);
}

int sfa_convolve(sfa_ctx *ctx, float *dst, const float *src, int w, int h, int stride, int order, int horizontal) {
    CHECK_ARGS(ctx && dst && src && w > 0 && h > 0 && stride >= w && (order == 1 || order == 2), "bad arguments");
    CHECK_ARGS(horizontal || h >= (order == 2 ? 4 : 2), "image too small for the vertical fast path");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, 2));
    SFA_TRY(s.up(0, src, stride));
    launch_convolve(ctx, s.geo(), s.plane(1), s.plane(0), order, horizontal, 1);
    SFA_TRY(s.down(dst, stride, 1));
    return sfa_ctx_sync(ctx);
}

int sfa_dpsis_weight(sfa_ctx *ctx, float *dst, const float *im3, int w, int h, int stride, float coef, const float avg[3], const float std_dev[3], int hbit) {
    CHECK_ARGS(ctx && dst && im3 && avg && std_dev && w > 0 && h >= 4 && stride >= w, "bad arguments");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, 4));
    SFA_TRY(s.up(0, im3, stride, 3));
    launch_dpsis(ctx, s.geo(), s.plane(3), s.plane(0), 0, coef, avg, std_dev, hbit);
    SFA_TRY(s.down(dst, stride, 3));
    return sfa_ctx_sync(ctx);
}

// computeSmoothnessWeight (dense_tracking.cpp:367-405) is compute_dpsis_weight's first output statement for statement: the same kernel
int sfa_dt_smoothness_weight(sfa_ctx *ctx, int w, int h, int stride, const float *frame0, float coef, const float avg[3], const float std_dev[3], int hbit,
                             float *out) {
    CHECK_ARGS(ctx && frame0 && avg && std_dev && out && w > 0 && h >= 4 && stride >= w, "bad arguments (w >= 1, h >= 4, stride >= w)");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, 4));
    SFA_TRY(s.up(0, frame0, stride, 3));
    launch_dpsis(ctx, s.geo(), s.plane(3), s.plane(0), 0, coef, avg, std_dev, hbit);
    SFA_TRY(s.down(out, w, 3));
    return sfa_ctx_sync(ctx);
}

int sfa_smoothness(sfa_ctx *ctx, int method, float *dst_horiz, float *dst_vert, const float *uu, const float *vv, const float *dpsis, int w, int h,
                   int stride, float alpha, const sfa_penalty *reg) {
    CHECK_ARGS(ctx && dst_horiz && dst_vert && uu && vv && dpsis && reg && w > 0 && h >= 2 && stride >= w, "bad arguments");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, 5));
    SFA_TRY(s.up(0, uu, stride)); SFA_TRY(s.up(1, vv, stride)); SFA_TRY(s.up(2, dpsis, stride));
    launch_smoothness(ctx, s.geo(), method, s.plane(3), s.plane(4), s.plane(0), s.plane(1), s.plane(2), alpha, pen(*reg));
    SFA_TRY(s.down(dst_horiz, stride, 3)); SFA_TRY(s.down(dst_vert, stride, 4));
    return sfa_ctx_sync(ctx);
}

int sfa_sub_laplacian(sfa_ctx *ctx, float *dst, const float *src, const float *wh, const float *wv, int w, int h, int stride) {
    CHECK_ARGS(ctx && dst && src && wh && wv && w > 0 && h > 0 && stride >= w, "bad arguments");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, 4));
    SFA_TRY(s.up(0, dst, stride)); SFA_TRY(s.up(1, src, stride)); SFA_TRY(s.up(2, wh, stride)); SFA_TRY(s.up(3, wv, stride));
    launch_sub_laplacian(ctx, s.geo(), s.plane(0), s.plane(1), s.plane(2), s.plane(3));
    SFA_TRY(s.down(dst, stride, 0));
    return sfa_ctx_sync(ctx);
}

int sfa_division_chain(sfa_ctx *ctx, const float *a, const float *b, float *q_chain, float *q_exact, unsigned char *admitted, size_t n) {
    CHECK_ARGS(ctx && a && b && q_chain && q_exact && admitted && n > 0, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem da, db, dq, de, dm;
    SFA_TRY(da.alloc(ctx, n * 4)); SFA_TRY(db.alloc(ctx, n * 4)); SFA_TRY(dq.alloc(ctx, n * 4)); SFA_TRY(de.alloc(ctx, n * 4)); SFA_TRY(dm.alloc(ctx, n));
    SFA_HIP(ctx, hipMemcpyAsync(da.p, a, n * 4, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(db.p, b, n * 4, hipMemcpyHostToDevice, ctx->stream));
    launch_division_chain(ctx, da.f(), db.f(), dq.f(), de.f(), (unsigned char *)dm.p, n);
    SFA_HIP(ctx, hipMemcpyAsync(q_chain, dq.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(q_exact, de.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(admitted, dm.p, n, hipMemcpyDeviceToHost, ctx->stream));
    return sfa_ctx_sync(ctx);
}

int sfa_occlusion_costs(sfa_ctx *ctx, const sfa_params *p, float *d0, float *d1, const float *const *masks, const float *const *succ1,
                        const float *const *succ2, const float *const *ref1, const float *const *ref2, int w, int h, int stride) {
    CHECK_ARGS(ctx && p && d0 && d1 && masks && succ1 && succ2 && ref1 && ref2 && w > 0 && h >= 4 && stride >= w, "bad arguments");
    CHECK_ARGS(p->S >= 2 && p->S - 1 <= SFA_MAX_REF, "unsupported slow_flow_S");
    const int ref = p->S - 1, ns = 2 * ref;
    Staging s;
    // planes: 0,1 costs; 2 .. 2+ns masks; then per slot 4 colour images
    SFA_TRY(s.init(ctx, w, h, 2 + ns + ns * 12));
    OccArgs oa;
    memset(&oa, 0, sizeof oa);
    oa.nslots = ns; oa.hd = p->delta / 3.0f; oa.hg = p->gamma / 3.0f; oa.penalty = p->occlusion_penalty;
    oa.color = pen(p->robust_color); oa.grad = pen(p->robust_grad);
    for (int k = 0; k < ns; k++) {
        const int i0 = 2 + ns + k * 12;
        SFA_TRY(s.up(2 + k, masks[k], stride));
        SFA_TRY(s.up(i0, succ1[k], stride, 3)); SFA_TRY(s.up(i0 + 3, succ2[k], stride, 3));
        SFA_TRY(s.up(i0 + 6, ref1[k], stride, 3)); SFA_TRY(s.up(i0 + 9, ref2[k], stride, 3));
        const int idx = std::max(ref - k - 1, k - ref);
        oa.slot[k] = OccSlot{i0 * s.pl, (i0 + 3) * s.pl, (i0 + 6) * s.pl, (i0 + 9) * s.pl, (2 + k) * s.pl, p->rho[idx], p->omega[idx], k >= ref ? 0 : 1};
    }
    launch_occ_costs(ctx, s.geo(), oa, s.plane(0), s.plane(0), s.plane(1), 0);
    SFA_TRY(s.down(d0, stride, 0)); SFA_TRY(s.down(d1, stride, 1));
    return sfa_ctx_sync(ctx);
}

// The cut of nb windows in the launches the job uses (optimize_occlusions, job.hip): cost and work planes packed [nb][pl]; the label planes sit in slots of
// 2 pl, as the job's sit L.es apart -- the label stride is not the plane stride.  Staged planes: [0, 2nb) label slots, then nb d0, nb d1, the work planes.
static int grid_cut_staged(sfa_ctx *ctx, const char *fn, float *occ, const float *d0, const float *d1, int nb, int w, int h, int stride, float alpha) {
    CHECK_ARGS_FN(fn, ctx, "ctx is null");
    CHECK_ARGS_FN(fn, nb >= 1 && nb <= kMaxBatch, "nb out of range (1 .. 128 windows)");
    CHECK_ARGS_FN(fn, occ, "occ is null");
    CHECK_ARGS_FN(fn, d0, "d0 is null");
    CHECK_ARGS_FN(fn, d1, "d1 is null");
    CHECK_ARGS_FN(fn, w > 0 && h > 0, "w and h must be positive");
    CHECK_ARGS_FN(fn, stride >= w, "stride is smaller than w");
    CHECK_ARGS_FN(fn, alpha >= 0, "alpha is negative (or not a number)");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, nb * (4 + kCutWorkPlanes)));
    const size_t hp = (size_t)stride * h;                        // one host plane
    const int i_d0 = 2 * nb, i_d1 = 3 * nb, i_work = 4 * nb;
    for (int b = 0; b < nb; b++) { SFA_TRY(s.up(i_d0 + b, d0 + b * hp, stride)); SFA_TRY(s.up(i_d1 + b, d1 + b * hp, stride)); }
    Geo g = s.geo();
    g.es = s.pl; g.nb = nb; g.active = WMask::first(nb);
    SFA_TRY(run_grid_cut(ctx, g, s.plane(0), 2 * s.pl, s.plane(i_d0), s.plane(i_d1), s.plane(i_work), alpha));
    for (int b = 0; b < nb; b++) SFA_TRY(s.down(occ + b * hp, stride, 2 * b));
    return sfa_ctx_sync(ctx);
}
int sfa_grid_cut(sfa_ctx *ctx, float *occ, const float *d0, const float *d1, int w, int h, int stride, float alpha) {
    return grid_cut_staged(ctx, __func__, occ, d0, d1, 1, w, h, stride, alpha);
}
int sfa_grid_cut_batch(sfa_ctx *ctx, float *occ, const float *d0, const float *d1, int nb, int w, int h, int stride, float alpha) {
    return grid_cut_staged(ctx, __func__, occ, d0, d1, nb, w, h, stride, alpha);
}

int sfa_add_data_and_match(sfa_ctx *ctx, float *a11, float *a12, float *a22, float *b1, float *b2, const float *mask, const float *du, const float *dv,
                           const float *D8x3, const float *const chw[3], int w, int h, int stride, float delta_over3, float gamma_over3, float sfac,
                           int ref_term, int dt_norm, const sfa_penalty *color, const sfa_penalty *grad) {
    CHECK_ARGS(ctx && a11 && a12 && a22 && b1 && b2 && mask && du && dv && D8x3 && color && grad && w > 0 && h > 0 && stride >= w, "bad arguments");
    if (ref_term && sfac == 0) return set_error(ctx, SFA_ERR_REF_FRAME, "Frame compared to reference frame is the reference frame itself!");
    Staging s;
    // planes: 0-4 system, 5 mask, 6 du, 7 dv, 8..31 stack, 32..34 chw
    SFA_TRY(s.init(ctx, w, h, 35));
    float *sysm[5] = {a11, a12, a22, b1, b2};
    for (int i = 0; i < 5; i++) SFA_TRY(s.up(i, sysm[i], stride));
    SFA_TRY(s.up(5, mask, stride)); SFA_TRY(s.up(6, du, stride)); SFA_TRY(s.up(7, dv, stride));
    SFA_TRY(s.up(8, D8x3, stride, 24));
    AssembleArgs aa;
    memset(&aa, 0, sizeof aa);
    aa.n = 1;
    aa.t[0] = Term{8 * s.pl, 5 * s.pl, delta_over3, gamma_over3, sfac, ref_term};
    aa.dt_norm = dt_norm; aa.color = pen(*color); aa.grad = pen(*grad);
    if (chw) {
        for (int k = 0; k < 3; k++) SFA_TRY(upload_plane(ctx, s.plane(32 + k), s.pitch, chw[k], stride, w, h));
        aa.chw = s.plane(32); aa.chw_pl = s.pl; aa.chw_es = 0; aa.chw_pitch = s.pitch; aa.chw_stride0 = stride; aa.lstride = stride;
    }
    aa.accumulate = 1; aa.do_laplacian = 0;
    launch_assemble(ctx, s.geo(), aa, s.plane(0), s.plane(0), s.plane(1), s.plane(2), s.plane(3), s.plane(4), s.plane(6), s.plane(7), nullptr, nullptr,
                    nullptr, nullptr);
    for (int i = 0; i < 5; i++) SFA_TRY(s.down(sysm[i], stride, i));
    return sfa_ctx_sync(ctx);
}

int sfa_gaussian_blur(sfa_ctx *ctx, float *dst, const float *src, int w, int h, int stride, float sigma) {
    CHECK_ARGS(ctx && dst && src && w > 0 && h > 0 && stride >= w && sigma > 0, "bad arguments");
    float taps[kMaxBlurTaps];
    CHECK_ARGS(sigma * 8 + 1 < 33, "sigma too large");
    const int r = cv_gauss_taps(sigma, taps);
    CHECK_ARGS(r >= 0, "sigma too large");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, 3));
    SFA_TRY(s.up(0, src, stride));
    SFA_TRY(launch_gauss_blur(ctx, s.geo(), s.plane(1), s.plane(2), s.plane(0), 1, taps, r));
    SFA_TRY(s.down(dst, stride, 1));
    return sfa_ctx_sync(ctx);
}

int sfa_resize_linear(sfa_ctx *ctx, float *dst, int dw, int dh, int dstride, const float *src, int sw, int sh, int sstride) {
    CHECK_ARGS(ctx && dst && src && dw > 0 && dh > 0 && sw > 0 && sh > 0 && dstride >= dw && sstride >= sw, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem a, b;
    const int sp = dev_pitch(sw), dp = dev_pitch(dw);
    SFA_TRY(a.alloc(ctx, (size_t)sp * sh * 4)); SFA_TRY(b.alloc(ctx, (size_t)dp * dh * 4));
    SFA_TRY(upload_plane(ctx, a.f(), sp, src, sstride, sw, sh));
    launch_resize(ctx, b.f(), dw, dh, dp, (long)dp * dh, 0, a.f(), sw, sh, sp, (long)sp * sh, 0, 1, 1, 1.0f);
    SFA_TRY(download_plane(ctx, dst, dstride, b.f(), dp, dw, dh));
    return sfa_ctx_sync(ctx);
}

int sfa_gaussian_presmooth(sfa_ctx *ctx, float *dst, const float *src, int w, int h, int stride, float sigma) {
    CHECK_ARGS(ctx && dst && src && w > 0 && h > 0 && stride >= w && sigma > 0, "bad arguments");
    const int order = std::max(1, (int)floor(3 * sigma) + 1);
    CHECK_ARGS(order <= 16 && w > 2 * order && h > 2 * order, "image smaller than the filter (image.c:545-574 assumes width > 2*order)");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, 3));
    SFA_TRY(s.up(0, src, stride));
    launch_presmooth(ctx, s.geo(), s.plane(1), s.plane(2), s.plane(0), 1, sigma);
    SFA_TRY(s.down(dst, stride, 1));
    return sfa_ctx_sync(ctx);
}

int sfa_resize_linear_fx(sfa_ctx *ctx, float *dst, int dw, int dh, int dstride, const float *src, int sw, int sh, int sstride, double fx, double fy) {
    CHECK_ARGS(ctx && dst && src && dw > 0 && dh > 0 && sw > 0 && sh > 0 && dstride >= dw && sstride >= sw && fx > 0 && fy > 0, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem a, b;
    const int sp = dev_pitch(sw), dp = dev_pitch(dw);
    SFA_TRY(a.alloc(ctx, (size_t)sp * sh * 4)); SFA_TRY(b.alloc(ctx, (size_t)dp * dh * 4));
    SFA_TRY(upload_plane(ctx, a.f(), sp, src, sstride, sw, sh));
    launch_resize_scaled(ctx, b.f(), dw, dh, dp, (long)dp * dh, 0, a.f(), sw, sh, sp, (long)sp * sh, 0, 1, 1, 1.0f, 1.0 / fx, 1.0 / fy);
    SFA_TRY(download_plane(ctx, dst, dstride, b.f(), dp, dw, dh));
    return sfa_ctx_sync(ctx);
}

// test hook: one pyramid step as sfa_job_run's pyramid takes it (pyramid_step, kernels.hip) on host planes: src[nb][nplanes][sh][sstride] -> dst[nb][nplanes][dh][dstride]
int sfa_pyramid_down(sfa_ctx *ctx, float *dst, int dw, int dh, int dstride, const float *src, int sw, int sh, int sstride, int nplanes, int nb, float sigma,
                     int info[3]) {
    CHECK_ARGS(ctx && dst && src && dw > 0 && dh > 0 && sw > 0 && sh > 0 && dstride >= dw && sstride >= sw, "bad arguments");
    CHECK_ARGS(nb >= 1 && nb <= kMaxBatch && nplanes >= 1 && (long)nb * nplanes <= 65535, "nb x nplanes out of range");
    float taps[kMaxBlurTaps];
    const int r = cv_gauss_taps(sigma, taps);
    if (r < 0) REFUSE("%s: sigma = %g: not a positive number, or a blur of more than %d taps", __func__, (double)sigma, kMaxBlurTaps);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem a, b;
    const int sp = dev_pitch(sw), dp = dev_pitch(dw);
    const long spl = (long)sp * sh, dpl = (long)dp * dh, ses = (nplanes + 6) * spl, des = nplanes * dpl;   // a window: its planes, then pyramid_step's scratch
    SFA_TRY(a.alloc(ctx, (size_t)nb * ses * sizeof(float))); SFA_TRY(b.alloc(ctx, (size_t)nb * des * sizeof(float)));
    SFA_HIP(ctx, hipMemsetAsync(a.p, 0, (size_t)nb * ses * sizeof(float), ctx->stream));
    SFA_HIP(ctx, hipMemsetAsync(b.p, 0, (size_t)nb * des * sizeof(float), ctx->stream));
    for (int i = 0; i < nb; i++)
        for (int k = 0; k < nplanes; k++)
            SFA_TRY(upload_plane(ctx, a.f() + i * ses + k * spl, sp, src + ((size_t)i * nplanes + k) * sstride * sh, sstride, sw, sh));
    PyrInfo pi;
    SFA_TRY(pyramid_step(ctx, b.f(), dw, dh, dp, dpl, des, a.f(), sw, sh, sp, spl, ses, nplanes, nb, taps, r, a.f() + nplanes * spl, &pi));
    for (int i = 0; i < nb; i++)
        for (int k = 0; k < nplanes; k++)
            SFA_TRY(download_plane(ctx, dst + ((size_t)i * nplanes + k) * dstride * dh, dstride, b.f() + i * des + k * dpl, dp, dw, dh));
    if (info) { info[0] = pi.fused; info[1] = pi.td; info[2] = pi.lds; }
    return sfa_ctx_sync(ctx);
}

// test hook: launch_resize_flow -- the flow's way from one pyramid level to the next, both planes, times post_x / post_y -- on host planes [nb][h][stride]
int sfa_resize_flow(sfa_ctx *ctx, float *dwx, float *dwy, int dw, int dh, int dstride, const float *swx, const float *swy, int sw, int sh, int sstride, int nb,
                    float post_x, float post_y) {
    CHECK_ARGS(ctx && dwx && dwy && swx && swy && dw > 0 && dh > 0 && sw > 0 && sh > 0 && dstride >= dw && sstride >= sw, "bad arguments");
    CHECK_ARGS(nb >= 1 && nb <= kMaxBatch, "nb out of range");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem a, b;
    const int sp = dev_pitch(sw), dp = dev_pitch(dw);
    const long spl = (long)sp * sh, dpl = (long)dp * dh;                                   // a window: its x plane, then its y plane
    SFA_TRY(a.alloc(ctx, (size_t)nb * 2 * spl * sizeof(float))); SFA_TRY(b.alloc(ctx, (size_t)nb * 2 * dpl * sizeof(float)));
    SFA_HIP(ctx, hipMemsetAsync(a.p, 0, (size_t)nb * 2 * spl * sizeof(float), ctx->stream));
    SFA_HIP(ctx, hipMemsetAsync(b.p, 0, (size_t)nb * 2 * dpl * sizeof(float), ctx->stream));
    for (int i = 0; i < nb; i++) {
        SFA_TRY(upload_plane(ctx, a.f() + i * 2 * spl, sp, swx + (size_t)i * sstride * sh, sstride, sw, sh));
        SFA_TRY(upload_plane(ctx, a.f() + i * 2 * spl + spl, sp, swy + (size_t)i * sstride * sh, sstride, sw, sh));
    }
    launch_resize_flow(ctx, b.f(), b.f() + dpl, dw, dh, dp, 2 * dpl, a.f(), a.f() + spl, sw, sh, sp, 2 * spl, nb, post_x, post_y);
    for (int i = 0; i < nb; i++) {
        SFA_TRY(download_plane(ctx, dwx + (size_t)i * dstride * dh, dstride, b.f() + i * 2 * dpl, dp, dw, dh));
        SFA_TRY(download_plane(ctx, dwy + (size_t)i * dstride * dh, dstride, b.f() + i * 2 * dpl + dpl, dp, dw, dh));
    }
    return sfa_ctx_sync(ctx);
}

// ---- SOR ----------------------------------------------------------------------------------------------------
struct sfa_sor_batch {
    sfa_ctx *ctx = nullptr;
    int w = 0, h = 0, nb = 0, pitch = 0;
    long pl = 0, es = 0;
    DevMem mem;          // nb x 9 planes: du dv a11 a12 a22 b1 b2 sh sv
    SorWorkspace ws;
    float *plane(int b, int i) const { return mem.f() + b * es + (long)i * pl; }
};

int sfa_sor_batch_create(sfa_ctx *ctx, int w, int h, int batch, sfa_sor_batch **out) {
    CHECK_ARGS(ctx && out && w > 0 && h > 0 && batch > 0 && batch <= kMaxBatch, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<sfa_sor_batch> sb(new sfa_sor_batch());
    sb->ctx = ctx; sb->w = w; sb->h = h; sb->nb = batch; sb->pitch = dev_pitch(w);
    sb->pl = (long)sb->pitch * h; sb->es = 9 * sb->pl;
    SFA_TRY(sb->mem.alloc(ctx, (size_t)batch * sb->es * sizeof(float)));
    SFA_HIP(ctx, hipMemsetAsync(sb->mem.p, 0, (size_t)batch * sb->es * sizeof(float), ctx->stream));
    *out = sb.release();
    return SFA_OK;
}
void sfa_sor_batch_destroy(sfa_sor_batch *sb) {
    if (!sb) return;
    (void)hipSetDevice(sb->ctx->device);
    (void)hipStreamSynchronize(sb->ctx->stream);
    delete sb;
}
int sfa_sor_batch_upload(sfa_sor_batch *sb, int b, const float *du, const float *dv, const float *a11, const float *a12, const float *a22, const float *b1,
                         const float *b2, const float *sh, const float *sv, int stride) {
    sfa_ctx *ctx = sb ? sb->ctx : nullptr;
    CHECK_ARGS(sb && b >= 0 && b < sb->nb && du && dv && a11 && a12 && a22 && b1 && b2 && sh && sv && stride >= sb->w, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const float *src[9] = {du, dv, a11, a12, a22, b1, b2, sh, sv};
    for (int i = 0; i < 9; i++) SFA_TRY(upload_plane(ctx, sb->plane(b, i), sb->pitch, src[i], stride, sb->w, sb->h));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}
int sfa_sor_batch_run(sfa_sor_batch *sb, int iterations, float omega) {
    sfa_ctx *ctx = sb ? sb->ctx : nullptr;
    CHECK_ARGS(sb, "null batch");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    Geo g{sb->w, sb->h, sb->pitch, sb->pl, sb->es, sb->nb, WMask::first(sb->nb), nullptr};
    return sor_run(ctx, sb->ws, g, sb->plane(0, 0), sb->plane(0, 1), sb->plane(0, 2), sb->plane(0, 3), sb->plane(0, 4), sb->plane(0, 5), sb->plane(0, 6),
                   sb->plane(0, 7), sb->plane(0, 8), iterations, omega, true);
}
int sfa_sor_batch_download(sfa_sor_batch *sb, int b, float *du, float *dv, int stride) {
    sfa_ctx *ctx = sb ? sb->ctx : nullptr;
    CHECK_ARGS(sb && b >= 0 && b < sb->nb && du && dv && stride >= sb->w, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(download_plane(ctx, du, stride, sb->plane(b, 0), sb->pitch, sb->w, sb->h));
    SFA_TRY(download_plane(ctx, dv, stride, sb->plane(b, 1), sb->pitch, sb->w, sb->h));
    return sfa_ctx_sync(ctx);
}

int sfa_sor_coupled(sfa_ctx *ctx, sfa_image *du, sfa_image *dv, sfa_image *a11, sfa_image *a12, sfa_image *a22, sfa_image *b1, sfa_image *b2,
                    sfa_image *dpsis_horiz, sfa_image *dpsis_vert, int iterations, float omega) {
    CHECK_ARGS(ctx && du && dv && a11 && a12 && a22 && b1 && b2 && dpsis_horiz && dpsis_vert, "null image");
    const int w = du->width, h = du->height, stride = du->stride;
    CHECK_ARGS(w > 0 && h > 0 && stride >= w, "bad image geometry");
    sfa_image *im[9] = {du, dv, a11, a12, a22, b1, b2, dpsis_horiz, dpsis_vert};
    for (auto *i : im) CHECK_ARGS(i->data && i->width == w && i->height == h && i->stride == stride, "images must share one geometry");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, 9));
    for (int i = 0; i < 9; i++) SFA_TRY(s.up(i, im[i]->data, stride));
    SorWorkspace ws;
    SFA_TRY(sor_run(ctx, ws, s.geo(), s.plane(0), s.plane(1), s.plane(2), s.plane(3), s.plane(4), s.plane(5), s.plane(6), s.plane(7), s.plane(8), iterations,
                    omega, true));
    SFA_TRY(s.down(du->data, stride, 0)); SFA_TRY(s.down(dv->data, stride, 1));
    if (!(w < 2 || h < 2 || iterations < 1))                                          // the fast path inverts the blocks in place (solver.c:104-106)
        for (int i = 2; i < 5; i++) SFA_TRY(s.down(im[i]->data, stride, i));
    return sfa_ctx_sync(ctx);
}

int sfa_sor_red_black(sfa_ctx *ctx, sfa_image *du, sfa_image *dv, sfa_image *a11, sfa_image *a12, sfa_image *a22, sfa_image *b1, sfa_image *b2,
                      sfa_image *dpsis_horiz, sfa_image *dpsis_vert, int iterations, float omega) {
    CHECK_ARGS(ctx && du && dv && a11 && a12 && a22 && b1 && b2 && dpsis_horiz && dpsis_vert, "null image");
    const int w = du->width, h = du->height, stride = du->stride;
    CHECK_ARGS(w > 0 && h > 0 && stride >= w, "bad image geometry");
    sfa_image *im[9] = {du, dv, a11, a12, a22, b1, b2, dpsis_horiz, dpsis_vert};
    for (auto *i : im) CHECK_ARGS(i->data && i->width == w && i->height == h && i->stride == stride, "images must share one geometry");
    Staging s;
    SFA_TRY(s.init(ctx, w, h, 9));
    for (int i = 0; i < 9; i++) SFA_TRY(s.up(i, im[i]->data, stride));
    SFA_TRY(sor_rb_run(ctx, s.geo(), s.plane(0), s.plane(1), s.plane(2), s.plane(3), s.plane(4), s.plane(5), s.plane(6), s.plane(7), s.plane(8), iterations, omega));
    for (int i = 0; i < 5; i++) SFA_TRY(s.down(im[i]->data, stride, i));
    return sfa_ctx_sync(ctx);
}

void sor_coupled(sfa_image *du, sfa_image *dv, sfa_image *a11, sfa_image *a12, sfa_image *a22, sfa_image *b1, sfa_image *b2, sfa_image *dpsis_horiz,
                 sfa_image *dpsis_vert, const int iterations, const float omega) {
    static std::mutex mu;
    static sfa_ctx *def = nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!def && sfa_ctx_create(0, &def) != SFA_OK) {
        fprintf(stderr, "error in sor_coupled(): %s\n", sfa_last_error(nullptr));
        exit(1);
    }
    if (sfa_sor_coupled(def, du, dv, a11, a12, a22, b1, b2, dpsis_horiz, dpsis_vert, iterations, omega) != SFA_OK) {
        fprintf(stderr, "error in sor_coupled(): %s\n", sfa_last_error(def));
        exit(1);
    }
}

// ---- frames resident in HBM, normalize (variational_mt.cpp:17-85) on them ------------------------------------------------------------

int sfa_sequence_create(sfa_ctx *ctx, int w, int h, int n_frames, sfa_sequence **out) {
    CHECK_ARGS(ctx && out && w > 0 && h > 0 && n_frames > 0, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<sfa_sequence> q(new sfa_sequence());
    q->ctx = ctx; q->w = w; q->h = h; q->n = n_frames; q->pitch = dev_pitch(w); q->pl = (long)q->pitch * h;
    SFA_TRY(q->mem.alloc(ctx, (size_t)n_frames * 3 * q->pl * sizeof(float)));
    SFA_HIP(ctx, hipMemsetAsync(q->mem.p, 0, (size_t)n_frames * 3 * q->pl * sizeof(float), ctx->stream));
    SFA_TRY(q->sums.alloc(ctx, (size_t)n_frames * 6 * sizeof(double)));
    *out = q.release();
    return SFA_OK;
}
void sfa_sequence_destroy(sfa_sequence *q) {
    if (!q) return;
    (void)hipSetDevice(q->ctx->device);
    (void)hipStreamSynchronize(q->ctx->stream);
    if (q->ev_mos) (void)hipEventDestroy(q->ev_mos);
    if (q->mos_stage) (void)hipHostFree(q->mos_stage);
    delete q;
}
int sfa_sequence_upload(sfa_sequence *q, int f, const float *frame3, int stride) {
    sfa_ctx *ctx = q ? q->ctx : nullptr;
    CHECK_ARGS(q && f >= 0 && f < q->n && frame3 && stride >= q->w, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    for (int k = 0; k < 3; k++) SFA_TRY(upload_plane(ctx, q->frame(f) + k * q->pl, q->pitch, frame3 + (size_t)k * stride * q->h, stride, q->w, q->h));
    // the copies read pageable host memory of the caller: wait for them, so that the buffer may be freed or reused on return (like sfa_job_upload;
    // the driver calls this from its decode threads, where the wait hides behind the decoding of the next frame)
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}
int sfa_sequence_download(sfa_sequence *q, int f, float *frame3, int stride) {
    sfa_ctx *ctx = q ? q->ctx : nullptr;
    CHECK_ARGS(q && f >= 0 && f < q->n && frame3 && stride >= q->w, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    for (int k = 0; k < 3; k++) SFA_TRY(download_plane(ctx, frame3 + (size_t)k * stride * q->h, stride, q->frame(f) + k * q->pl, q->pitch, q->w, q->h));
    return sfa_ctx_sync(ctx);
}
// normalize() over frames [f0, f0 + n): statistics over exactly these frames (the reference's `-jet k` mode normalises over that jet's frames only,
// slow_flow.cpp:418-424,673), every frame's sums by the same kernels in the same order whatever the number of frames
// normalize() (variational_mt.cpp:17-85) in its three parts, so that a sequence spread over several GPUs is normalised with ONE set of statistics: (1) the six
// fp64 sums of every frame -- a deterministic kernel: the same bits on whichever GPU holds the frame --, (2) the statistics from the per-frame sums in frame
// order, plain host arithmetic, (3) I <- (I - avg) / std on the resident frames.  sfa_sequence_normalize is the three in a row.
int sfa_sequence_frame_sums(sfa_sequence *q, int f0, int n, double *sums) {
    sfa_ctx *ctx = q ? q->ctx : nullptr;
    CHECK_ARGS(q && sums && f0 >= 0 && n > 0 && f0 + n <= q->n, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    double *dsum = reinterpret_cast<double *>(q->sums.p);
    for (int f = f0; f < f0 + n; f++) launch_normalize_sums(ctx, q->geo(), q->frame(f), dsum + 6 * f);
    SFA_HIP(ctx, hipMemcpyAsync(sums, dsum + 6 * f0, (size_t)6 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}
int sfa_normalize_statistics(const double *sums, int n, int w, int h, double avg[3], double std_dev[3]) {
    if (!sums || n <= 0 || w <= 0 || h <= 0 || !avg || !std_dev) return set_error(nullptr, SFA_ERR_ARG, "sfa_normalize_statistics: bad arguments");
    for (int k = 0; k < 3; k++) { avg[k] = 0; std_dev[k] = 0; }
    for (int f = 0; f < n; f++)
        for (int k = 0; k < 3; k++) {
            avg[k] += sums[6 * f + 2 * k] / (h * w);                                     // variational_mt.cpp:41-47
            std_dev[k] += sums[6 * f + 2 * k + 1] / (h * w);
        }
    for (int k = 0; k < 3; k++) {
        avg[k] /= n;
        std_dev[k] = sqrt((std_dev[k] / n) - avg[k] * avg[k]) / 255.0f;                 // :52
    }
    return SFA_OK;
}
int sfa_sequence_apply_normalization(sfa_sequence *q, int f0, int n, const double avg[3], const double std_dev[3]) {
    sfa_ctx *ctx = q ? q->ctx : nullptr;
    CHECK_ARGS(q && avg && std_dev && f0 >= 0 && n > 0 && f0 + n <= q->n, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    for (int f = f0; f < f0 + n; f++) launch_normalize_apply(ctx, q->geo(), q->frame(f), avg, std_dev);
    return sfa_ctx_sync(ctx);
}
int sfa_sequence_normalize(sfa_sequence *q, int f0, int n, double avg[3], double std_dev[3]) {
    sfa_ctx *ctx = q ? q->ctx : nullptr;
    CHECK_ARGS(q && avg && std_dev && f0 >= 0 && n > 0 && f0 + n <= q->n, "bad arguments");
    std::vector<double> hs((size_t)6 * n);
    SFA_TRY(sfa_sequence_frame_sums(q, f0, n, hs.data()));
    SFA_TRY(sfa_normalize_statistics(hs.data(), n, q->w, q->h, avg, std_dev));
    return sfa_sequence_apply_normalization(q, f0, n, avg, std_dev);
}

int sfa_normalize(sfa_ctx *ctx, float *const *frames, int F, int w, int h, int stride, double avg[3], double std_dev[3]) {
    CHECK_ARGS(ctx && frames && F > 0 && w > 0 && h > 0 && stride >= w && avg && std_dev, "bad arguments");
    for (int f = 0; f < F; f++) CHECK_ARGS(frames[f], "null frame");
    sfa_sequence *q = nullptr;
    SFA_TRY(sfa_sequence_create(ctx, w, h, F, &q));
    std::unique_ptr<sfa_sequence, void (*)(sfa_sequence *)> guard(q, sfa_sequence_destroy);
    for (int f = 0; f < F; f++) SFA_TRY(sfa_sequence_upload(q, f, frames[f], stride));
    SFA_TRY(sfa_sequence_normalize(q, 0, F, avg, std_dev));
    for (int f = 0; f < F; f++) SFA_TRY(sfa_sequence_download(q, f, frames[f], stride));
    return SFA_OK;
}

}  // extern "C"

// ---- the argument checks of the device seam (include/slowflow_amd.h; kernels: device_io.hip, mosaic.hip, track.hip, quantile.hip) -------------------
// A view's strides, extent, nesting and byte range are dev_view.h's arithmetic; here it meets the HIP runtime (check_device_pointer) and the messages.
// Every check is taken on the host before anything is launched; a refusal names the argument (REFUSE: sfa_internal.h).  Those declared in sfa_internal.h are
// shared with job.hip, two_frame.hip, track.hip, track_fill.hip and quantile.hip.
namespace sfa {

// `p` must be device memory of the context's GPU, and the view (its last element `last` elements of `elem` bytes further) must lie inside p's allocation
int check_device_pointer(sfa_ctx *ctx, const char *fn, const char *arg, const void *p, long long last, size_t elem) {
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        REFUSE("%s: %s is not device memory (hipPointerGetAttributes does not know the pointer: a host pointer?)", fn, arg);
    }
    if (at.type != hipMemoryTypeDevice) REFUSE("%s: %s is not device memory (host, managed or unregistered memory)", fn, arg);
    if (at.device != ctx->device) REFUSE("%s: %s lives on GPU %d, the job's context on GPU %d", fn, arg, at.device, ctx->device);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess) {
        (void)hipGetLastError();
        REFUSE("%s: the allocation %s lies in is unknown to hipMemGetAddressRange: the extent of the view cannot be checked", fn, arg);
    }
    const unsigned long long room = (unsigned long long)(static_cast<const char *>(base) + size - static_cast<const char *>(p));
    if ((unsigned long long)last >= room / elem) REFUSE("%s: the view of %s (%lld elements to its last one) ends beyond its allocation (%llu bytes from the pointer)", fn, arg, last, room);
    return SFA_OK;
}

static size_t dev_elem_size(int dtype) { return dtype == SFA_DEV_F32 ? 4 : dtype == SFA_DEV_U16 ? 2 : 1; }

// a strided view (dev_view.h).  Refused in this order: a null pointer or null strides; a negative stride, an innermost stride below min_inner, an extent
// beyond the signed 64-bit range; memory that is not the context's GPU's, or a last element outside its allocation
int check_view(sfa_ctx *ctx, const char *fn, const View &v, long long min_inner) {
    if (!v.p) REFUSE("%s: %s is null", fn, v.name);
    if (!v.st) REFUSE("%s: the strides of %s are null", fn, v.name);
    long long last;
    int at;
    const ViewFault fault = view_extent(v, min_inner, &last, &at);
    if (fault == VIEW_RANGE) REFUSE("%s: the strides of %s reach beyond the 64-bit range: the view cannot lie inside an allocation", fn, v.name);
    if (fault != VIEW_OK) {
        char nth[24];
        snprintf(nth, sizeof nth, "stride %d", at);
        const char *dim = v.dim ? v.dim[at] : at == v.nd - 1 ? "the column stride" : at == v.nd - 2 ? "the row stride" : nth;
        if (fault == VIEW_NEGATIVE) REFUSE("%s: %s of %s is a negative stride (%lld)", fn, dim, v.name, v.st[at]);
        REFUSE("%s: %s of %s is %lld: it must be >= %lld", fn, dim, v.name, v.st[at], min_inner);
    }
    return check_device_pointer(ctx, fn, v.name, v.p, last, v.elem);
}

// no two of the (checked) views share a byte; null pointers, optional arguments left out, are skipped.  why: what the overlap would break, for the message
int check_disjoint(sfa_ctx *ctx, const char *fn, std::initializer_list<View> views, const char *why) {
    std::vector<ByteRange> r;
    int a, b;
    for (const View &v : views) r.push_back(byte_range(v));
    if (!first_overlap(r.data(), (int)r.size(), &a, &b)) return SFA_OK;
    if (why) REFUSE("%s: %s overlaps %s: %s", fn, views.begin()[a].name, views.begin()[b].name, why);
    REFUSE("%s: %s and %s overlap", fn, views.begin()[a].name, views.begin()[b].name);
}

// the frames of `nwin` windows of F frames each (a sequence's n frames: one window of n): the layout's element type, and its view
int check_frames_source(sfa_ctx *ctx, const char *fn, const void *frames_dev, const sfa_dev_layout *l, long long win_stride, int nwin, int F, int w, int h) {
    if (!l) REFUSE("%s: layout is null", fn);
    if (l->dtype != SFA_DEV_F32 && l->dtype != SFA_DEV_U8 && l->dtype != SFA_DEV_U16) REFUSE("%s: layout.dtype %d is no element type (fp32 0, u8 1, u16 2)", fn, l->dtype);
    static const char *const dim[5] = {"layout.window", "layout.frame", "layout.channel", "layout.row", "layout.column"};
    const long long st[5] = {win_stride, l->frame, l->channel, l->row, l->column};
    return check_view(ctx, fn, View{"frames_dev", frames_dev, dev_elem_size(l->dtype), 5, {nwin, F, 3, h, w}, st, dim});
}

int check_batch_range(sfa_ctx *ctx, const char *fn, const char *what, int b0, int n, int nb) {
    if (b0 < 0 || n < 1 || (long)b0 + n > nb) REFUSE("%s: %s b0 = %d, n = %d lie outside the job's batch of %d", fn, what, b0, n, nb);
    return SFA_OK;
}

// download destinations: flow [n][2][h][w], occlusions [n][h][w] or null.  Each a checked view, and free of overlap by one of two sufficient conditions:
// (1) every (window, plane) in a byte range of its own, and each plane's strides nested; else (2) flow and occlusions apart, and each a layout of nested
// strides (which takes planes that lie interleaved).  What neither proves is refused.
int check_download_destination(sfa_ctx *ctx, const char *fn, int n, int w, int h, float *flow_dev, const long long strides[4], float *occ_dev,
                               const long long occ_strides[3]) {
    const View flow{"flow_dev", flow_dev, sizeof(float), 4, {n, 2, h, w}, strides}, occ{"occ_dev", occ_dev, sizeof(float), 3, {n, h, w}, occ_strides};
    SFA_TRY(check_view(ctx, fn, flow));
    if (occ_dev) SFA_TRY(check_view(ctx, fn, occ));
    bool ok = strides_nest(strides + 2, flow.n + 2, 2) && (!occ_dev || strides_nest(occ_strides + 1, occ.n + 1, 2));
    if (ok) {
        std::vector<ByteRange> r;
        r.reserve((size_t)3 * n);
        for (int i = 0; i < n; i++) {
            for (int p = 0; p < 2; p++) r.push_back(byte_range(View{"", flow_dev + i * strides[0] + p * strides[1], sizeof(float), 2, {h, w}, strides + 2}));
            if (occ_dev) r.push_back(byte_range(View{"", occ_dev + i * occ_strides[0], sizeof(float), 2, {h, w}, occ_strides + 1}));
        }
        int a, b;
        ok = !first_overlap(r.data(), (int)r.size(), &a, &b);
    }
    if (!ok) ok = strides_nest(strides, flow.n, 4) && (!occ_dev || (strides_nest(occ_strides, occ.n, 3) && !overlap(byte_range(flow), byte_range(occ))));
    if (!ok) REFUSE("%s: the destinations overlap: windows or planes of flow_dev%s share memory (or lie interleaved in a way the check cannot clear)", fn, occ_dev ? " / occ_dev" : "");
    return SFA_OK;
}

// the raw Bayer ingest's descriptors (sfa_demosaic_device, sfa_sequence_upload_mosaic*; the method also for sfa_job_set_raw_weights in job.hip)
int check_mosaic_method(sfa_ctx *ctx, const char *fn, int method, int red_x, int red_y) {
    if (method != 0 && method != 2)
        REFUSE("%s: method %d: 0 (bayer2rgbGR) and 2 (the 8-bit OpenCV conversion) exist; 1, Hamilton-Adams, is third-party code the reference does not ship", fn, method);
    if (red_x != 0 && red_x != 1) REFUSE("%s: red_x = %d: the red site's column parity is 0 or 1", fn, red_x);
    if (red_y != 0 && red_y != 1) REFUSE("%s: red_y = %d: the red site's row parity is 0 or 1", fn, red_y);
    return SFA_OK;
}
// the descriptor against the crop's size w x h; the pointer and the strides are check_view's
static int check_mosaic_geometry(sfa_ctx *ctx, const char *fn, int dtype, int W, int H, int x0, int y0, int w, int h, int method) {
    if (dtype != SFA_DEV_F32 && dtype != SFA_DEV_U8 && dtype != SFA_DEV_U16) REFUSE("%s: desc.dtype %d is no element type (fp32 0, u8 1, u16 2)", fn, dtype);
    if (w < 1 || h < 1) REFUSE("%s: w = %d, h = %d: the destination is empty", fn, w, h);
    if (W < 1 || H < 1) REFUSE("%s: desc.W = %d, desc.H = %d: the mosaic is empty", fn, W, H);
    if (method == 0 && (W < 2 || H < 2)) REFUSE("%s: desc.W = %d, desc.H = %d with method 0: the mirrored neighbours need W >= 2 and H >= 2 (the reference reads outside the image)", fn, W, H);
    if (x0 < 0 || y0 < 0 || (long)x0 + w > W || (long)y0 + h > H)
        REFUSE("%s: the crop desc.x0 = %d, desc.y0 = %d of %d x %d leaves the mosaic of desc.W = %d, desc.H = %d", fn, x0, y0, w, h, W, H);
    return SFA_OK;
}
// the view of mosaic_dev: all W x H elements of its n frames (the kernels read up to two pixels beyond the crop); st: room for its strides
static View mosaic_view(const void *mosaic_dev, const sfa_mosaic_desc *d, int n, long long st[3]) {
    static const char *const dim[3] = {"desc.frame", "desc.row", "desc.column"};
    st[0] = d->frame; st[1] = d->row; st[2] = d->column;
    return View{"mosaic_dev", mosaic_dev, dev_elem_size(d->dtype), 3, {n, d->H, d->W}, st, dim};
}

}  // namespace sfa

extern "C" {

void sfa_dev_layout_default(sfa_dev_layout *l, int w, int h, int n_frames) {
    if (!l) return;
    l->dtype = SFA_DEV_F32;
    l->column = 1; l->row = w; l->channel = (long long)w * h; l->frame = 3 * l->channel; l->window = (long long)n_frames * l->frame;
}

int sfa_sequence_upload_device(sfa_sequence *q, int f0, int n, const void *frames_dev, const sfa_dev_layout *l) {
    sfa_ctx *ctx = q ? q->ctx : nullptr;
    CHECK_ARGS(q, "seq is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    if (f0 < 0 || n < 1 || (long)f0 + n > q->n) REFUSE("%s: frames f0 = %d, n = %d lie outside the sequence of %d", __func__, f0, n, q->n);
    SFA_TRY(check_frames_source(ctx, __func__, frames_dev, l, 0, 1, n, q->w, q->h));
    const size_t elem = dev_elem_size(l->dtype);
    const int chunk = 16384;                                // 3 planes per frame in the grid's z: below 65536
    for (int i = 0; i < n; i += chunk) {
        const PackSrc src{static_cast<const char *>(frames_dev) + (size_t)i * l->frame * elem, l->dtype, l->frame, 0, l->channel, l->row, l->column};
        launch_pack_frames(ctx, q->frame(f0 + i), 3 * q->pl, q->pl, q->pitch, q->w, q->h, std::min(chunk, n - i), 1, src);
    }
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

// ---- raw Bayer ingest (include/slowflow_amd.h; kernels: mosaic.hip) ------------------------------------------------------------------------
int sfa_demosaic_device(sfa_ctx *ctx, int n, const void *mosaic_dev, const sfa_mosaic_desc *d, int method, int red_x, int red_y, float *dst_dev,
                        const long long st[4], int w, int h) {
    CHECK_ARGS(ctx, "ctx is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    if (n < 1) REFUSE("%s: n = %d frames", __func__, n);
    if (!d) REFUSE("%s: desc is null", __func__);
    SFA_TRY(check_mosaic_method(ctx, __func__, method, red_x, red_y));
    SFA_TRY(check_mosaic_geometry(ctx, __func__, d->dtype, d->W, d->H, d->x0, d->y0, w, h, method));
    long long sst[3];
    const View from = mosaic_view(mosaic_dev, d, n, sst), to{"dst_dev", dst_dev, sizeof(float), 4, {n, 3, h, w}, st};
    SFA_TRY(check_view(ctx, __func__, from));
    SFA_TRY(check_view(ctx, __func__, to));
    if (!strides_nest(st, to.n, 4)) REFUSE("%s: dst_strides let frames, channels or rows of dst_dev share memory (or interleave them in a way the check cannot clear)", __func__);
    SFA_TRY(check_disjoint(ctx, __func__, {to, from}, "the kernel reads a pixel's neighbours after other blocks have written theirs"));
    const MosaicSrc src{mosaic_dev, d->dtype, d->frame, d->row, d->column, d->W, d->H, d->x0, d->y0};
    const MosaicDst dst{dst_dev, st[0], st[1], st[2], st[3], w, h};
    launch_demosaic(ctx, src, dst, n, method, red_x, red_y);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_sequence_upload_mosaic_device(sfa_sequence *q, int f0, int n, const void *mosaic_dev, const sfa_mosaic_desc *d, int method, int red_x, int red_y) {
    sfa_ctx *ctx = q ? q->ctx : nullptr;
    CHECK_ARGS(q, "seq is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    if (f0 < 0 || n < 1 || (long)f0 + n > q->n) REFUSE("%s: frames f0 = %d, n = %d lie outside the sequence of %d", __func__, f0, n, q->n);
    if (!d) REFUSE("%s: desc is null", __func__);
    SFA_TRY(check_mosaic_method(ctx, __func__, method, red_x, red_y));
    SFA_TRY(check_mosaic_geometry(ctx, __func__, d->dtype, d->W, d->H, d->x0, d->y0, q->w, q->h, method));
    long long sst[3];
    SFA_TRY(check_view(ctx, __func__, mosaic_view(mosaic_dev, d, n, sst)));
    const MosaicSrc src{mosaic_dev, d->dtype, d->frame, d->row, d->column, d->W, d->H, d->x0, d->y0};
    const MosaicDst dst{q->frame(f0), 3 * (long long)q->pl, q->pl, q->pitch, 1, q->w, q->h};
    launch_demosaic(ctx, src, dst, n, method, red_x, red_y);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_sequence_upload_mosaic(sfa_sequence *q, int f, const void *mosaic_host, int dtype, long long host_stride, int W, int H, int x0, int y0, int method,
                               int red_x, int red_y) {
    sfa_ctx *ctx = q ? q->ctx : nullptr;
    CHECK_ARGS(q, "seq is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    if (f < 0 || f >= q->n) REFUSE("%s: frame f = %d lies outside the sequence of %d", __func__, f, q->n);
    if (!mosaic_host) REFUSE("%s: mosaic_host is null", __func__);
    SFA_TRY(check_mosaic_method(ctx, __func__, method, red_x, red_y));
    SFA_TRY(check_mosaic_geometry(ctx, __func__, dtype, W, H, x0, y0, q->w, q->h, method));
    if (host_stride < W) REFUSE("%s: host_stride = %lld is below W = %d", __func__, host_stride, W);
    const size_t elem = dev_elem_size(dtype), row = (size_t)W * elem, bytes = row * H;
    if (bytes > q->mos_stage_bytes) {                        // (a larger mosaic than before: the stream may still read the old buffers)
        SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        q->mos_stage_bytes = 0;                              // (stays 0 until all three exist: a failure here sends the next call through this branch again)
        if (q->mos_stage) { (void)hipHostFree(q->mos_stage); q->mos_stage = nullptr; }
        SFA_HIP(ctx, hipHostMalloc(&q->mos_stage, bytes, hipHostMallocDefault));
        SFA_TRY(q->mos_dev.alloc(ctx, bytes));
        if (!q->ev_mos) SFA_HIP(ctx, hipEventCreateWithFlags(&q->ev_mos, hipEventDisableTiming));
        q->mos_stage_bytes = bytes;
    } else {
        SFA_HIP(ctx, hipEventSynchronize(q->ev_mos));        // the previous call's copy out of the pinned buffer (not the stream's other work)
    }
    for (int y = 0; y < H; y++) memcpy(static_cast<char *>(q->mos_stage) + y * row, static_cast<const char *>(mosaic_host) + (size_t)y * host_stride * elem, row);
    SFA_HIP(ctx, hipMemcpyAsync(q->mos_dev.p, q->mos_stage, bytes, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipEventRecord(q->ev_mos, ctx->stream));
    const MosaicSrc src{q->mos_dev.p, dtype, (long long)W * H, W, 1, W, H, x0, y0};
    const MosaicDst dst{q->frame(f), 3 * (long long)q->pl, q->pl, q->pitch, 1, q->w, q->h};
    launch_demosaic(ctx, src, dst, 1, method, red_x, red_y);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_sequence_rescale(sfa_sequence *dq, int f_dst, sfa_sequence *sq, int f_src, int n, float scale) {
    sfa_ctx *ctx = dq ? dq->ctx : (sq ? sq->ctx : nullptr);
    CHECK_ARGS(dq, "dst_seq is null");
    CHECK_ARGS(sq, "src_seq is null");
    if (sq->ctx != ctx) REFUSE("%s: src_seq lives on another context than dst_seq: one stream orders the blur before the resize", __func__);
    if (sq == dq) REFUSE("%s: src_seq is dst_seq", __func__);
    if (!(scale > 0)) REFUSE("%s: scale = %g must be positive", __func__, (double)scale);
    if (n < 1 || f_src < 0 || (long)f_src + n > sq->n) REFUSE("%s: frames f_src = %d, n = %d lie outside src_seq of %d", __func__, f_src, n, sq->n);
    if (f_dst < 0 || (long)f_dst + n > dq->n) REFUSE("%s: frames f_dst = %d, n = %d lie outside dst_seq of %d", __func__, f_dst, n, dq->n);
    const int w = sq->w, h = sq->h;
    const int dw = (int)lrint((double)w * scale), dh = (int)lrint((double)h * scale);   // saturate_cast<int>(src.cols * fx) (ingest.cpp: color_image_rescale)
    if (dq->w != dw || dq->h != dh)
        REFUSE("%s: dst_seq is %d x %d; src_seq's %d x %d frames at scale %g give lrint(w scale) x lrint(h scale) = %d x %d", __func__, dq->w, dq->h, w, h, (double)scale, dw, dh);
    const float sigma = (float)(1 / sqrt(2 * scale));                                   // slow_flow.cpp:551
    float taps[kMaxBlurTaps];
    if (!(sigma * 8 + 1 < 33)) REFUSE("%s: scale = %g: sigma too large", __func__, (double)scale);
    const int r = cv_gauss_taps(sigma, taps);
    if (r < 0) REFUSE("%s: scale = %g: sigma too large", __func__, (double)scale);
    if (r > 8) REFUSE("%s: scale = %g needs a blur of %d taps; the blur kernel holds 17 (scale >= 0.125)", __func__, (double)scale, 2 * r + 1);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const int chunk = std::min(n, 8);                       // frames blurred per launch pair: bounds the scratch to 2 x 8 frames
    const size_t frame_floats = (size_t)3 * sq->pl;
    if ((size_t)2 * chunk * frame_floats * sizeof(float) > dq->rescale_tmp.bytes) {
        SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        SFA_TRY(dq->rescale_tmp.alloc(ctx, (size_t)2 * chunk * frame_floats * sizeof(float)));
    }
    float *blur = dq->rescale_tmp.f(), *tmp = blur + (size_t)chunk * frame_floats;
    for (int i = 0; i < n; i += chunk) {
        const int m = std::min(chunk, n - i);
        SFA_TRY(launch_gauss_blur(ctx, sq->geo(), blur, tmp, sq->frame(f_src + i), 3 * m, taps, r));
        launch_resize_scaled(ctx, dq->frame(f_dst + i), dw, dh, dq->pitch, dq->pl, 0, blur, w, h, sq->pitch, sq->pl, 0, 3 * m, 1, 1.0f, 1.0 / (double)scale,
                             1.0 / (double)scale);
    }
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_ctx_wait_stream(sfa_ctx *ctx, void *stream) {
    CHECK_ARGS(ctx, "ctx is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_HIP(ctx, hipEventRecord(ctx->ev_wait, static_cast<hipStream_t>(stream)));
    SFA_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_wait, 0));
    return SFA_OK;
}
int sfa_ctx_signal_stream(sfa_ctx *ctx, void *stream) {
    CHECK_ARGS(ctx, "ctx is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_HIP(ctx, hipEventRecord(ctx->ev_signal, ctx->stream));
    SFA_HIP(ctx, hipStreamWaitEvent(static_cast<hipStream_t>(stream), ctx->ev_signal, 0));
    return SFA_OK;
}

}  // extern "C"
