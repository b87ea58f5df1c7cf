// jet_resample.hip -- jets of another size than the tracking frames: dense_tracking crops every jet flow and occlusion image (crop, utils/utils.cpp:308-318),
// resizes it by rescale = (1.0f * sequence[0].cols) / flow.cols and, for a flow, multiplies by that factor (dense_tracking.cpp:1134-1146, :1171-1189) before
// anything reads it.  Here the planes are uploaded as read -- at slow_flow.cfg's scale 0.25 a sixteenth of the target's bytes -- and expanded on the GPU.
//
// OpenCV is not in this tree, so the resampling is parity-unpinned: it restates cv::resize's documented arithmetic (the coordinate rule of the pyramid's
// resize) and is pinned to tests/jet_resample_ref.py, a scalar numpy restatement, with IEEE equality.
//   k_jet_resample      INTER_LINEAR on CV_64FC2 (HResizeLinear / VResizeLinear<double, double, float>): float weights, fp64 samples, products and sums without
//                       contraction, rows then columns, then one fp64 multiply by (double)rescale.  One thread per target pixel and field, 4 taps of (u, v)
//                       from the two float source planes, one 16-byte double2 store.
//   k_jet_occ_decode    INTER_CUBIC on 8-bit (HResizeCubic<uchar, int, short>, VResizeCubic with FixedPtCast<int, uchar, 22>), medianBlur(3) with a replicated
//                       border, 255 - x.  One block per 64 x 4 tile of the target: the 66 x 6 resized values it needs go through LDS, so that the median's
//                       nine reads do not repeat the 16-tap cubic.
#include <algorithm>
#include <cmath>

#include "sfa_device.h"

#pragma clang fp contract(off)

namespace sfa {

constexpr int kJetThreads = 256;
constexpr int kOccTX = 64, kOccTY = 4;   // k_jet_occ_decode's tile of the target

// su, sv: np packed planes of cw x ch floats (the crop is the upload's).  out: np planes of w x h.  scale = 1.0 / (double)rescale, r = (double)rescale.
__global__ void __launch_bounds__(kJetThreads) k_jet_resample(const float *__restrict__ su, const float *__restrict__ sv, int cw, int ch, int w, int h, double scale,
                                                              double r, double2 *__restrict__ out, size_t total) {
    const size_t pl = (size_t)w * h, spl = (size_t)cw * ch;
    for (size_t i = (size_t)blockIdx.x * kJetThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kJetThreads) {
        const size_t k = i / pl, p = i % pl;
        const int dx = (int)(p % w), dy = (int)(p / w);
        float fx = (float)((dx + 0.5) * scale - 0.5), fy = (float)((dy + 0.5) * scale - 0.5);
        int sx = (int)floorf(fx), sy = (int)floorf(fy);
        fx -= sx; fy -= sy;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= cw - 1) { fx = 0; sx = cw - 1; }
        if (sy < 0) { fy = 0; sy = 0; }
        if (sy >= ch - 1) { fy = 0; sy = ch - 1; }
        const int sx1 = sx + 1 < cw ? sx + 1 : sx, sy1 = sy + 1 < ch ? sy + 1 : sy;
        const double a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;                // the float weights, widened
        const size_t o00 = k * spl + (size_t)sy * cw + sx, o10 = k * spl + (size_t)sy * cw + sx1;
        const size_t o01 = k * spl + (size_t)sy1 * cw + sx, o11 = k * spl + (size_t)sy1 * cw + sx1;
        const double u0 = (double)su[o00] * a0 + (double)su[o10] * a1, u1 = (double)su[o01] * a0 + (double)su[o11] * a1;
        const double v0 = (double)sv[o00] * a0 + (double)sv[o10] * a1, v1 = (double)sv[o01] * a0 + (double)sv[o11] * a1;
        out[i] = make_double2((u0 * b0 + u1 * b1) * r, (v0 * b0 + v1 * b1) * r);   // flow *= rescale (:1145-1146)
    }
}

// interpolateCubic (A = -0.75) in fp32, then saturate_cast<short>(c * INTER_RESIZE_COEF_SCALE): cvRound (halves to even) at 11 fractional bits
__device__ __forceinline__ void cubic_taps(float x, int c[4]) {
    const float A = -0.75f;
    float k[4];
    k[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    k[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    k[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    k[3] = 1.f - k[0] - k[1] - k[2];
    for (int j = 0; j < 4; j++) c[j] = clampi((int)rintf(k[j] * 2048.f), -32768, 32767);
}

// the cubic resize's value at target pixel (dx, dy), both inside the target; src: sw x sh packed bytes
__device__ __forceinline__ int cubic_resized(const unsigned char *__restrict__ src, int sw, int sh, double scale, int dx, int dy) {
    float fx = (float)((dx + 0.5) * scale - 0.5), fy = (float)((dy + 0.5) * scale - 0.5);
    const int sx = (int)floorf(fx), sy = (int)floorf(fy);
    fx -= sx; fy -= sy;
    int ca[4], cb[4];
    cubic_taps(fx, ca);
    cubic_taps(fy, cb);
    int sum = 0;
    for (int j = 0; j < 4; j++) {
        const unsigned char *row = src + (size_t)clampi(sy - 1 + j, 0, sh - 1) * sw;
        int hs = 0;
        for (int i = 0; i < 4; i++) hs += (int)row[clampi(sx - 1 + i, 0, sw - 1)] * ca[i];
        sum += hs * cb[j];
    }
    return clampi((sum + (1 << 21)) >> 22, 0, 255);
}

// src: np packed planes of sw x sh bytes; out: np packed planes of w x h
__global__ void __launch_bounds__(kOccTX * kOccTY) k_jet_occ_decode(const unsigned char *__restrict__ src, int sw, int sh, int w, int h, double scale, int np,
                                                                    unsigned char *__restrict__ out) {
    constexpr int LW = kOccTX + 2, LH = kOccTY + 2;
    __shared__ unsigned char tile[LH * LW];
    const int bx = blockIdx.x * kOccTX, by = blockIdx.y * kOccTY, t = threadIdx.y * kOccTX + threadIdx.x;
    for (int k = blockIdx.z; k < np; k += gridDim.z) {                          // uniform over the block: the barriers are met by all
        const unsigned char *S = src + (size_t)k * sw * sh;
        for (int q = t; q < LH * LW; q += kOccTX * kOccTY) {
            const int x = clampi(bx - 1 + q % LW, 0, w - 1), y = clampi(by - 1 + q / LW, 0, h - 1);   // the median's replicated border
            tile[q] = (unsigned char)cubic_resized(S, sw, sh, scale, x, y);
        }
        __syncthreads();
        const int x = bx + threadIdx.x, y = by + threadIdx.y;
        if (x < w && y < h) {
            int p[9];
            for (int j = 0; j < 3; j++)
                for (int i = 0; i < 3; i++) p[3 * j + i] = tile[(threadIdx.y + j) * LW + threadIdx.x + i];
#define SFA_SORT2(a, b) { const int lo = min(p[a], p[b]), hi = max(p[a], p[b]); p[a] = lo; p[b] = hi; }
            SFA_SORT2(1, 2) SFA_SORT2(4, 5) SFA_SORT2(7, 8) SFA_SORT2(0, 1) SFA_SORT2(3, 4) SFA_SORT2(6, 7) SFA_SORT2(1, 2) SFA_SORT2(4, 5) SFA_SORT2(7, 8)
            SFA_SORT2(0, 3) SFA_SORT2(5, 8) SFA_SORT2(4, 7) SFA_SORT2(3, 6) SFA_SORT2(1, 4) SFA_SORT2(2, 5) SFA_SORT2(4, 7) SFA_SORT2(4, 2) SFA_SORT2(6, 4)
            SFA_SORT2(4, 2)                                                     // the 19-exchange median of nine: p[4]
#undef SFA_SORT2
            out[(size_t)k * w * h + (size_t)y * w + x] = (unsigned char)(255 - p[4]);
        }
        __syncthreads();                                                        // before the next plane overwrites the tile
    }
}

int jet_source_check(sfa_ctx *ctx, const char *fn, const sfa_jet_source *s, int w, int h, bool *identity) {
    if (!s) return set_error(ctx, SFA_ERR_ARG, "%s: null source", fn);
    if (!(s->sw >= 1 && s->sh >= 1 && s->stride >= s->sw)) return set_error(ctx, SFA_ERR_ARG, "%s: source: %d x %d planes with row stride %d", fn, s->sw, s->sh, s->stride);
    if (!(s->x0 >= 0 && s->y0 >= 0 && s->cw >= 1 && s->ch >= 1 && (long)s->x0 + s->cw <= s->sw && (long)s->y0 + s->ch <= s->sh))
        return set_error(ctx, SFA_ERR_ARG, "%s: source: the crop of %d x %d at (%d, %d) leaves the %d x %d planes (the reference reads outside its Mat there)", fn,
                         s->cw, s->ch, s->x0, s->y0, s->sw, s->sh);
    if (!(s->rescale > 0) || std::isinf(s->rescale)) return set_error(ctx, SFA_ERR_ARG, "%s: source: rescale %g (a positive factor, (1.0f * w) / cw)", fn, (double)s->rescale);
    const double tw = std::rint((double)s->cw * (double)s->rescale), th = std::rint((double)s->ch * (double)s->rescale);   // cvRound: halves to even
    if (!(w >= 1 && h >= 1) || tw != (double)w || th != (double)h)
        return set_error(ctx, SFA_ERR_ARG, "%s: source: %d x %d rescaled by %.9g is %.0f x %.0f, not the target %d x %d (the reference would index a Mat of the wrong size)",
                         fn, s->cw, s->ch, (double)s->rescale, tw, th, w, h);
    *identity = s->x0 == 0 && s->y0 == 0 && s->cw == s->sw && s->ch == s->sh && s->sw == w && s->sh == h && s->rescale == 1.0f;
    return SFA_OK;
}

int launch_jet_resample(sfa_ctx *ctx, const sfa_jet_source &s, size_t np, const float *su, const float *sv, int w, int h, double2 *out) {
    const size_t total = np * (size_t)w * h;
    const unsigned blocks = (unsigned)std::min<size_t>((total + kJetThreads - 1) / kJetThreads, (size_t)ctx->cu_count * 16);
    hipLaunchKernelGGL(k_jet_resample, dim3(blocks), dim3(kJetThreads), 0, ctx->stream, su, sv, s.cw, s.ch, w, h, 1.0 / (double)s.rescale, (double)s.rescale, out, total);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int jet_resample_flows(sfa_ctx *ctx, const sfa_jet_source &s, size_t np, const float *const *u, const float *const *v, int w, int h, float *stage, double2 *out,
                       hipEvent_t before, hipEvent_t after) {
    const size_t spl = (size_t)s.cw * s.ch, off = (size_t)s.y0 * s.stride + s.x0;
    float *su = stage, *sv = stage + np * spl;
    for (size_t k = 0; k < np; k++) {                                           // the cropped columns of each plane, packed: padding is never read
        SFA_HIP(ctx, hipMemcpy2DAsync(su + k * spl, (size_t)s.cw * 4, u[k] + off, (size_t)s.stride * 4, (size_t)s.cw * 4, s.ch, hipMemcpyHostToDevice, ctx->stream));
        SFA_HIP(ctx, hipMemcpy2DAsync(sv + k * spl, (size_t)s.cw * 4, v[k] + off, (size_t)s.stride * 4, (size_t)s.cw * 4, s.ch, hipMemcpyHostToDevice, ctx->stream));
    }
    if (before) SFA_HIP(ctx, hipEventRecord(before, ctx->stream));
    SFA_TRY(launch_jet_resample(ctx, s, np, su, sv, w, h, out));
    if (after) SFA_HIP(ctx, hipEventRecord(after, ctx->stream));
    return SFA_OK;
}

int launch_jet_occ_decode(sfa_ctx *ctx, const sfa_jet_source &s, size_t np, const unsigned char *stage, int w, int h, unsigned char *out) {
    const dim3 grid((unsigned)((w + kOccTX - 1) / kOccTX), (unsigned)((h + kOccTY - 1) / kOccTY), (unsigned)std::min<size_t>(np, 65535));
    hipLaunchKernelGGL(k_jet_occ_decode, grid, dim3(kOccTX, kOccTY), 0, ctx->stream, stage, s.sw, s.sh, w, h, 1.0 / (double)s.rescale, (int)np, out);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int jet_decode_occlusions(sfa_ctx *ctx, const sfa_jet_source &s, size_t np, const unsigned char *const *occ, int w, int h, unsigned char *stage, unsigned char *out) {
    SFA_TRY(upload_masks(ctx, np, occ, s.stride, s.sw, s.sh, stage));             // the images as read, packed
    return launch_jet_occ_decode(ctx, s, np, stage, w, h, out);
}

}  // namespace sfa

using namespace sfa;

void sfa_jet_source_default(sfa_jet_source *src, int w, int h, int stride) {
    if (!src) return;
    *src = sfa_jet_source{w, h, stride, 0, 0, w, h, 1.0f};
}

// what the two stage bindings share: the source against the target, the count and the planes
static int stage_args(sfa_ctx *ctx, const char *fn, int n, const sfa_jet_source *src, int w, int h, const void *const *a, const void *const *b, bool *identity) {
    if (!ctx) return set_error(ctx, SFA_ERR_ARG, "%s: null context", fn);
    SFA_TRY(jet_source_check(ctx, fn, src, w, h, identity));
    if (!(n >= 1 && (size_t)n * w * h <= ((size_t)1 << 31))) return set_error(ctx, SFA_ERR_ARG, "%s: n = %d (n >= 1, n w h <= 2^31)", fn, n);
    if (!a || !b) return set_error(ctx, SFA_ERR_ARG, "%s: null argument", fn);
    for (int k = 0; k < n; k++)
        if (!a[k] || !b[k]) return set_error(ctx, SFA_ERR_ARG, "%s: null plane %d", fn, k);
    return SFA_OK;
}

int sfa_jet_flow_resample(sfa_ctx *ctx, int n, const sfa_jet_source *src, const float *const *u, const float *const *v, int w, int h, double *out_u, double *out_v) {
    bool identity;
    SFA_TRY(stage_args(ctx, __func__, n, src, w, h, reinterpret_cast<const void *const *>(u), reinterpret_cast<const void *const *>(v), &identity));
    if (!out_u || !out_v) return set_error(ctx, SFA_ERR_ARG, "%s: null output", __func__);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pl = (size_t)w * h, total = (size_t)n * pl;
    DevMem dstage, dout;
    SFA_TRY(dstage.alloc(ctx, 2 * (size_t)n * src->cw * src->ch * 4)); SFA_TRY(dout.alloc(ctx, total * 16));
    SFA_TRY(jet_resample_flows(ctx, *src, (size_t)n, u, v, w, h, dstage.f(), static_cast<double2 *>(dout.p), nullptr, nullptr));
    std::vector<double2> host(total);
    SFA_HIP(ctx, hipMemcpyAsync(host.data(), dout.p, total * 16, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < total; i++) { out_u[i] = host[i].x; out_v[i] = host[i].y; }   // the binding's planar layout; the kernels keep the pairs
    return SFA_OK;
}

int sfa_jet_occlusion_decode(sfa_ctx *ctx, int n, const sfa_jet_source *src, const unsigned char *const *occ, int w, int h, unsigned char *mask) {
    bool identity;
    SFA_TRY(stage_args(ctx, __func__, n, src, w, h, reinterpret_cast<const void *const *>(occ), reinterpret_cast<const void *const *>(occ), &identity));
    if (!mask) return set_error(ctx, SFA_ERR_ARG, "%s: null mask", __func__);
    if (src->x0 != 0 || src->y0 != 0 || src->cw != src->sw || src->ch != src->sh)
        return set_error(ctx, SFA_ERR_ARG, "%s: source: cropped occlusions are not supported (the reference's crop() reads the 8-bit Mat through at<Vec2d>)", __func__);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const size_t total = (size_t)n * w * h;
    DevMem dstage, dout;
    SFA_TRY(dstage.alloc(ctx, (size_t)n * src->sw * src->sh)); SFA_TRY(dout.alloc(ctx, total));
    SFA_TRY(jet_decode_occlusions(ctx, *src, (size_t)n, occ, w, h, static_cast<unsigned char *>(dstage.p), static_cast<unsigned char *>(dout.p)));
    SFA_HIP(ctx, hipMemcpyAsync(mask, dout.p, total, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}
