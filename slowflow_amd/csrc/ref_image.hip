// ref_image.hip -- dense_tracking's reduced reference image on the GPU (dense_tracking.cpp:931-955; include/slowflow_amd.h: sfa_reference_grid,
// sfa_reference_taps, sfa_reference_lab_device, sfa_reference_lab): frame 0 as 8 bits, OpenCV's 8-bit Gaussian blur, the bilinear reduction to the
// accumulation grid, EpicFlow's Lab image of the result and, where asked for, the 8-bit RGB image the edge detector reads.  The arithmetic is csrc/ref_image.h
// (taps, tie rule, sizes) and csrc/lab_math.h (the 8-bit step, rgb_to_lab); host/ref_image.cpp is the same stage in plain C++.
//   k_reference_lab<NT>     one workgroup per tile of 64 x TY grid pixels of one image.  Three phases with a barrier between them:
//                           A  the tile's source footprint (tile x (skip + 1) plus the radius, coordinates clamped: the replicated border) -> LDS as bytes,
//                              four columns packed per thread and stored as one dword: consecutive lanes, consecutive dwords
//                           B  the row pass, only at the two columns each grid pixel reduces over: both sums of a grid column in one dword (two 16-bit
//                              halves; at most 255 * 256).  A lane reads three aligned dwords of bytes: consecutive lanes are a dword apart at skip 3, half
//                              a dword at skip 1 (two lanes share a dword: a broadcast), and store consecutive dwords
//                           C  a grid pixel per thread: the column pass at the two rows it reduces over (NT + 1 dword reads, lanes along the row: one bank
//                              each), the rounding with its tie rule, the 2 x 2 reduction, rgb_to_lab from registers, rows written by consecutive lanes
//                           The blur is formed where the reduction reads it: everywhere at skip 1, at a quarter of the pixels at skip 3.
//   k_reference_rgb8        skip 0 with an 8-bit output: the samples as k_rgb8_to_lab rounds them.  The Lab image of skip 0 is k_rgb8_to_lab itself.
#include <algorithm>

#include "lab_math.h"
#include "ref_image.h"
#include "sfa_internal.h"

namespace sfa {
namespace {

constexpr int kRefThreads = 256, kRefTX = 64;                          // four rows of 64 grid pixels per pass of phases B and C

struct RefTaps { int k[refimg::kMaxTaps]; };

// the shapes of a tap count: NT 7 is skip 1 (tiles of 64 x 16), NT 9 skip 3 (64 x 8: the same footprint height)
template <int NT> struct RefShape {
    static constexpr int S = NT == 7 ? 2 : 4;                          // skip + 1
    static constexpr int TY = NT == 7 ? 16 : 8;
    static constexpr int R = NT / 2;
    static constexpr int FW = S * (kRefTX - 1) + NT + 1, FH = S * (TY - 1) + NT + 1;   // the footprint: the first column of the last pair, its taps, one more
    static constexpr int PD = (FW + 3) / 4;                            // dwords per footprint row
    static_assert(S * (kRefTX - 1) / 4 + 2 < PD, "phase B reads three dwords from the pair's first byte");
    static_assert((S * (kRefTX - 1) & 3) + NT + 1 <= 12, "which hold the NT + 1 bytes of a pair");
    static_assert((3 * FH * PD + 3 * FH * kRefTX) * 4 <= 64 * 1024, "static LDS");
};

__device__ inline unsigned byte_of(float s, float norm) {
    const float v = lab::sample_8bit(s, norm);
    return v == v ? (unsigned)v : 0u;                                  // saturate_cast<uchar>(cvRound(NaN)): 0
}

template <int NT>
__global__ void __launch_bounds__(kRefThreads) k_reference_lab(LabSrc s, LabDst d, Rgb8Dst q, int w, int h, int gw, int gh, float norm, RefTaps t) {
    using Sh = RefShape<NT>;
    constexpr int S = Sh::S, TY = Sh::TY, FH = Sh::FH, PD = Sh::PD;
    __shared__ unsigned src8[3 * FH * PD];                             // [c][r][dword of four columns]
    __shared__ unsigned row16[3 * FH * kRefTX];                        // [c][r][grid column]: the row sums of its two source columns
    const int tid = threadIdx.x, gx0 = blockIdx.x * kRefTX, gy0 = blockIdx.y * TY, img = blockIdx.z;
    const int x_first = refimg::first_source(gx0, S - 1) - Sh::R, y_first = refimg::first_source(gy0, S - 1) - Sh::R;
    const float *sp = s.p + (long long)img * s.sn;
    // ---- A
    for (int it = tid; it < 3 * FH * PD; it += kRefThreads) {
        const int dq = it % PD, r = (it / PD) % FH, c = it / (PD * FH);
        const int sy = min(max(y_first + r, 0), h - 1);
        const float *rp = sp + (long long)c * s.sc + (long long)sy * s.sr;
        unsigned pk = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int sx = min(max(x_first + 4 * dq + k, 0), w - 1);
            pk |= byte_of(rp[(long long)sx * s.sx], norm) << (8 * k);
        }
        src8[it] = pk;
    }
    __syncthreads();
    // ---- B
    for (int it = tid; it < 3 * FH * kRefTX; it += kRefThreads) {
        const int gxl = it % kRefTX, cr = it / kRefTX, b0 = S * gxl;
        const unsigned *rp = src8 + cr * PD + (b0 >> 2);
        unsigned w0 = rp[0], w1 = rp[1], w2 = rp[2];
        if (S == 2 && (b0 & 2)) { w0 = (w0 >> 16) | (w1 << 16); w1 = (w1 >> 16) | (w2 << 16); w2 >>= 16; }   // (S 4: the pair starts on a dword)
        int a0 = 0, a1 = 0;
#pragma unroll
        for (int j = 0; j <= NT; j++) {
            const int b = (int)(((j < 4 ? w0 : j < 8 ? w1 : w2) >> (8 * (j & 3))) & 255u);
            if (j < NT) a0 += t.k[j] * b;
            if (j > 0) a1 += t.k[j - 1] * b;
        }
        row16[it] = (unsigned)a0 | ((unsigned)a1 << 16);
    }
    __syncthreads();
    // ---- C
    const int gxl = tid % kRefTX, gx = gx0 + gxl;
    for (int gyl = tid / kRefTX; gyl < TY; gyl += kRefThreads / kRefTX) {
        const int gy = gy0 + gyl;
        if (gx >= gw || gy >= gh) continue;
        const int x = refimg::first_source(gx, S - 1);
        float px[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const unsigned *cp = row16 + (c * FH + S * gyl) * kRefTX + gxl;
            int v00 = 0, v01 = 0, v10 = 0, v11 = 0;                    // [row][column] of the 2 x 2
#pragma unroll
            for (int j = 0; j <= NT; j++) {
                const unsigned wv = cp[j * kRefTX];
                const int lo = (int)(wv & 0xffffu), hi = (int)(wv >> 16);
                if (j < NT) { v00 += t.k[j] * lo; v01 += t.k[j] * hi; }
                if (j > 0) { v10 += t.k[j - 1] * lo; v11 += t.k[j - 1] * hi; }
            }
            const int e = 3 * x + c;
            px[c] = (float)refimg::reduce4(refimg::round_blur(v00, e, w), refimg::round_blur(v01, e + 3, w), refimg::round_blur(v10, e, w),
                                           refimg::round_blur(v11, e + 3, w));
        }
        float L, a, b;
        lab::rgb8_to_lab_pixel(px[0], px[1], px[2], 1.0f, &L, &a, &b);   // the values are 8-bit already: rgb_to_lab
        float *dp = d.p + (long long)img * d.sn + (long long)gy * d.sr + (long long)gx * d.sx;
        dp[0] = L; dp[d.sc] = a; dp[2 * d.sc] = b;
        if (q.p) {
            unsigned char *qp = q.p + (long long)img * q.sn + (long long)gy * q.sr + (long long)gx * q.sx;
            qp[0] = (unsigned char)px[0]; qp[q.sc] = (unsigned char)px[1]; qp[2 * q.sc] = (unsigned char)px[2];
        }
    }
}

__global__ void __launch_bounds__(kRefThreads) k_reference_rgb8(LabSrc s, Rgb8Dst q, int w, float norm) {
    const int x = blockIdx.x * kRefThreads + threadIdx.x, y = blockIdx.y, c = blockIdx.z % 3, i = blockIdx.z / 3;
    if (x >= w) return;
    q.p[(long long)i * q.sn + (long long)c * q.sc + (long long)y * q.sr + (long long)x * q.sx] =
        (unsigned char)byte_of(s.p[(long long)i * s.sn + (long long)c * s.sc + (long long)y * s.sr + (long long)x * s.sx], norm);
}

template <int NT>
void launch_tiles(sfa_ctx *c, int n, int w, int h, int gw, int gh, const LabSrc &src, float norm, const LabDst &dst, const Rgb8Dst &rgb8, const RefTaps &t) {
    const int chunk = 32768;                                           // images in the grid's z
    for (int i = 0; i < n; i += chunk) {
        const LabSrc s{src.p + (long long)i * src.sn, src.sn, src.sc, src.sr, src.sx};
        const LabDst d{dst.p + (long long)i * dst.sn, dst.sn, dst.sc, dst.sr, dst.sx};
        const Rgb8Dst q{rgb8.p ? rgb8.p + (long long)i * rgb8.sn : nullptr, rgb8.sn, rgb8.sc, rgb8.sr, rgb8.sx};
        const dim3 grid((gw + kRefTX - 1) / kRefTX, (gh + RefShape<NT>::TY - 1) / RefShape<NT>::TY, std::min(chunk, n - i));
        hipLaunchKernelGGL(k_reference_lab<NT>, grid, dim3(kRefThreads), 0, c->stream, s, d, q, w, h, gw, gh, norm, t);
    }
}

}  // namespace

// what follows holds no kernel: checks, copies and launches.  Compiled for size (see track.hip)
#pragma clang attribute push(__attribute__((minsize)), apply_to = function)

int reference_check(sfa_ctx *ctx, const char *fn, int w, int h, int skip, int *gw, int *gh) {
    if (const char *why = refimg::refused_skip(skip)) REFUSE("%s: skip = %d is not served (%s)", fn, skip, why);
    if (sfa_accumulate_grid(w, h, skip, gw, gh) != SFA_OK) REFUSE("%s: skip: %s", fn, sfa_last_error(nullptr));
    const int rw = refimg::resized_extent(w, skip), rh = refimg::resized_extent(h, skip);
    if (rw != *gw || rh != *gh)
        REFUSE("%s: w x h = %d x %d with skip = %d: OpenCV's resize gives %d x %d, the accumulation grid is %d x %d (the reference reads its edge file at another "
               "size than its grid)", fn, w, h, skip, rw, rh, *gw, *gh);
    if (h > 65535 && skip == 0) REFUSE("%s: h = %d (at most 65535 at skip 0: a row per block)", fn, h);
    if ((*gh + 7) / 8 > 65535) REFUSE("%s: h = %d (too many tiles)", fn, h);
    return SFA_OK;
}

void launch_reference_lab(sfa_ctx *c, int n, int w, int h, int skip, const LabSrc &src, float norm, const LabDst &dst, const Rgb8Dst &rgb8) {
    if (skip == 0) {
        launch_rgb8_to_lab(c, src, dst, n, w, h, norm);
        if (rgb8.p)
            for (int i = 0; i < n; i += 16384)
                hipLaunchKernelGGL(k_reference_rgb8, dim3((w + kRefThreads - 1) / kRefThreads, h, 3 * std::min(16384, n - i)), dim3(kRefThreads), 0, c->stream,
                                   LabSrc{src.p + (long long)i * src.sn, src.sn, src.sc, src.sr, src.sx},
                                   Rgb8Dst{rgb8.p + (long long)i * rgb8.sn, rgb8.sn, rgb8.sc, rgb8.sr, rgb8.sx}, w, norm);
        return;
    }
    RefTaps t{};
    int nt = 0;
    refimg::taps(skip, t.k, &nt);
    const int gw = w / (skip + 1), gh = h / (skip + 1);                 // reference_check passed: the accumulation grid
    if (nt == 7) launch_tiles<7>(c, n, w, h, gw, gh, src, norm, dst, rgb8, t);
    else launch_tiles<9>(c, n, w, h, gw, gh, src, norm, dst, rgb8, t);
}

}  // namespace sfa

using namespace sfa;

extern "C" {

int sfa_reference_grid(int w, int h, int skip, int *gw, int *gh) {
    sfa_ctx *ctx = nullptr;
    if (!gw || !gh) REFUSE("%s: null output", __func__);
    return reference_check(ctx, __func__, w, h, skip, gw, gh);
}

int sfa_reference_taps(int skip, int *taps, int *n) {
    sfa_ctx *ctx = nullptr;
    if (!n) REFUSE("%s: n: null pointer", __func__);
    if (const char *why = refimg::refused_skip(skip)) REFUSE("%s: skip = %d is not served (%s)", __func__, skip, why);
    int k[refimg::kMaxTaps] = {}, nt = 0;
    if (skip) refimg::taps(skip, k, &nt);                               // skip 0: no blur, no tap
    *n = nt;
    for (int i = 0; taps && i < nt; i++) taps[i] = k[i];
    return SFA_OK;
}

int sfa_reference_lab_device(sfa_ctx *ctx, int n, int w, int h, int skip, const float *rgb_dev, const long long rgb_strides[4], float norm, float *lab_dev,
                             const long long lab_strides[4], unsigned char *rgb8_dev, const long long rgb8_strides[4]) {
    CHECK_ARGS(ctx, "ctx is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    if (n < 1) REFUSE("%s: n = %d images", __func__, n);
    if (w < 1 || h < 1) REFUSE("%s: w x h = %d x %d (both at least 1)", __func__, w, h);
    if (!(norm == norm)) REFUSE("%s: norm is NaN", __func__);
    int gw = 0, gh = 0;
    SFA_TRY(reference_check(ctx, __func__, w, h, skip, &gw, &gh));
    const View from{"rgb_dev", rgb_dev, sizeof(float), 4, {n, 3, h, w}, rgb_strides}, to{"lab_dev", lab_dev, sizeof(float), 4, {n, 3, gh, gw}, lab_strides};
    const View to8{"rgb8_dev", rgb8_dev, 1, 4, {n, 3, gh, gw}, rgb8_strides};
    SFA_TRY(check_view(ctx, __func__, from, 0));
    SFA_TRY(check_view(ctx, __func__, to));
    if (!strides_nest(lab_strides, to.n, 4)) REFUSE("%s: lab_strides let images, channels or rows of lab_dev share memory (or interleave them in a way the check cannot clear)", __func__);
    if (rgb8_dev) {
        SFA_TRY(check_view(ctx, __func__, to8));
        if (!strides_nest(rgb8_strides, to8.n, 4)) REFUSE("%s: rgb8_strides let images, channels or rows of rgb8_dev share memory (or interleave them in a way the check cannot clear)", __func__);
    }
    SFA_TRY(check_disjoint(ctx, __func__, {to, to8, from}, "a block may write a pixel's values before another has read its samples"));
    launch_reference_lab(ctx, n, w, h, skip, LabSrc{rgb_dev, rgb_strides[0], rgb_strides[1], rgb_strides[2], rgb_strides[3]}, norm,
                         LabDst{lab_dev, lab_strides[0], lab_strides[1], lab_strides[2], lab_strides[3]},
                         rgb8_dev ? Rgb8Dst{rgb8_dev, rgb8_strides[0], rgb8_strides[1], rgb8_strides[2], rgb8_strides[3]} : Rgb8Dst{nullptr, 0, 0, 0, 0});
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_reference_lab(sfa_ctx *ctx, int w, int h, int skip, const float *rgb, int stride, float norm, float *lab, int lab_stride, unsigned char *rgb8) {
    CHECK_ARGS(ctx, "ctx is null");
    if (!rgb || !lab) REFUSE("%s: %s is null", __func__, !rgb ? "rgb" : "lab");
    if (w < 1 || h < 1) REFUSE("%s: w x h = %d x %d (both at least 1)", __func__, w, h);
    if (stride < w) REFUSE("%s: stride = %d < w = %d", __func__, stride, w);
    if (!(norm == norm)) REFUSE("%s: norm is NaN", __func__);
    int gw = 0, gh = 0;
    SFA_TRY(reference_check(ctx, __func__, w, h, skip, &gw, &gh));
    if (lab_stride < gw) REFUSE("%s: lab_stride = %d < gw = %d", __func__, lab_stride, gw);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pl = (size_t)w * h, gpl = (size_t)gw * gh;
    DevMem src, dst, dst8;
    SFA_TRY(src.alloc(ctx, 3 * pl * sizeof(float)));
    SFA_TRY(dst.alloc(ctx, 3 * gpl * sizeof(float)));
    if (rgb8) SFA_TRY(dst8.alloc(ctx, 3 * gpl));
    for (int c = 0; c < 3; c++) SFA_TRY(upload_plane(ctx, src.f() + c * pl, w, rgb + (size_t)c * h * stride, stride, w, h));
    launch_reference_lab(ctx, 1, w, h, skip, LabSrc{src.f(), 0, (long long)pl, w, 1}, norm, LabDst{dst.f(), 0, (long long)gpl, gw, 1},
                         Rgb8Dst{rgb8 ? static_cast<unsigned char *>(dst8.p) : nullptr, 0, (long long)gpl, gw, 1});
    SFA_HIP(ctx, hipGetLastError());
    for (int c = 0; c < 3; c++) SFA_TRY(download_plane(ctx, lab + (size_t)c * gh * lab_stride, lab_stride, dst.f() + c * gpl, gw, gw, gh));
    if (rgb8) SFA_TRY(download(ctx, rgb8, dst8.p, 3 * gpl));
    return sfa_ctx_sync(ctx);
}

}  // extern "C"

#pragma clang attribute pop
