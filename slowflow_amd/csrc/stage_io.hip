// stage_io.hip -- the host side of dense_tracking's stages, written once for the stage wrappers (accumulate.hip, energy.hip, fuse.hip, neigh.hip) and the
// track job (track*.hip): the one-line forms of the stream calls, and the uploads that bring host planes at a row stride into the kernels' layouts -- frames
// and decoded masks packed, flow fields as planes of (u, v) pairs.  Only a row's valid columns are copied; everything enqueues and returns without waiting.
#include <algorithm>

#include "sfa_internal.h"

#pragma clang fp contract(off)

namespace sfa {

constexpr int kIoThreads = 256;

// (u, v) planes -> float2 planes, n planes of pl values each
__global__ void __launch_bounds__(kIoThreads) k_interleave(const float *__restrict__ u, const float *__restrict__ v, float2 *__restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * kIoThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kIoThreads) out[i] = make_float2(u[i], v[i]);
}

void launch_interleave(sfa_ctx *ctx, const float *u, const float *v, float2 *out, size_t n) {
    const int blocks = (int)std::min<size_t>((n + kIoThreads - 1) / kIoThreads, (size_t)ctx->cu_count * 8);
    hipLaunchKernelGGL(k_interleave, dim3(blocks), dim3(kIoThreads), 0, ctx->stream, u, v, out, n);
}

// The rest is a few microseconds of host code per call beside milliseconds of kernels: compiled for size, like the job's files (see track.hip)
#pragma clang attribute push(__attribute__((minsize)), apply_to = function)

int copy_on(sfa_ctx *ctx, void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    SFA_HIP(ctx, hipMemcpyAsync(dst, src, bytes, kind, ctx->stream));
    return SFA_OK;
}
int zero_on(sfa_ctx *ctx, void *dst, size_t bytes) {
    SFA_HIP(ctx, hipMemsetAsync(dst, 0, bytes, ctx->stream));
    return SFA_OK;
}
int mark(sfa_ctx *ctx, hipEvent_t e) {
    SFA_HIP(ctx, hipEventRecord(e, ctx->stream));
    return SFA_OK;
}
int copy_rows_on(sfa_ctx *ctx, void *dst, size_t dpitch, const void *src, size_t spitch, size_t row, size_t h, hipMemcpyKind kind) {
    SFA_HIP(ctx, hipMemcpy2DAsync(dst, dpitch, src, spitch, row, h, kind, ctx->stream));
    return SFA_OK;
}
int download(sfa_ctx *ctx, void *dst, const void *src, size_t bytes) { return dst ? copy_on(ctx, dst, src, bytes, hipMemcpyDeviceToHost) : (int)SFA_OK; }

int upload_frames(sfa_ctx *ctx, size_t nf, const float *const *frames, int stride, int w, int h, float *dst) {
    for (size_t k = 0; k < nf; k++)
        for (int c = 0; c < 3; c++)
            SFA_TRY(copy_rows_on(ctx, dst + (k * 3 + c) * w * h, (size_t)w * 4, frames[k] + (size_t)c * h * stride, (size_t)stride * 4, (size_t)w * 4, h, hipMemcpyHostToDevice));
    return SFA_OK;
}

int upload_masks(sfa_ctx *ctx, size_t np, const unsigned char *const *masks, int stride, int w, int h, unsigned char *dst) {
    for (size_t k = 0; k < np; k++) SFA_TRY(copy_rows_on(ctx, dst + k * (size_t)w * h, (size_t)w, masks[k], (size_t)stride, (size_t)w, h, hipMemcpyHostToDevice));
    return SFA_OK;
}

int upload_flow_pairs(sfa_ctx *ctx, const sfa_jet_source &src, bool identity, size_t np, const float *const *u, const float *const *v, int w, int h, float *stage,
                      void *dst, hipEvent_t before, hipEvent_t after) {
    if (!identity) return jet_resample_flows(ctx, src, np, u, v, w, h, stage, static_cast<double2 *>(dst), before, after);
    const size_t pl = (size_t)w * h;
    float *su = stage, *sv = stage + np * pl;
    for (size_t k = 0; k < np; k++) {                                           // the valid columns of each plane, packed, then interleaved
        SFA_TRY(copy_rows_on(ctx, su + k * pl, (size_t)w * 4, u[k], (size_t)src.stride * 4, (size_t)w * 4, h, hipMemcpyHostToDevice));
        SFA_TRY(copy_rows_on(ctx, sv + k * pl, (size_t)w * 4, v[k], (size_t)src.stride * 4, (size_t)w * 4, h, hipMemcpyHostToDevice));
    }
    if (before) SFA_TRY(mark(ctx, before));
    launch_interleave(ctx, su, sv, static_cast<float2 *>(dst), np * pl);
    SFA_HIP(ctx, hipGetLastError());
    if (after) SFA_TRY(mark(ctx, after));
    return SFA_OK;
}

#pragma clang attribute pop

}  // namespace sfa
