// epic_filter.hip -- what epic() (host/epic.cpp, epic_flow_extended/epic.cpp:15-123, :196-198) does between its graph searches and its fit, for a batch of
// images, operation for operation: every kernel runs one grid over the sub-batch with blockIdx.y as the image.  fp32 without contraction, as everywhere.
//   k_ef_clamp             the four columns of every match to [0, w - 1] / [0, h - 1] (epic.cpp:15-28)
//   k_ef_autocorr, k_ef_eigen   the two pixelwise steps of the saliency (image.c:729-791) between the Gaussian and the 3-tap launches of kernels.hip
//   k_ef_saliency_flags    keep match k when sal[(int)(y1 * stride + x1)] >= th: the host's FLOAT index with the host image's stride, truncated, then
//                          taken apart into the row and column it names; a column in the host image's padding reads 0 (image_erase left it so), and so does
//                          an index past the image (only a rounding of the float sum at more than 2^24 pixels gets there; the host reads out of bounds)
//   k_ef_consistency_flags keep when |estimate - vector|^2 < pref_th^2 (epic.cpp:77-123)
//   k_ef_block_count, k_ef_offsets, k_ef_scatter   stable compaction in list order, built as sfa_fill_matches' (fill.hip): the 1s of every block of 256, one
//                          block per image turns them into exclusive prefix sums and the total, then every kept match moves to offset + the 1s before it
//   k_ef_seeds_vects       seeds = ((int)x1, (int)y1), vects = (x2 - x1, y2 - y1) (epic.cpp:31-56)
// The kernel weights (epic_weights_device) are kernels.hip's k_epic_weights: they need glibc's expf as restated there (expf_glibc), and there is one copy of it.
#include "sfa_device.h"
#include "sfa_internal.h"

#pragma clang fp contract(off)

namespace sfa {
namespace {

constexpr int kEfThreads = 256;
inline int blocks(size_t n, int per) { return (int)((n + per - 1) / per); }

// std::max / std::min as the host code calls them: the first argument unless the comparison says otherwise, so max(0.f, -0.f) is +0 and a NaN gives way to 0
__device__ __forceinline__ float max_std(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ float min_std(float a, float b) { return b < a ? b : a; }

__global__ void __launch_bounds__(kEfThreads) k_ef_clamp(const EpicFilterImg *imgs, int w, int h) {
    const EpicFilterImg im = imgs[blockIdx.y];
    const int k = blockIdx.x * kEfThreads + threadIdx.x;
    if (k >= im.count) return;
    float4 m = im.in[k];
    const float xm = (float)(w - 1), ym = (float)(h - 1);
    m.x = max_std(0.f, min_std(m.x, xm)); m.y = max_std(0.f, min_std(m.y, ym));
    m.z = max_std(0.f, min_std(m.z, xm)); m.w = max_std(0.f, min_std(m.w, ym));
    im.in[k] = m;
}

// planes of image b: ix at dx + b es + c pl, iy at dy likewise; out: xx, xy, yy at o + b es + {0, 1, 2} pl
__global__ void k_ef_autocorr(const float *__restrict__ dx, const float *__restrict__ dy, float *__restrict__ o, Geo g) {
    const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y, b = blockIdx.z;
    if (x >= g.w || y >= g.h) return;
    const size_t p = (size_t)b * g.es + (size_t)y * g.pitch + x;
    const float x0 = dx[p], x1 = dx[p + g.pl], x2 = dx[p + 2 * g.pl], y0 = dy[p], y1 = dy[p + g.pl], y2 = dy[p + 2 * g.pl];
    o[p] = x0 * x0 + x1 * x1 + x2 * x2;                              // summed over the channels left to right
    o[p + g.pl] = x0 * y0 + x1 * y1 + x2 * y2;
    o[p + 2 * g.pl] = y0 * y0 + y1 * y1 + y2 * y2;
}

// the smallest eigenvalue of the smoothed matrix (xx, xy, yy at m + b es + {0, 1, 2} pl) -> out + b es
__global__ void k_ef_eigen(const float *__restrict__ m, float *__restrict__ out, Geo g) {
    const int x = blockIdx.x * BX + threadIdx.x, y = blockIdx.y * BY + threadIdx.y, b = blockIdx.z;
    if (x >= g.w || y >= g.h) return;
    const size_t p = (size_t)b * g.es + (size_t)y * g.pitch + x;
    const float xx = m[p], xy = m[p + g.pl], yy = m[p + 2 * g.pl];
    const float t = 0.5f * (xx + yy);
    const float d = max_std(0.0f, t * t + xy * xy - xx * yy);
    out[p] = sqrt_rn(max_std(0.0f, t - sqrt_rn(d)));
}

__global__ void __launch_bounds__(kEfThreads) k_ef_saliency_flags(const EpicFilterImg *imgs, int w, int h, int stride, int pitch, float th) {
    const EpicFilterImg im = imgs[blockIdx.y];
    const int k = blockIdx.x * kEfThreads + threadIdx.x;
    if (k >= im.count) return;
    const float4 m = im.in[k];
    const int idx = (int)(m.y * (float)stride + m.x);                // s->data[(int)(m[i + 1] * s->stride + m[i])]: int * float is a float product
    const int row = idx / stride, col = idx % stride;
    const float s = (idx >= 0 && row < h && col < w) ? im.sal[(size_t)row * pitch + col] : 0.0f;
    im.flag[k] = s >= th;
}

__global__ void __launch_bounds__(kEfThreads) k_ef_consistency_flags(const EpicFilterImg *imgs, float th2) {
    const EpicFilterImg im = imgs[blockIdx.y];
    const int k = blockIdx.x * kEfThreads + threadIdx.x;
    if (k >= im.count) return;
    const float2 v = im.vects[k];
    const float ex = im.est[2 * k] - v.x, ey = im.est[2 * k + 1] - v.y;
    im.flag[k] = ex * ex + ey * ey < th2;
}

__global__ void __launch_bounds__(kEfThreads) k_ef_block_count(const EpicFilterImg *imgs) {
    const EpicFilterImg im = imgs[blockIdx.y];
    const int k = blockIdx.x * kEfThreads + threadIdx.x;             // (a block is wholly inside or wholly outside the grid's x range of its image)
    if (blockIdx.x * kEfThreads >= im.count) return;
    const int c = __syncthreads_count(k < im.count && im.flag[k] != 0);
    if (threadIdx.x == 0) im.block_off[blockIdx.x] = c;
}

// one block per image: block_off -> its exclusive prefix sums, *kept = the total
__global__ void __launch_bounds__(kEfThreads) k_ef_offsets(const EpicFilterImg *imgs) {
    __shared__ int part[kEfThreads];
    const EpicFilterImg im = imgs[blockIdx.x];
    const int nblocks = (im.count + kEfThreads - 1) / kEfThreads;
    int carry = 0;
    for (int b0 = 0; b0 < nblocks; b0 += kEfThreads) {
        const int b = b0 + threadIdx.x, v = b < nblocks ? im.block_off[b] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < kEfThreads; d <<= 1) {                   // inclusive scan of the chunk
            const int t = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        if (b < nblocks) im.block_off[b] = carry + part[threadIdx.x] - v;
        carry += part[kEfThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) *im.kept = carry;
}

__global__ void __launch_bounds__(kEfThreads) k_ef_scatter(const EpicFilterImg *imgs) {
    __shared__ int wave_ones[kEfThreads / 64];
    const EpicFilterImg im = imgs[blockIdx.y];
    if (blockIdx.x * kEfThreads >= im.count) return;
    const int k = blockIdx.x * kEfThreads + threadIdx.x;
    const bool one = k < im.count && im.flag[k] != 0;
    const unsigned long long ballot = __ballot(one);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_ones[wave] = __popcll(ballot);
    __syncthreads();
    if (!one) return;
    int row = im.block_off[blockIdx.x] + __popcll(ballot & ((1ull << lane) - 1));
    for (int j = 0; j < wave; j++) row += wave_ones[j];
    im.out[row] = im.in[k];                                          // row <= k < the list's capacity
}

__global__ void __launch_bounds__(kEfThreads) k_ef_seeds_vects(const EpicFilterImg *imgs) {
    const EpicFilterImg im = imgs[blockIdx.y];
    const int k = blockIdx.x * kEfThreads + threadIdx.x;
    if (k >= im.count) return;
    const float4 m = im.in[k];
    im.seeds[k] = make_int2((int)m.x, (int)m.y);
    im.vects[k] = make_float2(m.z - m.x, m.w - m.y);
}

// The edge costs of the epic() calls of one rate's steps (the track job's fill-in, track.hip).  host/epic_fill.cpp:47-56 with epic()'s own addition (host/epic.cpp:342): the map is shared by every epic() call of
// a start_jet, and each call adds euc to it on entry, so step j of a rate whose first call has index c reads the file's map after c + j + 1 sequential fp32
// additions -- repeated additions, never a product.  run: [ns][cpl], the map after the c additions of the calls before this rate, left after c + rJ; cost:
// [ns][rJ][cpl], the planes the interpolation reads.  cpl is a multiple of 4 and the bases are 256-byte aligned: one thread carries four pixels of segment
// blockIdx.y through the steps with 16-byte accesses, the thread at a plane's end its 1 .. 3 pixels one by one.  euc == 0 adds nothing (`if (params->euc)`)
__global__ void __launch_bounds__(kEfThreads) k_ef_edge_costs(float *__restrict__ run, float *__restrict__ cost, int rJ, size_t cpl, int gpl, float euc) {
    const size_t i = ((size_t)blockIdx.x * kEfThreads + threadIdx.x) * 4;
    if (i >= (size_t)gpl) return;
    float *r = run + (size_t)blockIdx.y * cpl, *c = cost + (size_t)blockIdx.y * rJ * cpl;
    if (i + 4 <= (size_t)gpl) {
        float4 v = *reinterpret_cast<const float4 *>(r + i);
#pragma unroll 1
        for (int j = 0; j < rJ; j++) {
            if (euc != 0.0f) { v.x += euc; v.y += euc; v.z += euc; v.w += euc; }
            *reinterpret_cast<float4 *>(c + (size_t)j * cpl + i) = v;
        }
        *reinterpret_cast<float4 *>(r + i) = v;
        return;
    }
    for (size_t k = i; k < (size_t)gpl; k++) {
        float v = r[k];
#pragma unroll 1
        for (int j = 0; j < rJ; j++) {
            if (euc != 0.0f) v += euc;
            c[(size_t)j * cpl + k] = v;
        }
        r[k] = v;
    }
}

}  // namespace

// the launch functions: compiled for size (see track.hip)
#pragma clang attribute push(__attribute__((minsize)), apply_to = function)

void epic_clamp_device(sfa_ctx *ctx, int m, int count_max, int w, int h, const EpicFilterImg *d_imgs) {
    if (count_max > 0) hipLaunchKernelGGL(k_ef_clamp, dim3(blocks(count_max, kEfThreads), m), dim3(kEfThreads), 0, ctx->stream, d_imgs, w, h);
}
void epic_saliency_flags_device(sfa_ctx *ctx, int m, int count_max, int w, int h, int pitch, float th, const EpicFilterImg *d_imgs) {
    if (count_max > 0) {
        hipLaunchKernelGGL(k_ef_saliency_flags, dim3(blocks(count_max, kEfThreads), m), dim3(kEfThreads), 0, ctx->stream, d_imgs, w, h, host_stride(w), pitch, th);
    }
}
void epic_consistency_flags_device(sfa_ctx *ctx, int m, int count_max, float th2, const EpicFilterImg *d_imgs) {
    if (count_max > 0) hipLaunchKernelGGL(k_ef_consistency_flags, dim3(blocks(count_max, kEfThreads), m), dim3(kEfThreads), 0, ctx->stream, d_imgs, th2);
}
void epic_compact_device(sfa_ctx *ctx, int m, int count_max, const EpicFilterImg *d_imgs) {
    const dim3 grid(blocks(count_max, kEfThreads), m), block(kEfThreads);
    if (count_max > 0) hipLaunchKernelGGL(k_ef_block_count, grid, block, 0, ctx->stream, d_imgs);
    hipLaunchKernelGGL(k_ef_offsets, dim3(m), block, 0, ctx->stream, d_imgs);      // (an empty list: kept = 0)
    if (count_max > 0) hipLaunchKernelGGL(k_ef_scatter, grid, block, 0, ctx->stream, d_imgs);
}
void epic_seeds_vects_device(sfa_ctx *ctx, int m, int count_max, const EpicFilterImg *d_imgs) {
    if (count_max > 0) hipLaunchKernelGGL(k_ef_seeds_vects, dim3(blocks(count_max, kEfThreads), m), dim3(kEfThreads), 0, ctx->stream, d_imgs);
}

void epic_saliency_device(sfa_ctx *ctx, const Geo &g, float *planes, float sigma_image, float sigma_matrix) {
    float *lab = planes, *tmp = planes + 3 * g.pl, *sim = planes + 6 * g.pl, *ix = planes + 9 * g.pl, *iy = planes + 12 * g.pl;
    launch_presmooth(ctx, g, sim, tmp, lab, 3, sigma_image);         // smooth, then the 3-tap derivatives of the smoothed image
    launch_convolve(ctx, g, ix, sim, 1, 1, 3);
    launch_convolve(ctx, g, iy, sim, 1, 0, 3);
    hipLaunchKernelGGL(k_ef_autocorr, grid2d(g), block2d(), 0, ctx->stream, ix, iy, lab, g);       // xx, xy, yy over the Lab planes, which are not read again
    launch_presmooth(ctx, g, sim, tmp, lab, 3, sigma_matrix);        // integrate it
    hipLaunchKernelGGL(k_ef_eigen, grid2d(g), block2d(), 0, ctx->stream, sim, planes + (size_t)kEpicSaliencyOut * g.pl, g);
}

int epic_edge_costs_device(sfa_ctx *ctx, int ns, int rJ, size_t cpl, int gpl, float euc, float *run, float *cost) {
    const unsigned quads = (unsigned)(((size_t)gpl + 3) / 4);
    hipLaunchKernelGGL(k_ef_edge_costs, dim3(blocks(quads, kEfThreads), (unsigned)ns), dim3(kEfThreads), 0, ctx->stream, run, cost, rJ, cpl, gpl, euc);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

#pragma clang attribute pop

}  // namespace sfa
