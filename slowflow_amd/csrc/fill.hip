// fill.hip -- what dense_tracking does around its EpicFlow fill-in (dense_tracking.cpp:1265-1310), on the GPU, for batches of maps of one size:
//
//   sfa_consistent_regions   removeSmallSegments(r_consistent, 0.1, 100) (utils/utils.cpp:169-284) on r_consistent = (tracked == r_Jets) (:1223-1226, 1265)
//   sfa_fill_matches         the matches of the consistent trajectories at the sampled pixels (:1274-1289)
//   sfa_fill_trajectories    the interpolated planes as trajectories of every pixel (:1304-1310)
//
// Connected regions.  The reference grows segments from seeds in column-major scan order, marks every pixel it reaches as done -- the pixels of a segment
// it then rejects too, so they never join a later segment -- and zeroes the segments of fewer than min_size pixels.  With threshold 0.1 on a 0/1 int map
// "similar" is "equal", so a segment is a 4-connected component of equal values whatever the scan order, and a pixel stays 1 exactly when its component
// of 1s has at least min_size pixels.  That is what the kernels compute, for the whole batch in one launch sequence without a read-back:
//   k_ccl_local    a tile of 64 x 16 pixels in LDS: label equivalence (neighbour minima onto the roots, then flattening) until nothing changes; every
//                  component of the tile ends with the index of its first pixel in raster order, and that pixel holds the component's size
//   k_ccl_merge    the pixel pairs across tile borders: a union of the two tile components' trees, the larger root linked under the smaller by atomicMin
//   k_ccl_sum      every tile component finds its root and adds its size there
//   k_ccl_mask     mask = the root's sum >= min_size, and the number of 1s per map
// A component's root is the smallest pixel index it holds (links only ever go from a larger to a smaller index of the same component), and its size is
// an integer sum: neither depends on the order in which the atomics land, so neither does the mask.  The merge needs no rounds: one union per border pair.
#include "sfa_device.h"

#pragma clang fp contract(off)

namespace sfa {

constexpr int kFillThreads = 256;
constexpr int kTileW = 64, kTileH = 16, kTilePix = kTileW * kTileH;

// T: [n][pl] the tile component of every pixel as the map index of its first pixel, -1 where the map is 0; P: [n][pl] parents of the merge's trees, read
// at tile components' first pixels only; S: [n][pl] sizes there, 0 elsewhere
__global__ void __launch_bounds__(kFillThreads) k_ccl_local(const int *__restrict__ tracked, const int *__restrict__ full, int w, int h, int tiles_x, int tiles_y,
                                                            int *__restrict__ T, int *__restrict__ P, int *__restrict__ S) {
    __shared__ int lab[kTilePix], eq[kTilePix], cnt[kTilePix];
    const int tile = blockIdx.x % (tiles_x * tiles_y), m = blockIdx.x / (tiles_x * tiles_y);
    const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * kTileH;
    const size_t base = (size_t)m * w * h;
    const int want = full[m];
    for (int k = threadIdx.x; k < kTilePix; k += kFillThreads) {
        const int x = x0 + k % kTileW, y = y0 + k / kTileW;
        const bool one = x < w && y < h && tracked[base + (size_t)y * w + x] == want;
        lab[k] = eq[k] = one ? k : -1;
        cnt[k] = 0;
    }
    __syncthreads();
    for (;;) {
        // the smallest label next to each pixel goes onto the pixel's root: eq is written by atomics only, lab is only read
        int changed = 0;
        for (int k = threadIdx.x; k < kTilePix; k += kFillThreads) {
            const int l = lab[k];
            if (l < 0) continue;
            const int lx = k % kTileW, ly = k / kTileW;
            int mn = l;
            if (lx > 0 && lab[k - 1] >= 0) mn = min(mn, lab[k - 1]);
            if (lx + 1 < kTileW && lab[k + 1] >= 0) mn = min(mn, lab[k + 1]);
            if (ly > 0 && lab[k - kTileW] >= 0) mn = min(mn, lab[k - kTileW]);
            if (ly + 1 < kTileH && lab[k + kTileW] >= 0) mn = min(mn, lab[k + kTileW]);
            if (mn < l) { atomicMin(&eq[l], mn); changed = 1; }
        }
        if (!__syncthreads_or(changed)) break;
        // eq is a forest (eq[k] <= k): every pixel takes its root; eq is only read, lab only written
        for (int k = threadIdx.x; k < kTilePix; k += kFillThreads) {
            int l = eq[k];
            if (l < 0) continue;
            while (eq[l] != l) l = eq[l];
            lab[k] = l;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < kTilePix; k += kFillThreads) eq[k] = lab[k];
        __syncthreads();
    }
    for (int k = threadIdx.x; k < kTilePix; k += kFillThreads)
        if (lab[k] >= 0) atomicAdd(&cnt[lab[k]], 1);
    __syncthreads();
    for (int k = threadIdx.x; k < kTilePix; k += kFillThreads) {
        const int x = x0 + k % kTileW, y = y0 + k / kTileW;
        if (x >= w || y >= h) continue;
        const int l = lab[k], g = y * w + x;
        T[base + g] = l < 0 ? -1 : (y0 + l / kTileW) * w + x0 + l % kTileW;
        P[base + g] = g;
        S[base + g] = l == k ? cnt[k] : 0;
    }
}

// The parents change while the merge runs, under other blocks' atomics: they are read past this CU's L1.  A value read late is an ancestor the node had
// before, which is still a node of the same component with an index no smaller than the current one's; the union below is right for any such start.
__device__ __forceinline__ int ccl_parent(const int *P, int a) { return __hip_atomic_load(P + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ccl_find_live(const int *P, int a) {
    for (int p = ccl_parent(P, a); p != a; p = ccl_parent(P, a)) a = p;
    return a;
}
// the larger root goes under the smaller.  Where the node turns out to have a parent already (old != a: another union came first), that parent takes
// the node's place: whichever of the two values atomicMin left in P[a], the other one is united with it in the next turn
__device__ void ccl_union(int *P, int a, int b) {
    for (;;) {
        a = ccl_find_live(P, a);
        b = ccl_find_live(P, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(P + a, b);
        if (old == a) return;
        a = old;
    }
}

// one thread per pixel pair across a tile border: the left neighbours of the columns kTileW, 2 kTileW ..., then the upper neighbours of the rows kTileH ...
__global__ void __launch_bounds__(kFillThreads) k_ccl_merge(int w, int h, int vcols, size_t per_map, size_t total, const int *__restrict__ T,
                                                            int *__restrict__ P) {
    const size_t i = (size_t)blockIdx.x * kFillThreads + threadIdx.x;
    if (i >= total) return;
    const size_t m = i / per_map, k = i % per_map, nv = (size_t)vcols * h;
    int x, y, q;
    if (k < nv) { x = ((int)(k % vcols) + 1) * kTileW; y = (int)(k / vcols); q = y * w + x - 1; }
    else { const size_t e = k - nv; x = (int)(e % w); y = ((int)(e / w) + 1) * kTileH; q = (y - 1) * w + x; }
    const size_t base = m * (size_t)w * h;
    const int ta = T[base + y * w + x], tb = T[base + q];
    if (ta >= 0 && tb >= 0) ccl_union(P + base, ta, tb);
}

// P is final here.  A tile component's first pixel p (T[p] == p) finds its root r, adds its size there and leaves r in T[p]: T[T[q]] is then the root of
// every pixel q of a component (a root's own entry stays itself).  No thread reads another's T entry in this kernel.
__global__ void __launch_bounds__(kFillThreads) k_ccl_sum(int pl, const int *__restrict__ P, int *__restrict__ T, int *__restrict__ S) {
    const int p = blockIdx.x * kFillThreads + threadIdx.x;
    if (p >= pl) return;
    const size_t base = (size_t)blockIdx.y * pl;
    if (T[base + p] != p) return;
    int r = p;
    while (P[base + r] != r) r = P[base + r];
    if (r == p) return;
    T[base + p] = r;
    atomicAdd(S + base + r, S[base + p]);          // p is no root: nothing is added to S[p]
}

__global__ void __launch_bounds__(kFillThreads) k_ccl_mask(int pl, int min_size, const int *__restrict__ T, const int *__restrict__ S,
                                                           unsigned char *__restrict__ mask, int *__restrict__ kept) {
    const int p = blockIdx.x * kFillThreads + threadIdx.x;
    const size_t base = (size_t)blockIdx.y * pl;
    int one = 0;
    if (p < pl) {
        const int t = T[base + p];
        one = t >= 0 && S[base + T[base + t]] >= min_size;
        mask[base + p] = (unsigned char)one;
    }
    const int c = __syncthreads_count(one);
    if (threadIdx.x == 0 && c) atomicAdd(kept + blockIdx.y, c);
}

// ---- matches: the sampled mask in raster order (rows ys, columns xs), compacted by a prefix sum ------------------------------------------------------
// the 1s among a block's kFillThreads samples
__global__ void __launch_bounds__(kFillThreads) k_fill_count(int w, int h, const unsigned char *__restrict__ mask, const int *__restrict__ xs, int nx,
                                                             const int *__restrict__ ys, int ns, int *__restrict__ block_count) {
    const int i = blockIdx.x * kFillThreads + threadIdx.x;
    const int one = i < ns && mask[(size_t)blockIdx.y * w * h + (size_t)ys[i / nx] * w + xs[i % nx]] != 0;
    const int c = __syncthreads_count(one);
    if (threadIdx.x == 0) block_count[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = c;
}
// one block per map: block_count -> its exclusive prefix sums, count[map] = the total
__global__ void __launch_bounds__(kFillThreads) k_fill_offsets(int nblocks, int *__restrict__ block_count, int *__restrict__ count) {
    __shared__ int part[kFillThreads];
    int *bc = block_count + (size_t)blockIdx.x * nblocks;
    int carry = 0;
    for (int b0 = 0; b0 < nblocks; b0 += kFillThreads) {
        const int b = b0 + threadIdx.x, v = b < nblocks ? bc[b] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < kFillThreads; d <<= 1) {                            // inclusive scan of the chunk
            const int t = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += t;
            __syncthreads();
        }
        if (b < nblocks) bc[b] = carry + part[threadIdx.x] - v;
        carry += part[kFillThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) count[blockIdx.x] = carry;
}
// Sample i of a map with mask 1 is row (offset of its block + the 1s before it in the block) of all J steps.  :1283-1286: int + double / int, then the
// conversion to float
__global__ void __launch_bounds__(kFillThreads) k_fill_rows(int J, int w, int h, const double *__restrict__ acc_u, const double *__restrict__ acc_v,
                                                            const unsigned char *__restrict__ mask, const int *__restrict__ xs, int nx,
                                                            const int *__restrict__ ys, int ns, int divisor, const int *__restrict__ block_offset,
                                                            float4 *__restrict__ matches) {
    __shared__ int wave_ones[kFillThreads / 64];
    const int i = blockIdx.x * kFillThreads + threadIdx.x, m = blockIdx.y;
    const size_t pl = (size_t)w * h;
    int x = 0, y = 0;
    bool one = false;
    if (i < ns) {
        x = xs[i % nx]; y = ys[i / nx];
        one = mask[m * pl + (size_t)y * w + x] != 0;
    }
    const unsigned long long ballot = __ballot(one);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_ones[wave] = __popcll(ballot);
    __syncthreads();
    if (!one) return;
    int row = block_offset[(size_t)m * gridDim.x + blockIdx.x] + __popcll(ballot & ((1ull << lane) - 1));
    for (int k = 0; k < wave; k++) row += wave_ones[k];
    const size_t o = (size_t)y * w + x;
    for (int j = 0; j < J; j++) {
        const size_t plane = ((size_t)m * J + j) * pl;
        const double tx = x + acc_u[plane + o] / divisor, ty = y + acc_v[plane + o] / divisor;
        matches[((size_t)m * J + j) * ns + row] = make_float4((float)x, (float)y, (float)tx, (float)ty);
    }
}

// ---- trajectories: planes [np][h][stride] floats -> acc [np][h][w] doubles (:1304-1305: float * int, widened) and tracked [n][h][w] = J (:1299) -------
__global__ void __launch_bounds__(kFillThreads) k_fill_trajectories(int J, int w, int h, int stride, float scale, const float *__restrict__ fx,
                                                                    const float *__restrict__ fy, double *__restrict__ acc_u, double *__restrict__ acc_v,
                                                                    int *__restrict__ tracked) {
    const int p = blockIdx.x * kFillThreads + threadIdx.x;
    if (p >= w * h) return;
    const size_t plane = blockIdx.y, src = plane * h * stride + (size_t)(p / w) * stride + p % w, dst = plane * w * h + p;
    acc_u[dst] = (double)(fx[src] * scale);
    acc_v[dst] = (double)(fy[src] * scale);
    if (plane % J == 0) tracked[plane / J * w * h + p] = J;
}

int consistent_regions_device(sfa_ctx *ctx, int n, int w, int h, const int *tracked, const int *full, int min_size, int *T, int *P, int *S, unsigned char *mask,
                              int *kept) {
    const int tiles_x = (w + kTileW - 1) / kTileW, tiles_y = (h + kTileH - 1) / kTileH, pl = w * h;
    const int vcols = tiles_x - 1, hrows = tiles_y - 1;
    const size_t per_map = (size_t)vcols * h + (size_t)hrows * w, pairs = per_map * n;
    SFA_HIP(ctx, hipMemsetAsync(kept, 0, (size_t)n * sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_ccl_local, dim3((unsigned)((size_t)tiles_x * tiles_y * n)), dim3(kFillThreads), 0, ctx->stream, tracked, full, w, h, tiles_x, tiles_y, T, P, S);
    if (pairs)
        hipLaunchKernelGGL(k_ccl_merge, dim3((unsigned)((pairs + kFillThreads - 1) / kFillThreads)), dim3(kFillThreads), 0, ctx->stream, w, h, vcols, per_map, pairs,
                           T, P);
    const dim3 grid((unsigned)((pl + kFillThreads - 1) / kFillThreads), (unsigned)n);
    hipLaunchKernelGGL(k_ccl_sum, grid, dim3(kFillThreads), 0, ctx->stream, pl, P, T, S);
    hipLaunchKernelGGL(k_ccl_mask, grid, dim3(kFillThreads), 0, ctx->stream, pl, min_size, T, S, mask, kept);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

size_t fill_matches_blocks(int nx, int ny) { return ((size_t)nx * ny + kFillThreads - 1) / kFillThreads; }

int fill_matches_device(sfa_ctx *ctx, int n, int J, int w, int h, const double *acc_u, const double *acc_v, const unsigned char *mask, const int *xs, int nx,
                        const int *ys, int ny, int divisor, int *block_count, float *matches, int *count) {
    const int ns = nx * ny, nblocks = (int)fill_matches_blocks(nx, ny);
    const dim3 grid((unsigned)nblocks, (unsigned)n);
    hipLaunchKernelGGL(k_fill_count, grid, dim3(kFillThreads), 0, ctx->stream, w, h, mask, xs, nx, ys, ns, block_count);
    hipLaunchKernelGGL(k_fill_offsets, dim3((unsigned)n), dim3(kFillThreads), 0, ctx->stream, nblocks, block_count, count);
    hipLaunchKernelGGL(k_fill_rows, grid, dim3(kFillThreads), 0, ctx->stream, J, w, h, acc_u, acc_v, mask, xs, nx, ys, ns, divisor, block_count,
                       reinterpret_cast<float4 *>(matches));
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int fill_trajectories_device(sfa_ctx *ctx, int n, int J, int w, int h, int stride, const float *flow_x, const float *flow_y, int scale, double *acc_u,
                             double *acc_v, int *tracked) {
    const dim3 grid((unsigned)((w * h + kFillThreads - 1) / kFillThreads), (unsigned)(n * J));
    hipLaunchKernelGGL(k_fill_trajectories, grid, dim3(kFillThreads), 0, ctx->stream, J, w, h, stride, (float)scale, flow_x, flow_y, acc_u, acc_v, tracked);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

}  // namespace sfa

using namespace sfa;

// the entry points: argument checks, allocations, copies around the launch functions above.  Compiled for size (see track.hip)
#pragma clang attribute push(__attribute__((minsize)), apply_to = function)

constexpr int kMaxFillMaps = 65535;             // a map (or a plane) is a grid row

int sfa_fill_samples(int extent, float epic_skip, int *out, int *count) {
    if (!count) return set_error(nullptr, SFA_ERR_ARG, "sfa_fill_samples: count: null pointer");
    // x + epic_skip is an fp32 sum: up to extent + epic_skip <= 2^24 every int is a float and a step of at least 1 advances x
    if (extent < 1 || extent > (1 << 23)) return set_error(nullptr, SFA_ERR_ARG, "sfa_fill_samples: extent %d (1 .. 2^23)", extent);
    if (!(epic_skip >= 1.0f && epic_skip <= 1e6f)) return set_error(nullptr, SFA_ERR_ARG, "sfa_fill_samples: epic_skip %g (1 .. 1e6: a smaller step never advances)", epic_skip);
    int c = 0;
    for (int x = floor(0.5f * epic_skip); x < extent; x += epic_skip) {         // :1278-1279 as written: x += a float truncates the sum
        if (out) out[c] = x;
        c++;
    }
    *count = c;
    return SFA_OK;
}

int sfa_consistent_regions(sfa_ctx *ctx, int n, int w, int h, const int *tracked, const int *full, int min_size, unsigned char *mask, int *kept) {
    if (!ctx) return set_error(nullptr, SFA_ERR_ARG, "%s: ctx: null pointer", __func__);
    if (!tracked) REFUSE("%s: tracked: null pointer", __func__);
    if (!full) REFUSE("%s: full: null pointer", __func__);
    if (!mask) REFUSE("%s: mask: null pointer", __func__);
    if (!kept) REFUSE("%s: kept: null pointer", __func__);
    if (n < 1 || n > kMaxFillMaps) REFUSE("%s: n = %d (1 .. %d maps)", __func__, n, kMaxFillMaps);
    if (w < 1) REFUSE("%s: w = %d (>= 1)", __func__, w);
    if (h < 1) REFUSE("%s: h = %d (>= 1)", __func__, h);
    if (min_size < 1) REFUSE("%s: min_size = %d (>= 1)", __func__, min_size);
    if ((long long)w * h > (1ll << 29)) REFUSE("%s: w * h = %lld (at most 2^29: 32-bit pixel indices)", __func__, (long long)w * h);
    const size_t px = (size_t)n * w * h, tiles = (size_t)((w + kTileW - 1) / kTileW) * ((h + kTileH - 1) / kTileH) * n;
    if (tiles > 0x7fffffffull) REFUSE("%s: n = %d maps of %d x %d are %zu tiles (at most 2^31 - 1 in one launch)", __func__, n, w, h, tiles);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem dtr, dfull, dT, dP, dS, dmask, dkept;
    SFA_TRY(dtr.alloc(ctx, px * 4)); SFA_TRY(dfull.alloc(ctx, (size_t)n * 4)); SFA_TRY(dT.alloc(ctx, px * 4)); SFA_TRY(dP.alloc(ctx, px * 4));
    SFA_TRY(dS.alloc(ctx, px * 4)); SFA_TRY(dmask.alloc(ctx, px)); SFA_TRY(dkept.alloc(ctx, (size_t)n * 4));
    SFA_HIP(ctx, hipMemcpyAsync(dtr.p, tracked, px * 4, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(dfull.p, full, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    SFA_TRY(consistent_regions_device(ctx, n, w, h, static_cast<int *>(dtr.p), static_cast<int *>(dfull.p), min_size, static_cast<int *>(dT.p),
                                      static_cast<int *>(dP.p), static_cast<int *>(dS.p), static_cast<unsigned char *>(dmask.p), static_cast<int *>(dkept.p)));
    SFA_HIP(ctx, hipMemcpyAsync(mask, dmask.p, px, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(kept, dkept.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

int sfa_fill_matches(sfa_ctx *ctx, int n, int J, int w, int h, const double *acc_u, const double *acc_v, const unsigned char *mask, const int *xs, int nx,
                     const int *ys, int ny, int divisor, float *matches, int *count) {
    if (!ctx) return set_error(nullptr, SFA_ERR_ARG, "%s: ctx: null pointer", __func__);
    if (!acc_u) REFUSE("%s: acc_u: null pointer", __func__);
    if (!acc_v) REFUSE("%s: acc_v: null pointer", __func__);
    if (!mask) REFUSE("%s: mask: null pointer", __func__);
    if (!xs) REFUSE("%s: xs: null pointer", __func__);
    if (!ys) REFUSE("%s: ys: null pointer", __func__);
    if (!matches) REFUSE("%s: matches: null pointer", __func__);
    if (!count) REFUSE("%s: count: null pointer", __func__);
    if (n < 1 || n > kMaxFillMaps) REFUSE("%s: n = %d (1 .. %d maps)", __func__, n, kMaxFillMaps);
    if (J < 1) REFUSE("%s: J = %d (>= 1)", __func__, J);
    if (w < 1) REFUSE("%s: w = %d (>= 1)", __func__, w);
    if (h < 1) REFUSE("%s: h = %d (>= 1)", __func__, h);
    if ((long long)w * h > (1ll << 29)) REFUSE("%s: w * h = %lld (at most 2^29: 32-bit pixel indices)", __func__, (long long)w * h);
    if (nx < 1 || nx > w) REFUSE("%s: nx = %d (1 .. w)", __func__, nx);
    if (ny < 1 || ny > h) REFUSE("%s: ny = %d (1 .. h)", __func__, ny);
    if (divisor < 1) REFUSE("%s: divisor = %d (>= 1: acc_skip_pixel + 1)", __func__, divisor);
    for (int i = 0; i < nx; i++)
        if (xs[i] < 0 || xs[i] >= w) REFUSE("%s: xs[%d] = %d is outside the map (w = %d)", __func__, i, xs[i], w);
    for (int i = 0; i < ny; i++)
        if (ys[i] < 0 || ys[i] >= h) REFUSE("%s: ys[%d] = %d is outside the map (h = %d)", __func__, i, ys[i], h);
    const size_t pl = (size_t)w * h, ns = (size_t)nx * ny, nblocks = fill_matches_blocks(nx, ny);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem dau, dav, dmask, dxs, dys, dbc, dmatch, dcount;
    SFA_TRY(dau.alloc(ctx, (size_t)n * J * pl * 8)); SFA_TRY(dav.alloc(ctx, (size_t)n * J * pl * 8)); SFA_TRY(dmask.alloc(ctx, (size_t)n * pl));
    SFA_TRY(dxs.alloc(ctx, (size_t)nx * 4)); SFA_TRY(dys.alloc(ctx, (size_t)ny * 4)); SFA_TRY(dbc.alloc(ctx, (size_t)n * nblocks * 4));
    SFA_TRY(dmatch.alloc(ctx, (size_t)n * J * ns * 16)); SFA_TRY(dcount.alloc(ctx, (size_t)n * 4));
    SFA_HIP(ctx, hipMemcpyAsync(dau.p, acc_u, (size_t)n * J * pl * 8, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(dav.p, acc_v, (size_t)n * J * pl * 8, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(dmask.p, mask, (size_t)n * pl, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(dxs.p, xs, (size_t)nx * 4, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(dys.p, ys, (size_t)ny * 4, hipMemcpyHostToDevice, ctx->stream));
    SFA_TRY(fill_matches_device(ctx, n, J, w, h, static_cast<double *>(dau.p), static_cast<double *>(dav.p), static_cast<unsigned char *>(dmask.p),
                                static_cast<int *>(dxs.p), nx, static_cast<int *>(dys.p), ny, divisor, static_cast<int *>(dbc.p), dmatch.f(),
                                static_cast<int *>(dcount.p)));
    SFA_HIP(ctx, hipMemcpyAsync(count, dcount.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < (size_t)n * J; k++)                                  // the rows that exist: nothing is written behind a map's count
        if (count[k / J] > 0)
            SFA_HIP(ctx, hipMemcpyAsync(matches + k * ns * 4, dmatch.f() + k * ns * 4, (size_t)count[k / J] * 16, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

int sfa_fill_trajectories(sfa_ctx *ctx, int n, int J, int w, int h, int stride, const float *const *flow_x, const float *const *flow_y, int scale,
                          double *acc_u, double *acc_v, int *tracked) {
    if (!ctx) return set_error(nullptr, SFA_ERR_ARG, "%s: ctx: null pointer", __func__);
    if (!flow_x) REFUSE("%s: flow_x: null pointer", __func__);
    if (!flow_y) REFUSE("%s: flow_y: null pointer", __func__);
    if (!acc_u) REFUSE("%s: acc_u: null pointer", __func__);
    if (!acc_v) REFUSE("%s: acc_v: null pointer", __func__);
    if (!tracked) REFUSE("%s: tracked: null pointer", __func__);
    if (n < 1) REFUSE("%s: n = %d (>= 1)", __func__, n);
    if (J < 1) REFUSE("%s: J = %d (>= 1)", __func__, J);
    if ((long long)n * J > kMaxFillMaps) REFUSE("%s: n * J = %lld (at most %d planes)", __func__, (long long)n * J, kMaxFillMaps);
    if (w < 1) REFUSE("%s: w = %d (>= 1)", __func__, w);
    if (h < 1) REFUSE("%s: h = %d (>= 1)", __func__, h);
    if (stride < w) REFUSE("%s: stride = %d (>= w = %d)", __func__, stride, w);
    if ((long long)stride * h > (1ll << 29)) REFUSE("%s: stride * h = %lld (at most 2^29: 32-bit pixel indices)", __func__, (long long)stride * h);
    if (scale < 1) REFUSE("%s: scale = %d (>= 1: acc_skip_pixel + 1)", __func__, scale);
    const size_t np = (size_t)n * J, pl = (size_t)w * h, spl = (size_t)stride * h;
    for (size_t k = 0; k < np; k++) {
        if (!flow_x[k]) REFUSE("%s: flow_x[%zu]: null pointer", __func__, k);
        if (!flow_y[k]) REFUSE("%s: flow_y[%zu]: null pointer", __func__, k);
    }
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem dfx, dfy, dau, dav, dtr;
    SFA_TRY(dfx.alloc(ctx, np * spl * 4)); SFA_TRY(dfy.alloc(ctx, np * spl * 4)); SFA_TRY(dau.alloc(ctx, np * pl * 8)); SFA_TRY(dav.alloc(ctx, np * pl * 8));
    SFA_TRY(dtr.alloc(ctx, (size_t)n * pl * 4));
    const size_t last = (size_t)(h - 1) * stride + w;                           // a plane's last row may end at column w
    for (size_t k = 0; k < np; k++) {
        SFA_HIP(ctx, hipMemcpyAsync(dfx.f() + k * spl, flow_x[k], last * 4, hipMemcpyHostToDevice, ctx->stream));
        SFA_HIP(ctx, hipMemcpyAsync(dfy.f() + k * spl, flow_y[k], last * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    SFA_TRY(fill_trajectories_device(ctx, n, J, w, h, stride, dfx.f(), dfy.f(), scale, static_cast<double *>(dau.p), static_cast<double *>(dav.p),
                                     static_cast<int *>(dtr.p)));
    SFA_HIP(ctx, hipMemcpyAsync(acc_u, dau.p, np * pl * 8, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(acc_v, dav.p, np * pl * 8, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(tracked, dtr.p, (size_t)n * pl * 4, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

#pragma clang attribute pop
