// epic_fit.hip -- sfa_epic_interpolate_batch: EpicFlow's per-seed model fit and its dense application (host/epic.cpp: epic_fit_localaffine with solve3,
// epic_fit_nadarayawatson, the two apply loops of epic(); epic_aux.cpp:386-497) for a batch of images of one size, operation for operation, so that the models
// and both flow planes equal the host's bit for bit.  The library's -ffp-contract=off -fno-fast-math hold here as everywhere: no product is fused into a sum.
//   k_epic_fit<LA>   one lane owns one seed from its first list entry to the rounded model: fp32 products, fp64 sums of the normal matrix (six entries: the
//                    mirrored products are the same bits) and of the two right-hand sides in list order, the `s == i` rule, the four 0.1 px points, one
//                    elimination with partial pivoting that carries both right-hand sides (solve3's multipliers depend on the matrix alone, so the host's two
//                    eliminations are this one twice), the all-zero model on a zero pivot
//   k_epic_fit<NW>   fp32 u += d vx, v += d vy, s += d in list order, then u / s, v / s
//   k_epic_apply     one thread per pixel: the affine model of the pixel's label evaluated left to right in fp32, or the label's vector
// The lists are [seed][j] row-major and a lane walks one row, so a wave's plain loads would touch 64 rows per step.  Instead the 64 rows of a wave go through
// LDS in tiles of 32 columns: coalesced loads (a wave instruction reads two rows' 128 contiguous bytes), rows padded to 33 words so that both the
// stores (32 consecutive words of one row) and the loads (one column of 32 rows) are conflict-free.  The full build keeps the plain form behind the switch
// SFA_EPIC_FIT_PLAIN for the comparison in tools/bench_epic_fit.py.
// Entries with an index outside [0, ns) are skipped (the host skips the negative ones and would read out of bounds for the others); a pixel whose label
// lies outside [0, ns) gets 0.0f in both planes -- this library's choice, the host indexes out of bounds there.
#include <algorithm>
#include <climits>
#include <cstring>

#include "sfa_device.h"
#include "sfa_internal.h"

#pragma clang fp contract(off)

namespace sfa {
namespace {

constexpr int kFitLanes = 64;                                        // one wave per workgroup: its tile is its own
constexpr int kFitTile = 32, kFitRow = kFitTile + 1;                 // columns of a tile, words of a padded row
constexpr int kMaxSubBatch = 4096;                                   // images per launch (the grids' second dimension)
constexpr long long kMaxPixels = 1ll << 29;                          // as sfa_epic_nearest_seeds_batch, whose labels these are

using FitImg = EpicFitImg;                                           // what the kernels know of one image (sfa_internal.h)

// f(s, coef, seeds[s], vects[s]) for every entry of seed i's row with 0 <= s < ns, in list order.  Every lane of the workgroup calls this (the barriers);
// `live` says whether the lane has a seed.  The gathers of a tile's entries do not wait for the entry before them: an entry that is skipped reads seed 0
template <bool kStaged, bool kNeedXY, class F>
__device__ inline void for_each_entry(const FitImg &im, int nn, int seed0, int lane, bool live, F f) {
    __shared__ int s_idx[kStaged ? kFitLanes * kFitRow : 1];
    __shared__ float s_w[kStaged ? kFitLanes * kFitRow : 1];
    const int rows = min(kFitLanes, im.ns - seed0), i = seed0 + lane;
    for (int j0 = 0; j0 < nn; j0 += kFitTile) {
        const int cols = min(kFitTile, nn - j0);
        if (kStaged) {
            __syncthreads();                                         // the tile before has been consumed
            for (int e = lane; e < rows * kFitTile; e += kFitLanes) {
                const int r = e / kFitTile, c = e % kFitTile;
                if (c >= cols) continue;
                const size_t g = (size_t)(seed0 + r) * nn + j0 + c;
                s_idx[r * kFitRow + c] = im.index[g];
                s_w[r * kFitRow + c] = im.weight[g];
            }
            __syncthreads();
        }
        if (!live) continue;
#pragma unroll 4
        for (int c = 0; c < cols; c++) {
            int s;
            float coef;
            if (kStaged) {
                s = s_idx[lane * kFitRow + c]; coef = s_w[lane * kFitRow + c];
            } else {
                const size_t g = (size_t)i * nn + j0 + c;
                s = im.index[g]; coef = im.weight[g];
            }
            const bool valid = s >= 0 && s < im.ns;
            const int sc = valid ? s : 0;
            const int2 p = kNeedXY ? im.seeds[sc] : make_int2(0, 0);
            const float2 v = im.vects[sc];
            if (valid) f(s, coef, p, v);
        }
    }
}

// solve3 of host/epic.cpp for the symmetric matrix m (00 01 02 11 12 22) and two right-hand sides at once; out = (px, py) rounded to fp32
__device__ inline void solve3_pair(const double m[6], const double rx[3], const double ry[3], float out[6]) {
    double A[3][5] = {{m[0], m[1], m[2], rx[0], ry[0]}, {m[1], m[3], m[4], rx[1], ry[1]}, {m[2], m[4], m[5], rx[2], ry[2]}};
    bool singular = false;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        int piv = c;
        double best = fabs(A[c][c]);                                 // fabs(A[piv][c])
#pragma unroll
        for (int i = c + 1; i < 3; i++) {
            const double v = fabs(A[i][c]);
            if (v > best) { best = v; piv = i; }
        }
#pragma unroll
        for (int i = c + 1; i < 3; i++)
            if (piv == i) {
#pragma unroll
                for (int j = 0; j < 5; j++) { const double t = A[c][j]; A[c][j] = A[i][j]; A[i][j] = t; }
            }
        if (A[c][c] == 0) { singular = true; break; }
#pragma unroll
        for (int i = c + 1; i < 3; i++) {
            const double f = A[i][c] / A[c][c];
#pragma unroll
            for (int j = c + 1; j < 5; j++) A[i][j] -= f * A[c][j];  // (column c of the rows below is not read again)
        }
    }
    if (singular) {
        for (int k = 0; k < 6; k++) out[k] = 0.0f;
        return;
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
        double o[3];
#pragma unroll
        for (int i = 2; i >= 0; i--) {
            double s = A[i][3 + k];
#pragma unroll
            for (int j = i + 1; j < 3; j++) s -= A[i][j] * o[j];
            o[i] = s / A[i][i];
        }
        out[3 * k] = (float)o[0]; out[3 * k + 1] = (float)o[1]; out[3 * k + 2] = (float)o[2];
    }
}

template <int kMethod, bool kStaged>
__global__ void __launch_bounds__(kFitLanes) k_epic_fit(const FitImg *imgs) {
    const FitImg im = imgs[blockIdx.y];
    const int nn = im.nn;
    const int seed0 = blockIdx.x * kFitLanes, lane = threadIdx.x, i = seed0 + lane;
    if (seed0 >= im.ns) return;                                      // (the whole workgroup)
    const bool live = i < im.ns;
    if (kMethod == 0) {                                              // epic_fit_localaffine
        double m[6] = {0, 0, 0, 0, 0, 0}, rx[3] = {0, 0, 0}, ry[3] = {0, 0, 0};
        auto add = [&](float x, float y, float wx, float wy, float c) {
            const double X = (double)(x * c), Y = (double)(y * c), C = (double)c, tx = (double)((x + wx) * c), ty = (double)((y + wy) * c);
            m[0] += X * X; m[1] += X * Y; m[2] += X * C; m[3] += Y * Y; m[4] += Y * C; m[5] += C * C;
            rx[0] += X * tx; rx[1] += Y * tx; rx[2] += C * tx;
            ry[0] += X * ty; ry[1] += Y * ty; ry[2] += C * ty;
        };
        float coefi = 0.0f;
        for_each_entry<kStaged, true>(im, nn, seed0, lane, live, [&](int s, float coef, int2 p, float2 v) {
            if (s == i) { coefi = 0.01f * coef; coef *= 0.96f; }
            add((float)p.x, (float)p.y, v.x, v.y, coef);
        });
        if (!live) return;
        const int2 p = im.seeds[i];
        const float2 v = im.vects[i];
        const float xi = (float)p.x, yi = (float)p.y;
        add(xi + 0.1f, yi, v.x, v.y, coefi);
        add(xi, yi + 0.1f, v.x, v.y, coefi);
        add(xi - 0.1f, yi, v.x, v.y, coefi);
        add(xi, yi - 0.1f, v.x, v.y, coefi);
        float out[6];
        solve3_pair(m, rx, ry, out);
        float *aff = im.model + (size_t)i * 6;
        for (int k = 0; k < 6; k++) aff[k] = out[k];
    } else {                                                         // epic_fit_nadarayawatson
        float u = 0.0f, v = 0.0f, s = 0.0f;
        for_each_entry<kStaged, false>(im, nn, seed0, lane, live, [&](int, float d, int2, float2 vec) {
            u += d * vec.x;
            v += d * vec.y;
            s += d;
        });
        if (!live) return;
        im.model[(size_t)i * 2] = u / s;
        im.model[(size_t)i * 2 + 1] = v / s;
    }
}

__global__ void k_epic_apply(const FitImg *imgs, int w, int npix, int method) {
    const FitImg im = imgs[blockIdx.y];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const int l = im.lab[p];
    float fx = 0.0f, fy = 0.0f;                                      // a label that names no seed
    if (l >= 0 && l < im.ns) {
        if (method == 0) {                                           // epic.cpp: a[0] * i + a[1] * j + a[2] - i, the ints converted, left to right
            const float *a = im.model + (size_t)l * 6;
            const float x = (float)(p % w), y = (float)(p / w);
            fx = a[0] * x + a[1] * y + a[2] - x;
            fy = a[3] * x + a[4] * y + a[5] - y;
        } else {
            fx = im.model[(size_t)l * 2];
            fy = im.model[(size_t)l * 2 + 1];
        }
    }
    im.fx[p] = fx;
    im.fy[p] = fy;
}

inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }
inline int blocks(size_t n, int per) { return (int)((n + per - 1) / per); }

// one allocation cut into 256-byte aligned pieces
struct Bump {
    char *base = nullptr; size_t used = 0;
    template <class T> T *take(size_t count) { T *r = reinterpret_cast<T *>(base + used); used += al(count * sizeof(T)); return r; }
};

}  // namespace

// The two launches on records already in device memory (sfa_internal.h): no allocation, no copy, no wait
void epic_fit_device(sfa_ctx *ctx, int method, int m, int ns_max, const EpicFitImg *d_imgs) {
    const bool plain = sw_int(Switches::EPIC_FIT_PLAIN, 0) != 0;     // the lists read row by row from global memory (the release build: constant false)
    const dim3 grid(blocks(ns_max, kFitLanes), m), wave(kFitLanes);
    hipStream_t st = ctx->stream;
    if (method == 0 && !plain) hipLaunchKernelGGL((k_epic_fit<0, true>), grid, wave, 0, st, d_imgs);
    if (method == 1 && !plain) hipLaunchKernelGGL((k_epic_fit<1, true>), grid, wave, 0, st, d_imgs);
    SFA_FULL(if (method == 0 && plain) hipLaunchKernelGGL((k_epic_fit<0, false>), grid, wave, 0, st, d_imgs);)
    SFA_FULL(if (method == 1 && plain) hipLaunchKernelGGL((k_epic_fit<1, false>), grid, wave, 0, st, d_imgs);)
}
void epic_apply_device(sfa_ctx *ctx, int method, int m, int w, int h, const EpicFitImg *d_imgs) {
    const size_t npix = (size_t)w * h;
    hipLaunchKernelGGL(k_epic_apply, dim3(blocks(npix, 256), m), dim3(256), 0, ctx->stream, d_imgs, w, (int)npix, method);
}

}  // namespace sfa

using namespace sfa;

int sfa_epic_interpolate_batch(sfa_ctx *ctx, int n, int w, int h, int method, const int *const *labels, const int *const *seeds_xy, const float *const *vects,
                               const int *ns, int nn, const int *const *nn_index, const float *const *nn_weight, float *const *flow_x, float *const *flow_y,
                               int stride, float *const *model, size_t workspace_bytes, int *status) {
    const char *fn = __func__;
    if (!ctx) return set_error(nullptr, SFA_ERR_ARG, "%s: ctx is null", fn);
    if (n < 1) REFUSE("%s: n = %d (at least one image)", fn, n);
    if (w < 1 || h < 1) REFUSE("%s: w x h = %d x %d (both at least 1)", fn, w, h);
    if (nn < 1) REFUSE("%s: nn = %d (at least one neighbour)", fn, nn);
    if (method != 0 && method != 1) REFUSE("%s: method = %d (0: locally-weighted affine, 1: Nadaraya-Watson)", fn, method);
    if (stride < w) REFUSE("%s: stride = %d (at least w = %d)", fn, stride, w);
    const bool flows = flow_x || flow_y;                             // neither: the models only
    if (!seeds_xy || !vects || !ns || !nn_index || !nn_weight || !status) {
        REFUSE("%s: %s is null", fn, !seeds_xy ? "seeds_xy" : !vects ? "vects" : !ns ? "ns" : !nn_index ? "nn_index" : !nn_weight ? "nn_weight" : "status");
    }
    if (flows && (!flow_x || !flow_y || !labels)) REFUSE("%s: %s is null (flow_x and flow_y come together, and with labels)", fn, !flow_x ? "flow_x" : !flow_y ? "flow_y" : "labels");
    if (!flows && !model) REFUSE("%s: model is null, and so are flow_x and flow_y: nothing to compute", fn);
    if ((long long)w * h > kMaxPixels) REFUSE("%s: w * h = %lld pixels (at most 2^29: pixels are indexed with 32 bits)", fn, (long long)w * h);
    for (int i = 0; i < n; i++) {
        if (ns[i] < 1) REFUSE("%s: ns[%d] = %d (at least one seed)", fn, i, ns[i]);
        if (!seeds_xy[i] || !vects[i] || !nn_index[i] || !nn_weight[i]) {
            REFUSE("%s: %s[%d] is null", fn, !seeds_xy[i] ? "seeds_xy" : !vects[i] ? "vects" : !nn_index[i] ? "nn_index" : "nn_weight", i);
        }
        if (flows && (!labels[i] || !flow_x[i] || !flow_y[i])) REFUSE("%s: %s[%d] is null", fn, !labels[i] ? "labels" : !flow_x[i] ? "flow_x" : "flow_y", i);
        if (model && !model[i]) REFUSE("%s: model[%d] is null", fn, i);
        if ((long long)ns[i] * nn > INT_MAX) REFUSE("%s: ns[%d] * nn = %lld entries (the kernels index the lists with 32 bits)", fn, i, (long long)ns[i] * nn);
    }
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    size_t budget = workspace_bytes;
    if (!budget) {                                                   // half of what the GPU has free now
        size_t free_b = 0, total_b = 0;
        SFA_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
        budget = free_b / 2;
    }
    const size_t npix = (size_t)w * h;
    const int mf = method == 0 ? 6 : 2;                              // floats of a seed's model
    hipStream_t st = ctx->stream;
    // what an image needs, all of it known beforehand: its record, seeds, vectors, the two lists, the models, and for the flow its labels and two planes
    auto need = [&](int i) {
        return al(sizeof(FitImg)) + 2 * al((size_t)ns[i] * 8) + 2 * al((size_t)ns[i] * nn * 4) + al((size_t)ns[i] * mf * 4) + (flows ? 3 * al(npix * 4) : 0);
    };
    for (int i = 0; i < n; i++) status[i] = 0;
    struct Events {
        hipEvent_t e[3] = {};
        ~Events() { for (hipEvent_t v : e) if (v) (void)hipEventDestroy(v); }
    } ev;
    for (hipEvent_t &v : ev.e) SFA_HIP(ctx, hipEventCreate(&v));
    ctx->epic_fit_ms[0] = ctx->epic_fit_ms[1] = 0.f;
    int first = 0;
    while (first < n) {
        if (need(first) > budget) { status[first++] = 1; continue; } // not even alone: flagged, its outputs untouched
        int m = 0;
        size_t bytes = 0;
        while (first + m < n && m < kMaxSubBatch && bytes + need(first + m) <= budget) bytes += need(first + m++);
        DevMem mem;
        SFA_TRY(mem.alloc(ctx, bytes));
        Bump b{static_cast<char *>(mem.p)};
        FitImg *d_imgs = b.take<FitImg>(m);
        std::vector<FitImg> imgs(m);
        int ns_max = 0;
        for (int k = 0; k < m; k++) {
            const int i = first + k;
            const size_t list = (size_t)ns[i] * nn;
            FitImg &im = imgs[k];
            memset(&im, 0, sizeof im);
            int2 *s = b.take<int2>(ns[i]);
            float2 *v = b.take<float2>(ns[i]);
            int *ix = b.take<int>(list);
            float *wt = b.take<float>(list);
            im.seeds = s; im.vects = v; im.index = ix; im.weight = wt; im.ns = ns[i]; im.nn = nn;
            im.model = b.take<float>((size_t)ns[i] * mf);
            SFA_HIP(ctx, hipMemcpyAsync(s, seeds_xy[i], (size_t)ns[i] * 8, hipMemcpyHostToDevice, st));
            SFA_HIP(ctx, hipMemcpyAsync(v, vects[i], (size_t)ns[i] * 8, hipMemcpyHostToDevice, st));
            SFA_HIP(ctx, hipMemcpyAsync(ix, nn_index[i], list * 4, hipMemcpyHostToDevice, st));
            SFA_HIP(ctx, hipMemcpyAsync(wt, nn_weight[i], list * 4, hipMemcpyHostToDevice, st));
            if (flows) {
                int *l = b.take<int>(npix);
                im.lab = l; im.fx = b.take<float>(npix); im.fy = b.take<float>(npix);
                SFA_HIP(ctx, hipMemcpyAsync(l, labels[i], npix * 4, hipMemcpyHostToDevice, st));
            }
            ns_max = std::max(ns_max, ns[i]);
        }
        SFA_HIP(ctx, hipMemcpyAsync(d_imgs, imgs.data(), (size_t)m * sizeof(FitImg), hipMemcpyHostToDevice, st));
        (void)hipEventRecord(ev.e[0], st);
        epic_fit_device(ctx, method, m, ns_max, d_imgs);
        (void)hipEventRecord(ev.e[1], st);
        if (flows) epic_apply_device(ctx, method, m, w, h, d_imgs);
        (void)hipEventRecord(ev.e[2], st);
        SFA_HIP(ctx, hipGetLastError());
        for (int k = 0; k < m; k++) {
            const int i = first + k;
            if (model) SFA_HIP(ctx, hipMemcpyAsync(model[i], imgs[k].model, (size_t)ns[i] * mf * 4, hipMemcpyDeviceToHost, st));
            if (flows && stride == w) {                              // packed rows: one copy per plane
                SFA_HIP(ctx, hipMemcpyAsync(flow_x[i], imgs[k].fx, npix * 4, hipMemcpyDeviceToHost, st));
                SFA_HIP(ctx, hipMemcpyAsync(flow_y[i], imgs[k].fy, npix * 4, hipMemcpyDeviceToHost, st));
            } else if (flows) {                                      // the valid columns only: columns >= w of the caller's rows are not written
                SFA_HIP(ctx, hipMemcpy2DAsync(flow_x[i], (size_t)stride * 4, imgs[k].fx, (size_t)w * 4, (size_t)w * 4, h, hipMemcpyDeviceToHost, st));
                SFA_HIP(ctx, hipMemcpy2DAsync(flow_y[i], (size_t)stride * 4, imgs[k].fy, (size_t)w * 4, (size_t)w * 4, h, hipMemcpyDeviceToHost, st));
            }
        }
        SFA_TRY(sfa_ctx_sync(ctx));
        for (int k = 0; k < (flows ? 2 : 1); k++) {                  // (no application, no time: two events in a row are still microseconds apart)
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]) == hipSuccess) ctx->epic_fit_ms[k] += ms;
        }
        first += m;
    }
    return SFA_OK;
}

int sfa_epic_fit_stage_ms(sfa_ctx *ctx, float ms[2]) {
    if (!ctx || !ms) return set_error(ctx, SFA_ERR_ARG, "%s: %s is null", __func__, !ctx ? "ctx" : "ms");
    ms[0] = ctx->epic_fit_ms[0];
    ms[1] = ctx->epic_fit_ms[1];
    return SFA_OK;
}
