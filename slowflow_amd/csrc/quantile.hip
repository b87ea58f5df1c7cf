// quantile.hip -- the adaptiveFR program's flow-magnitude quantile (adaptiveFR.cpp:644-668) on the GPU: an exact radix select instead of std::sort.
//
// Magnitudes: m = sqrtf(fl(u s) fl(u s) + fl(v s) fl(v s)) in strict IEEE fp32 (round to nearest, no contraction; sqrt correctly rounded), s applied first
// as image_mul_scalar does (:612-613, image.c:49-57).  m >= +0 except NaN, so the 32-bit pattern of m orders the values like the numbers; the sign bit is
// cleared (a NaN input may carry one), which puts every NaN above +Inf -- std::sort with NaN is undefined in the reference, this is the order here.
//
// Selection, for the (at most three) ranks the rule needs -- k, k + 1 when it averages, N - 1 for the maximum:
//   pass 1  k_mag_keys_hist: scale + magnitude + key, histogram of key bits 31..21 (2048 bins) in LDS shared by the block's waves, one global integer add
//           per non-empty bin (cdna_hip_programming.md Guideline 12).  The keys are STORED (4 bytes per value): the later passes then read 4 bytes per value
//           where recomputing would read u and v again (8) and repeat the arithmetic -- 20 bytes per value over the three passes against 24.
//   scan    k_select_digit (one workgroup): per rank, the bin that holds it and the rank within that bin.
//   pass 2  bits 20..10 of the keys whose bits 31..21 are the chosen prefix (one LDS histogram per rank), scan; pass 3 bits 9..0, scan.
// After the third scan each rank's prefix IS its key.  Counts are integers, so the result does not depend on the order the adds arrive in: repeated runs
// give the same bits.
//
// Groups (sfa_flow_magnitude_quantiles_device): G sets of fields that already live in GPU memory, one quantile and one maximum each.  blockIdx.y is the group;
// a group has its own record (GroupSel: SelState, value count, which ranks answer), its own histograms and its own packed keys, so no block mixes two
// groups in its LDS histogram.  k_group_keys_hist is pass 1 reading u and v in place through element strides; passes 2, 3 and the scans are the bodies of
// k_digit_hist / k_select_digit on the group's pointers; k_group_result applies the rule of :663/:665/:668 and leaves {quantile, max} in GPU memory.
// Its pointers and strides are checked as views by check_view / check_disjoint (api.hip on dev_view.h); only the rule that rows too need a stride >= 1 is its own.
#include "sfa_device.h"

#pragma clang fp contract(off)

namespace sfa {

constexpr int kQBins = 2048, kQRanks = 3, kQThreads = 256;
struct SelState {
    unsigned prefix[kQRanks];    // key bits chosen so far, right-aligned
    unsigned rank[kQRanks];      // rank of the wanted value among the keys with that prefix
    int nr;
};
// digit of pass `level`: bits [shift, shift + bits) of the key; the prefix is the key shifted right by shift + bits
__host__ __device__ constexpr int digit_shift(int level) { return level == 0 ? 21 : level == 1 ? 10 : 0; }
__host__ __device__ constexpr int digit_bits(int level) { return level == 2 ? 10 : 11; }

__global__ void __launch_bounds__(kQThreads) k_mag_keys_hist(const float *__restrict__ u, const float *__restrict__ v, size_t N, float s,
                                                             unsigned *__restrict__ keys, unsigned *__restrict__ hist) {
    __shared__ unsigned lh[kQBins];
    for (int i = threadIdx.x; i < kQBins; i += kQThreads) lh[i] = 0;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * kQThreads + threadIdx.x; i < N; i += (size_t)gridDim.x * kQThreads) {
        const float a = u[i] * s, b = v[i] * s;                                   // image_mul_scalar (:612-613)
        const float m = sqrt_rn(a * a + b * b);                                   // :652, sqrt(float)
        const unsigned key = __float_as_uint(m) & 0x7fffffffu;
        keys[i] = key;
        atomicAdd(&lh[key >> 21], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kQBins; i += kQThreads)
        if (lh[i]) atomicAdd(&hist[i], lh[i]);
}

__device__ __forceinline__ void digit_hist(const unsigned *__restrict__ keys, size_t N, const SelState *__restrict__ st, int level,
                                           unsigned *__restrict__ hist /* [kQRanks][kQBins] */) {
    __shared__ unsigned lh[kQRanks * kQBins];
    const int nr = st->nr, sh = digit_shift(level), pre = sh + digit_bits(level);
    const unsigned mask = (1u << digit_bits(level)) - 1;
    unsigned prefix[kQRanks];
    for (int r = 0; r < kQRanks; r++) prefix[r] = r < nr ? st->prefix[r] : 0xffffffffu;
    for (int i = threadIdx.x; i < kQRanks * kQBins; i += kQThreads) lh[i] = 0;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * kQThreads + threadIdx.x; i < N; i += (size_t)gridDim.x * kQThreads) {
        const unsigned key = keys[i], hi = key >> pre, d = (key >> sh) & mask;
        for (int r = 0; r < kQRanks; r++)
            if (hi == prefix[r]) atomicAdd(&lh[r * kQBins + d], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nr * kQBins; i += kQThreads)
        if (lh[i]) atomicAdd(&hist[i], lh[i]);
}
__global__ void __launch_bounds__(kQThreads) k_digit_hist(const unsigned *__restrict__ keys, size_t N, const SelState *__restrict__ st, int level,
                                                          unsigned *__restrict__ hist) {
    digit_hist(keys, N, st, level, hist);
}

// one workgroup: for each rank, the bin of the level's histogram that holds it (pass 1 has one histogram for all ranks)
__device__ __forceinline__ void select_digit(const unsigned *__restrict__ hist, SelState *__restrict__ st, int level) {
    constexpr int per = kQBins / kQThreads;
    __shared__ unsigned part[kQThreads];
    const int nbins = 1 << digit_bits(level);
    for (int r = 0; r < st->nr; r++) {
        const unsigned *hr = hist + (level == 0 ? 0 : r * kQBins);
        const unsigned want = st->rank[r];
        unsigned mine = 0;
        for (int j = 0; j < per; j++) {
            const int b = threadIdx.x * per + j;
            if (b < nbins) mine += hr[b];
        }
        part[threadIdx.x] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {                                                  // exclusive scan of the 256 partial sums
            unsigned run = 0;
            for (int t = 0; t < kQThreads; t++) { const unsigned c = part[t]; part[t] = run; run += c; }
        }
        __syncthreads();
        unsigned before = part[threadIdx.x];
        for (int j = 0; j < per; j++) {
            const int b = threadIdx.x * per + j;
            if (b >= nbins) break;
            const unsigned c = hr[b];
            if (c && want >= before && want - before < c) {                     // exactly one bin holds the rank
                st->prefix[r] = (st->prefix[r] << digit_bits(level)) | (unsigned)b;
                st->rank[r] = want - before;
            }
            before += c;
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(kQThreads) k_select_digit(const unsigned *__restrict__ hist, SelState *__restrict__ st, int level) { select_digit(hist, st, level); }

// ---- groups of fields in GPU memory ---------------------------------------------------------------------------------------------------------------
constexpr int kQMaxGroups = 64;
struct GroupSel {
    SelState st;
    unsigned N;                  // values of the group: its count of fields x w x h
    unsigned char slot[3];       // the entries of st that hold rank k0, rank k1 and rank N - 1
    unsigned char average;
};
// every group's record as ONE kernel argument (36 bytes x 64 at most): the launch carries it, so no host buffer has to outlive the call
struct GroupSelAll { GroupSel g[kQMaxGroups]; };
// u and v of (group, field, row, column) at the element strides sg, sf, sr, sc; per = w h
struct GroupSrc { const float *u, *v; long long sg, sf, sr, sc; unsigned w, per; };

__global__ void __launch_bounds__(kQThreads) k_group_init(GroupSelAll all, int G, GroupSel *__restrict__ sel) {
    if ((int)threadIdx.x < G) sel[threadIdx.x] = all.g[threadIdx.x];
}

// pass 1 of group blockIdx.y: value i of the group is column i % w of row i % per / w of field i / per (i < 2^32: sfa_flow_magnitude_quantiles_device
// refuses more), read where it lies; the key goes to the group's packed keys[i]
__global__ void __launch_bounds__(kQThreads) k_group_keys_hist(GroupSrc s, float scale, const GroupSel *__restrict__ sel, unsigned *__restrict__ keys,
                                                               size_t key_stride, unsigned *__restrict__ hist) {
    __shared__ unsigned lh[kQBins];
    const int g = blockIdx.y;
    const size_t N = sel[g].N;
    const float *__restrict__ u = s.u + (long long)g * s.sg, *__restrict__ v = s.v + (long long)g * s.sg;
    keys += (size_t)g * key_stride;
    hist += (size_t)g * kQRanks * kQBins;
    for (int i = threadIdx.x; i < kQBins; i += kQThreads) lh[i] = 0;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * kQThreads + threadIdx.x; i < N; i += (size_t)gridDim.x * kQThreads) {
        const unsigned f = (unsigned)i / s.per, r = (unsigned)i - f * s.per, y = r / s.w, x = r - y * s.w;
        const long long o = (long long)f * s.sf + (long long)y * s.sr + (long long)x * s.sc;
        const float a = u[o] * scale, b = v[o] * scale;                           // as k_mag_keys_hist
        const float m = sqrt_rn(a * a + b * b);
        const unsigned key = __float_as_uint(m) & 0x7fffffffu;
        keys[i] = key;
        atomicAdd(&lh[key >> 21], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kQBins; i += kQThreads)
        if (lh[i]) atomicAdd(&hist[i], lh[i]);
}

__global__ void __launch_bounds__(kQThreads) k_group_digit_hist(const unsigned *__restrict__ keys, size_t key_stride, const GroupSel *__restrict__ sel, int level,
                                                                unsigned *__restrict__ hist) {
    const int g = blockIdx.y;
    digit_hist(keys + (size_t)g * key_stride, sel[g].N, &sel[g].st, level, hist + (size_t)g * kQRanks * kQBins);
}
// one workgroup per group
__global__ void __launch_bounds__(kQThreads) k_group_select_digit(const unsigned *__restrict__ hist, GroupSel *__restrict__ sel, int level) {
    select_digit(hist + (size_t)blockIdx.x * kQRanks * kQBins, &sel[blockIdx.x].st, level);
}
// one workgroup, thread g for group g: after the third scan a rank's prefix is its key
__global__ void __launch_bounds__(kQMaxGroups) k_group_result(const GroupSel *__restrict__ sel, int G, double *__restrict__ out) {
    const int g = threadIdx.x;
    if (g >= G) return;
    const GroupSel &s = sel[g];
    const double a = (double)__uint_as_float(s.st.prefix[s.slot[0]]), b = (double)__uint_as_float(s.st.prefix[s.slot[1]]);
    out[2 * g] = s.average ? 0.5f * (a + b) : a;                                  // :663, :665 (m[] holds doubles)
    out[2 * g + 1] = (double)__uint_as_float(s.st.prefix[s.slot[2]]);             // :668
}

}  // namespace sfa

using namespace sfa;

// adaptiveFR.cpp:660-666, the one statement of the rule (the program and the Python binding both come through here)
int sfa_quantile_ranks(size_t N, float q, size_t *k0, size_t *k1, int *average) {
    if (!k0 || !k1 || !average) return set_error(nullptr, SFA_ERR_ARG, "sfa_quantile_ranks: null output");
    if (N == 0) return set_error(nullptr, SFA_ERR_ARG, "sfa_quantile_ranks: no values (the reference indexes an empty array)");
    if (!(q > 0.0f && q <= 1.0f)) return set_error(nullptr, SFA_ERR_ARG, "sfa_quantile_ranks: q = %g outside (0, 1] (the reference indexes outside its array)", (double)q);
    const float np = q * (float)N - 1;                                          // float * size_t: N goes through float (exact up to 2^24)
    if (ceilf(np) < 0)                                                          // q * N rounds to 0: rank -1
        return set_error(nullptr, SFA_ERR_ARG, "sfa_quantile_ranks: N = %zu, q = %g selects rank -1 (the reference reads before its array)", N, (double)q);
    if (np < (float)(N - 1) && fmodf(np, 2.0f) == 0) {
        *average = 1; *k0 = (size_t)(int)np; *k1 = *k0 + 1;
    } else {
        *average = 0; *k0 = *k1 = (size_t)(int)ceilf(np);
    }
    if (*k1 >= N)
        return set_error(nullptr, SFA_ERR_ARG, "sfa_quantile_ranks: N = %zu, q = %g selects rank %zu (N rounded to float: the reference reads past its array)", N,
                         (double)q, *k1);
    return SFA_OK;
}

int sfa_flow_magnitude_quantile(sfa_ctx *ctx, int n, const float *const *u, const float *const *v, int w, int h, int stride, float flow_scale, float q,
                                double *quantile, double *max_magnitude) {
    if (!(ctx && n >= 1 && u && v && w > 0 && h > 0 && stride >= w && quantile && max_magnitude))
        return set_error(ctx, SFA_ERR_ARG, "sfa_flow_magnitude_quantile: bad arguments (n >= 1 fields of w x h, stride >= w)");
    for (int i = 0; i < n; i++)
        if (!u[i] || !v[i]) return set_error(ctx, SFA_ERR_ARG, "sfa_flow_magnitude_quantile: null field");
    const size_t per = (size_t)w * h, N = per * n;
    if (N > 0xffffffffull) return set_error(ctx, SFA_ERR_ARG, "sfa_flow_magnitude_quantile: %zu values, beyond the 32-bit counts", N);
    size_t k0, k1;
    int average;
    if (sfa_quantile_ranks(N, q, &k0, &k1, &average) != SFA_OK) return set_error(ctx, SFA_ERR_ARG, "%s", sfa_last_error(nullptr));
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem du, dv, dk, dh, ds;
    SFA_TRY(du.alloc(ctx, N * 4)); SFA_TRY(dv.alloc(ctx, N * 4)); SFA_TRY(dk.alloc(ctx, N * 4));
    SFA_TRY(dh.alloc(ctx, kQRanks * kQBins * 4)); SFA_TRY(ds.alloc(ctx, sizeof(SelState)));
    for (int i = 0; i < n; i++) {                                               // the valid columns of each field, packed
        SFA_HIP(ctx, hipMemcpy2DAsync(du.f() + i * per, (size_t)w * 4, u[i], (size_t)stride * 4, (size_t)w * 4, h, hipMemcpyHostToDevice, ctx->stream));
        SFA_HIP(ctx, hipMemcpy2DAsync(dv.f() + i * per, (size_t)w * 4, v[i], (size_t)stride * 4, (size_t)w * 4, h, hipMemcpyHostToDevice, ctx->stream));
    }
    SelState st{};
    const size_t want[kQRanks] = {k0, k1, N - 1};
    st.nr = 0;
    for (int r = 0; r < kQRanks; r++) {                                         // distinct ranks only
        bool dup = false;
        for (int t = 0; t < st.nr; t++) dup = dup || st.rank[t] == (unsigned)want[r];
        if (!dup) st.rank[st.nr++] = (unsigned)want[r];
    }
    const unsigned wanted[kQRanks] = {st.rank[0], st.rank[1], st.rank[2]};
    SFA_HIP(ctx, hipMemcpyAsync(ds.p, &st, sizeof st, hipMemcpyHostToDevice, ctx->stream));
    unsigned *hist = static_cast<unsigned *>(dh.p), *keys = static_cast<unsigned *>(dk.p);
    SelState *dst = static_cast<SelState *>(ds.p);
    const int blocks = (int)std::min<size_t>((N + kQThreads - 1) / kQThreads, (size_t)ctx->cu_count * 4);
    SFA_HIP(ctx, hipMemsetAsync(hist, 0, kQBins * 4, ctx->stream));
    hipLaunchKernelGGL(k_mag_keys_hist, dim3(blocks), dim3(kQThreads), 0, ctx->stream, du.f(), dv.f(), N, flow_scale, keys, hist);
    hipLaunchKernelGGL(k_select_digit, dim3(1), dim3(kQThreads), 0, ctx->stream, hist, dst, 0);
    for (int level = 1; level < 3; level++) {
        SFA_HIP(ctx, hipMemsetAsync(hist, 0, kQRanks * kQBins * 4, ctx->stream));
        hipLaunchKernelGGL(k_digit_hist, dim3(blocks), dim3(kQThreads), 0, ctx->stream, keys, N, dst, level, hist);
        hipLaunchKernelGGL(k_select_digit, dim3(1), dim3(kQThreads), 0, ctx->stream, hist, dst, level);
    }
    SFA_HIP(ctx, hipGetLastError());
    SFA_HIP(ctx, hipMemcpyAsync(&st, ds.p, sizeof st, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    auto value_of = [&](size_t k) {
        for (int r = 0; r < st.nr; r++)
            if (wanted[r] == (unsigned)k) return (double)__builtin_bit_cast(float, st.prefix[r]);
        return 0.0;                                                              // not reached: every wanted rank is in the state
    };
    *quantile = average ? 0.5f * (value_of(k0) + value_of(k1)) : value_of(k0);  // :663, :665 (m[] holds doubles)
    *max_magnitude = value_of(N - 1);                                            // :668
    return SFA_OK;
}

// adaptiveFR.cpp:644-668 for G groups of fields in GPU memory (include/slowflow_amd.h).  Every check, and every group's ranks (sfa_quantile_ranks), on the host
// before the first launch; then one launch sequence on the context's stream, no copy and no wait.  The scratch lives on the context: the records of 64
// groups, G x kQRanks histograms, G x n w h keys; a call that needs more than the context holds waits for the stream once and replaces it.
int sfa_flow_magnitude_quantiles_device(sfa_ctx *ctx, int G, int n, const int *counts, const float *u_dev, const float *v_dev, const long long strides[4], int w,
                                        int h, float flow_scale, float q, double *out_dev) {
    CHECK_ARGS(ctx, "ctx is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    if (G < 1 || G > kQMaxGroups) REFUSE("%s: G = %d groups; 1 to %d are taken", __func__, G, kQMaxGroups);
    if (n < 1) REFUSE("%s: n = %d fields per group", __func__, n);
    if (w < 1 || h < 1) REFUSE("%s: w = %d, h = %d: the fields are empty", __func__, w, h);
    int most = n;
    if (counts) {
        most = 0;
        for (int g = 0; g < G; g++) {
            if (counts[g] < 1 || counts[g] > n) REFUSE("%s: counts[%d] = %d lies outside 1..n = %d", __func__, g, counts[g], n);
            most = std::max(most, counts[g]);
        }
    }
    const size_t per = (size_t)w * h;
    if (per * (size_t)most > 0xffffffffull)
        REFUSE("%s: n = %d fields of w x h = %d x %d are %zu values in a group, beyond the 32-bit counts", __func__, most, w, h, per * (size_t)most);
    if (!strides) REFUSE("%s: strides is null", __func__);
    if (strides[2] < 1 || strides[3] < 1) REFUSE("%s: strides: row stride %lld, column stride %lld; both must be >= 1", __func__, strides[2], strides[3]);
    const long long pair[2] = {2, 1};
    const View u{"u_dev", u_dev, sizeof(float), 4, {G, n, h, w}, strides}, v{"v_dev", v_dev, sizeof(float), 4, {G, n, h, w}, strides},
        out{"out_dev", out_dev, sizeof(double), 2, {G, 2}, pair};
    SFA_TRY(check_view(ctx, __func__, u));
    SFA_TRY(check_view(ctx, __func__, v));
    if (!strides_nest(strides + 1, u.n + 1, 3))
        REFUSE("%s: strides (field %lld, row %lld, column %lld) let two elements of one group share an address (or interleave them in a way the check cannot clear)",
               __func__, strides[1], strides[2], strides[3]);
    SFA_TRY(check_view(ctx, __func__, out));
    for (const View &f : {u, v})                                                // (u and v may interleave: each against out_dev alone)
        SFA_TRY(check_disjoint(ctx, __func__, {out, f}, "the results would be written into flows still being read"));
    GroupSelAll all{};
    for (int g = 0; g < G; g++) {
        GroupSel &s = all.g[g];
        const size_t N = per * (size_t)(counts ? counts[g] : n);
        size_t k0, k1;
        int average;
        if (sfa_quantile_ranks(N, q, &k0, &k1, &average) != SFA_OK) REFUSE("%s: group %d: %s", __func__, g, sfa_last_error(nullptr));
        const size_t want[kQRanks] = {k0, k1, N - 1};
        for (int r = 0; r < kQRanks; r++) {                                      // distinct ranks only
            int t = 0;
            while (t < s.st.nr && s.st.rank[t] != (unsigned)want[r]) t++;
            if (t == s.st.nr) s.st.rank[s.st.nr++] = (unsigned)want[r];
            s.slot[r] = (unsigned char)t;
        }
        s.N = (unsigned)N;
        s.average = (unsigned char)average;
    }
    constexpr size_t sel_bytes = 4096, hist_bytes = (size_t)kQRanks * kQBins * 4;
    static_assert(sizeof(GroupSelAll) <= sel_bytes, "the records of all groups fit a kernel argument and the head of the scratch");
    const size_t key_stride = per * (size_t)most, need = sel_bytes + G * hist_bytes + G * key_stride * 4;
    if (need > ctx->q_tmp_bytes) {                                               // (the stream may still read the old scratch)
        SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->q_tmp_bytes = 0;
        if (ctx->q_tmp) { (void)hipFree(ctx->q_tmp); ctx->q_tmp = nullptr; }
        SFA_HIP(ctx, hipMalloc(&ctx->q_tmp, need));
        ctx->q_tmp_bytes = need;
    }
    GroupSel *sel = static_cast<GroupSel *>(ctx->q_tmp);
    unsigned *hist = reinterpret_cast<unsigned *>(static_cast<char *>(ctx->q_tmp) + sel_bytes), *keys = hist + (size_t)G * kQRanks * kQBins;
    const GroupSrc src{u_dev, v_dev, strides[0], strides[1], strides[2], strides[3], (unsigned)w, (unsigned)per};
    // as many blocks per group as the one-group path launches in all, shared among the groups
    const int blocks = (int)std::min<size_t>((key_stride + kQThreads - 1) / kQThreads, (size_t)std::max(1, ctx->cu_count * 4 / G));
    hipLaunchKernelGGL(k_group_init, dim3(1), dim3(kQMaxGroups), 0, ctx->stream, all, G, sel);
    SFA_HIP(ctx, hipMemsetAsync(hist, 0, G * hist_bytes, ctx->stream));
    hipLaunchKernelGGL(k_group_keys_hist, dim3(blocks, G), dim3(kQThreads), 0, ctx->stream, src, flow_scale, sel, keys, key_stride, hist);
    hipLaunchKernelGGL(k_group_select_digit, dim3(G), dim3(kQThreads), 0, ctx->stream, hist, sel, 0);
    for (int level = 1; level < 3; level++) {
        SFA_HIP(ctx, hipMemsetAsync(hist, 0, G * hist_bytes, ctx->stream));
        hipLaunchKernelGGL(k_group_digit_hist, dim3(blocks, G), dim3(kQThreads), 0, ctx->stream, keys, key_stride, sel, level, hist);
        hipLaunchKernelGGL(k_group_select_digit, dim3(G), dim3(kQThreads), 0, ctx->stream, hist, sel, level);
    }
    hipLaunchKernelGGL(k_group_result, dim3(1), dim3(kQMaxGroups), 0, ctx->stream, sel, G, out_dev);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}
