// accumulate.hip -- the first stage of dense_tracking (step 3 of the pipeline): accumulateConsistentBatches (utils/utils.cpp:517-617) with the
// bilinearInterp<double> it calls (utils/utils.h:182-217), on the GPU.
//
// Every pixel of the output grid follows the FF forward flows of its segment, interpolated bilinearly in fp64, checks each step against the backward
// flow, falls back to constant velocity where the check fails and records how many steps stayed consistent.  Pure fp64 arithmetic plus one sqrt, built
// with -ffp-contract=off: the same bits as a plain restatement of the reference's statements in their order (tests/accum_ref.py).
//
// Shape: one thread per (segment, grid pixel), looping over f inside it; the segment is blockIdx.y, so n independent segments (the reference's start_jet
// loop, dense_tracking.cpp:726, and its rates) cost one launch.  Each step gathers the forward flow at the tracked point and the backward flow at its
// target: 4 + 4 taps of (u, v), interleaved into float2 (a tap is one 8-byte load; double2 for jets resampled from another size).  Read where the trajectories
// go, so the work is bound by these gathers (not by the fp64 arithmetic: about 60 fp64 operations per step).
#include "sfa_device.h"

#pragma clang fp contract(off)

namespace sfa {

constexpr int kAccThreads = 256;

// fwd, bwd: n * FF float2 planes of w x h (segment s, step f at plane s * FF + f); masks: the same count of uint8 planes or null (0 = occluded, the
// reference's value after 255 - x, dense_tracking.cpp:1192).  acc_u, acc_v: n * S planes of gw x gh doubles, S = FF (all_steps) or 1 (the last step);
// tracked: n planes of gw x gh.  The reference's Vec2d holds (y, x) = (v, u): channel 0 is v (utils.cpp:364-369); here each channel has its name.
// T2 = float2: the flows as read; T2 = double2: flows resampled from jets of another size (jet_resample.hip), a tap being one 16-byte load.
template <class T2>
__global__ void __launch_bounds__(kAccThreads) k_accumulate(const T2 *__restrict__ fwd, const T2 *__restrict__ bwd, const unsigned char *__restrict__ masks,
                                                            int FF, int w, int h, int gw, int gh, int xy_incr, int xy_start, double epsilon, int discard, int all_steps,
                                                            double *__restrict__ acc_u, double *__restrict__ acc_v, int *__restrict__ tracked) {
    const int i = blockIdx.x * kAccThreads + threadIdx.x;
    if (i >= gw * gh) return;
    const int s = blockIdx.y, gx = i % gw, gy = i / gw;
    const size_t pl = (size_t)w * h, gpl = (size_t)gw * gh;
    const int oy = gy * xy_incr + xy_start, ox = gx * xy_incr + xy_start;      // on the image: checked by the host (sfa_accumulate_grid)
    const T2 *F = fwd + (size_t)s * FF * pl, *B = bwd + (size_t)s * FF * pl;
    const unsigned char *M = masks ? masks + (size_t)s * FF * pl : nullptr;
    // quirk: last_flow starts as forward[0] AT the grid point, not zero (utils.cpp:530-535: "avoid zero flow if directly occluded")
    const T2 f0 = F[(size_t)oy * w + ox];
    double last_u = f0.x, last_v = f0.y;
    double prev_u = 0, prev_v = 0;                                              // acc_forward[f - 1]
    bool occluded = false;                                                      // :537
    int tr = FF;                                                                // :538, "fully tracked"
    const int S = all_steps ? FF : 1;
    double *AU = acc_u + (size_t)s * S * gpl + i, *AV = acc_v + (size_t)s * S * gpl + i;
    for (int f = 0; f < FF; f++) {
        // quirk: acc_forward[f] starts at zero (:541), and an occluded pixel `continue`s (:547-548): its acc stays ZERO for every later f, it does not
        // carry its last value
        double au = 0, av = 0;
        if (!occluded) {
            double cy = oy, cx = ox;                                            // :550, f_corr = (y, x) of the grid point
            if (f > 0) { cy += prev_v; cx += prev_u; au = prev_u; av = prev_v; }   // :551-554
            bool fail;
            // quirk: the in-image test is >= 0 && < h on the doubles (:556), so a NaN position fails it
            if (cy >= 0 && cy < h && cx >= 0 && cx < w) {
                // quirk: the occlusion lookup truncates the double coordinates (at<uchar>(double, double) -> int, :557)
                if (M && M[(size_t)f * pl + (size_t)(int)cy * w + (int)cx] == 0) {
                    occluded = true;                                            // :558; this step is still accumulated below
                    if (tr == FF) tr = discard ? 0 : f + 1;                     // quirk: tracked changes once (:561-566)
                }
                double vu, vv;
                bilinear2(F + (size_t)f * pl, w, h, cx, cy, vu, vv);            // :570-571
                const double ny = cy + vv, nx = cx + vu;                        // :573
                // quirk: when the target leaves the image, diff = vec - last_flow (:574, "OUT OF IMAGE CONFIDENCE (FOR NOW CONSTANT VEL)")
                double dv = vv - last_v, du = vu - last_u;
                if (ny >= 0 && ny < h && nx >= 0 && nx < w) {                   // :575-576
                    double bu, bv;
                    bilinear2(B + (size_t)f * pl, w, h, nx, ny, bu, bv);
                    dv = vv + bv; du = vu + bu;
                }
                const double err = sqrt(dv * dv + du * du);                     // :579, sqrt(dy^2 + dx^2) in that order
                fail = err > epsilon;                                           // :581, NaN passes as consistent
                if (fail) { au += last_u; av += last_v; }                       // :583, constant velocity
                else { au += vu; av += vv; last_u = vu; last_v = vv; }          // :593-595
            } else {
                au += last_u; av += last_v;                                     // :598-599, constant velocity
                fail = true;
            }
            if (fail && tr == FF) tr = discard ? 0 : f + 1;                     // :586-591, :602-607: changes once
            prev_u = au; prev_v = av;
        }
        if (all_steps) { AU[(size_t)f * gpl] = au; AV[(size_t)f * gpl] = av; }
        else if (f == FF - 1) { AU[0] = au; AV[0] = av; }
    }
    tracked[(size_t)s * gpl + i] = tr;
}

}  // namespace sfa

using namespace sfa;

// utils.cpp:522-526 in its own arithmetic: xy_incr = skip + 1, xy_start = (int)(0.5f * skip), floor of float quotients
int sfa_accumulate_grid(int w, int h, int skip, int *gw, int *gh) {
    if (!gw || !gh) return set_error(nullptr, SFA_ERR_ARG, "sfa_accumulate_grid: null output");
    if (w < 1 || h < 1 || skip < 0 || skip >= w || skip >= h)
        return set_error(nullptr, SFA_ERR_ARG, "sfa_accumulate_grid: %d x %d with skip %d gives an empty grid (w, h >= 1, 0 <= skip < min(w, h))", w, h, skip);
    const int xy_incr = skip + 1, xy_start = (int)(0.5f * skip);
    const unsigned H = (unsigned)floorf((1.0f * h) / xy_incr), W = (unsigned)floorf((1.0f * w) / xy_incr);
    if (H < 1 || W < 1 || (long)(H - 1) * xy_incr + xy_start >= h || (long)(W - 1) * xy_incr + xy_start >= w)
        return set_error(nullptr, SFA_ERR_ARG, "sfa_accumulate_grid: %d x %d with skip %d: grid off the image", w, h, skip);
    *gw = (int)W;
    *gh = (int)H;
    return SFA_OK;
}

namespace sfa {

int accumulate_device(sfa_ctx *ctx, int n, int FF, int w, int h, int gw, int gh, int skip, bool identity, const void *fwd, const void *bwd,
                      const unsigned char *masks, double epsilon, int discard, int all_steps, double *acc_u, double *acc_v, int *tracked) {
    const int xy_incr = skip + 1, xy_start = (int)(0.5f * skip);
    const size_t gpl = (size_t)gw * gh;
    const dim3 grid((unsigned)((gpl + kAccThreads - 1) / kAccThreads), (unsigned)n);
    if (identity)
        hipLaunchKernelGGL(k_accumulate<float2>, grid, dim3(kAccThreads), 0, ctx->stream, static_cast<const float2 *>(fwd), static_cast<const float2 *>(bwd), masks, FF,
                           w, h, gw, gh, xy_incr, xy_start, epsilon, discard ? 1 : 0, all_steps ? 1 : 0, acc_u, acc_v, tracked);
    else
        hipLaunchKernelGGL(k_accumulate<double2>, grid, dim3(kAccThreads), 0, ctx->stream, static_cast<const double2 *>(fwd), static_cast<const double2 *>(bwd), masks,
                           FF, w, h, gw, gh, xy_incr, xy_start, epsilon, discard ? 1 : 0, all_steps ? 1 : 0, acc_u, acc_v, tracked);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

}  // namespace sfa

// sfa_accumulate_consistent and sfa_accumulate_consistent_scaled: the planes src describes, as float2 where src is the identity (masks: decoded masks or,
// with raw_occ, the occlusion images as read), else resampled to double2 (masks: raw occlusion images)
static int accumulate_run(sfa_ctx *ctx, const char *fn, int n, int FF, int w, int h, const sfa_jet_source *src, const float *const *fwd_u, const float *const *fwd_v,
                          const float *const *bwd_u, const float *const *bwd_v, const unsigned char *const *masks, bool raw_occ, double epsilon, int skip,
                          int discard, int all_steps, double *acc_u, double *acc_v, int *tracked, float *stage_ms) {
    if (!(ctx && fwd_u && fwd_v && bwd_u && bwd_v && acc_u && acc_v && tracked)) return set_error(ctx, SFA_ERR_ARG, "%s: null argument", fn);
    if (!(n >= 1 && n <= 65535 && FF >= 1 && w >= 1 && h >= 1 && src && src->stride >= src->sw))
        return set_error(ctx, SFA_ERR_ARG, "%s: bad sizes (1 <= n <= 65535 segments, FF >= 1, w, h >= 1, stride >= w)", fn);
    bool identity;
    SFA_TRY(jet_source_check(ctx, fn, src, w, h, &identity));
    if (masks && raw_occ && (src->x0 != 0 || src->y0 != 0 || src->cw != src->sw || src->ch != src->sh))
        return set_error(ctx, SFA_ERR_ARG, "%s: source: cropped occlusions are not supported (the reference's crop() reads the 8-bit Mat through at<Vec2d>)", fn);
    int gw, gh;
    if (sfa_accumulate_grid(w, h, skip, &gw, &gh) != SFA_OK) return set_error(ctx, SFA_ERR_ARG, "%s", sfa_last_error(nullptr));
    const size_t np = (size_t)n * FF, pl = (size_t)w * h, spl = identity ? pl : (size_t)src->cw * src->ch;
    for (size_t k = 0; k < np; k++)
        if (!fwd_u[k] || !fwd_v[k] || !bwd_u[k] || !bwd_v[k] || (masks && !masks[k])) return set_error(ctx, SFA_ERR_ARG, "%s: null plane %zu", fn, k);
    const int S = all_steps ? FF : 1;
    const size_t tap = identity ? 8 : 16;                                       // float2 or double2
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem dfw, dbw, dstage, dm, dms, dau, dav, dtr;
    SFA_TRY(dfw.alloc(ctx, np * pl * tap)); SFA_TRY(dbw.alloc(ctx, np * pl * tap)); SFA_TRY(dstage.alloc(ctx, np * spl * 8));
    if (masks) SFA_TRY(dm.alloc(ctx, np * pl));
    if (masks && raw_occ) SFA_TRY(dms.alloc(ctx, np * (size_t)src->sw * src->sh));
    const size_t gpl = (size_t)gw * gh;
    SFA_TRY(dau.alloc(ctx, (size_t)n * S * gpl * 8)); SFA_TRY(dav.alloc(ctx, (size_t)n * S * gpl * 8)); SFA_TRY(dtr.alloc(ctx, (size_t)n * gpl * 4));
    StageEvents ev;                                                             // around the forward and the backward flows' kernel and k_accumulate
    if (stage_ms) SFA_TRY(ev.make(ctx, 6));
    SFA_TRY(upload_flow_pairs(ctx, *src, identity, np, fwd_u, fwd_v, w, h, dstage.f(), dfw.p, ev.e[0], ev.e[1]));
    SFA_TRY(upload_flow_pairs(ctx, *src, identity, np, bwd_u, bwd_v, w, h, dstage.f(), dbw.p, ev.e[2], ev.e[3]));
    if (masks && raw_occ)
        SFA_TRY(jet_decode_occlusions(ctx, *src, np, masks, w, h, static_cast<unsigned char *>(dms.p), static_cast<unsigned char *>(dm.p)));
    else if (masks)
        SFA_TRY(upload_masks(ctx, np, masks, src->stride, w, h, static_cast<unsigned char *>(dm.p)));
    SFA_TRY(ev.mark(ctx, 4));
    SFA_TRY(accumulate_device(ctx, n, FF, w, h, gw, gh, skip, identity, dfw.p, dbw.p, static_cast<const unsigned char *>(dm.p), epsilon, discard, all_steps,
                              static_cast<double *>(dau.p), static_cast<double *>(dav.p), static_cast<int *>(dtr.p)));
    SFA_TRY(ev.mark(ctx, 5));
    SFA_HIP(ctx, hipMemcpyAsync(acc_u, dau.p, (size_t)n * S * gpl * 8, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(acc_v, dav.p, (size_t)n * S * gpl * 8, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(tracked, dtr.p, (size_t)n * gpl * 4, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stage_ms) {
        float span[5];                                                          // forward, (between), backward, (masks), accumulation
        SFA_TRY(ev.read(ctx, 6, span));
        stage_ms[0] = span[0] + span[2];
        stage_ms[1] = span[4];
    }
    return SFA_OK;
}

int sfa_accumulate_consistent(sfa_ctx *ctx, int n, int FF, int w, int h, int stride, const float *const *fwd_u, const float *const *fwd_v,
                              const float *const *bwd_u, const float *const *bwd_v, const unsigned char *const *masks, double epsilon, int skip, int discard,
                              int all_steps, double *acc_u, double *acc_v, int *tracked) {
    sfa_jet_source src;
    sfa_jet_source_default(&src, w, h, stride);
    return accumulate_run(ctx, __func__, n, FF, w, h, &src, fwd_u, fwd_v, bwd_u, bwd_v, masks, false, epsilon, skip, discard, all_steps, acc_u, acc_v, tracked, nullptr);
}

int sfa_accumulate_consistent_scaled(sfa_ctx *ctx, int n, int FF, int w, int h, const sfa_jet_source *src, const float *const *fwd_u,
                                     const float *const *fwd_v, const float *const *bwd_u, const float *const *bwd_v, const unsigned char *const *occ,
                                     double epsilon, int skip, int discard, int all_steps, double *acc_u, double *acc_v, int *tracked, float *stage_ms) {
    if (!src) return set_error(ctx, SFA_ERR_ARG, "%s: null source", __func__);
    return accumulate_run(ctx, __func__, n, FF, w, h, src, fwd_u, fwd_v, bwd_u, bwd_v, occ, true, epsilon, skip, discard, all_steps, acc_u, acc_v, tracked, stage_ms);
}
