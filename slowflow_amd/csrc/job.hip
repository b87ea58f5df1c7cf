// job.hip -- the resident multi-frame job behind the C-ABI of include/slowflow_amd.h: Variational_MT::variational and compute_one_level (variational_mt.cpp:169-493,
// 526-784) for a batch of frame windows in lockstep.  struct sfa_job and every sfa_job_* entry point (the device seam's too: its argument checks are api.hip's on dev_view.h, its
// kernels device_io.hip's), the pyramid geometry, and sfa_variational / sfa_compute_one_level on top.  All compute is in kernels.hip / sor*.hip / occlusion.hip.
//
// A job is ONE allocation of nb element arenas.  Element arena (floats, per window; the same element stride for every plane of every level), PL = pitch*h of the level:
//   PERSISTENT part, one per level (the pyramid is built before the coarse-to-fine loop and the flow travels from level to level):
//     wx wy (2 PL), frames F x 3 PL
//   TRANSIENT part, ONE for all levels (only one level is refined at a time), sized for the finest level:
//     planes : uu vv du dv odu odv sh sv a11 a12 a22 b1 b2 occ dpsis   (15 PL)
//     masks  : 2*ref PL
//     warped : [slot][w_s|w_sp1] (3 PL each); a factor-0 warp is the frame itself and is not materialised
//     stacks : [slot][succ|toref][24 PL] -- only in the unfused form (SFA_UNFUSED=1, kept to cross-check the fused kernel)
//     tmp    : two colour images for the pyramid / presmoothing: they are dead before the first warp, so they LIE ON the warped images (6 PL <= 12 ref PL)
// Offsets handed to kernels (Term, WarpJob, OccSlot) are relative to `base` (the transient part) and may point into the persistent part.
// Round 3, arena + solver workspaces: 0.43 -> 0.30 GB per 1024x436 window (S = 2, 5 levels), 4 -> 1.63 GB per 2048x2048 window (6 levels).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "sfa_internal.h"

#pragma clang fp contract(off)

namespace sfa {

// Level: device-resident state of `nb` frame windows at one pyramid level (a view of the arena above)
enum { P_WX = 0, P_WY, P_UU, P_VV, P_DU, P_DV, P_ODU, P_ODV, P_SH, P_SV, P_A11, P_A12, P_A22, P_B1, P_B2, P_OCC, P_DPSIS, P_COUNT };
struct Level {
    int w = 0, h = 0, pitch = 0, lstride = 0, ref = 0, F = 0, nb = 0;
    bool fused = true;
    long pl = 0, es = 0;
    long off_masks = 0, off_warp = 0, off_stacks = 0, off_tmp = 0;
    float *base = nullptr;    // transient part, element 0
    float *pbase = nullptr;   // this level's persistent part, element 0
    float *plane(int i) const { return i < 2 ? pbase + (long)i * pl : base + (long)(i - 2) * pl; }
    float *mask(int s) const { return base + off_masks + (long)s * pl; }
    float *stack(int s, int toref) const { return base + off_stacks + ((long)s * 2 + toref) * 24 * pl; }
    // frame s + sp1 warped by (s + sp1 - ref) flow steps.  Slot s's second image IS slot s + 1's first one (the same frame, the same number of steps): the reference
    // warps it once per slot (variational_mt.cpp:100,109); here the two slots read one buffer (S = 3: four warps per get_derivatives instead of six)
    float *warp(int s, int sp1) const { return base + off_warp + (long)(s + sp1) * 3 * pl; }
    float *frame(int f) const { return pbase + 2 * pl + (long)f * 3 * pl; }
    float *tmp() const { return base + off_tmp; }
    Geo geo() const { return Geo{w, h, pitch, pl, es, nb, WMask::first(nb), nullptr}; }
    Geo geo(const WMask &active) const { return Geo{w, h, pitch, pl, es, nb, active, nullptr}; }
    static long persistent_floats(int pitch, int h, int ref) { return (long)pitch * h * (2 + (2L * ref + 1) * 3); }
    static long transient_floats(int pitch, int h, int ref, bool fused) {
        return (long)pitch * h * ((P_COUNT - 2) + 2 * ref + (2L * ref + 1) * 3 + (fused ? 0 : 2L * ref * 2 * 24));     // masks, one warped image per frame (the reference frame's slot stays empty), stacks
    }
    void layout(float *transient, float *persistent, int w_, int h_, int lstride_, int ref_, int nb_, long es_, bool fused_) {
        base = transient; pbase = persistent; w = w_; h = h_; pitch = dev_pitch(w_); lstride = lstride_; ref = ref_; F = 2 * ref_ + 1; nb = nb_; es = es_; fused = fused_;
        pl = (long)pitch * h;
        off_masks = (long)(P_COUNT - 2) * pl;
        off_warp = off_masks + 2L * ref * pl;
        off_stacks = off_warp + (2L * ref + 1) * 3 * pl;
        off_tmp = off_warp;                                  // 6 PL inside the (2 ref + 1) * 3 >= 9 PL of the warped images (ref >= 1)
    }
};
struct ChannelWeights { const float *dev = nullptr; long pl = 0, es = 0; int pitch = 0, stride0 = 0; };

// the image pair of slot s (variational_mt.cpp:98-110): frames s, s+1 warped by (s-ref), (s-ref+1) flow steps
static const float *pair_image(const Level &L, int s, int sp1) { return (s + sp1 - L.ref == 0) ? L.frame(s + sp1) : L.warp(s, sp1); }

// get_derivatives (variational_mt.cpp:87-166).  Fused form: only the warps; the filters run inside the assembly kernel.
// with_smoothness: compute_smoothness (:333) of the same flow field leaves in the same pass (the caller's next step, fused form with one inner iteration); returns
// whether it did
static bool get_derivatives(sfa_ctx *c, const Level &L, const sfa_params &p, const Geo &g, const bool need_toref[2 * SFA_MAX_REF], bool with_smoothness = false) {
    const int ref = L.ref;
    WarpJobs J;
    J.n = 0;
    // one warp per frame f != ref, by f - ref steps: it is w_s of slot f (:100) and w_sp1 of slot f - 1 (:109) -- the same frame by the same steps -- and yields the mask
    // of the slot on its own side of the reference frame: slot f backwards (f < ref), slot f - 1 forwards (f > ref); a zero-step warp is a copy (:723-728): never made
    for (int f = p.one_direction ? ref + 1 : 0; f <= 2 * ref; f++) {
        if (f == ref) continue;
        const int s = f < ref ? f : f - 1;                       // the slot whose mask this warp yields; L.warp(f, 0) == L.warp(f - 1, 1)
        J.job[J.n++] = WarpJob{L.frame(f) - L.base, L.warp(f < ref ? f : f - 1, f < ref ? 0 : 1) - L.base, L.mask(s) - L.base, f - ref};
    }
    const bool smoothed = with_smoothness && L.fused &&
                          launch_warp_smooth(c, g, J, L.base, L.plane(P_WX), L.plane(P_WY), p.smoothing, L.plane(P_SH), L.plane(P_SV), L.plane(P_DPSIS), p.alpha, pen(p.robust_reg));
    if (!smoothed) launch_warp_jobs(c, g, J, L.base, L.plane(P_WX), L.plane(P_WY));
    for (int s = p.one_direction ? ref : 0; s < 2 * ref; s++) {
        if (L.fused) continue;
        const float *w_s = pair_image(L, s, 0), *w_sp1 = pair_image(L, s, 1);
        launch_deriv_stack(c, g, L.stack(s, 0), w_s, w_sp1, L.es, L.es);                                        // :113-133
        // the to-reference stack (:136-161) only feeds add_data_and_match_ref (omega > 0) and optimizeOcc
        if (need_toref[s]) {
            if (s < ref) launch_deriv_stack(c, g, L.stack(s, 1), w_s, L.frame(ref), L.es, L.es);                 // :139-141
            else         launch_deriv_stack(c, g, L.stack(s, 1), L.frame(ref), w_sp1, L.es, L.es);               // :143-144
        }
    }
    return smoothed;
}

// optimizeOcc (variational_aux_mt.cpp:758-887) for all windows: data costs from the warped pairs, exact two-label cut
static int optimize_occlusions(sfa_ctx *c, const Level &L, const sfa_params &p, const Geo &g, DevMem &scratch) {
    const int ref = L.ref;
    const size_t n = (size_t)L.nb * L.pl;
    SFA_TRY(scratch.alloc(c, (2 + kCutWorkPlanes) * n * sizeof(float)));
    float *d0 = scratch.f(), *d1 = d0 + n, *work = d1 + n;
    OccArgs oa;
    memset(&oa, 0, sizeof oa);
    oa.nslots = 2 * ref; oa.hd = p.delta / 3.0f; oa.hg = p.gamma / 3.0f; oa.penalty = p.occlusion_penalty;
    oa.color = pen(p.robust_color); oa.grad = pen(p.robust_grad);
    for (int s = 0; s < 2 * ref; s++) {
        const float *i1 = pair_image(L, s, 0), *i2 = pair_image(L, s, 1);
        const float *r1 = s < ref ? i1 : L.frame(ref), *r2 = s < ref ? L.frame(ref) : i2;                  // variational_mt.cpp:139-144
        const int idx = std::max(ref - s - 1, s - ref);
        oa.slot[s] = OccSlot{i1 - L.base, i2 - L.base, r1 - L.base, r2 - L.base, L.off_masks + (long)s * L.pl, p.rho[idx], p.omega[idx], s >= ref ? 0 : 1};
    }
    launch_occ_costs(c, g, oa, L.base, d0, d1, L.pl);
    return run_grid_cut(c, g, L.plane(P_OCC), L.es, d0, d1, work, p.occlusion_alpha);
}

// ---- compute_one_level (variational_mt.cpp:169-493) for all windows of a batch in lockstep: run_level, at the end of this section, and its steps ----

// one data term: `weight` (a rho or an omega) on slot `slot`, against the slot's next frame or (is_ref) the reference frame, `s` flow steps away
static Term data_term(const Level &L, const sfa_params &p, int slot, int is_ref, float weight, float s) {
    const float *i1 = pair_image(L, slot, 0), *i2 = pair_image(L, slot, 1);
    if (is_ref) { if (slot < L.ref) i2 = L.frame(L.ref); else i1 = L.frame(L.ref); }                         // :139-144
    return Term{L.off_stacks + ((long)slot * 2 + is_ref) * 24 * L.pl, L.off_masks + (long)slot * L.pl, weight * (p.delta / 3.0f), weight * (p.gamma / 3.0f), s, is_ref,
                i1 - L.base, i2 - L.base, slot < L.ref};                                                             // (delta, gamma over 3: :548-549)
}
// The level's data-term table: which terms are active (:343-361), in the reference's call order, and which slots need their to-reference stack (unfused form).  Host
// arithmetic only: it runs, and may refuse, before the level's first launch
static int data_terms(sfa_ctx *c, const Level &L, const sfa_params &p, const ChannelWeights &cw, AssembleArgs &aa, bool need_toref[2 * SFA_MAX_REF]) {
    const int ref = L.ref;
    memset(&aa, 0, sizeof aa);
    for (int s = 0; s < ref; s++) {
        const int a = ref - 1 - s;                                       // slot s looks back: the weights of a + 1 frames' distance
        if (!p.one_direction) {
            if (p.rho[a] > 0) aa.t[aa.n++] = data_term(L, p, s, 0, p.rho[a], (float)(s - ref));
            if (p.omega[a] > 0) { aa.t[aa.n++] = data_term(L, p, s, 1, p.omega[a], (float)(s - ref)); need_toref[s] = true; }
        }
        if (p.rho[s] > 0) aa.t[aa.n++] = data_term(L, p, ref + s, 0, p.rho[s], (float)s);
        if (p.omega[s] > 0) { aa.t[aa.n++] = data_term(L, p, ref + s, 1, p.omega[s], (float)(s + 1)); need_toref[ref + s] = true; }
        aa.data_norm += p.rho[s] + p.omega[s];                                                               // :223-226
    }
    for (int t = 0; t < aa.n; t++)
        if (aa.t[t].is_ref && aa.t[t].s == 0) return set_error(c, SFA_ERR_REF_FRAME, "Frame compared to reference frame is the reference frame itself!");
    aa.one_direction = p.one_direction; aa.dt_norm = p.dataterm_norm;
    aa.color = pen(p.robust_color); aa.grad = pen(p.robust_grad);
    aa.chw = cw.dev; aa.chw_pl = cw.pl; aa.chw_es = cw.es; aa.chw_pitch = cw.pitch; aa.chw_stride0 = cw.stride0; aa.lstride = L.lstride;
    aa.accumulate = 0; aa.do_laplacian = 1;
    return SFA_OK;
}

// What run_level decides once per level, and the level's planes under short names
struct LevelPlan {
    bool verbose;        // the reference's per-iteration lines are asked for: print_changes
    bool red_black;      // labelled mode: works on the row-major planes, never on the diagonal-major operands
    // the fused assembly can leave the solver's operands directly (no a11 .. b2 planes, no prepare pass) when the whole batch is solved in one launch.  In this form
    // the first inner iteration never touches du / dv / old du / old dv: they are zeros by construction
    bool direct;
    // uu = wx + du, vv = wy + dv (:396-397), and wx <- uu, wy <- vv at the end of every outer iteration (:428-429).  With ONE inner iteration and the fused update
    // (k_update_outer_x) the two pairs of planes always hold the same values when anybody reads them: smoothness and assembly then read wx, wy (UU, VV), and the
    // update writes 16 instead of 32 bytes per pixel.
    bool uv_alias;
    bool thres_in, thres_out;    // thresholds <= 0 never break, so no host round trip is needed
    float *wx, *wy, *uu, *vv, *du, *dv, *odu, *odv, *sh, *sv, *a11, *a12, *a22, *b1, *b2, *occ, *dpsis, *UU, *VV;
    // With an outer threshold the update leaves the per-pixel terms of the norms in the a11 / a12 planes (dead by then: the direct form never writes them, the other
    // forms' solver has read them), so that a window whose fp64 norm lies within break_band() of the threshold can be decided by the reference's own fp32 running
    // sums: dfa, dfb.  ifa, ifb: the same for the inner break, decided behind every inner iteration but the last
    float *dfa, *dfb, *ifa, *ifb;
    LevelPlan(const sfa_ctx *c, const Level &L, const sfa_params &p) {
        verbose = c->verbose_changes;
        red_black = p.sor_order == 1;
        direct = L.fused && !red_black && !sw_given(Switches::NO_DIRECT_OPERANDS);
        uv_alias = direct && p.niter_inner == 1 && !sw_given(Switches::NO_UV_ALIAS) && !verbose;
        thres_in = p.thres_inner > 0; thres_out = p.thres_outer > 0;
        wx = L.plane(P_WX); wy = L.plane(P_WY); uu = L.plane(P_UU); vv = L.plane(P_VV); du = L.plane(P_DU); dv = L.plane(P_DV);
        odu = L.plane(P_ODU); odv = L.plane(P_ODV); sh = L.plane(P_SH); sv = L.plane(P_SV); a11 = L.plane(P_A11); a12 = L.plane(P_A12);
        a22 = L.plane(P_A22); b1 = L.plane(P_B1); b2 = L.plane(P_B2); occ = L.plane(P_OCC); dpsis = L.plane(P_DPSIS);
        UU = uv_alias ? wx : uu; VV = uv_alias ? wy : vv;
        dfa = thres_out && !sw_given(Switches::NO_EXACT_BREAK) ? a11 : nullptr; dfb = dfa ? a12 : nullptr;
        ifa = thres_in && !sw_given(Switches::NO_EXACT_BREAK) ? a11 : nullptr; ifb = ifa ? a12 : nullptr;
    }
};

// The outer break (:431-436) is taken ON THE DEVICE: k_outer_threshold clears a window's bit in *d_amask when its norms meet the threshold, and every
// kernel (the solver included) leaves the windows without a bit alone.  The host never waits for the iteration it has just queued: it reads the mask
// of kMaskLag iterations ago (a superset -- windows only ever leave) to stop queueing once nothing iterates any more, so the GPU always has work queued
// and at most kMaskLag iterations of empty launches follow the last window's break.  One blocking read per level (the norms), not one per iteration.
// The masks travel through a ring of kMaskRing pinned words, one per outer iteration in flight, each with the event that says its copy has landed.
struct OuterBreak {
    sfa_ctx *c; bool on;             // on: an outer threshold is set; without one nothing is published and every window is known to iterate
    // the windows known to iterate at outer iteration n: `active` as it is before iteration kMaskLag, then what iteration n - kMaskLag published
    int known(int n, WMask &active) const {
        if (!on || n < kMaskLag) return SFA_OK;
        const int slot = (n - kMaskLag) % kMaskRing;
        SFA_HIP(c, hipEventSynchronize(c->ev_mask[slot]));
        for (int i = 0; i < kMaskWords; i++) active.w[i] = *(volatile unsigned long long *)&c->h_amask[slot].w[i];
        return SFA_OK;
    }
    // publish the device's mask as outer iteration n left it
    int publish(int n) const {
        if (!on) return SFA_OK;
        const int slot = n % kMaskRing;
        SFA_HIP(c, hipMemcpyAsync(&c->h_amask[slot], c->d_amask, sizeof(WMask), hipMemcpyDeviceToHost, c->stream));
        SFA_HIP(c, hipEventRecord(c->ev_mask[slot], c->stream));
        return SFA_OK;
    }
};

// The reference's per-iteration lines (variational_mt.cpp:404-405, 431-432: "inner it i avg change a,b" / "outer it i avg change a,b" under verbosity(VER_CMD)).
// Printing them needs the norms on the host after every iteration -- a synchronisation per iteration --, so it is off unless SFA_VERBOSE_CHANGES is set (the C++
// class and the driver set it when the cfg's `verbose` asks for it).  Batches print one line per window of `who`, in window order.
static void print_changes(sfa_ctx *c, const Level &L, const char *what, int it, const WMask &who) {
    if (hipMemcpyAsync(c->h_red, c->d_red, 2 * L.nb * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return;
    const double n = (double)L.w * L.h;
    for (int b = 0; b < L.nb; b++)
        if (who.test(b)) {
            if (L.nb > 1) printf("[window %d] ", b);
            printf("%s %d\tavg change %g,%g\n", what, it, (double)(float)(c->h_red[2 * b] / n), (double)(float)(c->h_red[2 * b + 1] / n));
        }
    fflush(stdout);
}

// One inner iteration up to its solve (:329-368) for the windows of gi: old du, smoothness, the linear system, SOR.  first_zero: du = dv = 0 known, planes possibly
// stale (LevelPlan::direct).  smoothed: get_derivatives left the smoothness weights of this flow in its own pass
static int assemble_and_solve(sfa_ctx *c, const Level &L, const sfa_params &p, const LevelPlan &P, AssembleArgs &aa, SorWorkspace &sorws, const Geo &gi, bool first_zero,
                       bool smoothed) {
    if (!first_zero) launch_copy_planes(c, gi, P.odu, P.du, 2, L.es, L.es);                                  // :329-330 (du, dv adjacent)
    if (!smoothed) launch_smoothness(c, gi, p.smoothing, P.sh, P.sv, P.UU, P.VV, P.dpsis, p.alpha, pen(p.robust_reg));   // :333
    aa.op = SorOperandOut();
    aa.zero_duv = first_zero ? 1 : 0;
    if (P.direct) SFA_TRY(sor_operand_target(c, sorws, gi, p.niter_solver, &aa.op));
    if (L.fused) SFA_TRY(launch_assemble_images(c, gi, aa, L.base, P.a11, P.a12, P.a22, P.b1, P.b2, P.du, P.dv, P.UU, P.VV, P.sh, P.sv, P.occ));   // :293-365
    else launch_assemble(c, gi, aa, L.base, P.a11, P.a12, P.a22, P.b1, P.b2, P.du, P.dv, P.uu, P.vv, P.sh, P.sv);                               // :336-365
    if (P.direct) return sor_run_prepared(c, sorws, gi, nullptr, nullptr, p.niter_solver, p.sor_omega);                                        // :368
    if (P.red_black) return sor_rb_run(c, gi, P.du, P.dv, P.a11, P.a12, P.a22, P.b1, P.b2, P.sh, P.sv, p.niter_solver, p.sor_omega);
    return sor_run(c, sorws, gi, P.du, P.dv, P.a11, P.a12, P.a22, P.b1, P.b2, P.sh, P.sv, p.niter_solver, p.sor_omega, false);                   // :368
}

// The flow update behind the solve (:371-402), from wherever the solver left du, dv.  true: the outer update (:412-429) has left in the same pass
static bool update_flow(sfa_ctx *c, const sfa_params &p, const LevelPlan &P, const SorOperandOut &x, const Geo &gi, int inner, bool first_zero) {
    const bool last = inner + 1 == p.niter_inner;
    float *const ia = last ? nullptr : P.ifa, *const ib = last ? nullptr : P.ifb;      // an inner break is decided behind this iteration
    if (P.direct && last && !P.verbose) {
        // last inner iteration: nothing reads its inner norms or du/dv; the flow update and the outer update run as one pass (with the per-iteration
        // lines on somebody does read the inner norms, :404-405: the two passes otherwise)
        launch_update_outer_x(c, gi, P.uv_alias ? nullptr : P.uu, P.uv_alias ? nullptr : P.vv, P.wx, P.wy, x, c->d_red, P.dfa, P.dfb);          // :396-397 + :412-429
        return true;
    }
    if (P.direct)                                                       // du, dv are read again only by a further inner iteration
        launch_update_inner_x(c, gi, P.uu, P.vv, P.wx, P.wy, x, first_zero ? nullptr : P.odu, first_zero ? nullptr : P.odv, last ? nullptr : P.du,
                              last ? nullptr : P.dv, c->d_red, ia, ib);
    else
        launch_update_inner(c, gi, P.uu, P.vv, P.wx, P.wy, P.du, P.dv, P.odu, P.odv, c->d_red, ia, ib);
    return false;
}

// The inner break (:407) behind an inner iteration that is not the last: the windows of in_active whose norms (c->d_red) meet the threshold leave it.  A blocking
// read; windows within break_band() of the threshold are decided by a second one, of the reference's own fp32 sums (P.ifa; not under SFA_NO_EXACT_BREAK)
static int inner_break(sfa_ctx *c, const Level &L, const sfa_params &p, const LevelPlan &P, const Geo &gi, WMask &in_active) {
    const double npx = (double)L.h * L.w;
    SFA_HIP(c, hipMemcpyAsync(c->h_red, c->d_red, 2 * L.nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    SFA_HIP(c, hipStreamSynchronize(c->stream));
    WMask close = WMask::none();
    for (int b = 0; b < L.nb; b++)
        if (in_active.test(b)) {
            const double ad = c->h_red[2 * b] / npx, dd = c->h_red[2 * b + 1] / npx, dm = (ad < dd) ? dd : ad;
            if (P.ifa && fabs(dm - (double)p.thres_inner) <= break_band(L.w, L.h) * (double)p.thres_inner) { close.set(b); continue; }
            if (std::max((float)ad, (float)dd) < p.thres_inner) in_active.clear(b);                          // :407
        }
    if (!close.any()) return SFA_OK;
    float *const dx = c->d_last->exact;
    const float *const hx = reinterpret_cast<const LastBlock *>(c->h_red)->exact;                             // pinned (a pageable target would be a staged, blocking copy)
    launch_exact_norms(c, gi, P.ifa, P.ifb, close, dx);
    SFA_HIP(c, hipMemcpyAsync(const_cast<float *>(hx), dx, 2 * L.nb * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SFA_HIP(c, hipStreamSynchronize(c->stream));
    for (int b = 0; b < L.nb; b++)
        if (close.test(b) && std::max(hx[2 * b], hx[2 * b + 1]) < p.thres_inner) in_active.clear(b);         // :407 on the reference's own sums
    return SFA_OK;
}

// The inner iterations (:326-409) of one outer iteration for the windows of g.active, and the outer update (:412-429) of every one of them.  Windows that already
// met a threshold stay in the lockstep launches as passengers: every kernel skips them (Geo::active and Geo::amask; the solver's workgroups of a passenger return
// as soon as they have drawn their ticket)
static int inner_iterations(sfa_ctx *c, const Level &L, const sfa_params &p, const LevelPlan &P, AssembleArgs &aa, SorWorkspace &sorws, const Geo &g, bool smoothed) {
    if (!P.direct) launch_zero_planes(c, g, P.du, 2);                                                        // :323-324 (du, dv adjacent)
    WMask in_active = g.active, outer_done = WMask::none();
    for (int inner = 0; inner < p.niter_inner; inner++) {
        Geo gi = g;
        gi.active = in_active;
        const bool first_zero = P.direct && inner == 0;
        SFA_TRY(assemble_and_solve(c, L, p, P, aa, sorws, gi, first_zero, smoothed && inner == 0));   // (uv_alias: one inner iteration, UU / VV are wx / wy -- what the fused pass read)
        if (update_flow(c, p, P, aa.op, gi, inner, first_zero)) outer_done = in_active;
        if (P.verbose) print_changes(c, L, "\tinner it", inner, in_active);                                  // :404-405
        if (P.thres_in && inner + 1 < p.niter_inner) {
            SFA_TRY(inner_break(c, L, p, P, gi, in_active));
            if (!in_active.any()) break;
        }
    }
    if (outer_done != g.active) {
        // windows that left the inner loop early (or the forms without the fused update): their outer update.  The reductions only write the result
        // words of the windows of their Geo::active, so the norms of the windows updated above stay in `red`.
        Geo go = g;
        go.active = g.active.andnot(outer_done);
        launch_update_outer(c, go, P.wx, P.wy, P.uu, P.vv, c->d_red, P.dfa, P.dfb);                             // :412-429
    }
    return SFA_OK;
}
// change: nb x 2 floats (host), or null.  occ_log (level 0 only, or null): [nb][niter_alter][pl] floats, the labels after the discrete step of alternation
// a >= 1 -- what the reference writes as <slow_flow_occlusions_output><a>.png at every level, the finest level's file surviving (:275-285)
static int run_level(sfa_ctx *c, const Level &L, const sfa_params &p, const ChannelWeights &cw, SorWorkspace &sorws, DevMem &cut_scratch, float *change, float *occ_log) {
    AssembleArgs aa;
    bool need_toref[2 * SFA_MAX_REF] = {false};
    SFA_TRY(data_terms(c, L, p, cw, aa, need_toref));
    const LevelPlan P(c, L, p);
    const OuterBreak brk{c, P.thres_out};
    const WMask all = WMask::first(L.nb);
    Geo g = L.geo(all);
    launch_fill_planes(c, g, P.occ, 1, (p.one_direction || p.occlusion_reasoning) ? -1.0f : 0.0f);           // occlusions: 0, or -1 (:216-220)
    launch_dpsis(c, g, P.dpsis, L.frame(L.ref), L.es, 5.0f, p.norm_avg, p.norm_std, p.hbit);                 // :257
    if (!P.uv_alias) launch_copy_planes(c, g, P.uu, P.wx, 2, L.es, L.es);                                    // :260-261 (wx,wy and uu,vv adjacent)
    g.amask = c->d_amask;
    SFA_HIP(c, hipMemsetAsync(c->d_last, 0, sizeof(LastBlock), c->stream));   // (the norms, the windows' finished-block counters of k_update_outer_x, ...)
    launch_set_mask(c, all);

    for (int alter = 0; alter < p.niter_alter; alter++) {
        WMask active = all;
        g.active = active;
        if (P.thres_out && alter > 0) launch_set_mask(c, all);
        bool smoothed = get_derivatives(c, L, p, g, need_toref, P.uv_alias);                                // :266 (+ :333 of the first outer iteration)
        if (alter > 0 && p.occlusion_reasoning && !p.one_direction) SFA_TRY(optimize_occlusions(c, L, p, g, cut_scratch));   // :269-272
        if (alter > 0 && p.occlusion_reasoning && occ_log)                                                  // :275-285
            launch_copy_planes(c, g, occ_log + (long)alter * L.pl, P.occ, 1, (long)p.niter_alter * L.pl, L.es);
        for (int outer = 0; outer < p.niter_outer; outer++) {
            SFA_TRY(brk.known(outer, active));
            if (!active.any()) break;                                                                    // :436, every window
            if (sw_given(Switches::DEBUG_ACTIVE)) fprintf(stderr, "level %dx%d alter %d outer %d known active %d\n", L.w, L.h, alter, outer, active.count());
            g.active = active;
            if (outer > 0) smoothed = get_derivatives(c, L, p, g, need_toref, P.uv_alias);                  // :289-290 (+ :333)
            if (!L.fused) launch_mask_weight(c, g, L.mask(0), P.occ, aa.data_norm, L.ref, p.one_direction);   // :293-320
            SFA_TRY(inner_iterations(c, L, p, P, aa, sorws, g, smoothed));                                   // :323-429
            if (P.verbose) print_changes(c, L, "outer it", outer, active);                                   // :431-432
            const bool last_iter = (alter == p.niter_alter - 1 && outer == p.niter_outer - 1);
            if (P.thres_out || last_iter) launch_outer_threshold(c, g, c->d_red, P.thres_out ? p.thres_outer : 0.0f, P.dfa, P.dfb);   // :431-436
            SFA_TRY(brk.publish(outer));
        }
    }
    // the norms of every window's last outer iteration -- where the caller wants them (the finest level: the coarser levels' are overwritten, variational_mt.cpp:761), and
    // only there does the host wait for the level: a blocking read per level left the GPU idle for ~30 us five times per run (a lone window: 2 % of its time)
    if (change) {
        SFA_HIP(c, hipMemcpyAsync(c->h_red, c->d_last->last, 2 * L.nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        SFA_HIP(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < 2 * L.nb; i++) change[i] = (float)c->h_red[i];
    }
    return SFA_OK;
}

// ---- pyramid geometry (variational_mt.cpp:576-652) ------------------------------------------------------------------------------------------------
static int gaussian_filter_order(float sigma) {      // image.c:320-322
    int order = (int)floor(3 * sigma) + 1;
    if (order == 0) order = 1;
    return order;
}
static int pyramid_sizes(int w, int h, int layers, float p_scale, int *ws, int *hs) {
    const float sigma = 1 / sqrtf(2 * p_scale);      // :578
    const int order = gaussian_filter_order(sigma);
    for (int l = 0; l < layers; l++) {
        ws[l] = l == 0 ? w : (int)(float)floor(ws[l - 1] * p_scale);   // :609-611 (product rounded to fp32 before the floor)
        hs[l] = l == 0 ? h : (int)(float)floor(hs[l - 1] * p_scale);
        if (floor(ws[l] * p_scale) <= order + 1 || floor(hs[l] * p_scale) <= order + 1) return l;   // :647-651
    }
    return layers;
}

}  // namespace sfa
using namespace sfa;

// ---- the resident job (variational over a batch): nb element arenas (the layout: top of this file) and what belongs to the windows besides ----------
struct sfa_job {
    sfa_ctx *ctx = nullptr;
    sfa_params p;
    int w = 0, h = 0, nb = 0, ref = 0, F = 0, L = 0;
    int ws[64], hs[64];
    long es = 0;                       // floats per element (all levels)
    std::vector<long> level_off;       // offset of each level's PERSISTENT part inside the element
    long trans_off = 0;                // offset of the transient part (shared by all levels)
    bool share_sor = false;            // large frames: one solver workspace for all levels (re-shaped per level), not one per level
    DevMem arena;                      // nb * es floats
    DevMem init_flow;                  // nb x 2 planes at level-0 pitch: the uploaded initial flow
    DevMem chw;                        // nb x 3 planes (level-0 pitch) or empty
    DevMem cut_scratch;                // occlusion step: 2 cost planes + the cut's work planes, [nb][pl] each, grown on demand
    bool has_chw = false;              // chw is in use,
    int chw_stride0 = 0;               // for host rows of chw_stride0 floats
    std::vector<std::unique_ptr<SorWorkspace>> sor;   // one per level: no re-allocation between runs
    std::vector<float> change;         // nb x 2
    double mpix_iters = 0;
    int host_stride0 = 0;              // the stride of the last upload's host planes (host_stride(w) before any): level 0's lstride
    bool fused = true;                 // false: SFA_UNFUSED=1 at creation (stack planes materialised; cross-check only)
    float pyr_taps[kMaxBlurTaps] = {}; // the pyramid's blur, sigma = 1 / sqrt(2 p_scale) (:578): sfa_job_create refuses a p_scale whose taps do not fit
    int pyr_radius = 0;
    Level level(int l) const {
        Level Lv;
        Lv.layout(arena.f() + trans_off, arena.f() + level_off[l], ws[l], hs[l], l == 0 ? host_stride0 : host_stride(ws[l]), ref, nb, es, fused);
        return Lv;
    }
    WMask presmoothed = WMask::none();    // windows whose level-0 frames already hold the presmoothed images (cfg sigma > 0): smoothing is applied once per upload
    bool keep_alt_occ = false;         // record the occlusion labels of every alternation (slow_flow_occlusions_output, variational_mt.cpp:275-285)
    DevMem occ_log;                    // [nb][niter_alter][pl(level 0)]
    // sfa_job_upload_device: the caller's host channel weights go through a pinned copy, so that the call need not wait for the stream; ev_chw says the copies
    // out of it have been made
    float *chw_stage = nullptr;
    hipEvent_t ev_chw = nullptr;
};

static int job_windows(sfa_ctx *ctx, const char *fn, const sfa_job *j, int b0, int n) { return check_batch_range(ctx, fn, "windows", b0, n, j->nb); }

// make sure the job has weight planes for rows of `stride` floats: ones for every window until set.  The first call fixes the job's stride; the callers refuse another
static int job_weight_planes(sfa_job *j, int stride) {
    if (j->has_chw) return SFA_OK;
    const size_t n = (size_t)j->nb * 3 * dev_pitch(stride) * j->h;
    SFA_TRY(j->chw.alloc(j->ctx, n * sizeof(float)));
    launch_fill(j->ctx, j->chw.f(), n, 1.0f);
    j->has_chw = true;
    j->chw_stride0 = stride;
    return SFA_OK;
}
static int job_set_channel_weights(sfa_job *j, int b, int stride, const float *const chw[3]) {
    sfa_ctx *ctx = j->ctx;
    if (chw) {
        // weights keep the level-0 host geometry, padding lanes included (the reference indexes them linearly)
        CHECK_ARGS((long)stride * j->h < (1L << 31), "channel weights: the linear pixel index must fit 31 bits");
        SFA_TRY(job_weight_planes(j, stride));
        CHECK_ARGS(j->chw_stride0 == stride, "channel weights of all elements must share one stride");
        const int cp = dev_pitch(stride);
        for (int k = 0; k < 3; k++) {
            CHECK_ARGS(chw[k], "null weight plane");
            SFA_TRY(upload_plane(ctx, j->chw.f() + ((long)b * 3 + k) * cp * j->h, cp, chw[k], stride, stride, j->h));
        }
    } else if (j->has_chw) {
        // a slot that held weighted channels before (jobs are reused for batch after batch) goes back to all ones
        launch_fill(ctx, j->chw.f() + (long)b * 3 * dev_pitch(j->chw_stride0) * j->h, (size_t)3 * dev_pitch(j->chw_stride0) * j->h, 1.0f);
    }
    return SFA_OK;
}
// the tail of an upload from the host: window b's initial flow from host planes (null: zeros), then its channel weights.  Enqueued; the caller waits
static int job_upload_flow_and_weights(sfa_job *j, int b, const float *wx, const float *wy, int stride, const float *const chw[3]) {
    sfa_ctx *ctx = j->ctx;
    const Level L0 = j->level(0);
    const float *const host[2] = {wx, wy};
    for (int k = 0; k < 2; k++) {
        float *dst = j->init_flow.f() + ((long)b * 2 + k) * L0.pl;
        if (host[k]) SFA_TRY(upload_plane(ctx, dst, L0.pitch, host[k], stride, j->w, j->h));
        else SFA_HIP(ctx, hipMemsetAsync(dst, 0, L0.pl * sizeof(float), ctx->stream));
    }
    return job_set_channel_weights(j, b, stride, chw);
}
// ---- sfa_job_run's stages: presmoothing, the pyramid, the coarsest level's initial flow -------------------------------------------------------------
static void job_presmooth(sfa_job *j) {                                                // :590-597
    const WMask all = WMask::first(j->nb);
    if (!(j->p.presmooth_sigma > 0) || (j->presmoothed & all) == all) return;
    // the smoothed frames replace the uploaded ones, once per upload: a job may be run again (warm-up + timed runs, a second pass
    // over the same windows) and must then start from the same images
    const Level L0 = j->level(0);
    float *tmp = L0.tmp();
    for (int f = 0; f < j->F; f++) {
        launch_presmooth(j->ctx, L0.geo(all), tmp + 3 * L0.pl, tmp, L0.frame(f), 3, j->p.presmooth_sigma);
        launch_copy_planes(j->ctx, L0.geo(all.andnot(j->presmoothed)), L0.frame(f), tmp + 3 * L0.pl, 3, L0.es, L0.es);
    }
    j->presmoothed = all;
}
static int job_pyramid(sfa_job *j) {                                                   // :583-652
    for (int l = 1; l < j->L; l++) {
        const Level Lp = j->level(l - 1), Lc = j->level(l);
        // all F frames (3 F consecutive planes per window) in one pass where :607 + :611 fuse, else frame by frame through the level's scratch (pyramid_step).
        // The taps are sfa_job_create's: a job whose blur the kernels do not hold is never created
        SFA_TRY(pyramid_step(j->ctx, Lc.frame(0), Lc.w, Lc.h, Lc.pitch, Lc.pl, Lc.es, Lp.frame(0), Lp.w, Lp.h, Lp.pitch, Lp.pl, Lp.es, 3 * j->F, j->nb, j->pyr_taps,
                             j->pyr_radius, Lp.tmp()));
    }
    return SFA_OK;
}
static void job_initial_flow(sfa_job *j) {                                             // :662-681
    const Level L0 = j->level(0), Lt = j->level(j->L - 1);
    if (j->L > 1) {
        const float fx = (1.0f * Lt.w) / j->w, fy = (1.0f * Lt.h) / j->h;
        launch_resize_flow(j->ctx, Lt.plane(P_WX), Lt.plane(P_WY), Lt.w, Lt.h, Lt.pitch, Lt.es, j->init_flow.f(), j->init_flow.f() + L0.pl, j->w, j->h, L0.pitch, 2 * L0.pl, j->nb, fx, fy);
    } else {
        launch_copy_planes(j->ctx, L0.geo(), L0.plane(P_WX), j->init_flow.f(), 2, L0.es, 2 * L0.pl);
    }
}

extern "C" {

int sfa_pyramid_sizes(int w, int h, int layers, float p_scale, int *ws, int *hs) {
    if (layers < 1 || layers > 64 || !ws || !hs) return 0;
    return pyramid_sizes(w, h, layers, p_scale, ws, hs);
}

int sfa_job_create(sfa_ctx *ctx, const sfa_params *p, int w, int h, int batch, sfa_job **out) {
    CHECK_ARGS(ctx && p && out && w >= 2 && h >= 5 && batch > 0 && batch <= kMaxBatch, "bad arguments (h >= 5, w >= 2)");
    CHECK_ARGS(p->S >= 2 && p->S - 1 <= SFA_MAX_REF && p->layers >= 1 && p->layers <= 64, "unsupported slow_flow_S / slow_flow_layers");
    CHECK_ARGS(2L * kMaxBatch + 2L * batch * ((w + 63) / 64) * 16 <= kRedDoubles, "batch x width beyond the change norms' scratch (sfa_internal.h: kRedDoubles)");
    // p_scale sizes the levels (:609-611) and the pyramid's blur (:578): outside (0, 1] the levels do not shrink or sigma is no number, and a very small
    // one asks for more taps than k_gauss_h / k_gauss_v carry
    if (!(p->p_scale > 0) || p->p_scale > 1) REFUSE("%s: p_scale = %g must lie in (0, 1]", __func__, (double)p->p_scale);
    float taps[kMaxBlurTaps] = {};
    const int radius = cv_gauss_taps(1 / sqrtf(2 * p->p_scale), taps);
    if (radius < 0)
        REFUSE("%s: p_scale = %g: the pyramid's blur, sigma = 1 / sqrt(2 p_scale) = %g, needs more than the %d taps the blur kernels hold", __func__,
               (double)p->p_scale, (double)(1 / sqrtf(2 * p->p_scale)), kMaxBlurTaps);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_ptr<sfa_job> j(new sfa_job());
    j->ctx = ctx; j->p = *p; j->w = w; j->h = h; j->nb = batch; j->ref = p->S - 1; j->F = 2 * j->ref + 1;
    memcpy(j->pyr_taps, taps, sizeof taps); j->pyr_radius = radius;
    j->L = pyramid_sizes(w, h, p->layers, p->p_scale, j->ws, j->hs);
    CHECK_ARGS(j->L >= 1, "image too small for even one pyramid level");
    j->fused = sw_int(Switches::UNFUSED, 0) == 0;
    long off = 0;
    double px = 0;
    for (int l = 0; l < j->L; l++) {
        j->level_off.push_back(off);
        off += Level::persistent_floats(dev_pitch(j->ws[l]), j->hs[l], j->ref);
        j->sor.emplace_back(new SorWorkspace());
        px += (double)j->ws[l] * j->hs[l];
    }
    j->trans_off = off;
    off += Level::transient_floats(dev_pitch(j->ws[0]), j->hs[0], j->ref, j->fused);     // level 0 is the largest
    j->es = off;
    // the solver workspaces (40 bytes per entry of the diagonal-major planes) of all levels together are 3.5 x the finest one's: from 2 Mpx on, one
    // workspace is re-shaped level by level (a few memsets per level against hundreds of ms of refinement); below that every level keeps its own
    j->share_sor = (double)w * h >= 2.0e6 || sw_given(Switches::SHARE_SOR);
    j->host_stride0 = host_stride(w);
    SFA_TRY(j->arena.alloc(ctx, (size_t)batch * j->es * sizeof(float)));
    SFA_HIP(ctx, hipMemsetAsync(j->arena.p, 0, (size_t)batch * j->es * sizeof(float), ctx->stream));
    SFA_TRY(j->init_flow.alloc(ctx, (size_t)batch * 2 * dev_pitch(w) * h * sizeof(float)));
    SFA_HIP(ctx, hipMemsetAsync(j->init_flow.p, 0, (size_t)batch * 2 * dev_pitch(w) * h * sizeof(float), ctx->stream));
    j->change.assign(2 * batch, 0.f);
    // sum over levels of outer x inner solves (thresholds may end earlier; this is the scheduled amount)
    j->mpix_iters = px * p->niter_alter * p->niter_outer * p->niter_inner * p->niter_solver * batch / 1e6;
    *out = j.release();
    return SFA_OK;
}
void sfa_job_destroy(sfa_job *j) {
    if (!j) return;
    (void)hipSetDevice(j->ctx->device);
    (void)hipStreamSynchronize(j->ctx->stream);
    if (j->ev_chw) (void)hipEventDestroy(j->ev_chw);
    if (j->chw_stage) (void)hipHostFree(j->chw_stage);
    delete j;
}
double sfa_job_mpix_iters(const sfa_job *j) { return j ? j->mpix_iters : 0; }
double sfa_job_device_bytes(const sfa_job *j) {
    if (!j) return 0;
    double b = (double)j->arena.bytes + j->init_flow.bytes + j->chw.bytes + j->cut_scratch.bytes + j->occ_log.bytes;
    for (const auto &w : j->sor) b += (double)w->sa.bytes + w->sb.bytes + w->x.bytes + w->flags.bytes + w->order.bytes + w->edge.bytes;
    return b;
}

int sfa_job_upload(sfa_job *j, int b, const float *const *frames, int n_frames, const float *wx, const float *wy, int stride, const float *const chw[3]) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j && b >= 0 && b < j->nb && frames && n_frames == j->F && stride >= j->w, "bad arguments (n_frames must be 2*(S-1)+1)");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    Level L0 = j->level(0);
    j->host_stride0 = stride;
    j->presmoothed.clear(b);
    for (int f = 0; f < j->F; f++) {
        CHECK_ARGS(frames[f], "null frame");
        for (int k = 0; k < 3; k++)
            SFA_TRY(upload_plane(ctx, L0.frame(f) + b * j->es + k * L0.pl, L0.pitch, frames[f] + (size_t)k * stride * j->h, stride, j->w, j->h));
    }
    SFA_TRY(job_upload_flow_and_weights(j, b, wx, wy, stride, chw));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

// the same as sfa_job_upload with the frames taken from a sequence resident on the job's GPU (device-to-device copies on the job's stream): a frame is
// sent over PCIe once however many windows it is part of (S=3: five windows, both directions) and normalize never brings it back to the host
int sfa_job_upload_resident(sfa_job *j, int b, const sfa_sequence *q, const int *frame_index, int n_frames, const float *wx, const float *wy, int stride,
                            const float *const chw[3]) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j && q && frame_index && b >= 0 && b < j->nb && n_frames == j->F && stride >= j->w, "bad arguments (n_frames must be 2*(S-1)+1)");
    CHECK_ARGS(q->w == j->w && q->h == j->h && q->ctx->device == ctx->device, "the sequence must have the job's frame size and live on the job's GPU");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    Level L0 = j->level(0);
    j->host_stride0 = stride;
    j->presmoothed.clear(b);
    for (int f = 0; f < j->F; f++) {
        CHECK_ARGS(frame_index[f] >= 0 && frame_index[f] < q->n, "frame index out of range");
        SFA_HIP(ctx, hipMemcpyAsync(L0.frame(f) + b * j->es, q->frame(frame_index[f]), (size_t)3 * L0.pl * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    }
    SFA_TRY(job_upload_flow_and_weights(j, b, wx, wy, stride, chw));
    if (wx || wy || chw) SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));   // host buffers may go away after the call
    return SFA_OK;
}

int sfa_job_reset_flow(sfa_job *j) { return j ? SFA_OK : SFA_ERR_ARG; }   // the initial flow is re-read by every run

int sfa_job_run(sfa_job *j) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "null job");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    job_presmooth(j);
    SFA_TRY(job_pyramid(j));
    job_initial_flow(j);
    ChannelWeights cw;
    if (j->has_chw) {
        cw.dev = j->chw.f(); cw.pitch = dev_pitch(j->chw_stride0); cw.pl = (long)cw.pitch * j->h; cw.es = 3 * cw.pl; cw.stride0 = j->chw_stride0;
    }
    // ---- coarse to fine (:684-762) -----------------------------------------------------------------------------
    for (int l = j->L - 1; l >= 0; l--) {
        Level Lc = j->level(l);
        if (l < j->L - 1) {
            Level Ln = j->level(l + 1);
            const float fx = (1.0f * Lc.w) / Ln.w, fy = (1.0f * Lc.h) / Ln.h;                                   // :703-704
            launch_resize_flow(ctx, Lc.plane(P_WX), Lc.plane(P_WY), Lc.w, Lc.h, Lc.pitch, Lc.es, Ln.plane(P_WX), Ln.plane(P_WY), Ln.w, Ln.h, Ln.pitch, Ln.es, j->nb, fx, fy);   // :711,716
        }
        SFA_TRY(run_level(ctx, Lc, j->p, cw, *j->sor[j->share_sor ? 0 : l], j->cut_scratch, l == 0 ? j->change.data() : nullptr, l == 0 && j->keep_alt_occ ? j->occ_log.f() : nullptr));   // :761
    }
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_job_download(sfa_job *j, int b, float *wx, float *wy, int stride, float change[2]) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j && b >= 0 && b < j->nb && wx && wy && stride >= j->w, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    Level L0 = j->level(0);
    SFA_TRY(download_plane(ctx, wx, stride, L0.plane(P_WX) + b * j->es, L0.pitch, j->w, j->h));
    SFA_TRY(download_plane(ctx, wy, stride, L0.plane(P_WY) + b * j->es, L0.pitch, j->w, j->h));
    if (change) { change[0] = j->change[2 * b]; change[1] = j->change[2 * b + 1]; }
    return sfa_ctx_sync(ctx);
}

int sfa_job_keep_alternation_occlusions(sfa_job *j, int on) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "null job");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    j->keep_alt_occ = on != 0;
    if (on) {
        const size_t n = (size_t)j->nb * std::max(1, j->p.niter_alter) * dev_pitch(j->w) * j->h * sizeof(float);
        SFA_TRY(j->occ_log.alloc(ctx, n));
        SFA_HIP(ctx, hipMemsetAsync(j->occ_log.p, 0, n, ctx->stream));
    }
    return SFA_OK;
}

int sfa_job_download_alternation_occlusions(sfa_job *j, int b, int alter, float *occ, int stride) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j && b >= 0 && b < j->nb && occ && stride >= j->w, "bad arguments");
    CHECK_ARGS(j->keep_alt_occ && j->occ_log.p, "sfa_job_keep_alternation_occlusions was not enabled before the run");
    CHECK_ARGS(alter >= 1 && alter < j->p.niter_alter, "alternation out of range: labels exist for 1 <= alter < niter_alter (variational_mt.cpp:269)");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const int pitch = dev_pitch(j->w);
    const long pl = (long)pitch * j->h;
    SFA_TRY(download_plane(ctx, occ, stride, j->occ_log.f() + ((long)b * j->p.niter_alter + alter) * pl, pitch, j->w, j->h));
    return sfa_ctx_sync(ctx);
}

int sfa_job_download_occlusions(sfa_job *j, int b, float *occ, int stride) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j && b >= 0 && b < j->nb && occ && stride >= j->w, "bad arguments");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    Level L0 = j->level(0);
    SFA_TRY(download_plane(ctx, occ, stride, L0.plane(P_OCC) + b * j->es, L0.pitch, j->w, j->h));
    return sfa_ctx_sync(ctx);
}

// test hook: the three planes of frame f of window b at pyramid level `level`, as the last run's pyramid (level 0: the upload, presmoothed if the cfg says so) left them
int sfa_job_download_level_frame(sfa_job *j, int b, int level, int f, float *frame3, int stride) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    CHECK_ARGS(frame3, "frame3 is null");
    if (b < 0 || b >= j->nb) REFUSE("%s: window b = %d outside the job's %d", __func__, b, j->nb);
    if (level < 0 || level >= j->L) REFUSE("%s: level = %d outside the job's %d pyramid levels", __func__, level, j->L);
    if (f < 0 || f >= j->F) REFUSE("%s: frame f = %d outside the window's %d", __func__, f, j->F);
    const Level Lv = j->level(level);
    if (stride < Lv.w) REFUSE("%s: stride = %d below level %d's width %d", __func__, stride, level, Lv.w);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    for (int k = 0; k < 3; k++)
        SFA_TRY(download_plane(ctx, frame3 + (size_t)k * stride * Lv.h, stride, Lv.frame(f) + b * j->es + k * Lv.pl, Lv.pitch, Lv.w, Lv.h));
    return sfa_ctx_sync(ctx);
}

// ---- the device seam (include/slowflow_amd.h; kernels: device_io.hip; the argument checks: dev_view.h and api.hip, declared in sfa_internal.h) -------
// Every check is taken on the host before anything is launched; a refusal names the argument.
int sfa_job_upload_device(sfa_job *j, int b0, int n, const void *frames_dev, const sfa_dev_layout *l, const float *const chw[3]) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(job_windows(ctx, __func__, j, b0, n));
    SFA_TRY(check_frames_source(ctx, __func__, frames_dev, l, l ? l->window : 0, n, j->F, j->w, j->h));
    const int stride = host_stride(j->w);
    if (chw) {
        CHECK_ARGS(chw[0] && chw[1] && chw[2], "chw holds a null weight plane");
        CHECK_ARGS(!j->has_chw || j->chw_stride0 == stride, "chw: the job already holds channel weights of another stride");
    }
    Level L0 = j->level(0);
    j->host_stride0 = stride;
    for (int b = b0; b < b0 + n; b++) j->presmoothed.clear(b);
    const PackSrc src{frames_dev, l->dtype, l->window, l->frame, l->channel, l->row, l->column};
    launch_pack_frames(ctx, L0.frame(0) + (long)b0 * j->es, j->es, L0.pl, L0.pitch, j->w, j->h, n, j->F, src);
    if (chw) {
        const size_t plane = (size_t)stride * j->h;
        if (!j->chw_stage) {
            SFA_HIP(ctx, hipHostMalloc((void **)&j->chw_stage, 3 * plane * sizeof(float), hipHostMallocDefault));
            SFA_HIP(ctx, hipEventCreateWithFlags(&j->ev_chw, hipEventDisableTiming));
        } else {
            SFA_HIP(ctx, hipEventSynchronize(j->ev_chw));      // the copies of an earlier call out of the staging planes (not the stream's other work)
        }
        for (int k = 0; k < 3; k++) memcpy(j->chw_stage + k * plane, chw[k], plane * sizeof(float));
        const float *const staged[3] = {j->chw_stage, j->chw_stage + plane, j->chw_stage + 2 * plane};
        for (int b = b0; b < b0 + n; b++) SFA_TRY(job_set_channel_weights(j, b, stride, staged));
        SFA_HIP(ctx, hipEventRecord(j->ev_chw, ctx->stream));
    } else {
        for (int b = b0; b < b0 + n; b++) SFA_TRY(job_set_channel_weights(j, b, stride, nullptr));
    }
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_job_set_flow_device(sfa_job *j, int b0, int n, const float *flow_dev, const long long strides[4]) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(job_windows(ctx, __func__, j, b0, n));
    if (flow_dev) {
        SFA_TRY(check_view(ctx, __func__, View{"flow_dev", flow_dev, sizeof(float), 4, {n, 2, j->h, j->w}, strides}));
    }
    Level L0 = j->level(0);
    launch_pack_flow(ctx, j->init_flow.f() + (long)b0 * 2 * L0.pl, 2 * L0.pl, L0.pl, L0.pitch, j->w, j->h, n, flow_dev, strides);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

// epic_to_initial_flow (kernel: epic_init.hip) from an epic job's fields into the initial flow of windows [b0, b0 + n)
int sfa_job_set_flow_epic(sfa_job *j, int b0, int n, const sfa_epic_job *e, int i0, float mul_u, float mul_v) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(job_windows(ctx, __func__, j, b0, n));
    if (!e) REFUSE("%s: epic_job is null", __func__);
    if (e->ctx != ctx) REFUSE("%s: epic_job lives on another context than the job: one stream orders its run before this call", __func__);
    SFA_TRY(check_batch_range(ctx, __func__, "images of epic_job", i0, n, e->n));
    const bool same = e->w == j->w && e->h == j->h;
    if (!same && (j->w % e->w != 0 || j->h % e->h != 0))
        REFUSE("%s: epic_job's fields are %d x %d, the job's frames %d x %d: neither the same size nor a divisor of it in both directions (the reference rescales by the "
               "integer ratio of the widths, slow_flow.cpp:827, and keeps a field of the reduced size where that is 1)", __func__, e->w, e->h, j->w, j->h);
    if (j->h > 65535) REFUSE("%s: h = %d (at most 65535: a row per block)", __func__, j->h);
    for (int k = 0; k < n; k++)
        if (e->rc[i0 + k] < 0) REFUSE("%s: image %d of epic_job holds no field (not run since its inputs changed, or flagged by the run)", __func__, i0 + k);
    Level L0 = j->level(0);
    launch_epic_initial_flow(ctx, j->init_flow.f() + (long)b0 * 2 * L0.pl, 2 * L0.pl, L0.pl, L0.pitch, j->w, j->h, n, e->u(i0), e->v(i0), (long)(2 * e->npix), e->w, e->h,
                             mul_u, mul_v);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_job_download_device(sfa_job *j, int b0, int n, float *flow_dev, const long long strides[4], float *occ_dev, const long long occ_strides[3]) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(job_windows(ctx, __func__, j, b0, n));
    SFA_TRY(check_download_destination(ctx, __func__, n, j->w, j->h, flow_dev, strides, occ_dev, occ_strides));
    Level L0 = j->level(0);
    launch_unpack_planes(ctx, L0.plane(P_WX) + (long)b0 * j->es, L0.plane(P_WY) + (long)b0 * j->es, L0.plane(P_OCC) + (long)b0 * j->es, j->es, L0.pitch, j->w, j->h, n,
                         flow_dev, strides, occ_dev, occ_strides);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int sfa_job_changes(const sfa_job *j, int b0, int n, float *out) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j && out, "job or out is null");
    SFA_TRY(job_windows(ctx, __func__, j, b0, n));
    for (int i = 0; i < 2 * n; i++) out[i] = j->change[2 * b0 + i];
    return SFA_OK;
}

// rawWeighting (kernel: mosaic.hip) into the weight planes of windows [b0, b0 + n)
int sfa_job_set_raw_weights(sfa_job *j, int b0, int n, int red_x, int red_y, float weight) {
    sfa_ctx *ctx = j ? j->ctx : nullptr;
    CHECK_ARGS(j, "job is null");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    SFA_TRY(job_windows(ctx, __func__, j, b0, n));
    SFA_TRY(check_mosaic_method(ctx, __func__, 0, red_x, red_y));
    if (!(weight == weight)) REFUSE("%s: weight is NaN", __func__);
    // the planes keep the level-0 host geometry of the job's uploads (the stride the last sfa_job_upload* gave; host_stride(w) before any), as chw planes
    // passed to that upload would: the data term indexes them by y * host_stride0 + x
    const int stride = j->host_stride0, cp = dev_pitch(stride);
    CHECK_ARGS((long)stride * j->h < (1L << 31), "channel weights: the linear pixel index must fit 31 bits");
    SFA_TRY(job_weight_planes(j, stride));
    if (j->chw_stride0 != stride)
        REFUSE("%s: the job holds channel weights of stride %d and its frames were uploaded with stride %d: one job keeps one stride", __func__, j->chw_stride0, stride);
    const long pl = (long)cp * j->h;
    launch_raw_weights(ctx, j->chw.f() + (long)b0 * 3 * pl, 3 * pl, pl, cp, stride, j->w, j->h, n, red_x, red_y, weight);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

// ---- host-plane convenience entry points ------------------------------------------------------------------------
int sfa_variational(sfa_ctx *ctx, const sfa_params *p, float *wx, float *wy, int w, int h, int stride, const float *const *frames, int n_frames,
                    const float *const chw[3], float *occlusions_out, float change[2]) {
    CHECK_ARGS(ctx && p && wx && wy && frames, "null argument");
    sfa_job *j = nullptr;
    SFA_TRY(sfa_job_create(ctx, p, w, h, 1, &j));
    std::unique_ptr<sfa_job, void (*)(sfa_job *)> guard(j, sfa_job_destroy);
    SFA_TRY(sfa_job_upload(j, 0, frames, n_frames, wx, wy, stride, chw));
    SFA_TRY(sfa_job_run(j));
    SFA_TRY(sfa_job_download(j, 0, wx, wy, stride, change));
    if (occlusions_out) SFA_TRY(sfa_job_download_occlusions(j, 0, occlusions_out, stride));
    return SFA_OK;
}

int sfa_compute_one_level(sfa_ctx *ctx, const sfa_params *p, float *wx, float *wy, int w, int h, int stride, const float *const *frames, int n_frames,
                          const float *const chw[3], float *occlusions_out, float change[2]) {
    CHECK_ARGS(ctx && p && wx && wy && frames, "null argument");
    sfa_params q = *p;
    q.layers = 1;
    q.presmooth_sigma = 0;
    return sfa_variational(ctx, &q, wx, wy, w, h, stride, frames, n_frames, chw, occlusions_out, change);
}

}  // extern "C"
