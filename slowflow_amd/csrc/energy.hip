// energy.hip -- dense_tracking's unary energy of every trajectory hypothesis (dense_tracking.cpp:1219-1257) on the GPU: for each fully tracked grid
// pixel of one rate, hypothesis::adaptFPS (utils/hypothesis.h:136-175), hypothesis::setOcclusions (utils/hypothesis.cpp:172-215), then
//     energy = addJC (:176-232) + addBCGC (:240-349) + addOC (:351-365) + weight_jet_estimation[r]      (four floats, added left to right in fp32)
// with the float-plane bilinearInterp (utils/utils.cpp:415-446) and bilinearInterp<double> (utils/utils.h:182-217).  fp64 statements in the reference's
// order, built with -ffp-contract=off: the same bits as a plain restatement (tests/energy_ref.py).  The Lorentzian's fp64 log is the device library's, not
// glibc's; after the rounding to fp32 the two agreed on every case of tests/test_hypothesis_energy.py on an MI355X, which compares them with ==.
//
// Where the reference's types differ from a first reading, the reference's hold:
//   - the penalties (penalty_functions/*.h) take `float e`, keep epsilon_sq = e * e (a float product) in a double, and evaluate sqrt / log in fp64 on
//     (double) xsq before the float return -- not an fp32 sqrt;
//   - addOC's and addBCGC's weights are double parameters: acc_occ, acc_bc and acc_gc are read as float (:606-609) and widened exactly;
//   - params.Jets in addJC / addBCGC / addOC is the segment's Jets (:564-568): every hypothesis has Jets steps after adaptFPS(Jets).
//
// Shape, three launches per call (n segments = blockIdx.y):
//   k_hyp_serial   one thread per grid pixel: adaptFPS, setOcclusions, addJC and addOC, serial over the Jets steps (6 flow gathers per step, float2 / double2 taps);
//                  writes the adapted flows, the occlusion bits and the two float terms.
//   k_hyp_bcgc     one thread per (hypothesis, neighbour) -- the (2r+1)^2 neighbours are independent until they are summed: the thread gathers its
//                  Jets + 1 frames x 9 values (I, dx, dy of c3, c2, c1) once into LDS, 9 (Jets + 1) doubles per lane laid out [value][frame][lane]
//                  so that a wave reads 64 consecutive doubles, then runs the pair chain i < j < visible in order: a strictly ordered fp64 sum of up
//                  to Jets (Jets + 1) / 2 pair terms, which stays one thread's.  One wave per workgroup: 64 x 9 x 33 x 8 = 152 KiB of LDS at Jets 32
//                  (one workgroup per CU), 78 KiB at Jets 16.  Re-gathering inside the pair loop instead would cost 4 taps x 9 values per pair
//                  rather than 9 LDS reads; the cap Jets <= 32 is this LDS bound.  Each frame is stored once as a 48-byte record per pixel (the
//                  9 values + 3 pad floats) so that a bilinear tap is three 16-byte loads.
//   k_hyp_sum      one thread per grid pixel: the neighbours' e_p in the reference's order (off_x outer, off_y inner), the division by neighs and the
//                  final fp32 sum.
// Measured on one MI355X at 1024 x 436, skip 1, one rate (111 616 hypotheses x 9 neighbours; profiles/hypothesis_energy_bench.txt): k_hyp_bcgc takes
// 0.12 / 0.44 / 1.34 / 6.55 ms at Jets 4 / 8 / 16 / 32, of 0.24 / 0.66 / 1.82 / 7.63 ms for all the call's kernels.  At Jets 32 the 152 KiB of LDS
// leave one wave per CU, and k_hyp_bcgc is 86 % of the kernel time: the figure a re-gathering shape would have to beat.
#include <atomic>

#include "sfa_device.h"

#pragma clang fp contract(off)

namespace sfa {

constexpr int kEnThreads = 256;          // the per-pixel kernels
constexpr int kBcThreads = 64;           // k_hyp_bcgc: one wave, LDS per lane
constexpr int kEnMaxJets = 32;           // the LDS bound above (and the 64-bit occlusion word needs Jets + 1 <= 64)

// AdaptTab (adaptFPS(Jets) of a hypothesis of F = r_Jets steps, its float index arithmetic done once on the host, hypothesis.h:140-171) and EnergyArgs:
// sfa_internal.h
static_assert(sizeof(AdaptTab::off) / sizeof(int) == kEnMaxJets, "AdaptTab holds kEnMaxJets steps");

// PenaltyFunction::apply(float xsq), float in, float out
__device__ __forceinline__ float phi_apply(int kind, double eps_sq, float xsq) {
    if (kind == 0) return xsq;                                                  // QuadraticFunction
    if (kind == 1) return (float)sqrt(xsq + eps_sq);                            // ModifiedL1Norm: sqrt(double), rounded on return
    return (float)log(1 + 0.5 * xsq / eps_sq);                                  // Lorentzian: 1 + ((0.5 * xsq) / eps_sq)
}

// frame k (3 planes c1, c2, c3 of pl floats), dx_k, dy_k -> one record of 12 floats per pixel: I c3, c2, c1, dx c3, c2, c1, dy c3, c2, c1, 0, 0, 0 (the
// reference reads the channels in the order c3, c2, c1, dense_tracking.cpp:266-274)
__global__ void __launch_bounds__(kEnThreads) k_energy_records(const float *__restrict__ fr, const float *__restrict__ dx, const float *__restrict__ dy,
                                                               float4 *__restrict__ rec, size_t pl, size_t n) {
    for (size_t i = (size_t)blockIdx.x * kEnThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kEnThreads) {
        const size_t k = i / pl, p = i % pl, b = k * 3 * pl + p;
        rec[3 * i + 0] = make_float4(fr[b + 2 * pl], fr[b + pl], fr[b], dx[b + 2 * pl]);
        rec[3 * i + 1] = make_float4(dx[b + pl], dx[b], dy[b + 2 * pl], dy[b + pl]);
        rec[3 * i + 2] = make_float4(dy[b], 0.f, 0.f, 0.f);
    }
}

// adaptFPS + setOcclusions + addJC + addOC of the hypothesis at grid pixel i of segment blockIdx.y.  acc_u, acc_v: [n][r_Jets][gpl] (all_steps layout);
// fwd, bwd: [n][J] planes of pairs or null (the empty Mats of a rate processed before acc_min_fps: fw = fh = 0).  U, V: [n][gpl][J] adapted flows.
// T2 = float2: the flows as read; T2 = double2: flows resampled from jets of another size (jet_resample.hip).
template <class T2>
__global__ void __launch_bounds__(kEnThreads) k_hyp_serial(const double *__restrict__ acc_u, const double *__restrict__ acc_v, const int *__restrict__ tracked,
                                                           const T2 *__restrict__ fwd, const T2 *__restrict__ bwd, int rJ, int J, int w, int h, int gw, int gpl,
                                                           int incr, int start, AdaptTab tab, EnergyArgs a, double *__restrict__ U, double *__restrict__ V,
                                                           unsigned long long *__restrict__ occ_out, float *__restrict__ jc_out, float *__restrict__ oc_out) {
    const int i = blockIdx.x * kEnThreads + threadIdx.x;
    if (i >= gpl) return;
    const int s = blockIdx.y;
    const size_t si = (size_t)s * gpl + i, pl = (size_t)w * h;
    if (tracked[si] != rJ) return;                                              // no hypothesis (:1225); k_hyp_sum writes +Inf
    const double px = (i % gw) * incr + start, py = (i / gw) * incr + start;   // p = (ox, oy) (:1230-1241)
    const double *AU = acc_u + (size_t)s * rJ * gpl + i, *AV = acc_v + (size_t)s * rJ * gpl + i;
    double *Us = U + si * J, *Vs = V + si * J;
    // ---- adaptFPS(Jets) (hypothesis.h:136-175)
    for (int t = 0; t < J; t++) {
        if (tab.up) {
            Us[t] = AU[(size_t)tab.off[t] * gpl];
            Vs[t] = AV[(size_t)tab.off[t] * gpl];
        } else {
            // quirk: last_x, last_y are float (:158-159): the double flow of the previous step is rounded to fp32
            float lx = 0, ly = 0;
            if (t > 0) { lx = (float)AU[(size_t)tab.offm1[t] * gpl]; ly = (float)AV[(size_t)tab.offm1[t] * gpl]; }
            Us[t] = lx + (double)tab.skip * (AU[(size_t)tab.off[t] * gpl] - lx);   // :166-167, skip a float widened
            Vs[t] = ly + (double)tab.skip * (AV[(size_t)tab.off[t] * gpl] - ly);
        }
    }
    // ---- setOcclusions (hypothesis.cpp:172-215); the bounds are forward_flow[t].rows / .cols, 0 for an empty Mat
    const int fw = fwd ? w : 0, fh = fwd ? h : 0;
    const T2 *F = fwd ? fwd + (size_t)s * J * pl : nullptr, *B = bwd ? bwd + (size_t)s * J * pl : nullptr;
    unsigned long long occ = 0;                                                 // bit 0: always visible in the reference frame (:176)
    for (int t = 0; t < J; t++) {
        if ((occ >> t) & 1ull) { occ |= 1ull << (t + 1); continue; }           // :180-183, occluded stays occluded
        double u_tm1 = 0, v_tm1 = 0;
        if (t > 0) { u_tm1 += Us[t - 1]; v_tm1 += Vs[t - 1]; }
        const double x_tm1 = px + u_tm1, y_tm1 = py + v_tm1;
        bool o = true;
        if (y_tm1 >= 0 && y_tm1 < fh && x_tm1 >= 0 && x_tm1 < fw) {
            double F_x, F_y;
            bilinear2(F + (size_t)t * pl, w, h, x_tm1, y_tm1, F_x, F_y);        // channel 1 = x = u, channel 0 = y = v
            const double ysq = (Vs[t] - v_tm1 - F_y), xsq = (Us[t] - u_tm1 - F_x);
            const double x_t = px + Us[t], y_t = py + Vs[t];
            if (y_t >= 0 && y_t < fh && x_t >= 0 && x_t < fw) {                 // quirk: forward_flow's size bounds the backward lookup too (:200)
                double bF_x, bF_y;
                bilinear2(B + (size_t)t * pl, w, h, x_t, y_t, bF_x, bF_y);
                const double fb_ysq = (bF_y + F_y), fb_xsq = (bF_x + F_x);
                o = !(sqrt(fb_ysq * fb_ysq + fb_xsq * fb_xsq) < a.fb_thr && sqrt(ysq * ysq + xsq * xsq) < a.thr);   // strict <, :207
            }
        }
        if (o) occ |= 1ull << (t + 1);
    }
    // ---- addJC (dense_tracking.cpp:176-232); obs = forward_flow, width / height of obs[0]
    double jenergy = 0, cvenergy = 0;
    int contribution = 0;
    for (int j = 0; j < J; j++) {
        const double u_j = Us[j], v_j = Vs[j];
        double u_jm1 = 0, v_jm1 = 0;
        if (j > 0) { u_jm1 = Us[j - 1]; v_jm1 = Vs[j - 1]; }
        if (u_j > 1e9 || v_j > 1e9) break;                                      // UNKNOWN_FLOW_THRESH (hypothesis.h:24)
        const double xi = px + u_jm1, yi = py + v_jm1;
        if (yi >= 0 && yi < fh && xi >= 0 && xi < fw) {                        // insideImg (:168-170)
            // quirk: this `continue` sits inside the in-image branch, so it also skips the constant-velocity term below (:197-198)
            if (((occ >> j) & 1ull) || ((occ >> (j + 1)) & 1ull)) continue;
            double I_x, I_y;
            bilinear2(F + (size_t)j * pl, w, h, xi, yi, I_x, I_y);
            const double du = u_j - u_jm1 - I_x, dv = v_j - v_jm1 - I_y;
            jenergy += 0.5 * phi_apply(a.penalty, a.eps_sq, (float)(du * du + dv * dv));   // apply takes and returns float
            contribution++;
        }
        double u_jp1 = 0, v_jp1 = 0;
        if (j + 1 < J) { u_jp1 = Us[j + 1]; v_jp1 = Vs[j + 1]; }
        double u_sq = 2 * u_j - u_jm1 - u_jp1, v_sq = 2 * v_j - v_jm1 - v_jp1;
        u_sq *= u_sq;
        v_sq *= v_sq;
        cvenergy += sqrt(u_sq + v_sq);
    }
    if (contribution > 0) jenergy /= contribution;
    jc_out[si] = (float)(a.acc_jc * jenergy + a.acc_cv * cvenergy);
    // ---- addOC (:351-365) over the frames 0 .. Jets
    int occlusions = 0, change = 0;
    for (int t = 0; t <= J; t++) {
        occlusions += (int)((occ >> t) & 1ull);
        if (t < J && ((occ >> t) & 1ull) != ((occ >> (t + 1)) & 1ull)) change++;
    }
    oc_out[si] = (float)(a.acc_occ * occlusions + a.acc_temporal_occ * change);
    occ_out[si] = occ;
}

// the float-plane bilinearInterp (utils.cpp:415-446) of the 9 values of one record plane at an in-image point, stored to LDS column j of this lane
__device__ __forceinline__ void bilinear9(const float4 *__restrict__ rec, int w, int h, double x, double y, double *__restrict__ out, int col_stride) {
    const int y0 = (int)y, x0 = (int)x;
    int y1 = y0, x1 = x0;
    double wx = 0, wy = 0;                                                      // the weight is 0 on the last column and row (:427-438)
    if (x0 + 1 < w) { wx = x - x0; x1++; }
    if (y0 + 1 < h) { wy = y - y0; y1++; }
    const float4 *r00 = rec + 3 * ((size_t)y0 * w + x0), *r10 = rec + 3 * ((size_t)y0 * w + x1);
    const float4 *r01 = rec + 3 * ((size_t)y1 * w + x0), *r11 = rec + 3 * ((size_t)y1 * w + x1);
    float a[12], b[12], c[12], d[12];
    for (int k = 0; k < 3; k++) {
        const float4 A = r00[k], Bq = r10[k], Cq = r01[k], D = r11[k];
        a[4 * k] = A.x; a[4 * k + 1] = A.y; a[4 * k + 2] = A.z; a[4 * k + 3] = A.w;
        b[4 * k] = Bq.x; b[4 * k + 1] = Bq.y; b[4 * k + 2] = Bq.z; b[4 * k + 3] = Bq.w;
        c[4 * k] = Cq.x; c[4 * k + 1] = Cq.y; c[4 * k + 2] = Cq.z; c[4 * k + 3] = Cq.w;
        d[4 * k] = D.x; d[4 * k + 1] = D.y; d[4 * k + 2] = D.z; d[4 * k + 3] = D.w;
    }
#pragma unroll
    for (int k = 0; k < 9; k++)                                                 // :441-444, left to right
        out[k * col_stride] = (1 - wy) * (1 - wx) * (double)a[k] + (1 - wy) * wx * (double)b[k] + wy * (1 - wx) * (double)c[k] + wy * wx * (double)d[k];
}

// addBCGC's e_p of neighbour k of the hypothesis at grid pixel i (dense_tracking.cpp:255-338).  rec: [n][J + 1][pl] records; ep: [n][gpl][NN].
__global__ void __launch_bounds__(kBcThreads) k_hyp_bcgc(const float4 *__restrict__ rec, const int *__restrict__ tracked, const double *__restrict__ U,
                                                         const double *__restrict__ V, const unsigned long long *__restrict__ occ_bits, int rJ, int J, int w, int h,
                                                         int gw, int gpl, int incr, int start, int r, double bcw, double gcw, double *__restrict__ ep) {
    extern __shared__ double lds[];                                             // [9][J + 1][kBcThreads]
    const int side = 2 * r + 1, NN = side * side;
    const long q = (long)blockIdx.x * kBcThreads + threadIdx.x;
    if (q >= (long)gpl * NN) return;                                            // no barrier below: every lane owns its LDS column
    const int i = (int)(q / NN), k = (int)(q % NN), s = blockIdx.y;
    const size_t si = (size_t)s * gpl + i, pl = (size_t)w * h;
    if (tracked[si] != rJ) return;
    const int px = (i % gw) * incr + start, py = (i / gw) * incr + start;
    const int off_x = px - r + k / side, off_y = py - r + k % side;             // off_x outer, off_y inner (:255-256)
    if (off_x < 0 || off_x >= w || off_y < 0 || off_y >= h) return;             // :257-258; k_hyp_sum skips it the same way
    const double *Us = U + si * J, *Vs = V + si * J;
    // which frames are inside the image (frame 0 always, :265-278); `visible` counts them
    unsigned long long inside = 1;
    for (int j = 1; j <= J; j++) {
        const double xj = off_x + Us[j - 1], yj = off_y + Vs[j - 1];
        if (yj >= 0 && yj < h && xj >= 0 && xj < w) inside |= 1ull << j;
    }
    const int visible = __popcll(inside);
    // quirk: the values stay at index j, but the pair loop runs over i < j < visible (:302-303): a frame outside the image in the middle of the trajectory
    // leaves a hole and the last frames are never compared.  A pair takes part where both frames are inside and neither is occluded (:312-316).
    const unsigned long long ok = inside & ~occ_bits[si] & ((1ull << visible) - 1);   // visible <= 33
    const float4 *R = rec + (size_t)s * (J + 1) * pl * 3;
    double *L = lds + threadIdx.x;
    const int cs = (J + 1) * kBcThreads;                                        // LDS stride between the 9 values
    for (int j = 0; j < visible; j++) {
        if (!((ok >> j) & 1ull)) continue;
        double *o = L + j * kBcThreads;
        if (j == 0) {                                                           // frame 0 at the integer pixel (:264-275)
            const float4 *p = R + 3 * ((size_t)off_y * w + off_x);
            const float4 A = p[0], Bq = p[1], Cq = p[2];
            o[0] = A.x; o[cs] = A.y; o[2 * cs] = A.z; o[3 * cs] = A.w; o[4 * cs] = Bq.x; o[5 * cs] = Bq.y; o[6 * cs] = Bq.z; o[7 * cs] = Bq.w; o[8 * cs] = Cq.x;
        } else {
            bilinear9(R + (size_t)j * pl * 3, w, h, off_x + Us[j - 1], off_y + Vs[j - 1], o, cs);
        }
    }
    double e_p = 0;
    int contribution = 0;
    for (int a = 0; a < visible; a++) {
        if (!((ok >> a) & 1ull)) continue;
        double vi[9];
#pragma unroll
        for (int c = 0; c < 9; c++) vi[c] = L[c * cs + a * kBcThreads];
        for (int b = a + 1; b < visible; b++) {
            if (!((ok >> b) & 1ull)) continue;
            double vj[9];
#pragma unroll
            for (int c = 0; c < 9; c++) vj[c] = L[c * cs + b * kBcThreads];
            // :318-319, bc term then gc term, each (acc * 0.3334) * (sum of |differences| left to right)
            e_p += bcw * (fabs(vi[0] - vj[0]) + fabs(vi[1] - vj[1]) + fabs(vi[2] - vj[2]));
            e_p += gcw * (fabs(vi[3] - vj[3]) + fabs(vi[4] - vj[4]) + fabs(vi[5] - vj[5]) + fabs(vi[6] - vj[6]) + fabs(vi[7] - vj[7]) + fabs(vi[8] - vj[8]));
            contribution++;
        }
    }
    if (contribution > 0) e_p /= contribution;                                  // :330
    ep[si * NN + k] = e_p;
}

// the adapted flows of k_hyp_serial ([n][gpl][J]) in the layout [J][gpl] the fusion reads, segment s at s * seg; 0 where there is no hypothesis
__global__ void __launch_bounds__(kEnThreads) k_hyp_adapted(const int *__restrict__ tracked, const double *__restrict__ U, const double *__restrict__ V, int rJ,
                                                            int J, int gpl, double *__restrict__ out_u, double *__restrict__ out_v, size_t seg) {
    const int i = blockIdx.x * kEnThreads + threadIdx.x;
    if (i >= gpl) return;
    const size_t si = (size_t)blockIdx.y * gpl + i;
    const bool have = tracked[si] == rJ;
    for (int t = 0; t < J; t++) {
        const size_t o = (size_t)blockIdx.y * seg + (size_t)t * gpl + i;
        out_u[o] = have ? U[si * J + t] : 0.0;
        out_v[o] = have ? V[si * J + t] : 0.0;
    }
}

// wenergy over the neighbours in order, / neighs (:332-346), and the energy: ((JC + BCGC) + OC) + weight in fp32 (:1250-1253)
__global__ void __launch_bounds__(kEnThreads) k_hyp_sum(const int *__restrict__ tracked, const unsigned long long *__restrict__ occ_bits,
                                                        const float *__restrict__ jc, const float *__restrict__ oc, const double *__restrict__ ep, int rJ, int w, int h,
                                                        int gw, int gpl, int incr, int start, int r, float weight, double *__restrict__ energy,
                                                        unsigned long long *__restrict__ occ_out, size_t out_seg) {
    const int i = blockIdx.x * kEnThreads + threadIdx.x;
    if (i >= gpl) return;
    const size_t si = (size_t)blockIdx.y * gpl + i, so = (size_t)blockIdx.y * out_seg + i;   // segment s's outputs start at s * out_seg
    if (tracked[si] != rJ) {                                                    // null hypothesis: sorted last by compareHypotheses (:172)
        energy[so] = __longlong_as_double(0x7ff0000000000000ll);
        occ_out[so] = 0;
        return;
    }
    const int side = 2 * r + 1, NN = side * side;
    const int px = (i % gw) * incr + start, py = (i / gw) * incr + start;
    double wenergy = 0, neighs = 0;
    for (int k = 0; k < NN; k++) {
        const int off_x = px - r + k / side, off_y = py - r + k % side;
        if (off_x < 0 || off_x >= w || off_y < 0 || off_y >= h) continue;
        wenergy += ep[si * NN + k];
        neighs++;
    }
    if (neighs > 0) wenergy /= neighs;
    float e = jc[si] + (float)wenergy;
    e = e + oc[si];
    e = e + weight;
    energy[so] = (double)e;
    occ_out[so] = occ_bits[si];
}

int energy_plan(sfa_ctx *ctx, const sfa_energy_params *p, int r_Jets, int Jets, int w, int h, EnergyPlan *out) {
    EnergyPlan &e = *out;
    e = EnergyPlan{};
    e.rJ = r_Jets; e.J = Jets; e.w = w; e.h = h;
    if (sfa_accumulate_grid(w, h, p->skip, &e.gw, &e.gh) != SFA_OK) return set_error(ctx, SFA_ERR_ARG, "%s", sfa_last_error(nullptr));
    // adaptFPS's indices in its own float arithmetic (hypothesis.h:139-171), each checked against the F = r_Jets flows it reads
    AdaptTab &tab = e.tab;
    tab.skip = (1.0f * r_Jets) / Jets;
    tab.up = tab.skip >= 1;
    for (int i = 0; i < Jets; i++) {
        if (tab.up) tab.off[i] = (int)(i * tab.skip + (tab.skip - 1));
        else { tab.off[i] = (int)floorf(i * tab.skip); tab.offm1[i] = (int)floorf((i - 1) * tab.skip); }
        if (tab.off[i] < 0 || tab.off[i] >= r_Jets || (!tab.up && i > 0 && (tab.offm1[i] < 0 || tab.offm1[i] >= r_Jets)))
            return set_error(ctx, SFA_ERR_ARG, "sfa_hypothesis_energies: adaptFPS(%d) of %d steps reads step %d", Jets, r_Jets, tab.off[i]);
    }
    e.r = (int)(0.5f * (p->skip + 1));                                          // :245
    const int side = 2 * e.r + 1;
    e.NN = side * side;
    e.lds = (size_t)kBcThreads * 9 * (Jets + 1) * sizeof(double);
    e.incr = p->skip + 1; e.start = (int)(0.5f * p->skip);
    EnergyArgs &a = e.a;
    a.acc_jc = p->acc_jc; a.acc_cv = p->acc_cv; a.acc_bc = p->acc_bc; a.acc_gc = p->acc_gc; a.acc_occ = p->acc_occ; a.acc_temporal_occ = p->acc_temporal_occ;
    a.thr = p->occlusion_threshold; a.fb_thr = p->occlusion_fb_threshold; a.penalty = p->penalty;
    const float eps = (float)p->penalty_eps;                                    // ModifiedL1Norm(float e) / Lorentzian(float e): epsilon_sq(e * e)
    a.eps_sq = (double)(eps * eps);
    a.weight = p->weight;
    return SFA_OK;
}

// dx, dy by the 5-tap derivative launcher (color_image_convolve_hv with {0, -8/12, 1/12}, :920-925), then the records
void energy_records_device(sfa_ctx *ctx, size_t nf, int w, int h, const float *frames, float *der, void *rec) {
    const size_t pl = (size_t)w * h;
    Geo g{};
    g.w = w; g.h = h; g.pitch = w; g.pl = (long)pl; g.es = (long)pl; g.nb = (int)(nf * 3);
    float *ddx = der, *ddy = der + nf * 3 * pl;
    launch_convolve(ctx, g, ddx, frames, 2, 1, 1);
    launch_convolve(ctx, g, ddy, frames, 2, 0, 1);
    hipLaunchKernelGGL(k_energy_records, dim3((unsigned)std::min<size_t>((nf * pl + kEnThreads - 1) / kEnThreads, (size_t)ctx->cu_count * 8)), dim3(kEnThreads), 0,
                       ctx->stream, frames, ddx, ddy, static_cast<float4 *>(rec), pl, nf * pl);
}

int energies_device(sfa_ctx *ctx, const EnergyPlan &e, int n, const double *acc_u, const double *acc_v, const int *tracked, const void *rec, bool identity,
                    const void *fwd, const void *bwd, const EnergyWork &wk, double *energy, unsigned long long *occ_out, size_t out_seg, double *adapted_u,
                    double *adapted_v, size_t adapted_seg) {
    // more than 64 KiB of dynamic LDS is allowed per function and device, once (the pattern of sor_chain.hip)
    static std::atomic<unsigned long long> attr_set{0};
    const unsigned long long bit = (ctx->device >= 0 && ctx->device < 64) ? 1ull << ctx->device : 0ull;
    if (e.lds > 64 * 1024 && !(attr_set.load(std::memory_order_relaxed) & bit)) {
        const hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hyp_bcgc), hipFuncAttributeMaxDynamicSharedMemorySize, (int)e.lds);
        if (err != hipSuccess) return set_error(ctx, SFA_ERR_HIP, "k_hyp_bcgc: %zu bytes of LDS refused on device %d: %s", e.lds, ctx->device, hipGetErrorString(err));
        attr_set.fetch_or(bit, std::memory_order_relaxed);
    }
    const size_t gpl = (size_t)e.gw * e.gh;
    const dim3 pix((unsigned)((gpl + kEnThreads - 1) / kEnThreads), (unsigned)n);
    if (identity)
        hipLaunchKernelGGL(k_hyp_serial<float2>, pix, dim3(kEnThreads), 0, ctx->stream, acc_u, acc_v, tracked, static_cast<const float2 *>(fwd),
                           static_cast<const float2 *>(bwd), e.rJ, e.J, e.w, e.h, e.gw, (int)gpl, e.incr, e.start, e.tab, e.a, wk.U, wk.V, wk.occ, wk.jc, wk.oc);
    else
        hipLaunchKernelGGL(k_hyp_serial<double2>, pix, dim3(kEnThreads), 0, ctx->stream, acc_u, acc_v, tracked, static_cast<const double2 *>(fwd),
                           static_cast<const double2 *>(bwd), e.rJ, e.J, e.w, e.h, e.gw, (int)gpl, e.incr, e.start, e.tab, e.a, wk.U, wk.V, wk.occ, wk.jc, wk.oc);
    SFA_HIP(ctx, hipGetLastError());
    const double bcw = e.a.acc_bc * 0.3334, gcw = e.a.acc_gc * 0.3334;          // acc_bc * 0.3334 * (...) groups left to right (:318-319)
    hipLaunchKernelGGL(k_hyp_bcgc, dim3((unsigned)((gpl * e.NN + kBcThreads - 1) / kBcThreads), (unsigned)n), dim3(kBcThreads), e.lds, ctx->stream,
                       static_cast<const float4 *>(rec), tracked, wk.U, wk.V, wk.occ, e.rJ, e.J, e.w, e.h, e.gw, (int)gpl, e.incr, e.start, e.r, bcw, gcw, wk.ep);
    SFA_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_hyp_sum, pix, dim3(kEnThreads), 0, ctx->stream, tracked, wk.occ, wk.jc, wk.oc, wk.ep, e.rJ, e.w, e.h, e.gw, (int)gpl, e.incr, e.start, e.r,
                       e.a.weight, energy, occ_out, out_seg);
    SFA_HIP(ctx, hipGetLastError());
    if (adapted_u) SFA_TRY(energies_adapted_device(ctx, e, n, tracked, wk, adapted_u, adapted_v, adapted_seg));
    return SFA_OK;
}

// k_hyp_serial's adaptFPS(Jets) out of the scratch of the energies_device call before it, transposed for the fusion
int energies_adapted_device(sfa_ctx *ctx, const EnergyPlan &e, int n, const int *tracked, const EnergyWork &wk, double *adapted_u, double *adapted_v, size_t adapted_seg) {
    const size_t gpl = (size_t)e.gw * e.gh;
    const dim3 pix((unsigned)((gpl + kEnThreads - 1) / kEnThreads), (unsigned)n);
    hipLaunchKernelGGL(k_hyp_adapted, pix, dim3(kEnThreads), 0, ctx->stream, tracked, wk.U, wk.V, e.rJ, e.J, (int)gpl, adapted_u, adapted_v, adapted_seg);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int EnergyMem::alloc(sfa_ctx *ctx, const EnergyPlan &e, int n, int work_n, const sfa_jet_source *flow_src, bool is_identity) {
    const size_t nf = (size_t)n * (e.J + 1), pl = (size_t)e.w * e.h, wg = (size_t)work_n * e.gw * e.gh;
    SFA_TRY(frames.alloc(ctx, nf * 3 * pl * 4)); SFA_TRY(der.alloc(ctx, nf * 6 * pl * 4)); SFA_TRY(rec.alloc(ctx, nf * pl * 48));
    SFA_TRY(U.alloc(ctx, wg * e.J * 8)); SFA_TRY(V.alloc(ctx, wg * e.J * 8)); SFA_TRY(occ.alloc(ctx, wg * 8));
    SFA_TRY(jc.alloc(ctx, wg * 4)); SFA_TRY(oc.alloc(ctx, wg * 4)); SFA_TRY(ep.alloc(ctx, wg * e.NN * 8));
    segments = n;
    if (flow_src) { flows = true; src = *flow_src; identity = is_identity; }
    return SFA_OK;
}

int EnergyMem::upload(sfa_ctx *ctx, const EnergyPlan &e, const float *const *host_frames, int stride, const float *const *fwd_u, const float *const *fwd_v,
                      const float *const *bwd_u, const float *const *bwd_v) {
    const size_t nf = (size_t)segments * (e.J + 1), nj = (size_t)segments * e.J, pl = (size_t)e.w * e.h;
    SFA_TRY(upload_frames(ctx, nf, host_frames, stride, e.w, e.h, frames.f()));
    energy_records_device(ctx, nf, e.w, e.h, frames.f(), der.f(), rec.p);
    SFA_HIP(ctx, hipGetLastError());
    if (!flows) return SFA_OK;
    const size_t tap = identity ? 8 : 16, spl = identity ? pl : (size_t)src.cw * src.ch;   // float2 or double2
    SFA_TRY(fwd.alloc(ctx, nj * pl * tap)); SFA_TRY(bwd.alloc(ctx, nj * pl * tap));   // while the records' kernels run: hipMalloc stays off the critical path
    SFA_TRY(stage.alloc(ctx, nj * spl * 8));
    // not the identity: r_forward_flow, resized and multiplied by rescale (:1142-1151)
    SFA_TRY(upload_flow_pairs(ctx, src, identity, nj, fwd_u, fwd_v, e.w, e.h, stage.f(), fwd.p, nullptr, nullptr));
    return upload_flow_pairs(ctx, src, identity, nj, bwd_u, bwd_v, e.w, e.h, stage.f(), bwd.p, nullptr, nullptr);
}

int energy_planes_check(sfa_ctx *ctx, const char *fn, bool with_index, size_t nf, const float *const *frames, size_t nj, const float *const *fwd_u,
                        const float *const *fwd_v, const float *const *bwd_u, const float *const *bwd_v, bool *flows) {
    *flows = fwd_u != nullptr;
    CHECK_ARGS_FN(fn, *flows == (fwd_v != nullptr) && *flows == (bwd_u != nullptr) && *flows == (bwd_v != nullptr), "the four flow arrays are all given or all null");
    for (size_t k = 0; k < nf; k++)
        if (!frames[k]) { if (with_index) REFUSE("%s: null frame %zu", fn, k); REFUSE("%s: null frame", fn); }
    for (size_t k = 0; *flows && k < nj; k++)
        if (!fwd_u[k] || !fwd_v[k] || !bwd_u[k] || !bwd_v[k]) { if (with_index) REFUSE("%s: null flow plane %zu", fn, k); REFUSE("%s: null flow plane", fn); }
    return SFA_OK;
}

}  // namespace sfa

using namespace sfa;

void sfa_energy_params_default(sfa_energy_params *p) {
    if (!p) return;
    *p = sfa_energy_params{};
    p->acc_jc = 1.0f;                    // setDefault (dense_tracking.cpp:118-165)
    p->acc_bc = 0.1f;
    p->acc_gc = 1.0f;
    p->acc_occ = 500.0f;
    p->acc_cv = 0.0;
    p->acc_temporal_occ = 10.0;
    p->occlusion_threshold = 5.0f;
    p->occlusion_fb_threshold = 5.0f;
    p->penalty = 1;
    p->penalty_eps = 0.001;
    p->weight = 0.0f;
    p->skip = 1;
}

int sfa_hypothesis_energies(sfa_ctx *ctx, const sfa_energy_params *p, int n, int r_Jets, int Jets, int w, int h, int stride, const double *acc_u,
                            const double *acc_v, const int *tracked, const float *const *frames, const float *const *fwd_u, const float *const *fwd_v,
                            const float *const *bwd_u, const float *const *bwd_v, double *energy, unsigned long long *occ_bits) {
    return sfa_hypothesis_energies_ex(ctx, p, n, r_Jets, Jets, w, h, stride, acc_u, acc_v, tracked, frames, fwd_u, fwd_v, bwd_u, bwd_v, energy, occ_bits,
                                      nullptr, nullptr);
}

int sfa_hypothesis_energies_ex(sfa_ctx *ctx, const sfa_energy_params *p, int n, int r_Jets, int Jets, int w, int h, int stride, const double *acc_u,
                               const double *acc_v, const int *tracked, const float *const *frames, const float *const *fwd_u, const float *const *fwd_v,
                               const float *const *bwd_u, const float *const *bwd_v, double *energy, unsigned long long *occ_bits, double *adapted_u,
                               double *adapted_v) {
    sfa_jet_source src;
    sfa_jet_source_default(&src, w, h, stride);
    return sfa_hypothesis_energies_scaled(ctx, p, n, r_Jets, Jets, w, h, stride, acc_u, acc_v, tracked, frames, &src, fwd_u, fwd_v, bwd_u, bwd_v, energy, occ_bits,
                                          adapted_u, adapted_v);
}

int sfa_hypothesis_energies_scaled(sfa_ctx *ctx, const sfa_energy_params *p, int n, int r_Jets, int Jets, int w, int h, int stride, const double *acc_u,
                                   const double *acc_v, const int *tracked, const float *const *frames, const sfa_jet_source *flow_src,
                                   const float *const *fwd_u, const float *const *fwd_v, const float *const *bwd_u, const float *const *bwd_v,
                                   double *energy, unsigned long long *occ_bits, double *adapted_u, double *adapted_v) {
    if (!(ctx && p && acc_u && acc_v && tracked && frames && energy && occ_bits)) return set_error(ctx, SFA_ERR_ARG, "sfa_hypothesis_energies: null argument");
    if ((adapted_u != nullptr) != (adapted_v != nullptr)) return set_error(ctx, SFA_ERR_ARG, "sfa_hypothesis_energies_ex: adapted_u and adapted_v are both given or both null");
    if (!(n >= 1 && r_Jets >= 1 && Jets >= 1 && Jets <= kEnMaxJets && (long)n * (Jets + 1) * 3 <= 65535 && w >= 1 && stride >= w))
        return set_error(ctx, SFA_ERR_ARG, "sfa_hypothesis_energies: bad sizes (n >= 1 with n (Jets + 1) <= 21845, r_Jets >= 1, 1 <= Jets <= %d, w >= 1, stride >= w)",
                         kEnMaxJets);
    if (h < 4)   // convolve_vert_fast_5 (image.c:425-458) runs its middle-row loop from height - 3 down through zero: undefined below 4 rows
        return set_error(ctx, SFA_ERR_ARG, "sfa_hypothesis_energies: h = %d; the reference's vertical 5-tap derivative needs h >= 4", h);
    const size_t nf = (size_t)n * (Jets + 1), nj = (size_t)n * Jets;
    bool flows, identity = true;                                                // without a source the flows are w x h float planes of the frames' stride
    SFA_TRY(energy_planes_check(ctx, "sfa_hypothesis_energies", true, nf, frames, nj, fwd_u, fwd_v, bwd_u, bwd_v, &flows));
    if (flows) SFA_TRY(jet_source_check(ctx, "sfa_hypothesis_energies: flow_src", flow_src, w, h, &identity));
    EnergyPlan plan;
    SFA_TRY(energy_plan(ctx, p, r_Jets, Jets, w, h, &plan));
    const size_t gpl = (size_t)plan.gw * plan.gh;

    SFA_HIP(ctx, hipSetDevice(ctx->device));
    EnergyMem in;
    DevMem dau, dav, dtr, den, docc_out, dad;
    SFA_TRY(in.alloc(ctx, plan, n, n, flows ? flow_src : nullptr, identity));
    SFA_TRY(dau.alloc(ctx, (size_t)n * r_Jets * gpl * 8)); SFA_TRY(dav.alloc(ctx, (size_t)n * r_Jets * gpl * 8)); SFA_TRY(dtr.alloc(ctx, (size_t)n * gpl * 4));
    SFA_TRY(den.alloc(ctx, (size_t)n * gpl * 8)); SFA_TRY(docc_out.alloc(ctx, (size_t)n * gpl * 8));
    SFA_TRY(in.upload(ctx, plan, frames, stride, fwd_u, fwd_v, bwd_u, bwd_v));
    SFA_TRY(copy_on(ctx, dau.p, acc_u, (size_t)n * r_Jets * gpl * 8, hipMemcpyHostToDevice));
    SFA_TRY(copy_on(ctx, dav.p, acc_v, (size_t)n * r_Jets * gpl * 8, hipMemcpyHostToDevice));
    SFA_TRY(copy_on(ctx, dtr.p, tracked, (size_t)n * gpl * 4, hipMemcpyHostToDevice));
    const EnergyWork wk = in.work();
    SFA_TRY(energies_device(ctx, plan, n, static_cast<const double *>(dau.p), static_cast<const double *>(dav.p), static_cast<const int *>(dtr.p), in.rec.p, identity,
                            in.fwd.p, in.bwd.p, wk, static_cast<double *>(den.p), static_cast<unsigned long long *>(docc_out.p), gpl, nullptr, nullptr, 0));
    SFA_HIP(ctx, hipMemcpyAsync(energy, den.p, (size_t)n * gpl * 8, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(occ_bits, docc_out.p, (size_t)n * gpl * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (adapted_u) {                                                            // allocated while the kernels above run: hipMalloc stays off the critical path
        SFA_TRY(dad.alloc(ctx, 2 * nj * gpl * 8));
        double *du = static_cast<double *>(dad.p), *dv = du + nj * gpl;
        SFA_TRY(energies_adapted_device(ctx, plan, n, static_cast<const int *>(dtr.p), wk, du, dv, (size_t)Jets * gpl));
        SFA_HIP(ctx, hipMemcpyAsync(adapted_u, du, nj * gpl * 8, hipMemcpyDeviceToHost, ctx->stream));
        SFA_HIP(ctx, hipMemcpyAsync(adapted_v, dv, nj * gpl * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}
