// fuse.hip -- dense_tracking's fusion of the trajectory hypotheses into one flow per start_jet (dense_tracking.cpp:1588-1905) on the GPU: the
// non-maximum suppression of :1592-1630, the pairwise potentials of :1716-1797 and TRW-S (Kolmogorov, PAMI 2006) in sequential raster order.
//
// The MRF library the reference links (TRWS_PATH) is not in the tree.  The solver is written from the paper, with one order fixed here and in
// INTEGRATION.md 4c, so the labels are not those of the reference's SetAutomaticOrdering; tests/fuse_ref.py restates every step in float64 numpy.
// fp64 without contraction throughout (-ffp-contract=off and the pragma below): the same bits as the restatement.
//
// Shape, four launches per call (n segments):
//   k_fuse_labels    one thread per grid pixel: the present slots sorted by their float score, ties to the lower slot (insertion sort over K <= 16), then
//                    the NMS with its `break`; writes the label list and the unary terms theta.
//   k_fuse_pairwise  one thread per (edge, label pair) -- the hot, fully parallel part: a trajectory distance over Jets steps and the occlusion
//                    disagreement per thread; P[s][dir][node][i * K + j], i the label of the earlier node.
//   k_trws           one workgroup per segment.  In raster order node (x, y) reads only what (x - 1, y) and (x, y - 1) wrote in the same pass, so the
//                    anti-diagonals x + y = d, one after another with a barrier between them, give exactly the sequential result; the messages live in
//                    global memory (L2), visible to the workgroup's own threads after __syncthreads().  No wait on another workgroup, no spin.
//   k_fuse_output    one thread per grid pixel: slot, flow, occlusion.
// Measured on one MI355X at a 512 x 218 grid, default keys (profiles/fuse_bench.txt): TRW-S is the cost.  One segment takes 26 / 33 / 60 ms per
// iteration at K 2 / 4 / 8 (one workgroup, 1 458 barrier steps per iteration); 16 segments side by side take 30 / 39 / 71 ms per iteration.  The pairwise
// kernel takes 0.05 / 0.18 / 0.68 ms at n = 1, Jets 16 (under 1 % of the call), so the per-edge shape with the labels in registers was not built.  A
// cross-workgroup pipeline of the diagonals, like sor_chain.hip's, is the step this measurement points to.
#include "hyp_device.h"

#pragma clang fp contract(off)

namespace sfa {

constexpr int kFuMaxK = 16;
constexpr int kFuMaxJets = 32;            // the energies' bound; the occlusion word holds Jets + 1 bits
constexpr int kFuThreads = 256;
constexpr int kTrwsThreads = 256;
constexpr int kTrwsChunk = 512;           // nodes whose energy / bound terms are staged in LDS per step of the ordered sum

struct FuseDims {
    int n, K, J, gw, gh, gpl, w, h, incr, start;
};

// labels: lab[(s, p)][i] = slot of label i, nl = label count, theta[(s, p)][i] = its energy (the unary term e_mex[h], :1680-1683)
__global__ void __launch_bounds__(kFuThreads) k_fuse_labels(const double *__restrict__ U, const double *__restrict__ V, const double *__restrict__ energy,
                                                            FuseDims d, int method, double thres, int pin, unsigned char *__restrict__ nl,
                                                            unsigned char *__restrict__ lab, double *__restrict__ theta) {
    const int p = blockIdx.x * kFuThreads + threadIdx.x;
    if (p >= d.gpl) return;
    const int s = blockIdx.y;
    const size_t sp = (size_t)s * d.gpl + p;
    // compareHypotheses compares score(), a float; a stable insertion sort keeps ties in slot order
    int order[kFuMaxK];
    float key[kFuMaxK];
    int m = 0;
    // pin: slot 0, where present, is the first label and the sort covers the others (:1601-1602); without it first = 0 and the code is what it was
    const int first = pin && present(energy[(size_t)s * d.K * d.gpl + p]) ? 1 : 0;
    if (first) { key[0] = 0; order[0] = 0; m = 1; }
    for (int k = first; k < d.K; k++) {
        const double e = energy[((size_t)s * d.K + k) * d.gpl + p];
        if (!present(e)) continue;
        const float f = (float)e;
        int j = m;
        while (j > first && f < key[j - 1]) { key[j] = key[j - 1]; order[j] = order[j - 1]; j--; }
        key[j] = f;
        order[j] = k;
        m++;
    }
    int kept[kFuMaxK];
    int nk = 0;
    if (m > 0) kept[nk++] = order[0];
    const size_t hs = (size_t)d.J * d.gpl;                                      // one slot's flows
    for (int c = 1; c < m; c++) {                                               // :1609-1626
        const size_t bc = ((size_t)s * d.K + order[c]) * hs + p;
        bool discard = false;
        for (int q = 0; q < nk; q++) {
            const size_t bq = ((size_t)s * d.K + kept[q]) * hs + p;
            if (traj_distance(U + bc, V + bc, U + bq, V + bq, d.gpl, d.J, method) < thres) discard = true;
        }
        if (discard) break;                                                     // quirk: the first discarded hypothesis ends the loop (:1624)
        kept[nk++] = order[c];
    }
    nl[sp] = (unsigned char)nk;
    for (int i = 0; i < nk; i++) {
        lab[sp * kFuMaxK + i] = (unsigned char)kept[i];
        theta[sp * kFuMaxK + i] = energy[((size_t)s * d.K + kept[i]) * d.gpl + p];
    }
}

// P(h1, h2) = (w[o1] + w[o2]) * (acc_beta * dist + acc_spatial_occ * smooth_occ) (:1752-1766): the weight sum in fp32, dist rounded to float, the bracket
// and the product in fp64.  Thread q of segment-direction blockIdx.y = 2 s + dir: node p = q / K^2, i = q / K % K, j = q % K.
__global__ void __launch_bounds__(kFuThreads) k_fuse_pairwise(const double *__restrict__ U, const double *__restrict__ V,
                                                              const unsigned long long *__restrict__ occ_bits, const float *__restrict__ weight, FuseDims d,
                                                              int method, double beta, double spatial_occ, const unsigned char *__restrict__ nl,
                                                              const unsigned char *__restrict__ lab, double *__restrict__ P) {
    const long q = (long)blockIdx.x * kFuThreads + threadIdx.x;
    const int KK = d.K * d.K;
    if (q >= (long)d.gpl * KK) return;
    const int s = blockIdx.y >> 1, dir = blockIdx.y & 1;
    const int p = (int)(q / KK), i = (int)(q / d.K % d.K), j = (int)(q % d.K);
    const int x = p % d.gw, y = p / d.gw;
    if (dir == 0 ? x + 1 >= d.gw : y + 1 >= d.gh) return;
    const int t = dir == 0 ? p + 1 : p + d.gw;
    const size_t sp = (size_t)s * d.gpl + p, st = (size_t)s * d.gpl + t;
    if (i >= nl[sp] || j >= nl[st]) return;                                     // no label there: never read
    const int a = lab[sp * kFuMaxK + i], b = lab[st * kFuMaxK + j];
    const size_t hs = (size_t)d.J * d.gpl;
    const size_t ba = ((size_t)s * d.K + a) * hs + p, bb = ((size_t)s * d.K + b) * hs + t;
    const float dist = (float)traj_distance(U + ba, V + ba, U + bb, V + bb, d.gpl, d.J, method);
    const unsigned long long mask = (2ull << d.J) - 1;                          // t = 0 .. Jets
    const float smooth_occ = (float)__popcll((occ_bits[((size_t)s * d.K + a) * d.gpl + p] ^ occ_bits[((size_t)s * d.K + b) * d.gpl + t]) & mask);
    const int o1 = (y * d.incr + d.start) * d.w + x * d.incr + d.start;        // oidx1, oidx2 (:1722, 1733, 1737) on the packed plane
    const int o2 = dir == 0 ? (y * d.incr + d.start) * d.w + (x + 1) * d.incr + d.start : ((y + 1) * d.incr + d.start) * d.w + x * d.incr + d.start;
    const float *W = weight + (size_t)s * d.w * d.h;
    const float wsum = W[o1] + W[o2];
    P[((size_t)blockIdx.y * d.gpl + p) * KK + i * d.K + j] = (double)wsum * (beta * (double)dist + spatial_occ * (double)smooth_occ);
}

struct TrwsBufs {
    const unsigned char *nl;
    const double *theta;                  // [n][gpl][kFuMaxK]
    const double *P;                      // [n][2][gpl][K * K]
    double *M;                            // [n][gpl][4][kFuMaxK]: the message INTO the node from its left, up, right, down neighbour
    unsigned char *xcur, *xbest;          // [n][gpl]
    double *seg_energy, *seg_bound;
    int *seg_iters;
};

// TRW-S of segment blockIdx.x, the order of INTEGRATION.md 4c.  MK: the register bound on the label count (>= K).
template <int MK>
__global__ void __launch_bounds__(kTrwsThreads) k_trws(TrwsBufs B, FuseDims d, double eps, int max_iter) {
    __shared__ double sE[3 * kTrwsChunk], sL[3 * kTrwsChunk];
    __shared__ int s_flags[2];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int gw = d.gw, gh = d.gh, gpl = d.gpl, K = d.K, KK = K * K;
    const unsigned char *nl = B.nl + (size_t)s * gpl;
    const double *theta = B.theta + (size_t)s * gpl * kFuMaxK;
    const double *PR = B.P + (size_t)(2 * s) * gpl * KK, *PD = PR + (size_t)gpl * KK;
    double *M = B.M + (size_t)s * gpl * 4 * kFuMaxK;
    unsigned char *xcur = B.xcur + (size_t)s * gpl, *xbest = B.xbest + (size_t)s * gpl;
    auto msg = [&](int p, int dir) { return M + ((size_t)p * 4 + dir) * kFuMaxK; };
    const int D = gw + gh - 1;
    double best = 0, lb_prev = 0;
    int iters = 0;
    // theta-hat: theta + M_left + M_up + M_right + M_down of the present neighbours, in that order; gamma = 1 / max(n_in, n_out)
    auto node_hat = [&](int p, int x, int y, int m, double *th, bool nb[4], double &gamma) {
        nb[0] = x > 0 && nl[p - 1] > 0;
        nb[1] = y > 0 && nl[p - gw] > 0;
        nb[2] = x + 1 < gw && nl[p + 1] > 0;
        nb[3] = y + 1 < gh && nl[p + gw] > 0;
        const int nin = (int)nb[0] + (int)nb[1], nout = (int)nb[2] + (int)nb[3];
        gamma = 1.0 / (double)(nin > nout ? (nin > 0 ? nin : 1) : (nout > 0 ? nout : 1));
#pragma unroll
        for (int i = 0; i < MK; i++)
            if (i < m) th[i] = theta[(size_t)p * kFuMaxK + i];
        for (int k = 0; k < 4; k++) {
            if (!nb[k]) continue;
            const double *mk = msg(p, k);
#pragma unroll
            for (int i = 0; i < MK; i++)
                if (i < m) th[i] = th[i] + mk[i];
        }
    };
    for (int it = 1; it <= max_iter; it++) {
        // ---- forward pass: diagonals 0 .. D - 1; labelling, then messages to the right and down neighbours
        for (int dg = 0; dg < D; dg++) {
            const int x0 = dg - (gh - 1) > 0 ? dg - (gh - 1) : 0, x1 = dg < gw - 1 ? dg : gw - 1;
            for (int x = x0 + tid; x <= x1; x += kTrwsThreads) {
                const int y = dg - x, p = y * gw + x, m = nl[p];
                if (m == 0) continue;
                double th[MK], a[MK];
                bool nb[4];
                double gamma;
                node_hat(p, x, y, m, th, nb, gamma);
                // x_s = argmin_i theta(i) + P_left(x_left, i) + P_up(x_up, i) + M_right(i) + M_down(i), ties to the lower label
                int xs = 0;
                double bv = 0;
#pragma unroll
                for (int i = 0; i < MK; i++) {
                    if (i >= m) continue;
                    double v = theta[(size_t)p * kFuMaxK + i];
                    if (nb[0]) v = v + PR[(size_t)(p - 1) * KK + xcur[p - 1] * K + i];
                    if (nb[1]) v = v + PD[(size_t)(p - gw) * KK + xcur[p - gw] * K + i];
                    if (nb[2]) v = v + msg(p, 2)[i];
                    if (nb[3]) v = v + msg(p, 3)[i];
                    if (i == 0 || v < bv) { bv = v; xs = i; }
                }
                xcur[p] = (unsigned char)xs;
                for (int k = 0; k < 2; k++) {                                   // right (edge stored at p in PR), then down (PD)
                    if (!nb[2 + k]) continue;
                    const int t = k == 0 ? p + 1 : p + gw, mt = nl[t];
                    const double *Mts = msg(p, 2 + k);
                    const double *Pst = (k == 0 ? PR : PD) + (size_t)p * KK;
#pragma unroll
                    for (int i = 0; i < MK; i++)
                        if (i < m) a[i] = gamma * th[i] - Mts[i];
                    double out[MK];
                    double mn = 0;
#pragma unroll
                    for (int j = 0; j < MK; j++) {
                        if (j >= mt) continue;
                        double v = 0;
#pragma unroll
                        for (int i = 0; i < MK; i++) {
                            if (i >= m) continue;
                            const double c = a[i] + Pst[i * K + j];
                            if (i == 0 || c < v) v = c;
                        }
                        out[j] = v;
                        if (j == 0 || v < mn) mn = v;
                    }
                    double *dst = msg(t, k);                                    // into t from its left (k 0) / up (k 1)
#pragma unroll
                    for (int j = 0; j < MK; j++)
                        if (j < mt) dst[j] = out[j] - mn;
                }
            }
            __syncthreads();
        }
        // ---- backward pass: diagonals D - 1 .. 0; messages to the left and up neighbours, P in its (earlier, later) orientation
        for (int dg = D - 1; dg >= 0; dg--) {
            const int x0 = dg - (gh - 1) > 0 ? dg - (gh - 1) : 0, x1 = dg < gw - 1 ? dg : gw - 1;
            for (int x = x0 + tid; x <= x1; x += kTrwsThreads) {
                const int y = dg - x, p = y * gw + x, m = nl[p];
                if (m == 0) continue;
                double th[MK], a[MK];
                bool nb[4];
                double gamma;
                node_hat(p, x, y, m, th, nb, gamma);
                for (int k = 0; k < 2; k++) {                                   // left (edge stored at p - 1 in PR), then up (at p - gw in PD)
                    if (!nb[k]) continue;
                    const int t = k == 0 ? p - 1 : p - gw, mt = nl[t];
                    const double *Mts = msg(p, k);
                    const double *Pts = (k == 0 ? PR : PD) + (size_t)t * KK;
#pragma unroll
                    for (int i = 0; i < MK; i++)
                        if (i < m) a[i] = gamma * th[i] - Mts[i];
                    double out[MK];
                    double mn = 0;
#pragma unroll
                    for (int j = 0; j < MK; j++) {
                        if (j >= mt) continue;
                        double v = 0;
#pragma unroll
                        for (int i = 0; i < MK; i++) {
                            if (i >= m) continue;
                            const double c = a[i] + Pts[j * K + i];
                            if (i == 0 || c < v) v = c;
                        }
                        out[j] = v;
                        if (j == 0 || v < mn) mn = v;
                    }
                    double *dst = msg(t, 2 + k);                                // into t from its right (k 0) / down (k 1)
#pragma unroll
                    for (int j = 0; j < MK; j++)
                        if (j < mt) dst[j] = out[j] - mn;
                }
            }
            __syncthreads();
        }
        // ---- energy of this iteration's labelling and the bound, summed row by row, left to right: unary, right edge, down edge (0 where absent:
        // the running sum starts at +0 and is never -0, so adding +0 changes no bit)
        double E = 0, LB = 0;
        for (int c0 = 0; c0 < gpl; c0 += kTrwsChunk) {
            for (int c = tid; c < kTrwsChunk && c0 + c < gpl; c += kTrwsThreads) {
                const int p = c0 + c, x = p % gw, y = p / gw, m = nl[p];
                double e[3] = {0, 0, 0}, l[3] = {0, 0, 0};
                if (m > 0) {
                    double th[MK];
                    bool nb[4];
                    double gamma;
                    node_hat(p, x, y, m, th, nb, gamma);
                    const int xs = xcur[p];
                    e[0] = theta[(size_t)p * kFuMaxK + xs];
                    double mn = 0;
#pragma unroll
                    for (int i = 0; i < MK; i++)
                        if (i < m && (i == 0 || th[i] < mn)) mn = th[i];
                    l[0] = mn;
                    for (int k = 0; k < 2; k++) {
                        if (!nb[2 + k]) continue;
                        const int t = k == 0 ? p + 1 : p + gw, mt = nl[t];
                        const double *Pst = (k == 0 ? PR : PD) + (size_t)p * KK;
                        const double *Mts = msg(p, 2 + k), *Mst = msg(t, k);
                        e[1 + k] = Pst[xs * K + xcur[t]];
                        double v = 0;
                        for (int i = 0; i < m; i++)
                            for (int j = 0; j < mt; j++) {
                                const double r = (Pst[i * K + j] - Mts[i]) - Mst[j];
                                if ((i == 0 && j == 0) || r < v) v = r;
                            }
                        l[1 + k] = v;
                    }
                }
                for (int k = 0; k < 3; k++) { sE[3 * c + k] = e[k]; sL[3 * c + k] = l[k]; }
            }
            __syncthreads();
            if (tid == 0) {
                const int cn = gpl - c0 < kTrwsChunk ? gpl - c0 : kTrwsChunk;
                for (int c = 0; c < 3 * cn; c++) { E = E + sE[c]; LB = LB + sL[c]; }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const bool improved = it == 1 || E < best;                         // ties keep the earliest iteration
            if (improved) best = E;
            s_flags[0] = improved;
            s_flags[1] = it >= 2 && LB - lb_prev < eps;
            lb_prev = LB;
            B.seg_bound[s] = LB;
        }
        __syncthreads();
        iters = it;
        if (s_flags[0])
            for (int p = tid; p < gpl; p += kTrwsThreads) xbest[p] = xcur[p];
        const bool stop = s_flags[1];
        __syncthreads();                                                        // s_flags and xcur are rewritten by the next iteration
        if (stop) break;
    }
    if (tid == 0) {
        B.seg_energy[s] = best;
        B.seg_iters[s] = iters;
    }
}

// :1843-1864: the chosen slot, u(Jets - 1) / xy_incr, v(Jets - 1) / xy_incr and max_t occluded(t), t = 0 .. Jets
__global__ void __launch_bounds__(kFuThreads) k_fuse_output(const double *__restrict__ U, const double *__restrict__ V,
                                                            const unsigned long long *__restrict__ occ_bits, FuseDims d, const unsigned char *__restrict__ nl,
                                                            const unsigned char *__restrict__ lab, const unsigned char *__restrict__ xbest,
                                                            int *__restrict__ slot, double *__restrict__ fu, double *__restrict__ fv,
                                                            unsigned char *__restrict__ occ) {
    const int p = blockIdx.x * kFuThreads + threadIdx.x;
    if (p >= d.gpl) return;
    const size_t sp = (size_t)blockIdx.y * d.gpl + p;
    if (nl[sp] == 0) {
        slot[sp] = -1;
        fu[sp] = 1e10;                                                          // UNKNOWN_FLOW (hypothesis.h:23)
        fv[sp] = 1e10;
        occ[sp] = 0;
        return;
    }
    const int k = lab[sp * kFuMaxK + xbest[sp]];
    const size_t b = (((size_t)blockIdx.y * d.K + k) * d.J + (d.J - 1)) * d.gpl + p;
    slot[sp] = k;
    fu[sp] = U[b] / d.incr;
    fv[sp] = V[b] / d.incr;
    occ[sp] = (occ_bits[((size_t)blockIdx.y * d.K + k) * d.gpl + p] & ((2ull << d.J) - 1)) != 0;
}

// messages and labellings start at 0; then the four launches
int fuse_device(sfa_ctx *ctx, const sfa_fuse_params *p, int n, int K, int Jets, int w, int h, int gw, int gh, const FuseWork &f, hipEvent_t *ev) {
    FuseDims d;
    d.n = n; d.K = K; d.J = Jets; d.gw = gw; d.gh = gh; d.gpl = gw * gh; d.w = w; d.h = h;
    d.incr = p->skip + 1; d.start = (int)(0.5f * p->skip);                     // xy_incr, xy_start (utils.cpp:522-526)
    const size_t gpl = (size_t)d.gpl, KK = (size_t)K * K;
    SFA_HIP(ctx, hipMemsetAsync(f.M, 0, (size_t)n * gpl * 4 * kFuMaxK * 8, ctx->stream));
    SFA_HIP(ctx, hipMemsetAsync(f.xcur, 0, (size_t)n * gpl, ctx->stream));
    SFA_HIP(ctx, hipMemsetAsync(f.xbest, 0, (size_t)n * gpl, ctx->stream));
    const dim3 pix((unsigned)((gpl + kFuThreads - 1) / kFuThreads), (unsigned)n);
    SFA_TRY(mark_if(ctx, ev, 0));
    hipLaunchKernelGGL(k_fuse_labels, pix, dim3(kFuThreads), 0, ctx->stream, f.U, f.V, f.energy, d, p->traj_sim_method, p->traj_sim_thres, p->pin_first != 0, f.nl, f.lab, f.theta);
    SFA_HIP(ctx, hipGetLastError());
    SFA_TRY(mark_if(ctx, ev, 1));
    hipLaunchKernelGGL(k_fuse_pairwise, dim3((unsigned)((gpl * KK + kFuThreads - 1) / kFuThreads), (unsigned)(2 * n)), dim3(kFuThreads), 0, ctx->stream, f.U, f.V,
                       f.occ, f.weight, d, p->traj_sim_method, p->acc_beta, p->acc_spatial_occ, f.nl, f.lab, f.P);
    SFA_HIP(ctx, hipGetLastError());
    SFA_TRY(mark_if(ctx, ev, 2));
    TrwsBufs tb;
    tb.nl = f.nl; tb.theta = f.theta; tb.P = f.P; tb.M = f.M;
    tb.xcur = f.xcur; tb.xbest = f.xbest; tb.seg_energy = f.seg_energy; tb.seg_bound = f.seg_bound; tb.seg_iters = f.seg_iters;
    if (K <= 4) hipLaunchKernelGGL(k_trws<4>, dim3(n), dim3(kTrwsThreads), 0, ctx->stream, tb, d, p->trws_eps, p->trws_max_iter);
    else if (K <= 8) hipLaunchKernelGGL(k_trws<8>, dim3(n), dim3(kTrwsThreads), 0, ctx->stream, tb, d, p->trws_eps, p->trws_max_iter);
    else hipLaunchKernelGGL(k_trws<16>, dim3(n), dim3(kTrwsThreads), 0, ctx->stream, tb, d, p->trws_eps, p->trws_max_iter);
    SFA_HIP(ctx, hipGetLastError());
    SFA_TRY(mark_if(ctx, ev, 3));
    hipLaunchKernelGGL(k_fuse_output, pix, dim3(kFuThreads), 0, ctx->stream, f.U, f.V, f.occ, d, f.nl, f.lab, f.xbest, f.slot, f.fu, f.fv, f.out_occ);
    SFA_HIP(ctx, hipGetLastError());
    SFA_TRY(mark_if(ctx, ev, 4));
    return SFA_OK;
}

}  // namespace sfa

using namespace sfa;

void sfa_fuse_params_default(sfa_fuse_params *p) {
    if (!p) return;
    *p = sfa_fuse_params{};
    p->acc_beta = 10.0;                  // setDefault (dense_tracking.cpp:136-152)
    p->acc_spatial_occ = 10.0;
    p->traj_sim_method = 1;
    p->traj_sim_thres = 0.1;
    p->trws_eps = 1e-5;
    p->trws_max_iter = 10;
    p->skip = 1;
}

int sfa_fuse_hypotheses(sfa_ctx *ctx, const sfa_fuse_params *p, int n, int K, int Jets, int w, int h, const double *U, const double *V, const double *energy,
                        const unsigned long long *occ_bits, const float *weight, int *slot, double *flow_u, double *flow_v, unsigned char *occ,
                        double *seg_energy, double *seg_bound, int *seg_iters, float *stage_ms) {
    if (!(ctx && p && U && V && energy && occ_bits && weight && slot && flow_u && flow_v && occ && seg_energy && seg_bound && seg_iters))
        return set_error(ctx, SFA_ERR_ARG, "sfa_fuse_hypotheses: null argument");
    if (!(n >= 1 && n <= 32767 && K >= 1 && K <= kFuMaxK && Jets >= 1 && Jets <= kFuMaxJets && w >= 1 && h >= 1))
        return set_error(ctx, SFA_ERR_ARG, "sfa_fuse_hypotheses: bad sizes (1 <= n <= 32767, 1 <= K <= %d, 1 <= Jets <= %d, w, h >= 1)", kFuMaxK, kFuMaxJets);
    if (p->traj_sim_method != 0 && p->traj_sim_method != 1)
        return set_error(ctx, SFA_ERR_ARG, "sfa_fuse_hypotheses: acc_traj_sim_method %d (0 ADJ, 1 ACC; 2 FINAL reads flow_y[Jets], past the array)",
                         p->traj_sim_method);
    if (p->trws_max_iter < 1) return set_error(ctx, SFA_ERR_ARG, "sfa_fuse_hypotheses: acc_trws_max_iter %d < 1", p->trws_max_iter);
    int gw, gh;
    if (sfa_accumulate_grid(w, h, p->skip, &gw, &gh) != SFA_OK) return set_error(ctx, SFA_ERR_ARG, "%s", sfa_last_error(nullptr));
    const size_t gpl = (size_t)gw * gh, KK = (size_t)K * K, nh = (size_t)n * K * Jets * gpl;
    if ((gpl * KK + kFuThreads - 1) / kFuThreads > 0x7fffffffull) return set_error(ctx, SFA_ERR_ARG, "sfa_fuse_hypotheses: grid too large");

    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem dU, dV, den, docc, dw, dnl, dlab, dth, dP, dM, dx, dslot, dfu, dfv, dout_occ, dseg;
    SFA_TRY(dU.alloc(ctx, nh * 8)); SFA_TRY(dV.alloc(ctx, nh * 8)); SFA_TRY(den.alloc(ctx, (size_t)n * K * gpl * 8));
    SFA_TRY(docc.alloc(ctx, (size_t)n * K * gpl * 8)); SFA_TRY(dw.alloc(ctx, (size_t)n * w * h * 4));
    SFA_TRY(dnl.alloc(ctx, (size_t)n * gpl)); SFA_TRY(dlab.alloc(ctx, (size_t)n * gpl * kFuMaxK)); SFA_TRY(dth.alloc(ctx, (size_t)n * gpl * kFuMaxK * 8));
    SFA_TRY(dP.alloc(ctx, (size_t)n * 2 * gpl * KK * 8)); SFA_TRY(dM.alloc(ctx, (size_t)n * gpl * 4 * kFuMaxK * 8)); SFA_TRY(dx.alloc(ctx, (size_t)n * gpl * 2));
    SFA_TRY(dslot.alloc(ctx, (size_t)n * gpl * 4)); SFA_TRY(dfu.alloc(ctx, (size_t)n * gpl * 8)); SFA_TRY(dfv.alloc(ctx, (size_t)n * gpl * 8));
    SFA_TRY(dout_occ.alloc(ctx, (size_t)n * gpl)); SFA_TRY(dseg.alloc(ctx, (size_t)n * 24));
    SFA_HIP(ctx, hipMemcpyAsync(dU.p, U, nh * 8, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(dV.p, V, nh * 8, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(den.p, energy, (size_t)n * K * gpl * 8, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(docc.p, occ_bits, (size_t)n * K * gpl * 8, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(dw.p, weight, (size_t)n * w * h * 4, hipMemcpyHostToDevice, ctx->stream));
    double *pseg = static_cast<double *>(dseg.p);
    unsigned char *px = static_cast<unsigned char *>(dx.p);
    FuseWork f;
    f.U = static_cast<const double *>(dU.p); f.V = static_cast<const double *>(dV.p); f.energy = static_cast<const double *>(den.p);
    f.occ = static_cast<const unsigned long long *>(docc.p); f.weight = dw.f();
    f.nl = static_cast<unsigned char *>(dnl.p); f.lab = static_cast<unsigned char *>(dlab.p); f.theta = static_cast<double *>(dth.p);
    f.P = static_cast<double *>(dP.p); f.M = static_cast<double *>(dM.p); f.xcur = px; f.xbest = px + (size_t)n * gpl;
    f.slot = static_cast<int *>(dslot.p); f.fu = static_cast<double *>(dfu.p); f.fv = static_cast<double *>(dfv.p); f.out_occ = static_cast<unsigned char *>(dout_occ.p);
    f.seg_energy = pseg; f.seg_bound = pseg + n; f.seg_iters = reinterpret_cast<int *>(pseg + 2 * n);
    StageEvents ev;
    if (stage_ms) SFA_TRY(ev.make(ctx, 5));
    SFA_TRY(fuse_device(ctx, p, n, K, Jets, w, h, gw, gh, f, stage_ms ? ev.e : nullptr));
    SFA_HIP(ctx, hipMemcpyAsync(slot, dslot.p, (size_t)n * gpl * 4, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(flow_u, dfu.p, (size_t)n * gpl * 8, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(flow_v, dfv.p, (size_t)n * gpl * 8, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(occ, dout_occ.p, (size_t)n * gpl, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(seg_energy, pseg, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(seg_bound, pseg + n, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(seg_iters, pseg + 2 * n, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stage_ms) SFA_TRY(ev.read(ctx, 5, stage_ms));
    return SFA_OK;
}
