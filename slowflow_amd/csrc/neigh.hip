// neigh.hip -- dense_tracking's alternation around the fusion (dense_tracking.cpp:1381-1583) on the GPU: the prune of every pixel's hypothesis list to the
// last selection plus the best few (:1384-1416), the hypotheses drawn from neighbouring pixels (:1432-1583) and their rescoring (:1549-1553).  The reference's result depends on FLANN's
// result order, on one random engine consumed pixel after pixel and on an out-of-bounds read; INTEGRATION.md 4d defines the stage as it is built here and
// tests/neigh_ref.py restates it.  fp64 without contraction where a flow is touched; everything else is integer arithmetic.
//
// A list has kNeighK = 16 positions per pixel: U, V [n][16][J][gpl], energy, occ, origin [n][16][gpl]; +Inf (or NaN) energy = absent.
//
// Shape:
//   k_neigh_flags    one thread per pixel: does it hold a hypothesis, which position a neighbour copies from it, is it a candidate of set 0 / set 1; the
//                    sets' sizes per segment.
//   k_neigh_prune    one thread per pixel: the map (new position -> old position) of the prune.
//   k_neigh_propose  one wave per pixel.  The candidates are lattice points, so the search is a count over the lattice points of a box, 64 per step
//                    (ballot + popcount); the 50-nearest fallback gallops and bisects on the integer d^2 with the same count.  All tryouts' draws are known
//                    beforehand (Philox is counter-based): lane i holds tryout i's index and ONE walk in raster order resolves them all.  Then the tryouts
//                    one after the other: lane l < 16 compares list entry l with the proposal (hypothesis::distance over Jets steps), a ballot decides.
//                    Writes the map (position -> pixel and position of the snapshot); no flow is copied here.
//   k_neigh_gather   one thread per (position, pixel): copies a hypothesis by the map -- the prune's and the proposals' common second half.
//   k_neigh_rescored one thread per pixel: after the energy stage's kernels (energy.hip) have scored a position's new proposals at their new place, the
//                    energy plus the weight of the rate the hypothesis was born in, and the occlusion word, go into the list.
// Measured on one MI355X at a 512 x 218 grid, Jets 32, 4 slots, default keys (profiles/neigh_bench.txt): the search-draw-accept kernel takes 8 - 12 ms a
// round, under a third of ONE TRW-S iteration at K 4 (34 ms); flags, prune and the gathers stay under 1 ms each.  The rescoring costs more, 12 - 15 ms a
// round: it runs the energy chain over the whole grid once per (start_jet, position) that holds a new proposal, up to ten times per start_jet; one launch
// over the (position, start_jet) pairs with work is the form a resident job should take.
#include "hyp_device.h"

#pragma clang fp contract(off)

namespace sfa {

constexpr int kNeighK = 16;
constexpr int kNeighThreads = 256;
constexpr int kNeighWaves = kNeighThreads / 64;
constexpr int kNeighNearest = 50;                 // knnSearch(..., 50, ...) (:1507)
constexpr int kNeighNew = 1 << 30;                // map entry: accepted as a proposal in this call
constexpr int kNeighMaxSide = 2896;               // d^2 < 2^24: exact in fp32, as FLANN forms it
constexpr int kNeighAll = 1 << 25;                // above every d^2

struct NeighDims { int n, J, gw, gh, gpl; };

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11)
__host__ __device__ inline void philox4x32_10(const unsigned ctr_in[4], const unsigned key_in[2], unsigned out[4]) {
    unsigned c0 = ctr_in[0], c1 = ctr_in[1], c2 = ctr_in[2], c3 = ctr_in[3], k0 = key_in[0], k1 = key_in[1];
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__global__ void __launch_bounds__(kNeighThreads) k_neigh_philox(const unsigned *__restrict__ ctr, const unsigned *__restrict__ key, unsigned *__restrict__ out, int n) {
    const int i = blockIdx.x * kNeighThreads + threadIdx.x;
    if (i >= n) return;
    philox4x32_10(ctr + 4 * i, key + 2 * i, out + 4 * i);
}

// the first lattice coordinate of set t: the smallest c >= 1 with (c - (t + 1)) % skip == 0 in C's remainder ((-1) % 1 == 0: skip 1 admits c = 1 in set 1)
__host__ __device__ inline int lattice_first(int t, int skip) { return 1 + (t % skip); }
__device__ __forceinline__ bool on_lattice(int c, int t, int skip) { const int c0 = lattice_first(t, skip); return c >= c0 && (c - c0) % skip == 0; }

// flags: bit t = candidate of set t, bit 2 = holds a hypothesis.  srcpos: the position a neighbour copies.  round 0: the lists are as the energies left them,
// so "holds" is any present position and the source the lowest float score, ties to the lower position; later rounds: position 0 of a pruned list
__global__ void __launch_bounds__(kNeighThreads) k_neigh_flags(const double *__restrict__ energy, const unsigned char *__restrict__ consistent, NeighDims d, int round,
                                                               int skip1, int skip2, unsigned char *__restrict__ flags, unsigned char *__restrict__ srcpos,
                                                               int *__restrict__ total) {
    const int p = blockIdx.x * kNeighThreads + threadIdx.x;
    const int s = blockIdx.y;
    int c0 = 0, c1 = 0;
    if (p < d.gpl) {
        const size_t sp = (size_t)s * d.gpl + p;
        int src = 0;
        bool has;
        if (round > 0) {
            has = present(energy[(size_t)s * kNeighK * d.gpl + p]);
        } else {
            has = false;
            float best = 0;
            for (int k = 0; k < kNeighK; k++) {
                const double e = energy[((size_t)s * kNeighK + k) * d.gpl + p];
                if (!present(e)) continue;
                const float f = (float)e;
                if (!has || f < best) { best = f; src = k; }
                has = true;
            }
        }
        const int x = p % d.gw, y = p / d.gw;
        const bool ok = has && (round > 0 || consistent[sp] == 1);
        c0 = ok && on_lattice(x, 0, skip1) && on_lattice(y, 0, skip1);
        c1 = ok && on_lattice(x, 1, skip2) && on_lattice(y, 1, skip2);
        flags[sp] = (unsigned char)(c0 | (c1 << 1) | ((int)has << 2));
        srcpos[sp] = (unsigned char)src;
    }
    const int n0 = __popcll(__ballot(c0)), n1 = __popcll(__ballot(c1));
    if ((threadIdx.x & 63) == 0) {
        if (n0) atomicAdd(total + 2 * s, n0);
        if (n1) atomicAdd(total + 2 * s + 1, n1);
    }
}

// map[(s, k, p)] = p * 16 + old position, or -1 (:1384-1416).  sel: the position the last fusion selected, -1 none; a selection that is absent counts as none
__global__ void __launch_bounds__(kNeighThreads) k_neigh_prune(const double *__restrict__ energy, const int *__restrict__ sel, NeighDims d, int keep,
                                                               int *__restrict__ map) {
    const int p = blockIdx.x * kNeighThreads + threadIdx.x;
    if (p >= d.gpl) return;
    const int s = blockIdx.y;
    int last = sel[(size_t)s * d.gpl + p];
    if (last < 0 || last >= kNeighK || !present(energy[((size_t)s * kNeighK + last) * d.gpl + p])) last = -1;
    int order[kNeighK];
    float key[kNeighK];
    int m = 0;
    for (int k = 0; k < kNeighK; k++) {                                          // compareHypotheses on the float score, a stable insertion sort
        if (k == last) continue;
        const double e = energy[((size_t)s * kNeighK + k) * d.gpl + p];
        if (!present(e)) continue;
        const float f = (float)e;
        int j = m;
        while (j > 0 && f < key[j - 1]) { key[j] = key[j - 1]; order[j] = order[j - 1]; j--; }
        key[j] = f;
        order[j] = k;
        m++;
    }
    int nk = 0;
    int *out = map + (size_t)s * kNeighK * d.gpl + p;
    if (last >= 0) out[(size_t)nk++ * d.gpl] = p * kNeighK + last;
    for (int c = 0; c < m; c++)
        if (nk <= keep && nk < kNeighK) out[(size_t)nk++ * d.gpl] = p * kNeighK + order[c];   // `size() <= perturb_keep` before each push (:1409)
    for (; nk < kNeighK; nk++) out[(size_t)nk * d.gpl] = -1;
}

struct NeighSearch { int skip[2]; int tdisc[2]; int quota1; int tryouts; int method; double thres; unsigned key0; };

// The lattice points of set t inside the square of half-side `rad` round (px, py), clipped to the grid, in raster order: nx * ny of them
struct NeighBox {
    int x0, y0, nx, ny, skip;
    __device__ NeighBox(int px, int py, int rad, int t, int skip_, int gw, int gh) : skip(skip_) {
        const int f = lattice_first(t, skip);
        auto range = [&](int c, int size, int &first, int &count) {
            const int lo = c - rad > f ? c - rad : f, hi = c + rad < size - 1 ? c + rad : size - 1;
            const int i0 = (lo - f + skip - 1) / skip;
            first = f + i0 * skip;
            count = hi >= first ? (hi - first) / skip + 1 : 0;
        };
        range(px, gw, x0, nx);
        range(py, gh, y0, ny);
        if (nx == 0 || ny == 0) nx = ny = 0;
    }
    __device__ int size() const { return nx * ny; }
    __device__ void at(int i, int &x, int &y) const { y = y0 + (i / nx) * skip; x = x0 + (i % nx) * skip; }
};

__device__ __forceinline__ int isqrt_floor(int v) {
    int r = (int)sqrtf((float)v);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
}

// candidates of set t with d^2 <= T (the pixel itself among them); the same value in every lane
__device__ int neigh_count(const unsigned char *__restrict__ fl, int px, int py, int t, int skip, int gw, int gh, int T, int lane) {
    const NeighBox b(px, py, T >= (kNeighMaxSide * kNeighMaxSide) ? kNeighMaxSide : isqrt_floor(T), t, skip, gw, gh);
    int cnt = 0;
    for (int c0 = 0; c0 < b.size(); c0 += 64) {
        bool in = false;
        if (c0 + lane < b.size()) {
            int x, y;
            b.at(c0 + lane, x, y);
            const int dx = x - px, dy = y - py;
            in = ((fl[y * gw + x] >> t) & 1) && dx * dx + dy * dy <= T;
        }
        cnt += __popcll(__ballot(in));
    }
    return cnt;
}

__global__ void __launch_bounds__(kNeighThreads) k_neigh_propose(const double *__restrict__ U, const double *__restrict__ V, const double *__restrict__ energy,
                                                                 const unsigned char *__restrict__ flags, const unsigned char *__restrict__ srcpos,
                                                                 const int *__restrict__ total, const unsigned *__restrict__ seq_start, NeighDims d,
                                                                 NeighSearch q, int *__restrict__ map) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * kNeighWaves + (threadIdx.x >> 6);
    if (p >= d.gpl) return;                                                      // the whole wave; no block-wide barrier below
    const int s = blockIdx.y, gw = d.gw, gh = d.gh;
    const int px = p % gw, py = p / gw;
    const unsigned char *fl = flags + (size_t)s * d.gpl;
    const unsigned char *sp = srcpos + (size_t)s * d.gpl;
    const size_t hs = (size_t)d.J * d.gpl, seg = (size_t)s * kNeighK * hs;
    // the list: lane l < 16 holds entry l as pixel * 16 + position of the snapshot
    int ent = -1;
    if (lane < kNeighK && present(energy[((size_t)s * kNeighK + lane) * d.gpl + p])) ent = p * kNeighK + lane;
    int added = 0;
    const unsigned key[2] = {q.key0, seq_start[s]};
    for (int t = 0; t < 2; t++) {
        const int quota = (t + 1) * q.quota1;
        if (added >= quota || q.tryouts == 0) continue;
        const int skip = q.skip[t], self = (fl[p] >> t) & 1, tot = total[2 * s + t];
        // ---- the result set as a threshold: members have d^2 < Ts, or d^2 == Ts and are among the first `meq` such in raster order
        int Ts, meq = 0, found;
        const int cdisc = neigh_count(fl, px, py, t, skip, gw, gh, q.tdisc[t], lane);
        if (cdisc >= kNeighNearest) {
            Ts = q.tdisc[t] + 1;
            found = cdisc - self;
        } else if (tot <= kNeighNearest) {
            Ts = kNeighAll;
            found = tot - self;
        } else {
            // the smallest T with count(T) >= 50; it exists, as count(every d^2) = tot > 50
            int lo = q.tdisc[t], clo = cdisc, hi = lo < 8 ? 16 : 2 * lo;
            for (;;) {
                if (hi >= kNeighAll) { hi = kNeighAll; break; }
                const int c = neigh_count(fl, px, py, t, skip, gw, gh, hi, lane);
                if (c >= kNeighNearest) break;
                lo = hi; clo = c; hi = 2 * hi;
            }
            while (hi - lo > 1) {
                const int mid = lo + (hi - lo) / 2;
                const int c = neigh_count(fl, px, py, t, skip, gw, gh, mid, lane);
                if (c >= kNeighNearest) hi = mid; else { lo = mid; clo = c; }
            }
            Ts = hi;
            meq = kNeighNearest - clo;
            found = kNeighNearest - self;
        }
        if (found <= 0) continue;
        const NeighBox b(px, py, Ts >= kNeighMaxSide * kNeighMaxSide ? kNeighMaxSide : isqrt_floor(Ts), t, skip, gw, gh);
        for (int tb = 0; tb < q.tryouts && added < quota; tb += 64) {
            const int nt = q.tryouts - tb < 64 ? q.tryouts - tb : 64;
            // ---- lane i: the draw of tryout tb + i
            int ridx = -1, res = -1;
            if (lane < nt) {
                const unsigned ctr[4] = {(unsigned)p, (unsigned)t, (unsigned)(tb + lane), 0u};
                unsigned r[4];
                philox4x32_10(ctr, key, r);
                ridx = (int)(((unsigned long long)r[0] * (unsigned)found) >> 32);
            }
            // ---- one walk in raster order resolves every draw
            int cnt = 0, ceq = 0;
            for (int c0 = 0; c0 < b.size(); c0 += 64) {
                bool cand = false, eq = false, less = false;
                if (c0 + lane < b.size()) {
                    int x, y;
                    b.at(c0 + lane, x, y);
                    const int dx = x - px, dy = y - py, d2 = dx * dx + dy * dy;
                    cand = ((fl[y * gw + x] >> t) & 1) && !(dx == 0 && dy == 0);
                    eq = cand && d2 == Ts;
                    less = cand && d2 < Ts;
                }
                const unsigned long long eqm = __ballot(eq);
                const int rank = ceq + __popcll(eqm & ((1ull << lane) - 1));
                const unsigned long long mm = __ballot(less || (eq && rank < meq));
                const int nm = __popcll(mm);
                ceq += __popcll(eqm);
                if (ridx >= cnt && ridx < cnt + nm) {
                    unsigned long long m2 = mm;
                    for (int k = ridx - cnt; k > 0; k--) m2 &= m2 - 1;
                    int x, y;
                    b.at(c0 + __ffsll((long long)m2) - 1, x, y);
                    res = y * gw + x;
                }
                cnt += nm;
                if (__ballot(lane < nt && res < 0) == 0) break;
            }
            // ---- the tryouts in their order (:1535-1568)
            for (int i = 0; i < nt && added < quota; i++) {
                const int c = __shfl(res, i);
                if (c < 0) continue;                                             // unreachable: ridx < found = the members the walk meets
                const unsigned long long freem = __ballot(lane < kNeighK && ent < 0);
                if (freem == 0) { added = quota; break; }                        // a guard only: neigh_check's limits and the entry point's scan keep a list from filling up
                const int cpos = sp[c];
                bool bad = false;
                if (ent >= 0) {
                    const size_t ba = seg + (size_t)(ent & (kNeighK - 1)) * hs + (size_t)((ent & ~kNeighNew) >> 4);
                    const size_t bb = seg + (size_t)cpos * hs + c;
                    bad = !(traj_distance(U + ba, V + ba, U + bb, V + bb, d.gpl, d.J, q.method) > q.thres);
                }
                if (__ballot(bad) != 0) continue;
                if (lane == __ffsll((long long)freem) - 1) ent = (c * kNeighK + cpos) | kNeighNew;
                added++;
            }
        }
    }
    if (lane < kNeighK) map[((size_t)s * kNeighK + lane) * d.gpl + p] = ent;
}

// position k of pixel p takes the hypothesis map names (bit 30 aside); -1: absent (+Inf, zeros).  An entry with bit 30 gets 0x80 or-ed into its origin
__global__ void __launch_bounds__(kNeighThreads) k_neigh_gather(NeighPlanes in, NeighPlanes out, const int *__restrict__ map, NeighDims d) {
    const int p = blockIdx.x * kNeighThreads + threadIdx.x;
    if (p >= d.gpl) return;
    const int sk = blockIdx.y;                                                   // s * 16 + k
    const size_t o = (size_t)sk * d.gpl + p, hs = (size_t)d.J * d.gpl;
    const int m = map[o];
    if (m < 0) {
        out.energy[o] = __longlong_as_double(0x7ff0000000000000ll);
        out.occ[o] = 0;
        out.origin[o] = 0;
        for (int f = 0; f < d.J; f++) { out.U[(size_t)sk * hs + f * (size_t)d.gpl + p] = 0; out.V[(size_t)sk * hs + f * (size_t)d.gpl + p] = 0; }
        return;
    }
    const int src = m & ~kNeighNew, spix = src >> 4, spos = src & (kNeighK - 1);
    const size_t ssk = (size_t)(sk / kNeighK) * kNeighK + spos, i = ssk * d.gpl + spix;
    out.energy[o] = in.energy[i];
    out.occ[o] = in.occ[i];
    out.origin[o] = (unsigned char)(in.origin[i] | ((m & kNeighNew) ? 0x80 : 0));
    for (int f = 0; f < d.J; f++) {
        out.U[(size_t)sk * hs + f * (size_t)d.gpl + p] = in.U[ssk * hs + f * (size_t)d.gpl + spix];
        out.V[(size_t)sk * hs + f * (size_t)d.gpl + p] = in.V[ssk * hs + f * (size_t)d.gpl + spix];
    }
}

static int neigh_gather(sfa_ctx *ctx, const NeighDims &d, const NeighPlanes &in, const NeighPlanes &out, const int *map) {
    hipLaunchKernelGGL(k_neigh_gather, dim3((unsigned)((d.gpl + kNeighThreads - 1) / kNeighThreads), (unsigned)(d.n * kNeighK)), dim3(kNeighThreads), 0, ctx->stream,
                       in, out, map, d);
    SFA_HIP(ctx, hipGetLastError());
    return SFA_OK;
}

int neigh_prune_device(sfa_ctx *ctx, int n, int Jets, int gw, int gh, int keep, const int *sel, const NeighPlanes &in, const NeighPlanes &out, int *map,
                       hipEvent_t *ev) {
    const NeighDims d{n, Jets, gw, gh, gw * gh};
    SFA_TRY(mark_if(ctx, ev, 0));
    hipLaunchKernelGGL(k_neigh_prune, dim3((unsigned)((d.gpl + kNeighThreads - 1) / kNeighThreads), (unsigned)n), dim3(kNeighThreads), 0, ctx->stream, in.energy, sel,
                       d, keep, map);
    SFA_HIP(ctx, hipGetLastError());
    SFA_TRY(mark_if(ctx, ev, 1));
    SFA_TRY(neigh_gather(ctx, d, in, out, map));
    SFA_TRY(mark_if(ctx, ev, 2));
    return SFA_OK;
}

// what the entry point and a job refuse alike, by the key's name
int neigh_check(sfa_ctx *ctx, const char *fn, const sfa_neigh_params *p, int gw, int gh, int round) {
    if (!(p->neigh_hyp_radius > 0)) REFUSE("%s: acc_neigh_hyp_radius %g <= 0 (the reference's knnSearch(acc_neigh_draws) branch is not built)", fn, (double)p->neigh_hyp_radius);
    if (p->neigh_skip1 < 1) REFUSE("%s: acc_neigh_skip1 %d < 1", fn, p->neigh_skip1);
    if (p->neigh_skip2 < 1) REFUSE("%s: acc_neigh_skip2 %d < 1", fn, p->neigh_skip2);
    if (p->hyp_neigh_tryouts < 0) REFUSE("%s: acc_hyp_neigh_tryouts %d < 0", fn, p->hyp_neigh_tryouts);
    if (p->neigh_hyp < 0 || 2 * p->neigh_hyp > kNeighK) REFUSE("%s: acc_neigh_hyp %d: 2 * acc_neigh_hyp outside 0 .. %d positions", fn, p->neigh_hyp, kNeighK);
    if (p->traj_sim_method != 0 && p->traj_sim_method != 1)
        REFUSE("%s: acc_traj_sim_method %d (0 ADJ, 1 ACC; 2 FINAL reads flow_y[Jets], past the array)", fn, p->traj_sim_method);
    // a list never overflows: what a pixel may hold before the draws, plus both sets' quotas, fits the 16 positions
    if (round == 0) {
        if (p->slots < 1 || p->slots > kNeighK) REFUSE("%s: slots %d outside 1 .. %d", fn, p->slots, kNeighK);
        if (p->slots + 2 * p->neigh_hyp > kNeighK) REFUSE("%s: slots + 2 * acc_neigh_hyp = %d + 2 * %d > %d positions", fn, p->slots, p->neigh_hyp, kNeighK);
    } else {
        if (p->perturb_keep < 0) REFUSE("%s: acc_perturb_keep is not set (it has no default; rounds after the first need it)", fn);
        if (p->perturb_keep + 1 + 2 * p->neigh_hyp > kNeighK)
            REFUSE("%s: acc_perturb_keep + 1 + 2 * acc_neigh_hyp = %d + 1 + 2 * %d > %d positions", fn, p->perturb_keep, p->neigh_hyp, kNeighK);
    }
    if (gw < 1 || gh < 1 || gw > kNeighMaxSide || gh > kNeighMaxSide) REFUSE("%s: grid %d x %d outside 1 .. %d a side (d^2 stays exact in fp32)", fn, gw, gh, kNeighMaxSide);
    return SFA_OK;
}

int neigh_propose_device(sfa_ctx *ctx, const sfa_neigh_params *p, int n, int Jets, int gw, int gh, int round, const unsigned *seq_start,
                         const unsigned char *consistent, const NeighPlanes &in, const NeighPlanes &out, const NeighWork &wk, hipEvent_t *ev) {
    const NeighDims d{n, Jets, gw, gh, gw * gh};
    NeighSearch q;
    q.skip[0] = p->neigh_skip1; q.skip[1] = p->neigh_skip2;
    for (int t = 0; t < 2; t++) {
        // FLANN's radius is a squared distance, compared in fp32: d^2 (an integer below 2^24, exact) <= (t + 1) * radius (:1505, a float product)
        const float r2 = (float)(t + 1) * p->neigh_hyp_radius;
        q.tdisc[t] = r2 >= (float)kNeighAll ? kNeighAll - 1 : (int)floorf(r2);
    }
    q.quota1 = p->neigh_hyp; q.tryouts = p->hyp_neigh_tryouts; q.method = p->traj_sim_method; q.thres = p->traj_sim_thres;
    q.key0 = p->seed + (unsigned)round;
    SFA_HIP(ctx, hipMemsetAsync(wk.total, 0, (size_t)n * 2 * sizeof(int), ctx->stream));
    const dim3 pix((unsigned)((d.gpl + kNeighThreads - 1) / kNeighThreads), (unsigned)n);
    SFA_TRY(mark_if(ctx, ev, 0));
    hipLaunchKernelGGL(k_neigh_flags, pix, dim3(kNeighThreads), 0, ctx->stream, in.energy, consistent, d, round, q.skip[0], q.skip[1], wk.flags, wk.srcpos, wk.total);
    SFA_HIP(ctx, hipGetLastError());
    SFA_TRY(mark_if(ctx, ev, 1));
    hipLaunchKernelGGL(k_neigh_propose, dim3((unsigned)((d.gpl + kNeighWaves - 1) / kNeighWaves), (unsigned)n), dim3(kNeighThreads), 0, ctx->stream, in.U, in.V,
                       in.energy, wk.flags, wk.srcpos, wk.total, seq_start, d, q, wk.map);
    SFA_HIP(ctx, hipGetLastError());
    SFA_TRY(mark_if(ctx, ev, 2));
    SFA_TRY(neigh_gather(ctx, d, in, out, wk.map));
    SFA_TRY(mark_if(ctx, ev, 3));
    return SFA_OK;
}

// the accepted proposals of one position of one segment take the energy scored at their new place plus weight_jet_estimation of the rate they were born in
// (:1551-1553: the fourth float of the fp32 sum; E holds the sum of the first three, a float widened) and the occlusion word set there
__global__ void __launch_bounds__(kNeighThreads) k_neigh_rescored(const int *__restrict__ tracked, int J, const double *__restrict__ E,
                                                                  const unsigned long long *__restrict__ O, const unsigned char *__restrict__ origin, NeighWeights wt,
                                                                  int gpl, double *__restrict__ energy, unsigned long long *__restrict__ occ) {
    const int p = blockIdx.x * kNeighThreads + threadIdx.x;
    if (p >= gpl || tracked[p] != J) return;
    const float e = (float)E[p] + wt.w[origin[p] & (kNeighK - 1)];
    energy[p] = (double)e;
    occ[p] = O[p];
}

// Position by position, segment by segment: the energy kernels on the list's own flow planes as full-length trajectories (adaptFPS(Jets) of Jets steps is the
// identity: AdaptTab::up with off[t] = t), tracked = Jets where the position was filled in this round, then the merge above.  todo [n][16] (host): positions
// with anything to score
int neigh_rescore_device(sfa_ctx *ctx, const EnergyPlan &plan, int n, const int *tracked, const unsigned char *todo, const void *rec, bool identity, const void *fwd,
                         const void *bwd, const EnergyWork &wk, double *E, unsigned long long *O, const NeighWeights &wt, const NeighPlanes &lists) {
    const size_t gpl = (size_t)plan.gw * plan.gh, pl = (size_t)plan.w * plan.h, hs = (size_t)plan.J * gpl, tap = identity ? 8 : 16;
    for (int s = 0; s < n; s++) {
        const char *rs = static_cast<const char *>(rec) + (size_t)s * (plan.J + 1) * pl * 48;
        const char *fs = fwd ? static_cast<const char *>(fwd) + (size_t)s * plan.J * pl * tap : nullptr;
        const char *bs = bwd ? static_cast<const char *>(bwd) + (size_t)s * plan.J * pl * tap : nullptr;
        for (int k = 0; k < kNeighK; k++) {
            if (!todo[s * kNeighK + k]) continue;
            const size_t sk = (size_t)s * kNeighK + k;
            SFA_TRY(energies_device(ctx, plan, 1, lists.U + sk * hs, lists.V + sk * hs, tracked + sk * gpl, rs, identity, fs, bs, wk, E, O, gpl, nullptr, nullptr, 0));
            hipLaunchKernelGGL(k_neigh_rescored, dim3((unsigned)((gpl + kNeighThreads - 1) / kNeighThreads)), dim3(kNeighThreads), 0, ctx->stream, tracked + sk * gpl,
                               plan.J, E, O, lists.origin + sk * gpl, wt, (int)gpl, lists.energy + sk * gpl, lists.occ + sk * gpl);
            SFA_HIP(ctx, hipGetLastError());
        }
    }
    return SFA_OK;
}

}  // namespace sfa

using namespace sfa;

void sfa_neigh_params_default(sfa_neigh_params *p) {
    if (!p) return;
    *p = sfa_neigh_params{};
    p->traj_sim_thres = 0.1;             // setDefault (dense_tracking.cpp:136-159)
    p->traj_sim_method = 1;
    p->neigh_hyp = 5;
    p->neigh_hyp_radius = 100.0f;
    p->neigh_skip1 = 2;
    p->neigh_skip2 = 4;
    p->hyp_neigh_tryouts = 20;
    p->seed = 0;
    p->slots = 4;                        // two rates with fill-in
    p->perturb_keep = -1;                // no default in setDefault: required from round 1 on
}

void sfa_philox4x32_10(const unsigned ctr[4], const unsigned key[2], unsigned out[4]) { philox4x32_10(ctr, key, out); }

int sfa_philox4x32_10_device(sfa_ctx *ctx, int n, const unsigned *ctr, const unsigned *key, unsigned *out) {
    CHECK_ARGS(ctx && ctr && key && out, "null argument");
    CHECK_ARGS(n >= 1 && n <= (1 << 20), "n outside 1 .. 2^20");
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    DevMem dc, dk, dout;
    SFA_TRY(dc.alloc(ctx, (size_t)n * 16)); SFA_TRY(dk.alloc(ctx, (size_t)n * 8)); SFA_TRY(dout.alloc(ctx, (size_t)n * 16));
    SFA_HIP(ctx, hipMemcpyAsync(dc.p, ctr, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(dk.p, key, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_neigh_philox, dim3((unsigned)((n + kNeighThreads - 1) / kNeighThreads)), dim3(kNeighThreads), 0, ctx->stream,
                       static_cast<const unsigned *>(dc.p), static_cast<const unsigned *>(dk.p), static_cast<unsigned *>(dout.p), n);
    SFA_HIP(ctx, hipGetLastError());
    SFA_HIP(ctx, hipMemcpyAsync(out, dout.p, (size_t)n * 16, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SFA_OK;
}

namespace {

// the five planes of n segments' lists in device memory, uploaded from `h` where given
struct ListMem {
    DevMem U, V, energy, occ, origin;
    int alloc(sfa_ctx *ctx, size_t n, size_t J, size_t gpl) {
        SFA_TRY(U.alloc(ctx, n * kNeighK * J * gpl * 8)); SFA_TRY(V.alloc(ctx, n * kNeighK * J * gpl * 8));
        SFA_TRY(energy.alloc(ctx, n * kNeighK * gpl * 8)); SFA_TRY(occ.alloc(ctx, n * kNeighK * gpl * 8));
        return origin.alloc(ctx, n * kNeighK * gpl);
    }
    NeighPlanes planes() const {
        return NeighPlanes{static_cast<double *>(U.p), static_cast<double *>(V.p), static_cast<double *>(energy.p), static_cast<unsigned long long *>(occ.p),
                           static_cast<unsigned char *>(origin.p)};
    }
    int copy(sfa_ctx *ctx, const sfa_hyp_lists &h, bool up) const {
        void *host[5] = {h.U, h.V, h.energy, h.occ_bits, h.origin};
        void *dev[5] = {U.p, V.p, energy.p, occ.p, origin.p};
        const size_t bytes[5] = {U.bytes, V.bytes, energy.bytes, occ.bytes, origin.bytes};
        for (int i = 0; i < 5; i++)
            SFA_HIP(ctx, up ? hipMemcpyAsync(dev[i], host[i], bytes[i], hipMemcpyHostToDevice, ctx->stream)
                            : hipMemcpyAsync(host[i], dev[i], bytes[i], hipMemcpyDeviceToHost, ctx->stream));
        return SFA_OK;
    }
};

bool lists_given(const sfa_hyp_lists *h) { return h && h->U && h->V && h->energy && h->occ_bits && h->origin; }

}  // namespace

int sfa_prune_hypotheses(sfa_ctx *ctx, int n, int Jets, int gw, int gh, int perturb_keep, const int *selected, const sfa_hyp_lists *in, const sfa_hyp_lists *out,
                         float *stage_ms) {
    CHECK_ARGS(ctx && selected && lists_given(in) && lists_given(out), "null argument");
    CHECK_ARGS(n >= 1 && n <= 2047 && Jets >= 1 && Jets <= 32, "bad sizes (1 <= n <= 2047, 1 <= Jets <= 32)");
    CHECK_ARGS(gw >= 1 && gh >= 1 && gw <= kNeighMaxSide && gh <= kNeighMaxSide, "grid outside 1 .. 2896 a side");
    if (perturb_keep < 0 || perturb_keep + 1 > kNeighK) REFUSE("%s: acc_perturb_keep %d: acc_perturb_keep + 1 outside 1 .. %d positions", __func__, perturb_keep, kNeighK);
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const size_t gpl = (size_t)gw * gh;
    ListMem a, b;
    DevMem dsel, dmap;
    SFA_TRY(a.alloc(ctx, n, Jets, gpl)); SFA_TRY(b.alloc(ctx, n, Jets, gpl));
    SFA_TRY(dsel.alloc(ctx, (size_t)n * gpl * 4)); SFA_TRY(dmap.alloc(ctx, (size_t)n * kNeighK * gpl * 4));
    SFA_TRY(a.copy(ctx, *in, true));
    SFA_HIP(ctx, hipMemcpyAsync(dsel.p, selected, (size_t)n * gpl * 4, hipMemcpyHostToDevice, ctx->stream));
    StageEvents ev;
    if (stage_ms) SFA_TRY(ev.make(ctx, 3));
    SFA_TRY(neigh_prune_device(ctx, n, Jets, gw, gh, perturb_keep, static_cast<const int *>(dsel.p), a.planes(), b.planes(), static_cast<int *>(dmap.p),
                               stage_ms ? ev.e : nullptr));
    SFA_TRY(b.copy(ctx, *out, false));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stage_ms) SFA_TRY(ev.read(ctx, 3, stage_ms));
    return SFA_OK;
}

int sfa_neighbour_proposals(sfa_ctx *ctx, const sfa_neigh_params *p, int n, int Jets, int gw, int gh, int round, const unsigned *sequence_start,
                            const unsigned char *consistent, const sfa_hyp_lists *in, const sfa_hyp_lists *out, int *src_pixel, unsigned char *src_position,
                            int *accepted, float *stage_ms) {
    CHECK_ARGS(ctx && p && sequence_start && lists_given(in) && lists_given(out) && src_pixel && src_position && accepted, "null argument");
    CHECK_ARGS(n >= 1 && n <= 2047 && Jets >= 1 && Jets <= 32, "bad sizes (1 <= n <= 2047, 1 <= Jets <= 32)");
    CHECK_ARGS(round >= 0, "round < 0");
    CHECK_ARGS(round > 0 || consistent, "round 0 needs the consistent mask");
    SFA_TRY(neigh_check(ctx, __func__, p, gw, gh, round));
    {   // the lists keep to the capacity the limits count on: no hypothesis at or beyond position `slots` (round 0) / acc_perturb_keep + 1 (later)
        const int cap = round == 0 ? p->slots : p->perturb_keep + 1;
        const size_t g = (size_t)gw * gh;
        for (int s = 0; s < n; s++)
            for (int k = cap; k < kNeighK; k++)
                for (size_t i = ((size_t)s * kNeighK + k) * g; i < ((size_t)s * kNeighK + k + 1) * g; i++)
                    if (in->energy[i] < HUGE_VAL)
                        REFUSE("%s: start_jet %d holds a hypothesis at position %d; round %d's lists end at position %d (%s)", __func__, s, k, round, cap - 1,
                               round == 0 ? "slots" : "acc_perturb_keep + 1");
    }
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    const size_t gpl = (size_t)gw * gh, nm = (size_t)n * kNeighK * gpl;
    ListMem a, b;
    DevMem dseq, dcons, dflags, dsrc, dtot, dmap;
    SFA_TRY(a.alloc(ctx, n, Jets, gpl)); SFA_TRY(b.alloc(ctx, n, Jets, gpl));
    SFA_TRY(dseq.alloc(ctx, (size_t)n * 4)); SFA_TRY(dcons.alloc(ctx, (size_t)n * gpl)); SFA_TRY(dflags.alloc(ctx, (size_t)n * gpl));
    SFA_TRY(dsrc.alloc(ctx, (size_t)n * gpl)); SFA_TRY(dtot.alloc(ctx, (size_t)n * 8)); SFA_TRY(dmap.alloc(ctx, nm * 4));
    SFA_TRY(a.copy(ctx, *in, true));
    SFA_HIP(ctx, hipMemcpyAsync(dseq.p, sequence_start, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    if (round == 0) SFA_HIP(ctx, hipMemcpyAsync(dcons.p, consistent, (size_t)n * gpl, hipMemcpyHostToDevice, ctx->stream));
    NeighWork wk{static_cast<unsigned char *>(dflags.p), static_cast<unsigned char *>(dsrc.p), static_cast<int *>(dtot.p), static_cast<int *>(dmap.p)};
    StageEvents ev;
    if (stage_ms) SFA_TRY(ev.make(ctx, 4));
    SFA_TRY(neigh_propose_device(ctx, p, n, Jets, gw, gh, round, static_cast<const unsigned *>(dseq.p), static_cast<const unsigned char *>(dcons.p), a.planes(),
                                 b.planes(), wk, stage_ms ? ev.e : nullptr));
    SFA_TRY(b.copy(ctx, *out, false));
    SFA_HIP(ctx, hipMemcpyAsync(src_pixel, dmap.p, nm * 4, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stage_ms) SFA_TRY(ev.read(ctx, 4, stage_ms));
    // the map -> the accepted proposals' source pixel and position; -1 / 0 at every other position
    for (int s = 0; s < n; s++) {
        int acc = 0;
        for (size_t i = (size_t)s * kNeighK * gpl; i < (size_t)(s + 1) * kNeighK * gpl; i++) {
            const int m = src_pixel[i];
            const bool is_new = m >= 0 && (m & kNeighNew);
            src_pixel[i] = is_new ? (m & ~kNeighNew) >> 4 : -1;
            src_position[i] = is_new ? (unsigned char)(m & (kNeighK - 1)) : 0;
            acc += is_new;
        }
        accepted[s] = acc;
    }
    return SFA_OK;
}

int sfa_rescore_proposals(sfa_ctx *ctx, const sfa_energy_params *p, int n, int Jets, int w, int h, int stride, const float *const *frames,
                          const float *const *fwd_u, const float *const *fwd_v, const float *const *bwd_u, const float *const *bwd_v, const float *slot_weight,
                          const int *src_pixel, const sfa_hyp_lists *lists, float *stage_ms) {
    CHECK_ARGS(ctx && p && frames && slot_weight && src_pixel && lists_given(lists), "null argument");
    CHECK_ARGS(n >= 1 && Jets >= 1 && Jets <= 32 && (long)n * (Jets + 1) * 3 <= 65535 && w >= 1 && stride >= w,
               "bad sizes (n >= 1 with n (Jets + 1) <= 21845, 1 <= Jets <= 32, w >= 1, stride >= w)");
    CHECK_ARGS(h >= 4, "the reference's vertical 5-tap derivative needs h >= 4");
    bool flows;
    SFA_TRY(energy_planes_check(ctx, __func__, false, (size_t)n * (Jets + 1), frames, (size_t)n * Jets, fwd_u, fwd_v, bwd_u, bwd_v, &flows));
    EnergyPlan plan;
    SFA_TRY(energy_plan(ctx, p, Jets, Jets, w, h, &plan));
    plan.a.weight = 0.0f;                                                       // the rate's weight is added per pixel, by the origin
    const size_t gpl = (size_t)plan.gw * plan.gh, nk = (size_t)n * kNeighK * gpl;
    // which positions were filled in this round, and by hypotheses born in which slot
    std::vector<int> tracked(nk);
    std::vector<unsigned char> todo((size_t)n * kNeighK, 0);
    for (size_t i = 0; i < nk; i++) {
        const bool is_new = src_pixel[i] >= 0;
        tracked[i] = is_new ? Jets : 0;
        if (!is_new) continue;
        if ((lists->origin[i] & 0x7f) >= kNeighK) REFUSE("%s: origin %d of a proposal names no slot (0 .. %d)", __func__, lists->origin[i] & 0x7f, kNeighK - 1);
        todo[i / gpl] = 1;
    }
    NeighWeights wt;
    for (int k = 0; k < kNeighK; k++) wt.w[k] = slot_weight[k];

    SFA_HIP(ctx, hipSetDevice(ctx->device));
    sfa_jet_source src;                                                         // the flows are w x h float planes of the frames' stride
    sfa_jet_source_default(&src, w, h, stride);
    ListMem a;
    EnergyMem in;                                                               // the scratch of one segment: the positions are scored one at a time
    DevMem dtr, dE, dO;
    SFA_TRY(a.alloc(ctx, n, Jets, gpl));
    SFA_TRY(in.alloc(ctx, plan, n, 1, flows ? &src : nullptr, true));
    SFA_TRY(dtr.alloc(ctx, nk * 4)); SFA_TRY(dE.alloc(ctx, gpl * 8)); SFA_TRY(dO.alloc(ctx, gpl * 8));
    SFA_TRY(a.copy(ctx, *lists, true));
    SFA_TRY(copy_on(ctx, dtr.p, tracked.data(), nk * 4, hipMemcpyHostToDevice));
    SFA_TRY(in.upload(ctx, plan, frames, stride, fwd_u, fwd_v, bwd_u, bwd_v));
    StageEvents ev;
    if (stage_ms) SFA_TRY(ev.make(ctx, 2));
    SFA_TRY(ev.mark(ctx, 0));
    SFA_TRY(neigh_rescore_device(ctx, plan, n, static_cast<const int *>(dtr.p), todo.data(), in.rec.p, true, in.fwd.p, in.bwd.p, in.work(),
                                 static_cast<double *>(dE.p), static_cast<unsigned long long *>(dO.p), wt, a.planes()));
    SFA_TRY(ev.mark(ctx, 1));
    SFA_HIP(ctx, hipMemcpyAsync(lists->energy, a.energy.p, a.energy.bytes, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipMemcpyAsync(lists->occ_bits, a.occ.p, a.occ.bytes, hipMemcpyDeviceToHost, ctx->stream));
    SFA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (stage_ms) SFA_TRY(ev.read(ctx, 2, stage_ms));
    return SFA_OK;
}
