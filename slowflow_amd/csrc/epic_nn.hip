// epic_nn.hip -- sfa_epic_nearest_seeds_batch: EpicFlow's geodesic k nearest seeds (host/epic.cpp: epic_nearest_seeds, epic_aux.cpp:44-380) for a batch of
// images of one size, operation for operation, so that labels, neighbour indices and distance bit patterns equal the host's.
//   k_epic_init, k_epic_seed_label, k_epic_seed_cost   dmap = 0x7F7F7F7F, labels = -1, then the seeds (atomicMax: the later seed of a pixel wins)
//   k_epic_sweeps        one workgroup per image runs ALL sweeps of the distance transform.  In the sweep's own orientation cell (u, v) reads only (u, v - 1) and
//                        (u - 1, v), both on the anti-diagonal before its own, so walking the diagonals with a barrier between them is the raster order (the scheme
//                        of k_trws, fuse.hip).  A diagonal hands its (distance, label) on through LDS; cost and the old value of a thread's first cell are fetched
//                        one diagonal ahead (a diagonal longer than the workgroup loads its further cells in place).  The largest decrease of a sweep is a maximum (order-independent), and the `end_iter` rule is applied by the workgroup itself
//   k_epic_count_borders, k_epic_insert    the region graph: border pairs counted, then inserted into an open-addressing table sized from that count -- a 64-bit
//                        key CAS plus atomicMin on the length's bit pattern (lengths are sums of distances, +0 and above once border_pairs has turned a -0.0 into +0.0: unsigned order = float order)
//   k_epic_degrees, k_epic_rows, k_epic_fill, k_epic_sort_rows   adjacency rows in ascending neighbour index (keys are unique: the result does not depend on the
//                        order the atomics ran in), the largest degree
//   k_epic_dijkstra      one thread per (image, seed): `done` a dense row of ns floats, the heap (epic_heap.h: libstdc++'s push_heap / pop_heap) in global memory,
//                        its capacity the bound 1 + min((nn - 1) maxdeg, 2 E): every push follows the expansion of one directed edge, at most nn - 1 nodes expand
//   k_epic_search        the compact mode's search (sfa_ctx_set_epic_search): the same walk for one slice of an image's seeds, over a dense row or a sparse
//                        open-addressing map per seed; the slices of a sub-batch run one after the other in one workspace (epic_nn_plan.h)
//   k_epic_assemble      query q takes the list of the seed whose region its pixel lies in, plus its own distance
// epic_nn_device (sfa_internal.h) is the stage on buffers already in device memory, with the neighbour count per image; the entry point wraps it (allocate, upload,
// call, download, wait) and runs the batch in sub-batches that fit a workspace budget; an image that does not fit alone is flagged, never truncated.  In the
// default mode an image fits when its ns * ns floats and all its heaps do; in the compact mode when one 64-seed workgroup's search does.
#include <algorithm>
#include <climits>
#include <cstring>

#include "epic_heap.h"
#include "epic_nn_plan.h"
#include "sfa_device.h"
#include "sfa_internal.h"

namespace sfa {
namespace {

constexpr unsigned kHugeBits = 0x7F7F7F7Fu;                          // memset(.., 0x7F, ..) of the reference
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr int kSweepThreads = 512, kMaxShortSide = 4000;             // LDS: two diagonals of (distance, label) = 16 bytes per cell of the shorter side
constexpr int kMaxIter = 40;
constexpr int kMaxSubBatch = 4096;                                   // images per launch (the grids' second dimension)
constexpr long long kMaxPixels = 1ll << 29;                           // twice the border pairs (at most two per pixel) still index a table of 2^31 slots

// What the kernels know of one image: all pointers device memory
struct EpicImg {
    const float *cost; float *dmap; int *lab; const int *seeds; int ns, nn;
    unsigned *cnt;                                                   // [0] border pairs, [1] edges E, [2] largest degree, [3] heap overflow (never, by the bound)
    unsigned long long *keys; unsigned *lens; int log_cap;           // the table: 1 << log_cap slots
    int *deg, *rowptr, *cursor; int *adj_n; float *adj_l;
    float *done; epic_heap_item *heap; int heap_cap;
    int *nnf; float *dis; int *out_index; float *out_dist;
};

__global__ void k_epic_init(const EpicImg *imgs, int npix) {
    const EpicImg im = imgs[blockIdx.y];
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < npix) { im.dmap[p] = __uint_as_float(kHugeBits); im.lab[p] = -1; }
    if (p < 4) im.cnt[p] = 0;
}

__global__ void k_epic_seed_label(const EpicImg *imgs, int tx) {
    const EpicImg im = imgs[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < im.ns) atomicMax(&im.lab[im.seeds[2 * i] + im.seeds[2 * i + 1] * tx], i);
}

__global__ void k_epic_seed_cost(const EpicImg *imgs, int tx) {
    const EpicImg im = imgs[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= im.ns) return;
    const int p = im.seeds[2 * i] + im.seeds[2 * i + 1] * tx;
    if (im.lab[p] == i) im.dmap[p] = im.cost[p];
}

struct SweepCell { float C, a; int l; int p; };

__global__ void __launch_bounds__(kSweepThreads) k_epic_sweeps(const EpicImg *imgs, int tx, int ty) {
    extern __shared__ float lds[];
    __shared__ unsigned s_change[2];
    const EpicImg im = imgs[blockIdx.x];
    const int M = min(tx, ty), tid = threadIdx.x, ndiag = tx + ty - 1;
    float *pt = lds;                                                 // [2][M] distances of the last two diagonals
    int *pl = reinterpret_cast<int *>(lds + 2 * M);                  // [2][M] their labels
    const bool kx = tx <= ty;                                        // a diagonal's cells are told apart by u where the image is narrow, else by v
    const float INF = __uint_as_float(0x7F800000u);
    int i = 0, end_iter = 4;
    while (++i <= end_iter) {                                        // weighted_distance_transform (epic_aux.cpp:160-180)
        const int dir = i & 3;
        const bool xpos = dir == 1 || dir == 2, ypos = dir == 0 || dir == 1;       // {-1,1,1,-1} / {1,1,-1,-1}
        if (tid == 0) s_change[i & 1] = 0;
        __syncthreads();                                             // the stores of the sweep before are visible to this one's loads
        auto fetch = [&](int d, int c) {
            SweepCell s{0.0f, 0.0f, -1, -1};
            const int ulo = max(0, d - (ty - 1)), uhi = min(d, tx - 1);
            if (c > uhi - ulo) return s;
            const int u = ulo + c, v = d - u;
            s.p = (xpos ? u : tx - 1 - u) + (ypos ? v : ty - 1 - v) * tx;
            s.C = im.cost[s.p]; s.a = im.dmap[s.p]; s.l = im.lab[s.p];
            return s;
        };
        float mx = 0.0f;
        SweepCell pre = fetch(0, tid);
        for (int d = 0; d < ndiag; d++) {
            const int ulo = max(0, d - (ty - 1)), uhi = min(d, tx - 1), len = uhi - ulo + 1;
            const SweepCell first = pre;
            if (d + 1 < ndiag) pre = fetch(d + 1, tid);              // the next diagonal's operands: in flight across the barrier
            const float *rt = pt + ((d & 1) ^ 1) * M;
            const int *rl = pl + ((d & 1) ^ 1) * M;
            float *wt = pt + (d & 1) * M;
            int *wl = pl + (d & 1) * M;
            for (int c = tid; c < len; c += kSweepThreads) {
                const SweepCell s = c == tid ? first : fetch(d, c);
                const int u = ulo + c, v = d - u;
                float t1 = INF, t2 = INF;
                int l1 = -1, l2 = -1;
                if (v > 0) { const int k = kx ? u : v - 1; t1 = rt[k]; l1 = rl[k]; }
                if (u > 0) { const int k = kx ? u - 1 : v; t2 = rt[k]; l2 = rl[k]; }
                const float dt12 = fabsf(t1 - t2);
                float t0;
                int l0;
                if (dt12 > s.C) {                                    // degenerate case: the front comes from one side only
                    if (t1 < t2) { t0 = t1 + s.C; l0 = l1; } else { t0 = t2 + s.C; l0 = l2; }
                } else {
                    t0 = 0.5f * (t1 + t2 + sqrt_rn(2 * s.C * s.C - dt12 * dt12));
                    l0 = (t1 < t2) ? l1 : l2;
                }
                float a = s.a;
                int l = s.l;
                if (t0 < a) {
                    mx = fmaxf(mx, a - t0);
                    a = t0; l = l0;
                    im.dmap[s.p] = a; im.lab[s.p] = l;
                }
                const int k0 = kx ? u : v;
                wt[k0] = a; wl[k0] = l;
            }
            __syncthreads();
        }
        if (mx > 0.0f) atomicMax(&s_change[i & 1], __float_as_uint(mx));       // decreases are positive: the unsigned order is the float order
        __syncthreads();
        if (__uint_as_float(s_change[i & 1]) > 1.0f) end_iter = min(kMaxIter, i + 3);     // finish the turn
    }
}

// the (up to two) border pairs of pixel o = (i, j), i, j >= 1, with both labels in 0 .. ns - 1: key = smaller label | larger << 32, length = the sum of the two distances
__device__ inline int border_pairs(const EpicImg &im, int tx, int o, unsigned long long key[2], float len[2]) {
    const int l0 = im.lab[o];
    if (l0 < 0 || l0 >= im.ns) return 0;
    int n = 0;
    const int nb[2] = {o - 1, o - tx};
    for (int k = 0; k < 2; k++) {
        const int l = im.lab[nb[k]];
        if (l == l0 || l < 0 || l >= im.ns) continue;
        key[n] = (unsigned long long)min(l0, l) | ((unsigned long long)max(l0, l) << 32);
        len[n] = (im.dmap[o] + im.dmap[nb[k]]) + 0.0f;                // -0.0 (two seeds' pixels of cost -0.0) becomes +0.0: k_epic_insert orders lengths by their bits
        n++;
    }
    return n;
}

__global__ void k_epic_count_borders(const EpicImg *imgs, int tx, int ty) {
    __shared__ unsigned s_n;
    const EpicImg im = imgs[blockIdx.y];
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int q = blockIdx.x * blockDim.x + threadIdx.x;             // over the (tx - 1) x (ty - 1) pixels with i, j >= 1
    if (q < (tx - 1) * (ty - 1)) {
        unsigned long long key[2];
        float len[2];
        const int n = border_pairs(im, tx, 1 + q % (tx - 1) + (1 + q / (tx - 1)) * tx, key, len);
        if (n) atomicAdd(&s_n, (unsigned)n);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(&im.cnt[0], s_n);
}

__global__ void k_epic_insert(const EpicImg *imgs, int tx, int ty) {
    const EpicImg im = imgs[blockIdx.y];
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (tx - 1) * (ty - 1)) return;
    unsigned long long key[2];
    float len[2];
    const int n = border_pairs(im, tx, 1 + q % (tx - 1) + (1 + q / (tx - 1)) * tx, key, len);
    const unsigned mask = (1u << im.log_cap) - 1;
    for (int k = 0; k < n; k++) {
        unsigned h = (unsigned)((key[k] * 0x9E3779B97F4A7C15ull) >> (64 - im.log_cap));
        for (unsigned probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {        // the table holds twice the pairs: a free slot is met
            const unsigned long long old = atomicCAS(&im.keys[h], kEmptyKey, key[k]);
            if (old == kEmptyKey) atomicAdd(&im.cnt[1], 1u);
            if (old == kEmptyKey || old == key[k]) { atomicMin(&im.lens[h], __float_as_uint(len[k])); break; }
        }
    }
}

__global__ void k_epic_degrees(const EpicImg *imgs) {
    const EpicImg im = imgs[blockIdx.y];
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (1u << im.log_cap) || im.keys[s] == kEmptyKey) return;
    atomicAdd(&im.deg[(int)(im.keys[s] & 0xffffffffu)], 1);
    atomicAdd(&im.deg[(int)(im.keys[s] >> 32)], 1);
}

// rowptr = exclusive scan of deg over the ns seeds of the block's image, cursor = 0, cnt[2] = the largest degree
__global__ void __launch_bounds__(256) k_epic_rows(const EpicImg *imgs) {
    __shared__ int s_sum[256];
    __shared__ int s_max;
    const EpicImg im = imgs[blockIdx.x];
    const int tid = threadIdx.x, per = (im.ns + 255) / 256, lo = min(im.ns, tid * per), hi = min(im.ns, lo + per);
    if (tid == 0) s_max = 0;
    int sum = 0, mx = 0;
    for (int k = lo; k < hi; k++) { sum += im.deg[k]; mx = max(mx, im.deg[k]); }
    s_sum[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off *= 2) {                         // inclusive scan of the 256 partial sums
        const int v = tid >= off ? s_sum[tid - off] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    atomicMax(&s_max, mx);
    int run = s_sum[tid] - sum;
    for (int k = lo; k < hi; k++) { im.rowptr[k] = run; run += im.deg[k]; im.cursor[k] = 0; }
    __syncthreads();
    if (tid == 255) im.rowptr[im.ns] = s_sum[255];
    if (tid == 0) im.cnt[2] = (unsigned)s_max;
}

__global__ void k_epic_fill(const EpicImg *imgs) {
    const EpicImg im = imgs[blockIdx.y];
    const unsigned s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (1u << im.log_cap) || im.keys[s] == kEmptyKey) return;
    const int a = (int)(im.keys[s] & 0xffffffffu), b = (int)(im.keys[s] >> 32);
    const float len = __uint_as_float(im.lens[s]);
    const int pa = im.rowptr[a] + atomicAdd(&im.cursor[a], 1), pb = im.rowptr[b] + atomicAdd(&im.cursor[b], 1);
    im.adj_n[pa] = b; im.adj_l[pa] = len;
    im.adj_n[pb] = a; im.adj_l[pb] = len;
}

// every row into ascending neighbour index (in-place heapsort: a row can be long, and its neighbours are distinct)
__global__ void k_epic_sort_rows(const EpicImg *imgs) {
    const EpicImg im = imgs[blockIdx.y];
    const int node = blockIdx.x * blockDim.x + threadIdx.x;
    if (node >= im.ns) return;
    int *kn = im.adj_n + im.rowptr[node];
    float *kl = im.adj_l + im.rowptr[node];
    const int n = im.rowptr[node + 1] - im.rowptr[node];
    auto sift = [&](int root, int end) {                             // max-heap on the neighbour index over [0, end)
        const int vn = kn[root];
        const float vl = kl[root];
        int hole = root;
        for (int child = 2 * hole + 1; child < end; child = 2 * hole + 1) {
            if (child + 1 < end && kn[child + 1] > kn[child]) child++;
            if (kn[child] <= vn) break;
            kn[hole] = kn[child]; kl[hole] = kl[child];
            hole = child;
        }
        kn[hole] = vn; kl[hole] = vl;
    };
    for (int r = n / 2 - 1; r >= 0; r--) sift(r, n);
    for (int end = n - 1; end > 0; end--) {
        const int tn = kn[0]; const float tl = kl[0];
        kn[0] = kn[end]; kl[0] = kl[end];
        kn[end] = tn; kl[end] = tl;
        sift(0, end);
    }
}

struct StridedHeap {                                                 // entry k of a thread's heap lies `stride` entries after entry k - 1: the threads of an image interleave
    epic_heap_item *p; size_t stride;
    __device__ epic_heap_item &operator[](int k) const { return p[(size_t)k * stride]; }
};

__global__ void __launch_bounds__(64) k_epic_dijkstra(const EpicImg *imgs) {                  // epic_aux.cpp:44-87
    const EpicImg im = imgs[blockIdx.y];
    const int nn = im.nn;
    const int seed = blockIdx.x * blockDim.x + threadIdx.x;
    if (seed >= im.ns) return;
    float *done = im.done + (size_t)seed * im.ns;                    // cleared to 0x7F bytes by the host
    StridedHeap heap{im.heap + seed, (size_t)im.ns};
    int size = 0, n = 0;
    epic_heap_push(heap, size, epic_heap_item{seed, 0.f});
    done[seed] = 0;
    while (size > 0) {
        const epic_heap_item cur = epic_heap_pop(heap, size);
        if (cur.dis > done[cur.node]) continue;
        im.nnf[(size_t)seed * nn + n] = cur.node;
        im.dis[(size_t)seed * nn + n] = cur.dis;
        if (++n >= nn) break;
        for (int e = im.rowptr[cur.node]; e < im.rowptr[cur.node + 1]; e++) {
            const int to = im.adj_n[e];
            const float newd = cur.dis + im.adj_l[e];
            if (newd >= done[to]) continue;
            if (size >= im.heap_cap) { atomicAdd(&im.cnt[3], 1u); return; }       // cannot happen (the bound above); reported, never written past the end
            epic_heap_push(heap, size, epic_heap_item{to, newd});
            done[to] = newd;
        }
    }
}

// ---- the compact search (sfa_ctx_set_epic_search, epic_nn_plan.h): k_epic_dijkstra's walk, statement for statement, for the seeds first .. first + count - 1
// of one image, over a visited set of either form.  A set answers find(node) with the place of the node's distance and the distance held there, 0x7F7F7F7F
// for a node never written, so every comparison -- and with them the heap's order and every output bit -- is the default kernel's.
struct DenseSet {                                                    // the default mode's row, of this slice
    float *row;
    struct Ref { float *p; float value; };
    __device__ DenseSet(void *ws, int local, int, int ns, int) : row(static_cast<float *>(ws) + (size_t)local * ns) {}
    __device__ Ref find(int node) const { return Ref{row + node, row[node]}; }
    __device__ bool store(const Ref &r, int, float d) const { *r.p = d; return true; }
};
#ifndef SFA_EPIC_NN_INTERLEAVED
#define SFA_EPIC_NN_INTERLEAVED 0
#endif
// node -> distance bits: the key in a slot's upper half, all ones = empty; a multiplicative hash and linear probing.  A thread's slots lie together, so a
// probe sequence stays in one or two cache lines.  SFA_EPIC_NN_INTERLEAVED (what-if): slot k of a thread lies `count` slots after its slot k - 1, like
// StridedHeap's entries; DESIGN.md 8 holds both measurements
struct SparseSet {
    unsigned long long *slot; size_t stride; unsigned mask; int shift;           // 1 <= log_slots <= 31 (epic_nn_plan.h: searchable)
    struct Ref { unsigned long long *p; float value; };
    __device__ SparseSet(void *ws, int local, int count, int, int log_slots)
        : slot(static_cast<unsigned long long *>(ws) + (SFA_EPIC_NN_INTERLEAVED ? (size_t)local : (size_t)local << log_slots)),
          stride(SFA_EPIC_NN_INTERLEAVED ? (size_t)count : 1), mask((1u << log_slots) - 1), shift(32 - log_slots) {}
    __device__ Ref find(int node) const {
        unsigned h = ((unsigned)node * 0x9E3779B1u) >> shift;
        for (unsigned probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {  // bounded by the capacity
            unsigned long long *p = slot + h * stride;
            const unsigned long long s = *p;
            const unsigned key = (unsigned)(s >> 32);
            if (key == (unsigned)node) return Ref{p, __uint_as_float((unsigned)s)};
            if (key == 0xFFFFFFFFu) return Ref{p, __uint_as_float(kHugeBits)};
        }
        return Ref{nullptr, __uint_as_float(kHugeBits)};             // a full map without the node (the load is at most 1/2: never)
    }
    __device__ bool store(const Ref &r, int node, float d) const {
        if (!r.p) return false;
        *r.p = ((unsigned long long)(unsigned)node << 32) | __float_as_uint(d);
        return true;
    }
};

template <class Set>
__global__ void __launch_bounds__(kEpicNnGroup) k_epic_search(const EpicImg *imgs, int image, int first, int count, void *ws, epic_heap_item *heaps, int log_slots) {
    const EpicImg im = imgs[image];
    const int nn = im.nn;
    const int local = blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= count) return;
    const int seed = first + local;
    const Set done(ws, local, count, im.ns, log_slots);              // cleared by the host: 0x7F bytes (dense), 0xFF bytes (sparse)
    StridedHeap heap{heaps + local, (size_t)count};
    int size = 0, n = 0;
    epic_heap_push(heap, size, epic_heap_item{seed, 0.f});
    if (!done.store(done.find(seed), seed, 0)) { atomicAdd(&im.cnt[3], 1u); return; }
    while (size > 0) {
        const epic_heap_item cur = epic_heap_pop(heap, size);
        if (cur.dis > done.find(cur.node).value) continue;
        im.nnf[(size_t)seed * nn + n] = cur.node;
        im.dis[(size_t)seed * nn + n] = cur.dis;
        if (++n >= nn) break;
        for (int e = im.rowptr[cur.node]; e < im.rowptr[cur.node + 1]; e++) {
            const int to = im.adj_n[e];
            const float newd = cur.dis + im.adj_l[e];
            const typename Set::Ref r = done.find(to);
            if (newd >= r.value) continue;
            if (size >= im.heap_cap || !r.p) { atomicAdd(&im.cnt[3], 1u); return; }      // cannot happen (the bounds of epic_nn_plan.h); reported, never written past the end
            epic_heap_push(heap, size, epic_heap_item{to, newd});
            done.store(r, to, newd);
        }
    }
}

__global__ void k_epic_assemble(const EpicImg *imgs, int tx) {                // epic_aux.cpp:366-374
    const EpicImg im = imgs[blockIdx.y];
    const int nn = im.nn;
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (size_t)im.ns * nn) return;
    const int q = (int)(k / nn), j = (int)(k % nn);
    const int p = im.seeds[2 * q] + im.seeds[2 * q + 1] * tx;
    const int s = im.lab[p];
    if (s < 0 || s >= im.ns) { im.out_index[k] = -1; im.out_dist[k] = __uint_as_float(kHugeBits); return; }    // (a seed's pixel carries a seed's label)
    im.out_index[k] = im.nnf[(size_t)s * nn + j];
    im.out_dist[k] = im.dmap[p] + im.dis[(size_t)s * nn + j];
}

inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }
inline int blocks(size_t n, int per) { return (int)((n + per - 1) / per); }

// one allocation cut into 256-byte aligned pieces
struct Bump {
    char *base = nullptr; size_t used = 0;
    template <class T> T *take(size_t count) { T *r = reinterpret_cast<T *>(base + used); used += al(count * sizeof(T)); return r; }
};

}  // namespace
}  // namespace sfa

using namespace sfa;

// The stage on buffers already in device memory (sfa_internal.h).  What it allocates besides -- the records, dmap, the search's own lists, then the table and
// rows, then `done` and the heaps, each sized by the counts the host reads in between -- stays within `budget`; the leading *done images that fit whole are
// computed, and when the call returns the stream has been waited for
int sfa::epic_nn_device(sfa_ctx *ctx, const char *fn, int m, int w, int h, const EpicNnIo *io, size_t budget, int *done_out, size_t *estimate, float ms_out[5], long long info[4]) {
    *done_out = 0;
    const size_t npix = (size_t)w * h;
    hipStream_t st = ctx->stream;
    // what an image needs here: before anything ran (record, dmap, the search's lists, counters), once its border pairs are counted (table, degrees), once
    // its graph is known (rows, search)
    auto need1 = [&](int k) { return al(sizeof(EpicImg)) + al(npix * 4) + 2 * al((size_t)io[k].ns * io[k].nn * 4) + al(16); };
    auto log_cap_of = [](unsigned pairs) { int l = 4; while (l < 31 && (1ull << l) < 2ull * pairs) l++; return l; };
    auto need2 = [&](int k, unsigned pairs) { return al((size_t)8 << log_cap_of(pairs)) + al((size_t)4 << log_cap_of(pairs)) + 2 * al((size_t)io[k].ns * 4) + al(((size_t)io[k].ns + 1) * 4); };
    auto heap_cap_of = [&](int k, unsigned E, unsigned maxdeg) { return (size_t)1 + std::min((size_t)(io[k].nn - 1) * maxdeg, (size_t)2 * E); };
    auto need3 = [&](int k, unsigned E, unsigned maxdeg) {
        return 2 * al((size_t)2 * E * 4 + 4) + al((size_t)io[k].ns * io[k].ns * 4) + al((size_t)io[k].ns * heap_cap_of(k, E, maxdeg) * sizeof(epic_heap_item));
    };
    // the kernels' time by group (sfa_epic_nn_stage_ms): events around them, read after each stage's wait
    struct Events {
        hipEvent_t e[10] = {};
        ~Events() { for (hipEvent_t v : e) if (v) (void)hipEventDestroy(v); }
    } ev;
    for (hipEvent_t &v : ev.e) SFA_HIP(ctx, hipEventCreate(&v));
    auto mark = [&](int k) { (void)hipEventRecord(ev.e[k], st); };
    auto spent = [&](int slot, int k) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev.e[k], ev.e[k + 1]) == hipSuccess) ms_out[slot] += ms; };
    // ---- stage 1: seeds, sweeps, border pairs ---------------------------------------------------------------------------------------------------------
    DevMem mem1, mem2, mem3;
    size_t bytes1 = 0;
    for (int k = 0; k < m; k++) bytes1 += need1(k);
    if (bytes1 > budget) return SFA_OK;
    SFA_TRY(mem1.alloc(ctx, bytes1));
    Bump b1{static_cast<char *>(mem1.p)};
    EpicImg *d_imgs = b1.take<EpicImg>(m);
    std::vector<EpicImg> imgs(m);
    std::vector<unsigned *> cnts(m);
    int ns_max = 0;
    for (int k = 0; k < m; k++) {
        EpicImg &im = imgs[k];
        memset(&im, 0, sizeof im);
        const size_t list = (size_t)io[k].ns * io[k].nn;
        im.cost = io[k].cost; im.seeds = io[k].seeds; im.ns = io[k].ns; im.nn = io[k].nn;
        im.dmap = b1.take<float>(npix); im.lab = io[k].lab;
        im.nnf = b1.take<int>(list); im.dis = b1.take<float>(list);
        im.out_index = io[k].index; im.out_dist = io[k].dist;
        im.cnt = cnts[k] = b1.take<unsigned>(4);
        SFA_HIP(ctx, hipMemsetAsync(im.nnf, 0xFF, list * 4, st));                     // -1
        SFA_HIP(ctx, hipMemsetAsync(im.dis, 0x7F, list * 4, st));                     // 0x7F7F7F7F
        ns_max = std::max(ns_max, im.ns);
    }
    auto put_imgs = [&](int count) { return hipMemcpyAsync(d_imgs, imgs.data(), (size_t)count * sizeof(EpicImg), hipMemcpyHostToDevice, st); };
    SFA_HIP(ctx, put_imgs(m));
    mark(0);
    hipLaunchKernelGGL(k_epic_init, dim3(blocks(std::max(npix, (size_t)4), 256), m), dim3(256), 0, st, d_imgs, (int)npix);
    hipLaunchKernelGGL(k_epic_seed_label, dim3(blocks(ns_max, 256), m), dim3(256), 0, st, d_imgs, w);
    hipLaunchKernelGGL(k_epic_seed_cost, dim3(blocks(ns_max, 256), m), dim3(256), 0, st, d_imgs, w);
    mark(1);
    hipLaunchKernelGGL(k_epic_sweeps, dim3(m), dim3(kSweepThreads), (size_t)16 * std::min(w, h), st, d_imgs, w, h);
    mark(2);
    const size_t inner = (size_t)(w - 1) * (h - 1);                  // pixels with a left and an upper neighbour
    if (inner) hipLaunchKernelGGL(k_epic_count_borders, dim3(blocks(inner, 256), m), dim3(256), 0, st, d_imgs, w, h);
    mark(3);
    std::vector<unsigned> cnt((size_t)4 * m);
    for (int k = 0; k < m; k++) SFA_HIP(ctx, hipMemcpyAsync(&cnt[4 * k], cnts[k], 16, hipMemcpyDeviceToHost, st));
    SFA_TRY(sfa_ctx_sync(ctx));
    spent(0, 0); spent(1, 1); spent(2, 2);
    // ---- stage 2: the region graph of the images whose tables fit too ----------------------------------------------------------------------------------
    int k1 = 0;
    size_t bytes2 = 0;
    for (; k1 < m; k1++) {
        const size_t add = need2(k1, cnt[4 * k1]);
        if (bytes1 + bytes2 + add > budget) break;
        bytes2 += add;
    }
    if (k1 == 0) return SFA_OK;
    SFA_TRY(mem2.alloc(ctx, bytes2));
    Bump b2{static_cast<char *>(mem2.p)};
    int log_cap_max = 0;
    for (int k = 0; k < k1; k++) {
        EpicImg &im = imgs[k];
        im.log_cap = log_cap_of(cnt[4 * k]);
        log_cap_max = std::max(log_cap_max, im.log_cap);
        im.keys = b2.take<unsigned long long>((size_t)1 << im.log_cap);
        im.lens = b2.take<unsigned>((size_t)1 << im.log_cap);
        im.deg = b2.take<int>(im.ns); im.cursor = b2.take<int>(im.ns); im.rowptr = b2.take<int>((size_t)im.ns + 1);
        SFA_HIP(ctx, hipMemsetAsync(im.keys, 0xFF, (size_t)8 << im.log_cap, st));         // kEmptyKey
        SFA_HIP(ctx, hipMemsetAsync(im.lens, 0xFF, (size_t)4 << im.log_cap, st));         // above every length
        SFA_HIP(ctx, hipMemsetAsync(im.deg, 0, (size_t)im.ns * 4, st));
    }
    SFA_HIP(ctx, put_imgs(k1));
    const int slot_blocks = blocks((size_t)1 << log_cap_max, 256);
    mark(4);
    if (inner) hipLaunchKernelGGL(k_epic_insert, dim3(blocks(inner, 256), k1), dim3(256), 0, st, d_imgs, w, h);
    hipLaunchKernelGGL(k_epic_degrees, dim3(slot_blocks, k1), dim3(256), 0, st, d_imgs);
    hipLaunchKernelGGL(k_epic_rows, dim3(k1), dim3(256), 0, st, d_imgs);
    mark(5);
    for (int k = 0; k < k1; k++) SFA_HIP(ctx, hipMemcpyAsync(&cnt[4 * k], cnts[k], 16, hipMemcpyDeviceToHost, st));
    SFA_TRY(sfa_ctx_sync(ctx));
    spent(2, 4);
    // ---- stage 3, compact mode: rows, the search slice by slice in one shared workspace, the lists (epic_nn_plan.h) -----------------------------------------
    if (ctx->epic_search == SFA_EPIC_SEARCH_COMPACT) {
        std::vector<EpicNnGraph> graphs(k1);
        for (int k = 0; k < k1; k++) graphs[k] = EpicNnGraph{io[k].ns, io[k].nn, cnt[4 * k + 1], cnt[4 * k + 2]};
        const int slice_cap = sw_given(Switches::EPIC_NN_SLICE) ? std::max(kEpicNnGroup, sw_int(Switches::EPIC_NN_SLICE, 0) / kEpicNnGroup * kEpicNnGroup) : 0;
        const EpicNnPlan plan = epic_nn_plan(graphs.data(), k1, budget - bytes1 - bytes2, sw_int(Switches::EPIC_NN_SET, -1), slice_cap);
        for (int k = 0; k < k1 && estimate; k++)
            if (plan.img[k].searchable) *estimate = std::max(*estimate, need1(k) + need2(k, cnt[4 * k]) + epic_nn_rows_bytes(graphs[k].E) + plan.img[k].group_bytes);
        const int kc = plan.images;
        if (kc == 0) return SFA_OK;
        SFA_TRY(mem3.alloc(ctx, plan.rows + plan.workspace));
        Bump b3{static_cast<char *>(mem3.p)};
        for (int k = 0; k < kc; k++) {
            EpicImg &im = imgs[k];
            im.adj_n = b3.take<int>((size_t)2 * graphs[k].E + 1); im.adj_l = b3.take<float>((size_t)2 * graphs[k].E + 1);
            im.heap_cap = (int)plan.img[k].heap_cap;
        }
        char *ws = b3.base + b3.used;                                // plan.workspace bytes, every slice's in turn
        SFA_HIP(ctx, put_imgs(kc));
        mark(6);
        hipLaunchKernelGGL(k_epic_fill, dim3(slot_blocks, kc), dim3(256), 0, st, d_imgs);
        hipLaunchKernelGGL(k_epic_sort_rows, dim3(blocks(ns_max, 64), kc), dim3(64), 0, st, d_imgs);
        mark(7);
        for (const EpicNnSlice &s : plan.slices) {                   // (in stream order: a slice has finished with the workspace before the next one clears it)
            const EpicNnImage &pi = plan.img[s.image];
            const size_t set_bytes = (size_t)s.count * pi.set_bytes;
            epic_heap_item *heaps = reinterpret_cast<epic_heap_item *>(ws + al(set_bytes));
            const dim3 grid(blocks(s.count, kEpicNnGroup));
            if (pi.form == EPIC_NN_SPARSE) {
                SFA_HIP(ctx, hipMemsetAsync(ws, 0xFF, set_bytes, st));                     // the empty key
                hipLaunchKernelGGL(k_epic_search<SparseSet>, grid, dim3(kEpicNnGroup), 0, st, d_imgs, s.image, s.first, s.count, (void *)ws, heaps, pi.log_slots);
            } else {
                SFA_HIP(ctx, hipMemsetAsync(ws, 0x7F, set_bytes, st));
                hipLaunchKernelGGL(k_epic_search<DenseSet>, grid, dim3(kEpicNnGroup), 0, st, d_imgs, s.image, s.first, s.count, (void *)ws, heaps, 0);
            }
        }
        mark(8);
        size_t list_max = 0;
        for (int k = 0; k < kc; k++) list_max = std::max(list_max, (size_t)imgs[k].ns * imgs[k].nn);
        hipLaunchKernelGGL(k_epic_assemble, dim3(blocks(list_max, 256), kc), dim3(256), 0, st, d_imgs, w);
        mark(9);
        for (int k = 0; k < kc; k++) SFA_HIP(ctx, hipMemcpyAsync(&cnt[4 * k], cnts[k], 16, hipMemcpyDeviceToHost, st));
        SFA_TRY(sfa_ctx_sync(ctx));
        spent(2, 6); spent(3, 7); spent(4, 8);
        for (int k = 0; k < kc; k++)
            if (cnt[4 * k + 3]) return set_error(ctx, SFA_ERR_HIP, "%s: image %d of the sub-batch: the search's heap met its capacity of %d entries, or its visited set its 2^%d slots", fn, k, imgs[k].heap_cap, plan.img[k].log_slots);
        if (info) {
            info[0] += (long long)plan.slices.size();
            for (int k = 0; k < kc; k++) info[plan.img[k].form == EPIC_NN_SPARSE ? 2 : 1]++;
            info[3] = std::max(info[3], (long long)plan.workspace);
        }
        *done_out = kc;
        return SFA_OK;
    }
    // ---- stage 3: rows, the search, the lists of the images that fit whole ------------------------------------------------------------------------------
    int k2 = 0;
    size_t bytes3 = 0;
    for (; k2 < k1; k2++) {
        if (heap_cap_of(k2, cnt[4 * k2 + 1], cnt[4 * k2 + 2]) > (size_t)INT_MAX) break;   // (a heap the search could not index: far beyond any budget)
        const size_t add = need3(k2, cnt[4 * k2 + 1], cnt[4 * k2 + 2]);
        if (estimate) *estimate = std::max(*estimate, need1(k2) + need2(k2, cnt[4 * k2]) + add);
        if (bytes1 + bytes2 + bytes3 + add > budget) break;
        bytes3 += add;
    }
    if (k2 == 0) return SFA_OK;
    SFA_TRY(mem3.alloc(ctx, bytes3));
    Bump b3{static_cast<char *>(mem3.p)};
    for (int k = 0; k < k2; k++) {
        EpicImg &im = imgs[k];
        const unsigned E = cnt[4 * k + 1];
        im.adj_n = b3.take<int>((size_t)2 * E + 1); im.adj_l = b3.take<float>((size_t)2 * E + 1);
        im.done = b3.take<float>((size_t)im.ns * im.ns);
        im.heap_cap = (int)heap_cap_of(k, E, cnt[4 * k + 2]);
        im.heap = b3.take<epic_heap_item>((size_t)im.ns * im.heap_cap);
        SFA_HIP(ctx, hipMemsetAsync(im.done, 0x7F, (size_t)im.ns * im.ns * 4, st));
    }
    SFA_HIP(ctx, put_imgs(k2));
    mark(6);
    hipLaunchKernelGGL(k_epic_fill, dim3(slot_blocks, k2), dim3(256), 0, st, d_imgs);
    hipLaunchKernelGGL(k_epic_sort_rows, dim3(blocks(ns_max, 64), k2), dim3(64), 0, st, d_imgs);
    mark(7);
    hipLaunchKernelGGL(k_epic_dijkstra, dim3(blocks(ns_max, 64), k2), dim3(64), 0, st, d_imgs);
    mark(8);
    size_t list_max = 0;
    for (int k = 0; k < k2; k++) list_max = std::max(list_max, (size_t)imgs[k].ns * imgs[k].nn);
    hipLaunchKernelGGL(k_epic_assemble, dim3(blocks(list_max, 256), k2), dim3(256), 0, st, d_imgs, w);
    mark(9);
    for (int k = 0; k < k2; k++) SFA_HIP(ctx, hipMemcpyAsync(&cnt[4 * k], cnts[k], 16, hipMemcpyDeviceToHost, st));
    SFA_TRY(sfa_ctx_sync(ctx));
    spent(2, 6); spent(3, 7); spent(4, 8);
    for (int k = 0; k < k2; k++)
        if (cnt[4 * k + 3]) return set_error(ctx, SFA_ERR_HIP, "%s: image %d of the sub-batch: the search's heap met its capacity of %d entries", fn, k, imgs[k].heap_cap);
    if (info) {                                                      // one slice per image, all dense; the workspace: `done` and the heaps of the sub-batch
        info[0] += k2; info[1] += k2;
        size_t held = bytes3;
        for (int k = 0; k < k2; k++) held -= epic_nn_rows_bytes(cnt[4 * k + 1]);
        info[3] = std::max(info[3], (long long)held);
    }
    *done_out = k2;
    return SFA_OK;
}

// what epic_nn_device allocates for an image before it has seen it: the part known beforehand and, in the default mode, `done`
size_t sfa::epic_nn_need0(const sfa_ctx *ctx, int w, int h, int ns, int nn) {
    const size_t known = al(sizeof(EpicImg)) + al((size_t)w * h * 4) + 2 * al((size_t)ns * nn * 4) + al(16);
    return ctx->epic_search == SFA_EPIC_SEARCH_COMPACT ? known : known + al((size_t)ns * ns * 4);
}

// the image sizes the kernels take, refused in the name of entry point `fn`
int sfa::epic_nn_check_sizes(sfa_ctx *ctx, const char *fn, int w, int h) {
    if ((long long)w * h > kMaxPixels) REFUSE("%s: w * h = %lld pixels (at most 2^29: pixels and the border table are indexed with 32 bits)", fn, (long long)w * h);
    if (std::min(w, h) > kMaxShortSide) REFUSE("%s: w x h = %d x %d (the shorter side is at most %d: two diagonals of the sweep live in LDS)", fn, w, h, kMaxShortSide);
    return SFA_OK;
}

// Outside +0 ... +Inf the reference itself is undefined (a NaN among the border lengths breaks its sort's ordering) and the search loses the bound its heap
// is sized by: `newd >= done[to]` no longer stops a walk that a negative length shortens or a NaN never compares
int sfa::epic_check_costs(sfa_ctx *ctx, const char *fn, const char *what, int image, const float *cost, int w, int h) {
    for (size_t p = 0; p < (size_t)w * h; p++) {
        if (cost[p] >= 0) continue;                                  // -0.0 passes: border_pairs and the sweep treat it as +0
        char name[64];
        snprintf(name, sizeof name, what, image);
        REFUSE("%s: %s: pixel (%d, %d) holds the cost %g (costs are +0 ... +Inf: not NaN, not below 0)", fn, name, (int)(p % w), (int)(p / w), (double)cost[p]);
    }
    return SFA_OK;
}

int sfa_epic_nearest_seeds_batch(sfa_ctx *ctx, int n, int w, int h, const float *const *cost, const int *const *seeds_xy, const int *ns, int nn,
                                 int *const *labels, int *const *nn_index, float *const *nn_dist, size_t workspace_bytes, int *status) {
    const char *fn = __func__;
    if (!ctx) return set_error(nullptr, SFA_ERR_ARG, "%s: ctx is null", fn);
    if (n < 1) REFUSE("%s: n = %d (at least one image)", fn, n);
    if (w < 1 || h < 1) REFUSE("%s: w x h = %d x %d (both at least 1)", fn, w, h);
    if (nn < 1) REFUSE("%s: nn = %d (at least one neighbour)", fn, nn);
    if (!cost || !seeds_xy || !ns || !labels || !nn_index || !nn_dist || !status) {
        REFUSE("%s: %s is null", fn, !cost ? "cost" : !seeds_xy ? "seeds_xy" : !ns ? "ns" : !labels ? "labels" : !nn_index ? "nn_index" : !nn_dist ? "nn_dist" : "status");
    }
    SFA_TRY(epic_nn_check_sizes(ctx, fn, w, h));
    for (int i = 0; i < n; i++) {
        if (ns[i] < 1) REFUSE("%s: ns[%d] = %d (at least one seed)", fn, i, ns[i]);
        if (!cost[i] || !seeds_xy[i] || !labels[i] || !nn_index[i] || !nn_dist[i]) {
            REFUSE("%s: %s[%d] is null", fn, !cost[i] ? "cost" : !seeds_xy[i] ? "seeds_xy" : !labels[i] ? "labels" : !nn_index[i] ? "nn_index" : "nn_dist", i);
        }
        if ((long long)ns[i] * nn > INT_MAX) REFUSE("%s: ns[%d] * nn = %lld entries (the kernels index the lists with 32 bits)", fn, i, (long long)ns[i] * nn);
        for (int k = 0; k < ns[i]; k++) {
            const int x = seeds_xy[i][2 * k], y = seeds_xy[i][2 * k + 1];
            if (x < 0 || x >= w || y < 0 || y >= h) REFUSE("%s: seeds_xy[%d]: seed %d = (%d, %d) lies outside the %d x %d image", fn, i, k, x, y, w, h);
        }
        SFA_TRY(epic_check_costs(ctx, fn, "cost[%d]", i, cost[i], w, h));
    }
    SFA_HIP(ctx, hipSetDevice(ctx->device));
    size_t budget = workspace_bytes;
    if (!budget) {                                                   // half of what the GPU has free now
        size_t free_b = 0, total_b = 0;
        SFA_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
        budget = free_b / 2;
    }
    const size_t npix = (size_t)w * h;
    hipStream_t st = ctx->stream;
    // what the call itself holds of an image: cost, labels, seeds, the two lists
    auto need_io = [&](int i) { return 2 * al(npix * 4) + al((size_t)ns[i] * 8) + 2 * al((size_t)ns[i] * nn * 4); };
    for (int i = 0; i < n; i++) status[i] = 0;
    for (float &v : ctx->epic_ms) v = 0.f;
    for (long long &v : ctx->epic_info) v = 0;
    // A sub-batch is sized by what is known beforehand (planes, lists, `done`) or, once an image has been through, by the largest whole need seen.  What is
    // allocated never exceeds the budget: where the tables or heaps of a sub-batch's first image do not fit beside what the sub-batch already holds, that
    // image is tried alone before it is flagged
    auto need0 = [&](int i) { return need_io(i) + epic_nn_need0(ctx, w, h, ns[i], nn); };
    size_t estimate = 0;                                             // (of epic_nn_device's part)
    bool alone = false;
    int first = 0;
    while (first < n) {
        int m = 0;
        for (size_t used = 0; first + m < n && m < kMaxSubBatch && !(alone && m == 1); m++) {
            used += std::max(need0(first + m), estimate ? estimate + need_io(first + m) : 0);
            if (used > budget) break;
        }
        if (m == 0 && need0(first) > budget) { status[first++] = 1; alone = false; continue; }
        m = std::max(m, 1);                                          // (the estimate is another image's: this one may still fit)
        DevMem mem;
        size_t bytes = 0;
        for (int k = 0; k < m; k++) bytes += need_io(first + k);
        SFA_TRY(mem.alloc(ctx, bytes));
        Bump b{static_cast<char *>(mem.p)};
        std::vector<EpicNnIo> io(m);
        for (int k = 0; k < m; k++) {
            const int i = first + k;
            float *c = b.take<float>(npix);
            int *s = b.take<int>((size_t)ns[i] * 2);
            io[k].cost = c; io[k].seeds = s; io[k].ns = ns[i]; io[k].nn = nn;
            io[k].lab = b.take<int>(npix);
            io[k].index = b.take<int>((size_t)ns[i] * nn); io[k].dist = b.take<float>((size_t)ns[i] * nn);
            SFA_HIP(ctx, hipMemcpyAsync(c, cost[i], npix * 4, hipMemcpyHostToDevice, st));
            SFA_HIP(ctx, hipMemcpyAsync(s, seeds_xy[i], (size_t)ns[i] * 8, hipMemcpyHostToDevice, st));
        }
        int done = 0;
        SFA_TRY(epic_nn_device(ctx, fn, m, w, h, io.data(), budget - bytes, &done, &estimate, ctx->epic_ms, ctx->epic_info));
        if (done == 0) {                                             // the first image of the sub-batch: alone next time, or flagged if it was alone
            if (m > 1) alone = true;
            else { status[first++] = 1; alone = false; }
            continue;
        }
        for (int k = 0; k < done; k++) {
            const int i = first + k;
            SFA_HIP(ctx, hipMemcpyAsync(labels[i], io[k].lab, npix * 4, hipMemcpyDeviceToHost, st));
            SFA_HIP(ctx, hipMemcpyAsync(nn_index[i], io[k].index, (size_t)ns[i] * nn * 4, hipMemcpyDeviceToHost, st));
            SFA_HIP(ctx, hipMemcpyAsync(nn_dist[i], io[k].dist, (size_t)ns[i] * nn * 4, hipMemcpyDeviceToHost, st));
        }
        SFA_TRY(sfa_ctx_sync(ctx));
        first += done;
        alone = false;
    }
    return SFA_OK;
}

int sfa_epic_nn_search_info(sfa_ctx *ctx, long long info[4]) {
    if (!ctx || !info) return set_error(ctx, SFA_ERR_ARG, "%s: %s is null", __func__, !ctx ? "ctx" : "info");
    for (int k = 0; k < 4; k++) info[k] = ctx->epic_info[k];
    return SFA_OK;
}

int sfa_epic_nn_stage_ms(sfa_ctx *ctx, float ms[5]) {
    if (!ctx || !ms) return set_error(ctx, SFA_ERR_ARG, "%s: %s is null", __func__, !ctx ? "ctx" : "ms");
    for (int k = 0; k < 5; k++) ms[k] = ctx->epic_ms[k];
    return SFA_OK;
}
