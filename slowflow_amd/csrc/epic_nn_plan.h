// epic_nn_plan.h -- the compact search of the nearest-seeds stage (epic_nn.hip, SFA_EPIC_SEARCH_COMPACT) as arithmetic: what one seed's search holds in
// either form of its visited set, which form an image takes, which leading images of a sub-batch fit, and how their seeds are cut into slices that share one
// workspace.  Host code only, nothing from HIP and nothing from sfa_internal.h: tests/host/test_epic_nn_plan.cpp compiles it with plain g++.
//   dense   the visited set is a row of ns floats per seed (the default mode's `done`, indexed inside a slice by seed - first)
//   sparse  one open-addressing map per seed, node -> distance bits in 8-byte slots; its capacity is the smallest power of two >= 2 * heap_cap: a search
//           writes its set at no more nodes than it pushes, and heap_cap bounds the pushes, so the load stays at or below 1/2
// A slice is a run of whole 64-seed workgroups of one image (only an image's last workgroup is ragged); slices are taken in (image, seed) order and run one
// after the other in a workspace as large as the largest of them.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <vector>

namespace sfa {

constexpr int kEpicNnGroup = 64;                                     // k_epic_search's workgroup: one seed per thread
enum EpicNnForm { EPIC_NN_DENSE = 0, EPIC_NN_SPARSE = 1 };

inline size_t epic_nn_al(size_t b) { return (b + 255) & ~(size_t)255; }

// the heap's bound (epic_nn.hip): every push follows the expansion of one directed edge, at most nn - 1 nodes expand
inline size_t epic_nn_heap_cap(int nn, unsigned E, unsigned maxdeg) { return (size_t)1 + std::min((size_t)(nn - 1) * maxdeg, (size_t)2 * E); }
// log2 of a sparse map's slots
inline int epic_nn_log_slots(size_t heap_cap) { int l = 1; while (l < 63 && ((size_t)1 << l) < 2 * heap_cap) l++; return l; }
// the adjacency rows of an image (neighbours and lengths, 2 E entries each and one to spare)
inline size_t epic_nn_rows_bytes(unsigned E) { return 2 * epic_nn_al((size_t)2 * E * 4 + 4); }

struct EpicNnGraph { int ns, nn; unsigned E, maxdeg; };              // what the host knows of an image once its graph is counted

struct EpicNnImage {
    size_t heap_cap = 0; int log_slots = 0; int form = EPIC_NN_DENSE;
    size_t set_bytes = 0;                                            // the visited set of one seed, in the form chosen
    size_t group_bytes = 0;                                          // the workspace of one workgroup (min(64, ns) seeds)
    bool searchable = false;                                         // the kernel can index its heap and its map
};
struct EpicNnSlice { int image, first, count; size_t bytes; };
struct EpicNnPlan {
    std::vector<EpicNnImage> img;                                    // of all m images
    int images = 0;                                                  // the leading images that are computed
    size_t rows = 0;                                                 // the bytes of their adjacency rows
    size_t workspace = 0;                                            // the largest slice
    std::vector<EpicNnSlice> slices;
};

// the workspace of `count` seeds of an image: their visited sets, then their heaps
inline size_t epic_nn_slice_bytes(const EpicNnImage &im, size_t count) { return epic_nn_al(count * im.set_bytes) + epic_nn_al(count * im.heap_cap * 8); }

// force_form: -1 the smaller form (dense on a tie), else the form for every image
inline EpicNnImage epic_nn_image(const EpicNnGraph &g, int force_form) {
    EpicNnImage im;
    im.heap_cap = epic_nn_heap_cap(g.nn, g.E, g.maxdeg);
    im.log_slots = epic_nn_log_slots(im.heap_cap);
    const size_t dense = (size_t)4 * g.ns, sparse = (size_t)8 << im.log_slots;
    im.form = force_form >= 0 ? force_form : (sparse < dense ? EPIC_NN_SPARSE : EPIC_NN_DENSE);
    im.set_bytes = im.form == EPIC_NN_SPARSE ? sparse : dense;
    im.searchable = im.heap_cap <= (size_t)INT_MAX && (im.form == EPIC_NN_DENSE || im.log_slots <= 31);
    im.group_bytes = epic_nn_slice_bytes(im, (size_t)std::min(g.ns, kEpicNnGroup));
    return im;
}

// The plan of a sub-batch of m images.  avail: the bytes left of the budget after stages 1 and 2.  The leading images whose rows fit beside the largest of
// their single workgroups are computed (an image alone is left out -- flagged by the caller -- exactly when its rows and one workgroup exceed avail); what
// the rows leave is the room of a slice.  slice_cap: 0, or the most seeds of a slice (a multiple of 64).
inline EpicNnPlan epic_nn_plan(const EpicNnGraph *g, int m, size_t avail, int force_form, int slice_cap) {
    EpicNnPlan p;
    p.img.resize((size_t)m);
    for (int k = 0; k < m; k++) p.img[(size_t)k] = epic_nn_image(g[k], force_form);
    size_t group_max = 0;
    for (; p.images < m; p.images++) {
        const EpicNnImage &im = p.img[(size_t)p.images];
        if (!im.searchable) break;
        const size_t rows = epic_nn_rows_bytes(g[p.images].E), group = std::max(group_max, im.group_bytes);
        if (rows > avail || p.rows > avail - rows || group > avail - rows - p.rows) break;
        p.rows += rows;
        group_max = group;
    }
    const size_t room = avail - p.rows;
    for (int k = 0; k < p.images; k++) {
        const EpicNnImage &im = p.img[(size_t)k];
        const size_t ns = (size_t)g[k].ns, per_seed = im.set_bytes + im.heap_cap * 8;
        size_t step = ns;                                            // the whole image if it fits
        if (epic_nn_slice_bytes(im, ns) > room || (slice_cap && ns > (size_t)slice_cap)) {
            step = room > 512 ? (room - 512) / per_seed / kEpicNnGroup * kEpicNnGroup : 0;     // (512: what the two roundings to 256 bytes can add)
            if (slice_cap) step = std::min(step, (size_t)slice_cap);
            step = std::max(step, (size_t)kEpicNnGroup);             // one workgroup fits: the image is among the computed
        }
        for (size_t first = 0; first < ns; first += step) {
            const size_t count = std::min(step, ns - first);
            const EpicNnSlice s{k, (int)first, (int)count, epic_nn_slice_bytes(im, count)};
            p.workspace = std::max(p.workspace, s.bytes);
            p.slices.push_back(s);
        }
    }
    return p;
}

}  // namespace sfa
