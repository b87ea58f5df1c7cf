// The compact search's planner (slowflow_amd/csrc/epic_nn_plan.h) on the CPU: forms, the images that fit, the slices and their bytes, over a sweep of seed
// counts, neighbour counts, graphs and budgets, each against the rule written out here a second time in 128-bit arithmetic.  Built with the address and
// undefined-behaviour sanitizers by tests/test_epic_nn_plan_host.py; includes nothing but the header.
#include <cstdio>
#include <cstdlib>

#include "epic_nn_plan.h"

using namespace sfa;
typedef unsigned __int128 u128;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static u128 al128(u128 b) { return (b + 255) / 256 * 256; }

// the issue's rule, in words: dense costs 4 ns + 8 heap_cap bytes per seed, sparse 8 slots + 8 heap_cap, slots the smallest power of two >= 2 heap_cap
struct Rule { u128 heap_cap, slots, set; int form; bool searchable; };
static Rule rule_of(const EpicNnGraph &g, int force) {
    Rule r;
    const u128 a = (u128)(g.nn - 1) * g.maxdeg, b = (u128)2 * g.E;
    r.heap_cap = 1 + (a < b ? a : b);
    r.slots = 1;
    while (r.slots < 2 * r.heap_cap) r.slots *= 2;
    const u128 dense = (u128)4 * (u128)g.ns, sparse = 8 * r.slots;
    r.form = force >= 0 ? force : (sparse < dense ? EPIC_NN_SPARSE : EPIC_NN_DENSE);
    r.set = r.form == EPIC_NN_SPARSE ? sparse : dense;
    r.searchable = r.heap_cap <= (u128)INT_MAX && (r.form == EPIC_NN_DENSE || r.slots <= ((u128)1 << 31));
    return r;
}
static u128 slice128(const Rule &r, u128 count) { return al128(count * r.set) + al128(count * r.heap_cap * 8); }
static u128 rows128(unsigned E) { return 2 * al128((u128)2 * E * 4 + 4); }

static long checked_plans = 0, checked_slices = 0, flagged = 0;

static void check(const EpicNnGraph *g, int m, size_t avail, int force, int cap) {
    const EpicNnPlan p = epic_nn_plan(g, m, avail, force, cap);
    checked_plans++;
    EXPECT((int)p.img.size() == m && p.images >= 0 && p.images <= m);
    // forms and sizes of every image; the leading images that fit: rows so far and the largest single workgroup among them within avail
    int want_images = 0;
    u128 rows = 0, group = 0;
    bool open = true;
    for (int k = 0; k < m; k++) {
        const Rule r = rule_of(g[k], force);
        const EpicNnImage &im = p.img[(size_t)k];
        EXPECT(im.form == r.form && (u128)im.heap_cap == r.heap_cap && (u128)im.set_bytes == r.set && im.searchable == r.searchable);
        EXPECT(r.slots == (u128)1 << im.log_slots);
        if (force < 0) EXPECT(r.form == EPIC_NN_SPARSE ? 8 * r.slots < (u128)4 * (u128)g[k].ns : 8 * r.slots >= (u128)4 * (u128)g[k].ns);       // the smaller, dense on a tie
        const u128 one = slice128(r, (u128)std::min(g[k].ns, 64));
        EXPECT((u128)im.group_bytes == one);
        if (open && r.searchable && rows + rows128(g[k].E) + std::max(group, one) <= (u128)avail) {
            rows += rows128(g[k].E); group = std::max(group, one); want_images++;
        } else {
            open = false;
        }
    }
    EXPECT(p.images == want_images && (u128)p.rows == rows);
    if (m == 1) {                                                    // an image alone is flagged exactly when its rows and one workgroup do not fit
        const Rule r = rule_of(g[0], force);
        const bool fits = r.searchable && rows128(g[0].E) + slice128(r, (u128)std::min(g[0].ns, 64)) <= (u128)avail;
        EXPECT((p.images == 1) == fits);
        flagged += !fits;
    }
    // every seed of every computed image in exactly one slice, in order; whole workgroups but an image's last; no slice beyond what the rows leave
    const u128 room = (u128)avail - rows;
    size_t at = 0, largest = 0;
    for (int k = 0; k < p.images; k++) {
        const Rule r = rule_of(g[k], force);
        int next = 0, n_slices = 0;
        while (next < g[k].ns) {
            EXPECT(at < p.slices.size());
            const EpicNnSlice &s = p.slices[at++];
            EXPECT(s.image == k && s.first == next && s.count >= 1 && s.count <= g[k].ns - next);
            EXPECT(s.first % 64 == 0 && (s.count % 64 == 0 || s.first + s.count == g[k].ns));
            EXPECT((u128)s.bytes == slice128(r, (u128)s.count) && (u128)s.bytes <= room);
            if (cap) EXPECT(s.count <= cap);
            largest = std::max(largest, s.bytes);
            next += s.count;
            n_slices++;
            checked_slices++;
        }
        if (slice128(r, (u128)g[k].ns) <= room && (!cap || g[k].ns <= cap)) EXPECT(n_slices == 1);      // an image whose whole search fits is one slice
    }
    EXPECT(at == p.slices.size() && p.workspace == largest);
}

int main() {
    const int ns_list[] = {1, 63, 64, 65, 700, 111616};
    const int nn_list[] = {1, 5, 26, 160};
    const unsigned deg_list[] = {0, 3, 12, 40};
    for (int ns : ns_list)
        for (int nn : nn_list)
            for (unsigned maxdeg : deg_list)
                for (int dense_graph = 0; dense_graph < 2; dense_graph++) {
                    // E: none without neighbours; else a sparse planar-like graph (3 ns) or one so small that 2 E bounds the heap
                    const unsigned E = maxdeg == 0 ? 0 : dense_graph ? 3u * (unsigned)ns : std::max(1u, (unsigned)ns / 2);
                    const EpicNnGraph g{ns, nn, E, maxdeg};
                    for (int force = -1; force <= 1; force++) {
                        const EpicNnImage im = epic_nn_image(g, force);
                        const size_t rows = epic_nn_rows_bytes(E), whole = epic_nn_slice_bytes(im, (size_t)ns), one = im.group_bytes;
                        const size_t budgets[] = {0, rows, rows + one - 1, rows + one, rows + one + 1, rows + 2 * one, rows + 3 * one + 777, rows + whole / 2,
                                                  rows + whole - 1, rows + whole, rows + 10 * whole};
                        for (size_t avail : budgets)
                            for (int cap : {0, 64, 128, 4096}) check(&g, 1, avail, force, cap);
                    }
                }
    // sub-batches: the six images of the GPU tests and mixed sizes, at budgets around each prefix
    {
        const EpicNnGraph six[6] = {{250, 5, 700, 14}, {300, 5, 850, 15}, {262, 5, 740, 13}, {287, 5, 800, 16}, {275, 5, 770, 12}, {700, 5, 2000, 17}};
        const EpicNnGraph mixed[4] = {{111616, 160, 330000, 14}, {1, 3, 0, 0}, {65, 26, 190, 9}, {700, 701, 2000, 17}};
        for (int force = -1; force <= 1; force++)
            for (int cap : {0, 64, 128}) {
                for (size_t avail = 0; avail < 1500000; avail += 4099) check(six, 6, avail, force, cap);
                for (size_t avail : {(size_t)0, (size_t)3000000, (size_t)30000000, (size_t)300000000, (size_t)3000000000u, (size_t)1 << 40}) check(mixed, 4, avail, force, cap);
            }
    }
    // ties and tiny maps: E = 0 gives a heap of 1 entry and a map of 2 slots (16 bytes); a row of 4 floats ties with it and stays dense
    {
        const EpicNnGraph tie{4, 3, 0, 0}, above{5, 3, 0, 0}, below{3, 3, 0, 0};
        EXPECT(epic_nn_image(tie, -1).form == EPIC_NN_DENSE && epic_nn_image(above, -1).form == EPIC_NN_SPARSE && epic_nn_image(below, -1).form == EPIC_NN_DENSE);
        EXPECT(epic_nn_image(above, -1).log_slots == 1 && epic_nn_image(above, -1).heap_cap == 1);
    }
    // no size expression wraps at ns = 2^24: whole-image slices of 2^50 bytes and more, a heap bound at and beyond what the kernel indexes
    {
        const int ns = 1 << 24;
        const EpicNnGraph big[] = {{ns, 160, 3u << 24, 20}, {ns, ns, 3u << 24, 1u << 20}, {ns, ns, 1u << 29, 1u << 20}, {ns, ns, 1u << 30, 1u << 20},
                                   {ns, INT_MAX / ns, 0xFFFFFFFFu, 0xFFFFFFFFu}};
        for (const EpicNnGraph &g : big)
            for (int force = -1; force <= 1; force++)
                for (size_t avail : {(size_t)1 << 30, (size_t)1 << 40, (size_t)1 << 52, (size_t)1 << 62, ~(size_t)0})
                    for (int cap : {0, 1 << 20}) check(&g, 1, avail, force, cap);
        EXPECT(!epic_nn_image(big[3], -1).searchable);               // 1 + 2^31 heap entries: beyond INT_MAX
        EXPECT(epic_nn_image(big[2], -1).searchable && !epic_nn_image(big[2], EPIC_NN_SPARSE).searchable);      // 2^32 slots: dense only
    }
    EXPECT(flagged > 100 && checked_slices > 100000);
    printf("epic_nn_plan tests OK (%ld plans, %ld slices, %ld flagged)\n", checked_plans, checked_slices, flagged);
    return 0;
}
