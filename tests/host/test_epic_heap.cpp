// slowflow_amd/csrc/epic_heap.h against the heap it restates: std::priority_queue<node_dist, std::vector<node_dist>, smallest_on_top> of host/epic.cpp.
// Both get the same sequences of pushes and pops; every pop must return the same (node, dis), ties included -- the order of equal keys is the point.
// Includes nothing of the project but that header.
#include <cstdio>
#include <cstdlib>
#include <queue>
#include <vector>

#include "epic_heap.h"

struct node_dist { int node; float dis; };
struct smallest_on_top { bool operator()(const node_dist &a, const node_dist &b) const { return a.dis > b.dis; } };

static int failures = 0;
static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(rng_state >> 33); }

struct Pair {
    std::priority_queue<node_dist, std::vector<node_dist>, smallest_on_top> ref;
    std::vector<epic_heap_item> store;
    int size = 0, next_node = 0;
    const char *name;
    explicit Pair(const char *n) : name(n) {}
    void push(float dis) {
        ref.push(node_dist{next_node, dis});
        if ((int)store.size() < size + 1) store.resize((size_t)size + 1);
        epic_heap_push(store, size, epic_heap_item{next_node, dis});
        next_node++;
    }
    void pop() {
        const node_dist a = ref.top();
        ref.pop();
        const epic_heap_item b = epic_heap_pop(store, size);
        if (a.node != b.node || a.dis != b.dis) {
            if (failures++ < 10) fprintf(stderr, "%s: pop gives (%d, %g), the priority_queue (%d, %g)\n", name, b.node, b.dis, a.node, a.dis);
        }
    }
    void drain() { while (!ref.empty()) pop(); if (size != 0) { failures++; fprintf(stderr, "%s: %d entries left\n", name, size); } }
};

enum Keys { EQUAL, FEW, ASCENDING, DESCENDING, RANDOM };
static float key(Keys k, int i, int n) {
    switch (k) {
        case EQUAL: return 0.25f;
        case FEW: return 0.5f * (float)(rnd() % 3);
        case ASCENDING: return (float)i;
        case DESCENDING: return (float)(n - i);
        default: return (float)(rnd() % 100000) * 1e-3f;
    }
}

int main() {
    static const char *names[] = {"equal", "few", "ascending", "descending", "random"};
    std::vector<int> sizes = {1, 2, 3};
    for (int p = 4; p <= 4096; p *= 2) { sizes.push_back(p - 1); sizes.push_back(p); sizes.push_back(p + 1); }
    long pops = 0;
    for (int k = EQUAL; k <= RANDOM; k++)
        for (int n : sizes) {
            {                                                       // n pushes, then n pops
                Pair h(names[k]);
                for (int i = 0; i < n; i++) h.push(key((Keys)k, i, n));
                pops += n;
                h.drain();
            }
            {                                                       // interleaved, the heap growing on average: Dijkstra's pattern
                Pair h(names[k]);
                for (int i = 0; i < n; i++) {
                    const int burst = 1 + (int)(rnd() % 6);
                    for (int b = 0; b < burst; b++) h.push(key((Keys)k, i + b, n));
                    const int take = (int)(rnd() % 3);
                    for (int b = 0; b < take && h.size > 0; b++, pops++) h.pop();
                }
                h.drain();
            }
            {                                                       // interleaved around a small heap: it runs empty again and again
                Pair h(names[k]);
                for (int i = 0; i < n; i++) {
                    if (h.size == 0 || rnd() % 2) h.push(key((Keys)k, i, n));
                    else { h.pop(); pops++; }
                }
                h.drain();
            }
        }
    if (failures) { fprintf(stderr, "%d pops differ\n", failures); return 1; }
    printf("epic_heap tests OK (%ld checked pops before the drains)\n", pops);
    return 0;
}
