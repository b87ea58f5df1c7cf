// epic_heap.h -- the binary heap of EpicFlow's graph search (host/epic.cpp: std::priority_queue<node_dist, std::vector<node_dist>, smallest_on_top>) as plain
// functions over an indexable store, for host and device.  Entries of equal distance leave a heap in an order that the sift rules decide, and that order
// decides the neighbour lists (epic_nn.hip), so push and pop are libstdc++'s std::push_heap / std::pop_heap with comp(a, b) = a.dis > b.dis, step for step:
//   push  append, then move the hole up while the parent's dis is greater (__push_heap)
//   pop   take the root; move the hole down to a leaf, at each level to the second child unless second.dis > first.dis (then the first), a lone last child
//         is followed (__adjust_heap); then sift the former last element up from there (__push_heap)
// tests/host/test_epic_heap.cpp drives both with the same operation sequences.  Includes nothing; Store is anything with operator[](int) -> epic_heap_item &.
#pragma once

#if defined(__HIPCC__)
#define EPIC_HEAP_FN __host__ __device__ inline
#else
#define EPIC_HEAP_FN inline
#endif

struct epic_heap_item { int node; float dis; };

// __push_heap: `value` goes to the place the hole reaches when it moves up from `hole`, not above `top`
template <class Store>
EPIC_HEAP_FN void epic_heap_sift_up(Store &s, int hole, int top, epic_heap_item value) {
    int parent = (hole - 1) / 2;
    while (hole > top && s[parent].dis > value.dis) {
        s[hole] = s[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    s[hole] = value;
}

// priority_queue::push; the store holds at least size + 1 entries
template <class Store>
EPIC_HEAP_FN void epic_heap_push(Store &s, int &size, epic_heap_item value) {
    epic_heap_sift_up(s, size, 0, value);
    size++;
}

// priority_queue::top + pop; size >= 1
template <class Store>
EPIC_HEAP_FN epic_heap_item epic_heap_pop(Store &s, int &size) {
    const epic_heap_item root = s[0];
    const int len = --size;                                         // the heap that remains
    if (len == 0) return root;
    const epic_heap_item value = s[len];                            // the former last element
    int hole = 0, child = 0;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);                                    // the second child
        if (s[child].dis > s[child - 1].dis) child--;
        s[hole] = s[child];
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {                 // a lone last child
        child = 2 * (child + 1);
        s[hole] = s[child - 1];
        hole = child - 1;
    }
    epic_heap_sift_up(s, hole, 0, value);
    return root;
}
