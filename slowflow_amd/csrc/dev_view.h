// dev_view.h -- the arithmetic of the device seam's argument checks: a strided view of device memory, the offset of its last element, whether its strides
// keep any two elements apart, its byte range and whether byte ranges overlap.  Host code only, nothing from HIP and nothing from sfa_internal.h:
// tests/host/test_dev_view.cpp compiles it with plain g++.  What asks the HIP runtime about a pointer (check_view, check_disjoint) is api.hip's.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace sfa {

constexpr int kViewDims = 5;
// element (i0, ..) of `nd` <= 5 dimensions lies at p + sum i_k st[k], in elements of `elem` bytes; the last dimension is the innermost.  A stride may be 0
// (a source that repeats).  dim: what a refusal calls each stride (null: "the column stride", "the row stride", "stride k").
struct View {
    const char *name;
    const void *p;
    size_t elem;
    int nd;
    int n[kViewDims];
    const long long *st;
    const char *const *dim = nullptr;
};

// *acc += steps * stride without wrapping; false: the sum leaves the signed 64-bit range (a view no allocation can hold)
inline bool extent_add(long long *acc, long long steps, long long stride) {
    long long t;
    return !__builtin_mul_overflow(steps, stride, &t) && !__builtin_add_overflow(*acc, t, acc);
}

enum ViewFault { VIEW_OK, VIEW_NEGATIVE, VIEW_BELOW_MIN, VIEW_RANGE };
// the sign and extent rule: no stride negative, the innermost at least min_inner, and the offset of the last element (*last, in elements) inside the signed
// 64-bit range.  *at: the dimension that broke the rule.
inline ViewFault view_extent(const View &v, long long min_inner, long long *last, int *at) {
    *last = 0;
    for (int i = 0; i < v.nd; i++) {
        *at = i;
        if (v.st[i] < 0) return VIEW_NEGATIVE;
        if (i == v.nd - 1 && v.st[i] < min_inner) return VIEW_BELOW_MIN;
        if (!extent_add(last, v.n[i] - 1, v.st[i])) return VIEW_RANGE;
    }
    return VIEW_OK;
}

// strides sorted, each larger than the extent of all smaller ones: no two elements share an address (dimensions of size 1 do not count).  A sufficient
// condition: 3 x 2 at (2, 3) has six addresses and is refused.  For strides that passed view_extent (the extent does not wrap).
inline bool strides_nest(const long long *st, const int *n, int nd) {
    int order[kViewDims], m = 0;
    for (int i = 0; i < nd; i++)
        if (n[i] > 1) order[m++] = i;
    std::sort(order, order + m, [&](int a, int b) { return st[a] < st[b]; });
    long long extent = 0;                                  // offset of the last element of the dimensions so far
    for (int k = 0; k < m; k++) {
        if (st[order[k]] <= extent) return false;
        extent += (n[order[k]] - 1) * st[order[k]];
    }
    return true;
}

// [first byte, last byte] of a view that passed view_extent; a null pointer (an optional argument left out) gives the empty range that overlaps nothing
struct ByteRange { uintptr_t lo, hi; };
inline ByteRange byte_range(const View &v) {
    if (!v.p) return ByteRange{1, 0};
    long long last;
    int at;
    view_extent(v, 0, &last, &at);
    const uintptr_t lo = reinterpret_cast<uintptr_t>(v.p);
    return ByteRange{lo, lo + (uintptr_t)last * v.elem + v.elem - 1};
}
inline bool overlap(const ByteRange &a, const ByteRange &b) { return a.lo <= a.hi && b.lo <= b.hi && a.lo <= b.hi && b.lo <= a.hi; }
// the first pair (in argument order) of r[0..n) that overlaps: true and *a < *b; false: all disjoint.  Sorted by first byte, disjoint ranges end before
// their successor begins: the common answer "none" costs one sort (a download of 128 windows has 384 planes), and only a refusal looks at every pair.
inline bool first_overlap(const ByteRange *r, int n, int *a, int *b) {
    std::vector<int> o;
    for (int i = 0; i < n; i++)
        if (r[i].lo <= r[i].hi) o.push_back(i);
    std::sort(o.begin(), o.end(), [&](int x, int y) { return r[x].lo < r[y].lo; });
    size_t k = 1;
    while (k < o.size() && r[o[k - 1]].hi < r[o[k]].lo) k++;
    if (k >= o.size()) return false;
    for (*a = 0; *a < n; ++*a)
        for (*b = *a + 1; *b < n; ++*b)
            if (overlap(r[*a], r[*b])) return true;
    return false;
}

}  // namespace sfa
