// The arithmetic of the device seam's argument checks (slowflow_amd/csrc/dev_view.h) on the CPU: the sign and extent rule, strides_nest, byte ranges and
// their overlap.  Built with the address and undefined-behaviour sanitizers by tests/test_dev_view_host.py; includes nothing but the header.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "dev_view.h"

using namespace sfa;

#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            printf("%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static char memory[1 << 16];   // addresses for the views; nothing reads or writes through them

static View view(int nd, const int *n, const long long *st, size_t elem = 4, const void *p = memory) {
    View v{"v", p, elem, nd, {1, 1, 1, 1, 1}, st};
    for (int i = 0; i < nd; i++) v.n[i] = n[i];
    return v;
}
static ViewFault extent(int nd, const int *n, const long long *st, long long min_inner, long long *last, int *at = nullptr) {
    int a;
    const ViewFault f = view_extent(view(nd, n, st), min_inner, last, &a);
    if (at) *at = a;
    return f;
}

// sizes 1..3 and strides 0..7 in nd dimensions: the extent is the offset of the last element, and where strides_nest says yes no address repeats
static int exhaustive(int nd) {
    int accepted = 0, n[3];
    long long st[3];
    for (int code = 0; code < (nd == 1 ? 24 : nd == 2 ? 24 * 24 : 24 * 24 * 24); code++) {
        for (int i = 0, c = code; i < nd; i++, c /= 24) { n[i] = 1 + c % 3; st[i] = c % 24 / 3; }
        long long last, want = 0;
        for (int i = 0; i < nd; i++) want += (n[i] - 1) * st[i];
        EXPECT(extent(nd, n, st, 0, &last) == VIEW_OK && last == want);
        if (!strides_nest(st, n, nd)) continue;
        accepted++;
        std::set<long long> seen;
        for (int i = 0; i < n[0]; i++)
            for (int j = 0; j < (nd > 1 ? n[1] : 1); j++)
                for (int k = 0; k < (nd > 2 ? n[2] : 1); k++) EXPECT(seen.insert(i * st[0] + (nd > 1 ? j * st[1] : 0) + (nd > 2 ? k * st[2] : 0)).second);
        EXPECT((long long)seen.size() == (long long)n[0] * (nd > 1 ? n[1] : 1) * (nd > 2 ? n[2] : 1) && *seen.rbegin() == last);
    }
    return accepted;
}

int main() {
    const int a1 = exhaustive(1), a2 = exhaustive(2), a3 = exhaustive(3);
    printf("strides_nest accepts %d / %d / %d of the 1-, 2- and 3-dimensional cases\n", a1, a2, a3);
    EXPECT(a1 == 8 + 2 * 7 && a3 == 6296);                 // size 1: any stride; sizes 2, 3: strides 1..7.  6296: counted for three dimensions before

    // ---- strides_nest, pinned ----
    const int h = 5, w = 7;
    {
        const int n4[4] = {2, 3, h, w}, n1[4] = {1, 3, h, w}, n2[2] = {3, 2};
        const long long dense[4] = {3 * h * w, h * w, w, 1}, padded[4] = {3 * h * (w + 3), h * (w + 3), w + 3, 1}, chlast[4] = {3 * h * w, 1, 3 * w, 3};
        const long long one0[4] = {0, h * w, w, 1}, two0[4] = {0, h * w, w, 1}, narrow[4] = {3 * h * w, h * w, w - 1, 1}, odd[2] = {2, 3};
        EXPECT(strides_nest(dense, n4, 4) && strides_nest(padded, n4, 4) && strides_nest(chlast, n4, 4));
        EXPECT(strides_nest(one0, n1, 4));                  // a dimension of size 1 does not count, whatever its stride
        EXPECT(!strides_nest(two0, n4, 4));                 // stride 0 on a dimension of size 2
        EXPECT(!strides_nest(narrow, n4, 4));               // rows closer than the width
        EXPECT(!strides_nest(odd, n2, 2));                  // 3 x 2 at (2, 3): six distinct addresses (0 3 2 5 4 7), refused all the same
        // ---- the extent on the same cases ----
        long long last;
        EXPECT(extent(4, n4, dense, 1, &last) == VIEW_OK && last == 2 * 3 * h * w - 1);
        EXPECT(extent(4, n4, padded, 1, &last) == VIEW_OK && last == 3 * h * (w + 3) + 2 * h * (w + 3) + (h - 1) * (w + 3) + w - 1);
        EXPECT(extent(4, n4, chlast, 1, &last) == VIEW_OK && last == 2 * 3 * h * w - 1);
        EXPECT(extent(4, n1, one0, 1, &last) == VIEW_OK && last == 3 * h * w - 1);
        EXPECT(extent(4, n4, two0, 1, &last) == VIEW_OK && last == 3 * h * w - 1);
        EXPECT(extent(4, n4, narrow, 1, &last) == VIEW_OK && last == 3 * h * w + 2 * h * w + (h - 1) * (w - 1) + w - 1);
        EXPECT(extent(2, n2, odd, 1, &last) == VIEW_OK && last == 7);
    }
    // ---- the sign and extent rule's refusals ----
    {
        long long last;
        int at;
        const int n2[2] = {4, 2}, n3[3] = {2, 2, 2};
        const long long big[2] = {1LL << 62, 1}, sum[3] = {(1LL << 62) + (1LL << 61), (1LL << 62) + (1LL << 61), 1}, fits[3] = {1LL << 61, 1LL << 61, 1};
        EXPECT(extent(2, n2, big, 1, &last, &at) == VIEW_RANGE && at == 0);            // 3 x 2^62: the product leaves the range
        EXPECT(extent(3, n3, sum, 1, &last, &at) == VIEW_RANGE && at == 1);            // each product fits, their sum crosses 2^63
        EXPECT(extent(3, n3, fits, 1, &last) == VIEW_OK && last == (1LL << 62) + 1);
        const long long neg_row[2] = {-2, 1}, neg_col[2] = {2, -1}, zero_col[2] = {2, 0};
        EXPECT(extent(2, n2, neg_row, 1, &last, &at) == VIEW_NEGATIVE && at == 0);
        EXPECT(extent(2, n2, neg_col, 0, &last, &at) == VIEW_NEGATIVE && at == 1);
        EXPECT(extent(2, n2, zero_col, 1, &last, &at) == VIEW_BELOW_MIN && at == 1);
        EXPECT(extent(2, n2, zero_col, 0, &last) == VIEW_OK && last == 6);
        const long long zero_row[2] = {0, 1};                                          // only the innermost stride has a minimum
        EXPECT(extent(2, n2, zero_row, 1, &last) == VIEW_OK && last == 1);
    }
    // ---- byte ranges and their overlap, element sizes 1, 4 and 8 ----
    for (size_t elem : {(size_t)1, (size_t)4, (size_t)8}) {
        const int n[1] = {10};
        const long long st[1] = {1};
        const uintptr_t base = reinterpret_cast<uintptr_t>(memory);
        const View a = view(1, n, st, elem, memory), touch = view(1, n, st, elem, memory + 10 * elem), share = view(1, n, st, elem, memory + 10 * elem - 1);
        const View none = view(1, n, st, elem, nullptr), far = view(1, n, st, elem, memory + 100 * elem);
        EXPECT(byte_range(a).lo == base && byte_range(a).hi == base + 10 * elem - 1);
        EXPECT(byte_range(a).hi + 1 == byte_range(touch).lo && !overlap(byte_range(a), byte_range(touch)));
        EXPECT(byte_range(share).lo == byte_range(a).hi && overlap(byte_range(a), byte_range(share)) && overlap(byte_range(share), byte_range(a)));
        EXPECT(!overlap(byte_range(none), byte_range(a)) && !overlap(byte_range(none), byte_range(none)));
        int x = -1, y = -1;
        const ByteRange apart[4] = {byte_range(far), byte_range(none), byte_range(touch), byte_range(a)};      // not in address order
        EXPECT(!first_overlap(apart, 4, &x, &y));
        const ByteRange with_null[3] = {byte_range(a), byte_range(none), byte_range(share)};                   // the null entry is skipped
        EXPECT(first_overlap(with_null, 3, &x, &y) && x == 0 && y == 2);
        // far | share overlaps a and touch | a | touch: (0, 1) is no pair, the first in argument order is (1, 2)
        const ByteRange many[4] = {byte_range(far), byte_range(share), byte_range(a), byte_range(touch)};
        EXPECT(first_overlap(many, 4, &x, &y) && x == 1 && y == 2);
        // a strided view's range ends at its last element
        const int n2[2] = {3, 4};
        const long long st2[2] = {16, 2};
        EXPECT(byte_range(view(2, n2, st2, elem)).hi == base + (2 * 16 + 3 * 2) * elem + elem - 1);
    }
    // ---- a long list: 40 planes of 10 floats in a scrambled order are disjoint; one more laid over two of them is found as the first pair ----
    {
        const int n[1] = {10};
        const long long st[1] = {1};
        ByteRange planes[41];
        for (int i = 0; i < 40; i++) planes[i] = byte_range(view(1, n, st, 4, memory + 40 * ((i * 17) % 40)));
        int x = -1, y = -1;
        EXPECT(!first_overlap(planes, 40, &x, &y));
        planes[40] = byte_range(view(1, n, st, 4, memory + 40 * 5 + 39));          // the last byte of plane 5's memory and the head of plane 6's
        EXPECT(first_overlap(planes, 41, &x, &y) && y == 40 && planes[x].lo == reinterpret_cast<uintptr_t>(memory) + 40 * (x * 17 % 40));
        int first = -1;
        for (int i = 39; i >= 0; i--)
            if (i * 17 % 40 == 5 || i * 17 % 40 == 6) first = i;
        EXPECT(x == first);
    }
    printf("dev_view tests OK\n");
    return 0;
}
