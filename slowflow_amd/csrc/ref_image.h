// ref_image.h -- the arithmetic of dense_tracking's reduced reference image (dense_tracking.cpp:931-936: frame 0 as 8 bits, OpenCV's 8-bit GaussianBlur,
// resize(INTER_LINEAR) to the accumulation grid), one statement for host and device code in the manner of lab_math.h and dev_view.h: the taps, the tie rule
// of the blur's rounding, the size rule and the served values of acc_skip_pixel.  OpenCV is not in this tree: the arithmetic is INTEGRATION.md 4c''s
// definition, restated from OpenCV 2.4's x86-64 source, and parity-unpinned against OpenCV itself.  Nothing from HIP: plain g++
// compiles it (tests/host/test_ref_image.cpp), csrc/ref_image.hip and host/ref_image.cpp share it.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SFA_REF_FN __host__ __device__ inline
#else
#define SFA_REF_FN inline
#endif

namespace sfa {
namespace refimg {

constexpr int kMaxTaps = 9;                                             // skip 3; skip 1 has 7

// why `skip` is not served, or null.  0: the 8-bit step alone; 1 and 3: dyadic scales whose bilinear coefficients are 1024 / 1024 of 2048
inline const char *refused_skip(int skip) {
    if (skip == 0 || skip == 1 || skip == 3) return nullptr;
    if (skip < 0) return "a negative acc_skip_pixel";
    if (skip == 7) return "its blur taps sum to 257 of 256: OpenCV's float path is no longer exact and the integer blur is not its restatement";
    if (skip > 7) return "only 0, 1 and 3 are served";
    return "1 / (skip + 1) is not dyadic: resize's float coefficient arithmetic is not restated";
}

// getGaussianKernel's taps for GaussianBlur(Size(0, 0), sigma) on CV_8U with sigma = 1 / sqrt(2 img_scale), img_scale = (double)(1.0f / (skip + 1))
// (:932-935), in the 8 fractional bits of the 8-bit filter engine: k[0 .. *n).  Host only; skip as refused_skip serves it, not 0
inline void taps(int skip, int k[kMaxTaps], int *n) {
    const double img_scale = (double)(1.0f / (float)(skip + 1));
    const double sigma = 1.0 / std::sqrt(2.0 * img_scale);
    const int nt = (int)std::rint(sigma * 6 + 1) | 1;                   // cvRound(sigma * 3 * 2 + 1) | 1 for CV_8U
    const double scale2x = -0.5 / (sigma * sigma);
    float c[kMaxTaps];
    double sum = 0;
    for (int i = 0; i < nt; i++) {
        const double x = i - (nt - 1) * 0.5;
        c[i] = (float)std::exp(scale2x * x * x);
        sum += c[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < nt; i++) {
        c[i] = (float)(c[i] * sum);
        k[i] = (int)std::rint((double)c[i] * 256);
    }
    *n = nt;
}

// the size OpenCV's resize gives an extent: cvRound(extent * img_scale), ties to even.  The stage is served where this is the accumulation grid's extent
inline int resized_extent(int extent, int skip) { return (int)std::rint(extent * (double)(1.0f / (float)(skip + 1))); }

// val / 65536 rounded to nearest, val the column pass's sum (at most 255 * 65536).  An exact tie goes to even where the SSE2 column pass handles the element
// (e = 3 x + c below 3 w & ~3: the interleaved row in fours), half up in its scalar tail
SFA_REF_FN int round_blur(int val, int e, int w) {
    const int q = val >> 16;
    if ((val & 65535) == 32768 && e < ((3 * w) & ~3)) return q + (q & 1);
    return (val + 32768) >> 16;
}

// the first of the two source rows (columns) grid row (column) g reduces over: bilinear sampling at (g + 0.5)(skip + 1) - 0.5 lands between them
SFA_REF_FN int first_source(int g, int skip) { return (skip + 1) * g + (skip - 1) / 2; }

// resize's fixed-point vertical pass at coefficients 1024 / 1024 of 2048 in both directions: the rounded mean of the 2 x 2 pixels
SFA_REF_FN int reduce4(int a, int b, int c, int d) { return (a + b + c + d + 2) >> 2; }

}  // namespace refimg
}  // namespace sfa
