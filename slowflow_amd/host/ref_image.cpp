// ref_image.cpp -- see ref_image.h.  Whole planes in the order of the definition: 8 bits, row pass, column pass with its rounding, 2 x 2 reduction.
#include "ref_image.h"

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../csrc/lab_math.h"
#include "../csrc/ref_image.h"

color_image_t *reference_rgb8(const color_image_t *rgb, float norm, int skip) {
    using namespace sfa::refimg;
    const int w = rgb->width, h = rgb->height, S = skip + 1;
    if (refused_skip(skip) || w < S || h < S) return nullptr;
    const int gw = w / S, gh = h / S;
    if (resized_extent(w, skip) != gw || resized_extent(h, skip) != gh) return nullptr;
    const size_t pl = (size_t)w * h;
    std::vector<uint8_t> p8(3 * pl);
    for (int c = 0; c < 3; c++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const float v = sfa::lab::sample_8bit(rgb->c1[((size_t)c * h + y) * rgb->stride + x], norm);
                p8[c * pl + (size_t)y * w + x] = v == v ? (uint8_t)v : 0;   // saturate_cast<uchar>(cvRound(NaN)): 0
            }
    color_image_t *out = color_image_new(gw, gh);
    color_image_erase(out);
    if (skip == 0) {
        for (int c = 0; c < 3; c++)
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) out->c1[((size_t)c * h + y) * out->stride + x] = p8[c * pl + (size_t)y * w + x];
        return out;
    }
    int k[kMaxTaps], n = 0;
    taps(skip, k, &n);
    const int r = n / 2;
    std::vector<uint16_t> row(3 * pl);
    for (int c = 0; c < 3; c++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                int a = 0;
                for (int i = 0; i < n; i++) a += k[i] * p8[c * pl + (size_t)y * w + std::min(std::max(x + i - r, 0), w - 1)];
                row[c * pl + (size_t)y * w + x] = (uint16_t)a;             // at most 255 * 256
            }
    std::vector<uint8_t> b8(3 * pl);
    for (int c = 0; c < 3; c++)
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                int val = 0;
                for (int i = 0; i < n; i++) val += k[i] * row[c * pl + (size_t)std::min(std::max(y + i - r, 0), h - 1) * w + x];
                b8[c * pl + (size_t)y * w + x] = (uint8_t)std::min(round_blur(val, 3 * x + c, w), 255);
            }
    for (int c = 0; c < 3; c++)
        for (int gy = 0; gy < gh; gy++)
            for (int gx = 0; gx < gw; gx++) {
                const uint8_t *p = &b8[c * pl + (size_t)first_source(gy, skip) * w + first_source(gx, skip)];
                out->c1[((size_t)c * gh + gy) * out->stride + gx] = (float)reduce4(p[0], p[1], p[w], p[w + 1]);
            }
    return out;
}
