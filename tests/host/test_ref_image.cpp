// Host side of tests/test_ref_image_host.py: csrc/ref_image.h and host/ref_image.cpp alone, no GPU and no library.
//   test_ref_image                                     the tap tables as literals, every refused skip, the size rule's cases
//   test_ref_image run <in> <w> <h> <skip> <norm> <out>   <in>: [3][h][w] floats as read -> reference_rgb8 -> <out>: [3][gh][gw] bytes
// Built with the address and undefined-behaviour sanitizers by the test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ref_image.h"                  // host/
#include "../csrc/ref_image.h"

using namespace sfa::refimg;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static bool served_size(int w, int h, int skip, int gw, int gh) {
    color_image_t *in = color_image_new(w, h);
    color_image_erase(in);
    color_image_t *out = reference_rgb8(in, 1.0f, skip);
    const bool ok = out && out->width == gw && out->height == gh;
    color_image_delete(in);
    if (out) color_image_delete(out);
    return ok;
}

static int self_test() {
    int k[kMaxTaps], n = 0;
    const int k1[7] = {1, 14, 62, 102, 62, 14, 1}, k3[9] = {1, 8, 27, 56, 72, 56, 27, 8, 1};
    taps(1, k, &n);
    CHECK(n == 7 && !memcmp(k, k1, sizeof k1));
    taps(3, k, &n);
    CHECK(n == 9 && !memcmp(k, k3, sizeof k3));
    for (int skip : {0, 1, 3}) CHECK(refused_skip(skip) == nullptr);
    for (int skip : {-1, 2, 4, 5, 6, 7, 8, 9, 15, 100}) {
        CHECK(refused_skip(skip) != nullptr);
        color_image_t *in = color_image_new(240, 240);                  // a multiple of every skip + 1 up to 16: only the skip can be refused
        color_image_erase(in);
        CHECK(reference_rgb8(in, 1.0f, skip) == nullptr);
        color_image_delete(in);
    }
    // the size rule: cvRound(w / (skip + 1)), ties to even, against floor(w / (skip + 1))
    CHECK(resized_extent(7, 1) == 4 && !served_size(7, 8, 1, 3, 4) && !served_size(8, 7, 1, 4, 3));
    CHECK(resized_extent(5, 1) == 2 && served_size(5, 8, 1, 2, 4));
    CHECK(served_size(1024, 436, 1, 512, 218) && served_size(1024, 436, 3, 256, 109));
    CHECK(served_size(9, 5, 1, 4, 2) && served_size(13, 9, 3, 3, 2) && served_size(9, 5, 0, 9, 5));
    // the tie rule: to even in the SSE2 part of the interleaved row, half up in its tail
    CHECK(round_blur(32768, 0, 10) == 0 && round_blur(32768 + 65536, 0, 10) == 2 && round_blur(32768, 28, 10) == 1 && round_blur(32768, 27, 10) == 0);
    CHECK(round_blur(32767, 0, 10) == 0 && round_blur(32769, 0, 10) == 1 && round_blur(255 * 65536, 5, 10) == 255);
    CHECK(first_source(0, 1) == 0 && first_source(3, 1) == 6 && first_source(0, 3) == 1 && first_source(2, 3) == 9 && reduce4(1, 1, 1, 0) == 1 && reduce4(1, 0, 0, 0) == 0);
    if (failures) return 1;
    printf("ref_image tests OK\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 1) return self_test();
    if (argc != 8 || strcmp(argv[1], "run")) { fprintf(stderr, "usage: test_ref_image [run in w h skip norm out]\n"); return 2; }
    const int w = atoi(argv[3]), h = atoi(argv[4]), skip = atoi(argv[5]);
    const float norm = (float)atof(argv[6]);
    std::vector<float> in((size_t)3 * w * h);
    FILE *f = fopen(argv[2], "rb");
    if (!f || fread(in.data(), sizeof(float), in.size(), f) != in.size()) { fprintf(stderr, "%s unreadable\n", argv[2]); return 2; }
    fclose(f);
    color_image_t *rgb = color_image_new(w, h);
    color_image_erase(rgb);
    for (int c = 0; c < 3; c++)
        for (int y = 0; y < h; y++) memcpy(rgb->c1 + ((size_t)c * h + y) * rgb->stride, &in[((size_t)c * h + y) * w], (size_t)w * sizeof(float));
    color_image_t *out = reference_rgb8(rgb, norm, skip);
    color_image_delete(rgb);
    if (!out) { fprintf(stderr, "refused\n"); return 1; }
    std::vector<unsigned char> o((size_t)3 * out->width * out->height);
    for (int c = 0; c < 3; c++)
        for (int y = 0; y < out->height; y++)
            for (int x = 0; x < out->width; x++) o[((size_t)c * out->height + y) * out->width + x] = (unsigned char)out->c1[((size_t)c * out->height + y) * out->stride + x];
    color_image_delete(out);
    f = fopen(argv[7], "wb");
    if (!f || fwrite(o.data(), 1, o.size(), f) != o.size()) { fprintf(stderr, "%s not written\n", argv[7]); return 2; }
    fclose(f);
    return 0;
}
