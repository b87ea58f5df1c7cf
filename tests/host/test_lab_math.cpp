// The Lab arithmetic of slowflow_amd/csrc/lab_math.h against the host's: every one of the 2^24 8-bit triples at norm 1, then the rounding step and the
// special values, bit pattern against bit pattern (NaN against NaN).  Two builds of this one file (tests/test_lab_math_host.py):
//   -DWITH_HOST_EPIC, linked against libslowflow_host.a: the reference is rgb8_to_lab of host/epic.cpp itself;
//   without it, the header and libm alone (the build that runs under the address and undefined-behaviour sanitizers): the reference is rgb8_to_lab's
//   statements (host/epic.cpp:19-28, 57-73) repeated below with nearbyintf, pow and exp.
// No GPU.  Prints "lab_math tests OK" and exits with 0 where nothing differs.
// With arguments the program is the GPU tests' host side (tests/test_epic_init.py), the reference alone:
//   test_lab_math conv <rgb.bin> <n> <norm> <lab.bin>    n pixels, planar r g b floats -> planar L a b
//   test_lab_math header <rgb.bin> <n> <norm> <lab.bin>  the same through the header's function
//   test_lab_math all8 <lab.bin>                         the 2^24 8-bit triples at norm 1, pixel t = (t >> 16, (t >> 8) & 255, t & 255)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <vector>

#include "lab_math.h"
#ifdef WITH_HOST_EPIC
#include "epic.h"
#endif

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, sizeof u); return u; }
static bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b); }

// n pixels (planar r, g, b) -> planar L, a, b by the reference
static void reference(const float *rgb, size_t n, float norm, float *lab) {
#ifdef WITH_HOST_EPIC
    const int w = 4096, h = (int)((n + w - 1) / w);
    color_image_t *im = color_image_new(w, h);
    const size_t pl = (size_t)im->stride * h;
    for (size_t i = 0; i < 3 * pl; i++) im->c1[i] = 0.f;
    for (int c = 0; c < 3; c++)
        for (size_t i = 0; i < n; i++) im->c1[c * pl + (i / w) * im->stride + i % w] = rgb[c * n + i];
    color_image_t *out = rgb8_to_lab(im, norm);
    for (int c = 0; c < 3; c++)
        for (size_t i = 0; i < n; i++) lab[c * n + i] = out->c1[c * pl + (i / w) * out->stride + i % w];
    color_image_delete(im);
    color_image_delete(out);
#else
    for (size_t i = 0; i < n; i++) {
        float c8[3];
        for (int c = 0; c < 3; c++) {
            const float v = nearbyintf(rgb[c * n + i] * norm);
            c8[c] = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
        }
        const float T = 0.008856;
        const float color_attenuation = 1.5f;
        const float r = c8[0] / 255.f, g = c8[1] / 255.f, b = c8[2] / 255.f;
        float X = 0.412453 * r + 0.357580 * g + 0.180423 * b;
        float Y = 0.212671 * r + 0.715160 * g + 0.072169 * b;
        float Z = 0.019334 * r + 0.119193 * g + 0.950227 * b;
        X /= 0.950456;
        Z /= 1.088754;
        const float Y3 = pow(Y, 1. / 3);
        const float fX = X > T ? pow(X, 1. / 3) : 7.787 * X + 16 / 116.;
        const float fY = Y > T ? Y3 : 7.787 * Y + 16 / 116.;
        const float fZ = Z > T ? pow(Z, 1. / 3) : 7.787 * Z + 16 / 116.;
        const float L = Y > T ? 116 * Y3 - 16.0 : 903.3 * Y;
        const float A = 500 * (fX - fY), B = 200 * (fY - fZ);
        const float l2 = (L / 100) * (L / 100);
        const float q = l2 - 0.6;
        const float correct_lab = exp(-color_attenuation * (q * q));
        lab[i] = L; lab[n + i] = A * correct_lab; lab[2 * n + i] = B * correct_lab;
    }
#endif
}

// the header on the same pixels; returns the number of values that differ and prints the first few
static size_t compare(const char *what, const std::vector<float> &rgb, float norm) {
    const size_t n = rgb.size() / 3;
    std::vector<float> want(3 * n);
    reference(rgb.data(), n, norm, want.data());
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) {
        float got[3];
        sfa::lab::rgb8_to_lab_pixel(rgb[i], rgb[n + i], rgb[2 * n + i], norm, &got[0], &got[1], &got[2]);
        for (int c = 0; c < 3; c++)
            if (!same(got[c], want[c * n + i])) {
                if (bad++ < 10)
                    fprintf(stderr, "%s: (%.9g, %.9g, %.9g) norm %.9g, output %d: header %.9g (%08x), reference %.9g (%08x)\n", what, rgb[i], rgb[n + i], rgb[2 * n + i],
                            norm, c, got[c], bits(got[c]), want[c * n + i], bits(want[c * n + i]));
            }
    }
    return bad;
}

// every ordered triple of `vals`, planar
static std::vector<float> triples_of(const std::vector<float> &vals) {
    const size_t m = vals.size(), n = m * m * m;
    std::vector<float> rgb(3 * n);
    for (size_t i = 0; i < n; i++) {
        rgb[i] = vals[i / (m * m)]; rgb[n + i] = vals[(i / m) % m]; rgb[2 * n + i] = vals[i % m];
    }
    return rgb;
}

static int convert(const std::vector<float> &rgb, float norm, const char *path, bool header = false) {
    const size_t n = rgb.size() / 3;
    std::vector<float> lab(rgb.size());
    if (!header) reference(rgb.data(), n, norm, lab.data());
    for (size_t i = 0; header && i < n; i++) sfa::lab::rgb8_to_lab_pixel(rgb[i], rgb[n + i], rgb[2 * n + i], norm, &lab[i], &lab[n + i], &lab[2 * n + i]);
    std::ofstream out(path, std::ios::binary);
    out.write(reinterpret_cast<const char *>(lab.data()), (std::streamsize)(lab.size() * sizeof(float)));
    return out.good() ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc == 6 && (!strcmp(argv[1], "conv") || !strcmp(argv[1], "header"))) {
        const size_t n = (size_t)atol(argv[3]);
        std::vector<float> rgb(3 * n);
        std::ifstream in(argv[2], std::ios::binary);
        if (!in.read(reinterpret_cast<char *>(rgb.data()), (std::streamsize)(rgb.size() * sizeof(float)))) { fprintf(stderr, "%s: not 3 x %zu floats\n", argv[2], n); return 2; }
        return convert(rgb, (float)atof(argv[4]), argv[5], !strcmp(argv[1], "header"));
    }
    if (argc == 3 && !strcmp(argv[1], "all8")) {
        const size_t n = (size_t)1 << 24;
        std::vector<float> rgb(3 * n);
        for (size_t t = 0; t < n; t++) { rgb[t] = (float)(t >> 16); rgb[n + t] = (float)((t >> 8) & 255); rgb[2 * n + t] = (float)(t & 255); }
        return convert(rgb, 1.0f, argv[2]);
    }
    if (argc != 1) { fprintf(stderr, "usage: test_lab_math [conv|header rgb.bin n norm lab.bin | all8 lab.bin]\n"); return 2; }
    size_t bad = 0;
    {   // the whole domain of the conversion: rgb8_to_lab rounds to 8 bits first
        const size_t chunk = (size_t)1 << 20;
        std::vector<float> rgb(3 * chunk);
        for (size_t base = 0; base < ((size_t)1 << 24); base += chunk) {
            for (size_t i = 0; i < chunk; i++) {
                const size_t t = base + i;
                rgb[i] = (float)(t >> 16); rgb[chunk + i] = (float)((t >> 8) & 255); rgb[2 * chunk + i] = (float)(t & 255);
            }
            bad += compare("all 8-bit triples", rgb, 1.0f);
        }
        printf("all 2^24 8-bit triples at norm 1: %zu values differ\n", bad);
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    {   // ties on both sides of even, just off a tie, outside 0 .. 255, -0.0, Inf, NaN
        const std::vector<float> vals = {0.5f, 1.5f, 2.5f, 253.5f, 254.5f, 255.5f, 0.49999997f, 0.50000006f, 1.4999999f, 2.5000002f, 254.49998f, 254.50002f, -0.5f, -0.25f,
                                         -0.0f, 0.0f, -1.0f, -3.5f, -1e30f, 255.0f, 256.0f, 300.25f, 1e30f, 8388607.5f, 8388608.0f, 16777216.0f, 1e-45f, -1e-45f, inf, -inf, nan,
                                         100.0f, 17.0f};
        const size_t b = compare("rounding and special values at norm 1", triples_of(vals), 1.0f);
        printf("rounding and special values at norm 1: %zu values differ\n", b);
        bad += b;
    }
    {   // 16-bit samples at norm 1/255: x * norm is a float product, rounded before the 8-bit step sees it
        std::vector<float> vals = {0.f, 1.f, 127.f, 128.f, 65535.f, 65534.f, 65408.f, 65407.f, 65409.f, 65280.f, 32767.f, 32768.f, 70000.f, -0.0f, -300.f, inf, -inf, nan};
        for (int k = 0; k < 8; k++)                                   // the samples around the ties (k + 0.5) * 255 = 127.5, 382.5, ...: 127, 128, 382, 383 ...
            for (int d = -1; d <= 2; d++) vals.push_back((float)((2 * k + 1) * 255 / 2 + d));
        const size_t b = compare("16-bit samples at norm 1/255", triples_of(vals), 1.0f / 255.0f);
        printf("16-bit samples at norm 1/255f: %zu values differ\n", b);
        bad += b;
    }
    {   // every 16-bit sample once per channel (grey, and against two fixed channels) at norm 1/255
        const size_t n = 65536;
        std::vector<float> rgb(3 * 3 * n);
        const size_t N = 3 * n;
        for (size_t i = 0; i < n; i++) {
            rgb[i] = rgb[N + i] = rgb[2 * N + i] = (float)i;
            rgb[n + i] = (float)i; rgb[N + n + i] = 12345.f; rgb[2 * N + n + i] = 54321.f;
            rgb[2 * n + i] = 60000.f; rgb[N + 2 * n + i] = 255.f; rgb[2 * N + 2 * n + i] = (float)i;
        }
        const size_t b = compare("every 16-bit sample at norm 1/255", rgb, 1.0f / 255.0f);
        printf("every 16-bit sample at norm 1/255f: %zu values differ\n", b);
        bad += b;
    }
    if (bad) { fprintf(stderr, "lab_math: %zu values differ\n", bad); return 1; }
    printf("lab_math tests OK\n");
    return 0;
}
