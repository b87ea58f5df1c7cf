// Host side of tests/test_epic_fit.py and tools/bench_epic_fit.py: the model fits and apply loops of slowflow_amd/host/epic.cpp on arrays the caller writes.
//   epic_fit_tool fit <dir> <w> <h> <ns> <nn> <LA|NW> <stride> [reps]
//       <dir>/seeds.bin (x y ints), vects.bin (floats), index.bin (ns*nn ints), weight.bin (ns*nn floats: the lists with the kernel function applied),
//       labels.bin (w*h ints).  epic_fit_localaffine or epic_fit_nadarayawatson -> model.bin; then epic()'s apply loop of that method into planes of h rows of
//       <stride> floats that start out as NaN -> fx.bin, fy.bin.  With reps: everything reps times, printing "expf_ms", "fit_ms" and "apply_ms" with the
//       milliseconds of each round (expf: exp(-0.8 * d) + 1e-8 over <dir>/dist.bin, ns*nn raw distances, or else over a copy of the weights: the cost of
//       epic.cpp's kernel()).  No GPU.
//   epic_fit_tool epic <dir> <count> <method> <saliency_th> <pref_nn> <pref_th> <nn> <coef_kernel> <euc> [workspace_bytes [reps]]
//       scene k of <dir>/sizes.txt (one "w h" per line): rgb_k.bin (3 planes of h*stride floats), matches_k.txt, edges_k.bin.  epic() image by image -> fx_k.bin,
//       fy_k.bin; epic_batch over all of them at once -> bfx_k.bin, bfy_k.bin; prints "rc k <epic> <epic_batch>" per scene.  With reps: epic_batch reps times
//       on fresh copies of the edges, printing "batch_ms" and the milliseconds of each.  Needs the GPU.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "epic.h"

template <class T>
static void wr(const std::string &p, const T *d, size_t n) { std::ofstream f(p.c_str(), std::ios::binary); f.write(reinterpret_cast<const char *>(d), (std::streamsize)(n * sizeof(T))); }
template <class T>
static bool rd(const std::string &p, std::vector<T> &out) {
    std::ifstream f(p.c_str(), std::ios::binary | std::ios::ate);
    if (!f) return false;
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    out.resize((size_t)bytes / sizeof(T));
    f.read(reinterpret_cast<char *>(out.data()), bytes);
    return (bool)f || bytes == 0;
}
static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

#ifndef EPIC_FIT_TOOL_EPIC_ONLY                                      // (bench_epic_fit.py builds the `epic` mode alone against a tree without the public NW fit)
static int run_fit(int argc, char **argv) {
    if (argc < 9) return 2;
    const std::string dir = argv[2];
    const int w = atoi(argv[3]), h = atoi(argv[4]), ns = atoi(argv[5]), nn = atoi(argv[6]), stride = atoi(argv[8]), reps = argc > 9 ? atoi(argv[9]) : 0;
    const bool la = !strcmp(argv[7], "LA");
    if (!la && strcmp(argv[7], "NW")) return 2;
    std::vector<int> seeds, labels;
    std::vector<float> vects;
    epic_nn k;
    k.nn = nn;
    if (!rd(dir + "/seeds.bin", seeds) || !rd(dir + "/vects.bin", vects) || !rd(dir + "/index.bin", k.index) || !rd(dir + "/weight.bin", k.dist) || !rd(dir + "/labels.bin", labels) ||
        seeds.size() != (size_t)2 * ns || vects.size() != (size_t)2 * ns || k.index.size() != (size_t)ns * nn || k.dist.size() != (size_t)ns * nn ||
        labels.size() != (size_t)w * h || stride < w) {
        fprintf(stderr, "inputs unreadable or of the wrong size\n");
        return 2;
    }
    std::vector<float> model, fx((size_t)h * stride, std::numeric_limits<float>::quiet_NaN()), fy(fx);
    std::vector<double> t_exp, t_fit, t_apply;
    for (int r = 0; r < (reps ? reps : 1); r++) {
        if (reps) {                                                  // epic.cpp: kernel(), on the raw distances where the caller wrote them
            std::vector<float> d;
            if (!rd(dir + "/dist.bin", d) || d.size() != k.dist.size()) d = k.dist;
            const auto t0 = std::chrono::steady_clock::now();
            for (float &v : d) v = expf(-0.8f * v) + 1e-08;
            t_exp.push_back(ms_since(t0));
            if (d.empty() || d[0] != d[0]) fprintf(stderr, " ");     // (the loop's result is used)
        }
        auto t0 = std::chrono::steady_clock::now();
        if (la) epic_fit_localaffine(model, k, seeds, vects);
        else epic_fit_nadarayawatson(model, k, vects);
        t_fit.push_back(ms_since(t0));
        t0 = std::chrono::steady_clock::now();
        if (la) {                                                    // epic.cpp, epic(): the apply loop of LA
            for (int j = 0; j < h; j++)
                for (int i = 0; i < w; i++) {
                    const float *a = &model[(size_t)labels[(size_t)j * w + i] * 6];
                    fx[(size_t)j * stride + i] = a[0] * i + a[1] * j + a[2] - i;
                    fy[(size_t)j * stride + i] = a[3] * i + a[4] * j + a[5] - j;
                }
        } else {                                                     // and of NW
            for (int j = 0; j < h; j++)
                for (int i = 0; i < w; i++) {
                    const int s = labels[(size_t)j * w + i];
                    fx[(size_t)j * stride + i] = model[2 * s];
                    fy[(size_t)j * stride + i] = model[2 * s + 1];
                }
        }
        t_apply.push_back(ms_since(t0));
    }
    if (reps) {
        const std::pair<const char *, std::vector<double> *> all[3] = {{"expf_ms", &t_exp}, {"fit_ms", &t_fit}, {"apply_ms", &t_apply}};
        for (const auto &p : all) {
            printf("%s", p.first);
            for (double v : *p.second) printf(" %.3f", v);
            printf("\n");
        }
    }
    wr(dir + "/model.bin", model.data(), model.size());
    wr(dir + "/fx.bin", fx.data(), fx.size());
    wr(dir + "/fy.bin", fy.data(), fy.size());
    return 0;
}
#else
static int run_fit(int, char **) { return 2; }
#endif

static int run_epic(int argc, char **argv) {
    if (argc < 11) return 2;
    const std::string dir = argv[2];
    const int count = atoi(argv[3]);
    epic_params_t p;
    epic_params_default(&p);
    strncpy(p.method, argv[4], sizeof p.method - 1);
    p.saliency_th = (float)atof(argv[5]); p.pref_nn = atoi(argv[6]); p.pref_th = (float)atof(argv[7]); p.nn = atoi(argv[8]); p.coef_kernel = (float)atof(argv[9]);
    p.euc = (float)atof(argv[10]);
    const size_t budget = argc > 11 ? (size_t)atoll(argv[11]) : 0;
    const int reps = argc > 12 ? atoi(argv[12]) : 0;
    std::vector<int> ws(count), hs(count);
    {
        std::ifstream f((dir + "/sizes.txt").c_str());
        for (int k = 0; k < count; k++) if (!(f >> ws[k] >> hs[k])) { fprintf(stderr, "sizes.txt unreadable\n"); return 2; }
    }
    sfa_ctx *ctx = nullptr;
    if (sfa_ctx_create(0, &ctx) != SFA_OK) { fprintf(stderr, "%s\n", sfa_last_error(nullptr)); return 3; }
    std::vector<color_image_t *> lab(count);
    std::vector<epic_matches> m(count);
    std::vector<epic_edges> e0(count), e1(count), e2(count);         // epic() and epic_batch each add euc to their own copy
    std::vector<image_t *> fx(count), fy(count), bx(count), by(count);
    std::vector<int> rc1(count), rc2(count);
    for (int k = 0; k < count; k++) {
        const std::string s = std::to_string(k);
        color_image_t *rgb = color_image_new(ws[k], hs[k]);
        std::vector<float> planes;
        if (!rd(dir + "/rgb_" + s + ".bin", planes) || planes.size() != (size_t)3 * rgb->stride * hs[k]) { fprintf(stderr, "rgb_%d.bin unreadable\n", k); return 2; }
        memcpy(rgb->c1, planes.data(), planes.size() * sizeof(float));
        lab[k] = rgb_to_lab(rgb);
        color_image_delete(rgb);
        if (!read_matches((dir + "/matches_" + s + ".txt").c_str(), m[k]) || !read_edges((dir + "/edges_" + s + ".bin").c_str(), ws[k], hs[k], e0[k])) {
            fprintf(stderr, "matches / edges of scene %d unreadable\n", k);
            return 2;
        }
        e1[k] = e0[k];
        image_t **all[4] = {&fx[k], &fy[k], &bx[k], &by[k]};
        for (image_t **im : all) { *im = image_new(ws[k], hs[k]); image_erase(*im); }
        if (!reps) {
            rc1[k] = epic(ctx, fx[k], fy[k], lab[k], m[k], e1[k], &p);
            if (rc1[k] < 0) { fprintf(stderr, "epic: %s\n", sfa_last_error(ctx)); return 3; }
        }
    }
    std::vector<const color_image_t *> labs(lab.begin(), lab.end());
    std::vector<const epic_matches *> ms(count);
    std::vector<epic_edges *> es(count);
    for (int k = 0; k < count; k++) { ms[k] = &m[k]; es[k] = &e2[k]; }
    if (reps) printf("batch_ms");
    for (int r = 0; r < (reps ? reps : 1); r++) {
        for (int k = 0; k < count; k++) e2[k] = e0[k];
        const auto t0 = std::chrono::steady_clock::now();
        epic_batch(ctx, count, bx.data(), by.data(), labs.data(), ms.data(), es.data(), &p, rc2.data(), budget);
        if (reps) printf(" %.3f", ms_since(t0));
    }
    if (reps) printf("\n");
    for (int k = 0; k < count; k++) {
        if (rc2[k] < 0) { fprintf(stderr, "epic_batch: %s\n", sfa_last_error(ctx)); return 3; }
        const std::string s = std::to_string(k);
        wr(dir + "/fx_" + s + ".bin", fx[k]->data, (size_t)fx[k]->stride * hs[k]);
        wr(dir + "/fy_" + s + ".bin", fy[k]->data, (size_t)fy[k]->stride * hs[k]);
        wr(dir + "/bfx_" + s + ".bin", bx[k]->data, (size_t)bx[k]->stride * hs[k]);
        wr(dir + "/bfy_" + s + ".bin", by[k]->data, (size_t)by[k]->stride * hs[k]);
        printf("rc %d %d %d\n", k, rc1[k], rc2[k]);
    }
    sfa_ctx_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    int rc = 2;
    if (argc > 1 && !strcmp(argv[1], "fit")) rc = run_fit(argc, argv);
    else if (argc > 1 && !strcmp(argv[1], "epic")) rc = run_epic(argc, argv);
    if (rc == 2) fprintf(stderr, "usage: epic_fit_tool fit dir w h ns nn LA|NW stride [reps] | epic_fit_tool epic dir count method saliency_th pref_nn pref_th nn coef_kernel euc [workspace_bytes [reps]]\n");
    return rc;
}
