// Host side of tests/test_epic_batch.py: epic()'s chain built out of the public pieces of slowflow_amd/host/epic.cpp, next to epic() and epic_batch.
//   epic_batch_tool sal <dir> <count> <sigma_image> <sigma_matrix>
//       scene k of <dir>/sizes.txt (one "w h" per line): lab_k.bin (3 planes of h*stride floats, stride = ceil(w / 4) * 4) -> saliency() -> sal_k.bin.
//   epic_batch_tool run <dir> <count> <method> <saliency_th> <pref_nn> <pref_th> <nn> <coef_kernel> <euc> [workspace_bytes]
//       scene k: rgb_k.bin (3 planes of h*stride floats), matches_k.bin (rows of 4 floats), edges_k.bin (w*h floats).  Writes
//         lab_k.bin                   rgb_to_lab's image
//         sal_k.bin                   saliency() of it (only with a saliency threshold)
//         keep1_k.bin, keep2_k.bin    the matches left after the saliency filter and after the consistency filter (a filter that is off keeps all): the
//                                     chain restated with saliency(), epic_nearest_seeds, epic_fit_nadarayawatson and the two-line helpers of epic.cpp
//         fx_k.bin, fy_k.bin          epic()'s fields (planes prefilled with 0)
//         bfx_k.bin, bfy_k.bin        epic_batch's over all scenes at once
//       and prints "rc k <epic> <epic_batch>" per scene, then "stage_ms" with the eight stage times of the library's chain after epic_batch.
//   epic_batch_tool time <dir> <count> <method> <saliency_th> <pref_nn> <pref_th> <nn> <coef_kernel> <euc> <workspace_bytes> <reps>
//       the same inputs; epic_batch alone, <reps> times on fresh copies of the edges: prints "batch_ms" with the wall milliseconds of each and one "stage_ms"
//       line per repetition (tools/bench_epic_batch.py, which builds this mode alone, with -DEPIC_BATCH_TOOL_NO_STAGES, against a tree without the chain).
// Needs the GPU.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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

static bool read_sizes(const std::string &dir, int count, std::vector<int> &ws, std::vector<int> &hs) {
    ws.resize(count); hs.resize(count);
    std::ifstream f((dir + "/sizes.txt").c_str());
    for (int k = 0; k < count; k++) if (!(f >> ws[k] >> hs[k])) return false;
    return true;
}

static color_image_t *read_color(const std::string &path, int w, int h) {
    color_image_t *im = color_image_new(w, h);
    std::vector<float> planes;
    if (!rd(path, planes) || planes.size() != (size_t)3 * im->stride * h) { color_image_delete(im); return nullptr; }
    memcpy(im->c1, planes.data(), planes.size() * sizeof(float));
    return im;
}

// epic.cpp:31-56 and :196-198, restated
static void to_seeds_and_vects(const std::vector<float> &m, std::vector<int> &seeds, std::vector<float> &vects) {
    const size_t n = m.size() / 4;
    seeds.resize(2 * n); vects.resize(2 * n);
    for (size_t i = 0; i < n; i++) {
        seeds[2 * i] = (int)m[4 * i]; seeds[2 * i + 1] = (int)m[4 * i + 1];
        vects[2 * i] = m[4 * i + 2] - m[4 * i]; vects[2 * i + 1] = m[4 * i + 3] - m[4 * i + 1];
    }
}
static void kernel(epic_nn &k, float coef) { for (float &d : k.dist) d = expf(-coef * d) + 1e-08; }

static void stage_times(sfa_ctx *ctx, float stage[8]) {
    for (int k = 0; k < 8; k++) stage[k] = 0.f;
#ifndef EPIC_BATCH_TOOL_NO_STAGES
    if (sfa_epic_batch_stage_ms(ctx, stage) != SFA_OK) fprintf(stderr, "%s\n", sfa_last_error(ctx));
#else
    (void)ctx;
#endif
}

static int run_time(int argc, char **argv) {
    if (argc < 13) return 2;
    const std::string dir = argv[2];
    const int count = atoi(argv[3]), reps = atoi(argv[12]);
    epic_params_t p;
    epic_params_default(&p);
    strncpy(p.method, argv[4], sizeof p.method - 1);
    p.saliency_th = (float)atof(argv[5]); p.pref_nn = atoi(argv[6]); p.pref_th = (float)atof(argv[7]); p.nn = atoi(argv[8]); p.coef_kernel = (float)atof(argv[9]);
    p.euc = (float)atof(argv[10]);
    const size_t budget = (size_t)atoll(argv[11]);
    std::vector<int> ws, hs;
    if (!read_sizes(dir, count, ws, hs)) { fprintf(stderr, "sizes.txt unreadable\n"); return 2; }
    sfa_ctx *ctx = nullptr;
    if (sfa_ctx_create(0, &ctx) != SFA_OK) { fprintf(stderr, "%s\n", sfa_last_error(nullptr)); return 3; }
    std::vector<color_image_t *> lab(count);
    std::vector<epic_matches> m(count);
    std::vector<epic_edges> e0(count), e2(count);
    std::vector<image_t *> bx(count), by(count);
    std::vector<int> rc(count);
    for (int k = 0; k < count; k++) {
        const std::string s = std::to_string(k);
        color_image_t *rgb = read_color(dir + "/rgb_" + s + ".bin", ws[k], hs[k]);
        if (!rgb) { fprintf(stderr, "rgb_%d.bin unreadable\n", k); return 2; }
        lab[k] = rgb_to_lab(rgb);
        color_image_delete(rgb);
        if (!rd(dir + "/matches_" + s + ".bin", m[k].m) || m[k].m.size() % 4 || !read_edges((dir + "/edges_" + s + ".bin").c_str(), ws[k], hs[k], e0[k])) {
            fprintf(stderr, "matches / edges of scene %d unreadable\n", k);
            return 2;
        }
        bx[k] = image_new(ws[k], hs[k]); by[k] = image_new(ws[k], hs[k]);
    }
    std::vector<const color_image_t *> labs(lab.begin(), lab.end());
    std::vector<const epic_matches *> ms(count);
    std::vector<epic_edges *> es(count);
    for (int k = 0; k < count; k++) { ms[k] = &m[k]; es[k] = &e2[k]; }
    std::vector<double> wall;
    std::vector<std::vector<float>> stages;
    for (int r = 0; r < reps; r++) {
        for (int k = 0; k < count; k++) e2[k] = e0[k];
        const auto t0 = std::chrono::steady_clock::now();
        epic_batch(ctx, count, bx.data(), by.data(), labs.data(), ms.data(), es.data(), &p, rc.data(), budget);
        wall.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        float stage[8];
        stage_times(ctx, stage);
        stages.push_back(std::vector<float>(stage, stage + 8));
        for (int k = 0; k < count; k++) if (rc[k] != 0) { fprintf(stderr, "epic_batch: rc[%d] = %d %s\n", k, rc[k], rc[k] < 0 ? sfa_last_error(ctx) : ""); return 3; }
    }
    printf("batch_ms");
    for (double v : wall) printf(" %.3f", v);
    printf("\n");
    for (const auto &st : stages) {
        printf("stage_ms");
        for (float v : st) printf(" %.4f", v);
        printf("\n");
    }
    sfa_ctx_destroy(ctx);
    return 0;
}

static int run_sal(int argc, char **argv) {
    if (argc < 6) return 2;
    const std::string dir = argv[2];
    const int count = atoi(argv[3]);
    const float s1 = (float)atof(argv[4]), s2 = (float)atof(argv[5]);
    std::vector<int> ws, hs;
    if (!read_sizes(dir, count, ws, hs)) return 2;
    sfa_ctx *ctx = nullptr;
    if (sfa_ctx_create(0, &ctx) != SFA_OK) { fprintf(stderr, "%s\n", sfa_last_error(nullptr)); return 3; }
    for (int k = 0; k < count; k++) {
        color_image_t *lab = read_color(dir + "/lab_" + std::to_string(k) + ".bin", ws[k], hs[k]);
        if (!lab) { fprintf(stderr, "lab_%d.bin unreadable\n", k); return 2; }
        image_t *s = saliency(ctx, lab, s1, s2);
        if (!s) { fprintf(stderr, "saliency: %s\n", sfa_last_error(ctx)); return 3; }
        wr(dir + "/sal_" + std::to_string(k) + ".bin", s->data, (size_t)s->stride * hs[k]);
        image_delete(s);
        color_image_delete(lab);
    }
    sfa_ctx_destroy(ctx);
    return 0;
}

static int run(int argc, char **argv) {
    if (argc < 11) return 2;
    const std::string dir = argv[2];
    const int count = atoi(argv[3]);
    epic_params_t p;
    epic_params_default(&p);
    strncpy(p.method, argv[4], sizeof p.method - 1);
    p.saliency_th = (float)atof(argv[5]); p.pref_nn = atoi(argv[6]); p.pref_th = (float)atof(argv[7]); p.nn = atoi(argv[8]); p.coef_kernel = (float)atof(argv[9]);
    p.euc = (float)atof(argv[10]);
    const size_t budget = argc > 11 ? (size_t)atoll(argv[11]) : 0;
    std::vector<int> ws, hs;
    if (!read_sizes(dir, count, ws, hs)) { fprintf(stderr, "sizes.txt unreadable\n"); return 2; }
    sfa_ctx *ctx = nullptr;
    if (sfa_ctx_create(0, &ctx) != SFA_OK) { fprintf(stderr, "%s\n", sfa_last_error(nullptr)); return 3; }
    std::vector<color_image_t *> lab(count);
    std::vector<epic_matches> m(count);
    std::vector<epic_edges> e0(count), e1(count), e2(count);         // epic() and epic_batch each add euc to their own copy
    std::vector<image_t *> fx(count), fy(count), bx(count), by(count);
    std::vector<int> rc1(count), rc2(count);
    for (int k = 0; k < count; k++) {
        const std::string s = std::to_string(k);
        const int w = ws[k], h = hs[k];
        color_image_t *rgb = read_color(dir + "/rgb_" + s + ".bin", w, h);
        if (!rgb) { fprintf(stderr, "rgb_%d.bin unreadable\n", k); return 2; }
        lab[k] = rgb_to_lab(rgb);
        color_image_delete(rgb);
        wr(dir + "/lab_" + s + ".bin", lab[k]->c1, (size_t)3 * lab[k]->stride * h);
        if (!rd(dir + "/matches_" + s + ".bin", m[k].m) || m[k].m.size() % 4 || !read_edges((dir + "/edges_" + s + ".bin").c_str(), w, h, e0[k])) {
            fprintf(stderr, "matches / edges of scene %d unreadable\n", k);
            return 2;
        }
        // ---- the chain out of the public pieces ---------------------------------------------------------------------------------------------------
        std::vector<float> mm(m[k].m);
        for (size_t i = 0; i + 3 < mm.size(); i += 4) {              // epic.cpp:15-28
            mm[i] = std::max(0.f, std::min(mm[i], (float)(w - 1)));         mm[i + 1] = std::max(0.f, std::min(mm[i + 1], (float)(h - 1)));
            mm[i + 2] = std::max(0.f, std::min(mm[i + 2], (float)(w - 1))); mm[i + 3] = std::max(0.f, std::min(mm[i + 3], (float)(h - 1)));
        }
        epic_edges ec = e0[k];
        if (p.euc) for (float &c : ec.cost) c += p.euc;
        if (p.saliency_th) {                                         // :59-74
            image_t *sal = saliency(ctx, lab[k], 0.8f, 1.0f);
            if (!sal) { fprintf(stderr, "saliency: %s\n", sfa_last_error(ctx)); return 3; }
            wr(dir + "/sal_" + s + ".bin", sal->data, (size_t)sal->stride * h);
            std::vector<float> keep;
            for (size_t i = 0; i + 3 < mm.size(); i += 4)
                if (sal->data[(int)(mm[i + 1] * sal->stride + mm[i])] >= p.saliency_th) keep.insert(keep.end(), mm.begin() + i, mm.begin() + i + 4);
            image_delete(sal);
            mm.swap(keep);
        }
        wr(dir + "/keep1_" + s + ".bin", mm.data(), mm.size());
        if (p.pref_nn && !mm.empty()) {                              // :77-123
            std::vector<int> seeds, labels;
            std::vector<float> vects, est, keep;
            to_seeds_and_vects(mm, seeds, vects);
            epic_nn nnl;
            epic_nearest_seeds(seeds, ec, std::min(p.pref_nn + 1, (int)(mm.size() / 4)), nnl, labels);
            kernel(nnl, p.coef_kernel);
            epic_fit_nadarayawatson(est, nnl, vects);
            for (size_t i = 0; i < mm.size() / 4; i++) {
                const float ex = est[2 * i] - vects[2 * i], ey = est[2 * i + 1] - vects[2 * i + 1];
                if (ex * ex + ey * ey < p.pref_th * p.pref_th) keep.insert(keep.end(), mm.begin() + 4 * i, mm.begin() + 4 * i + 4);
            }
            mm.swap(keep);
        }
        wr(dir + "/keep2_" + s + ".bin", mm.data(), mm.size());
        // ---- epic() ---------------------------------------------------------------------------------------------------------------------------------
        e1[k] = e0[k];
        image_t **all[4] = {&fx[k], &fy[k], &bx[k], &by[k]};
        for (image_t **im : all) { *im = image_new(w, h); image_erase(*im); }
        rc1[k] = epic(ctx, fx[k], fy[k], lab[k], m[k], e1[k], &p);
        if (rc1[k] < 0) { fprintf(stderr, "epic: %s\n", sfa_last_error(ctx)); return 3; }
    }
    std::vector<const color_image_t *> labs(lab.begin(), lab.end());
    std::vector<const epic_matches *> ms(count);
    std::vector<epic_edges *> es(count);
    for (int k = 0; k < count; k++) { ms[k] = &m[k]; es[k] = &e2[k]; e2[k] = e0[k]; }
    epic_batch(ctx, count, bx.data(), by.data(), labs.data(), ms.data(), es.data(), &p, rc2.data(), budget);
    float stage[8];
    stage_times(ctx, stage);
    for (int k = 0; k < count; k++) {
        if (rc2[k] < 0) { fprintf(stderr, "epic_batch: %s\n", sfa_last_error(ctx)); return 3; }
        if (e2[k].cost != e1[k].cost) { fprintf(stderr, "epic_batch: the edges of scene %d do not hold euc once\n", k); return 3; }
        const std::string s = std::to_string(k);
        wr(dir + "/fx_" + s + ".bin", fx[k]->data, (size_t)fx[k]->stride * hs[k]);
        wr(dir + "/fy_" + s + ".bin", fy[k]->data, (size_t)fy[k]->stride * hs[k]);
        wr(dir + "/bfx_" + s + ".bin", bx[k]->data, (size_t)bx[k]->stride * hs[k]);
        wr(dir + "/bfy_" + s + ".bin", by[k]->data, (size_t)by[k]->stride * hs[k]);
        printf("rc %d %d %d\n", k, rc1[k], rc2[k]);
    }
    printf("stage_ms");
    for (float v : stage) printf(" %.6f", v);
    printf("\n");
    sfa_ctx_destroy(ctx);
    return 0;
}

int main(int argc, char **argv) {
    int rc = 2;
    if (argc > 1 && !strcmp(argv[1], "sal")) rc = run_sal(argc, argv);
    else if (argc > 1 && !strcmp(argv[1], "run")) rc = run(argc, argv);
    else if (argc > 1 && !strcmp(argv[1], "time")) rc = run_time(argc, argv);
    if (rc == 2) fprintf(stderr, "usage: epic_batch_tool sal dir count sigma_image sigma_matrix | epic_batch_tool run|time dir count method saliency_th pref_nn pref_th nn coef_kernel euc [workspace_bytes [reps]]\n");
    return rc;
}
