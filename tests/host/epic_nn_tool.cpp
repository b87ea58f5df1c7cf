// Host side of tests/test_epic_nn.py: slowflow_amd/host/epic.cpp on scenes the test writes.
//   epic_nn_tool seeds <dir> <w> <h> <nn>
//       epic_nearest_seeds on <dir>/cost.bin (w*h floats) and <dir>/seeds.bin (x y ints) -> labels.bin, index.bin (ints), dist.bin (floats).  No GPU.
//   epic_nn_tool time <dir> <w> <h> <nn> <reps>
//       the same call <reps> times: prints "host_ms" and the milliseconds of each (tools/bench_epic_nn.py); writes the outputs like `seeds`.  No GPU.
//   epic_nn_tool epic <dir> <count> <method> <saliency_th> <pref_nn> <pref_th> <nn> <coef_kernel> <euc> [workspace_bytes]
//       scene k of <dir>/sizes.txt (one "w h" per line): rgb_k.bin (3 planes of h*stride floats), matches_k.txt, edges_k.bin.  epic() image by image -> fx_k.bin,
//       fy_k.bin; epic_batch over all of them at once -> bfx_k.bin, bfy_k.bin; prints "rc k <epic> <epic_batch>" per scene.  Needs the GPU.
#include <chrono>
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

static int run_seeds(int argc, char **argv) {
    if (argc < 6) return 2;
    const std::string dir = argv[2];
    const int w = atoi(argv[3]), h = atoi(argv[4]), nn = atoi(argv[5]);
    epic_edges e;
    e.width = w; e.height = h;
    std::vector<int> seeds, labels;
    if (!rd(dir + "/cost.bin", e.cost) || e.cost.size() != (size_t)w * h || !rd(dir + "/seeds.bin", seeds)) { fprintf(stderr, "cost / seeds unreadable\n"); return 2; }
    epic_nn k;
    const int reps = argc > 6 ? atoi(argv[6]) : 0;                   // `time`
    if (reps) printf("host_ms");
    for (int r = 0; r < (reps ? reps : 1); r++) {
        const auto t0 = std::chrono::steady_clock::now();
        epic_nearest_seeds(seeds, e, nn, k, labels);
        if (reps) printf(" %.3f", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    if (reps) printf("\n");
    wr(dir + "/labels.bin", labels.data(), labels.size());
    wr(dir + "/index.bin", k.index.data(), k.index.size());
    wr(dir + "/dist.bin", k.dist.data(), k.dist.size());
    return 0;
}

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
    std::vector<int> ws(count), hs(count);
    {
        std::ifstream f((dir + "/sizes.txt").c_str());
        for (int k = 0; k < count; k++) if (!(f >> ws[k] >> hs[k])) { fprintf(stderr, "sizes.txt unreadable\n"); return 2; }
    }
    sfa_ctx *ctx = nullptr;
    if (sfa_ctx_create(0, &ctx) != SFA_OK) { fprintf(stderr, "%s\n", sfa_last_error(nullptr)); return 3; }
    std::vector<color_image_t *> lab(count);
    std::vector<epic_matches> m(count);
    std::vector<epic_edges> e1(count), e2(count);                    // epic() and epic_batch each add euc to their own copy
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
        if (!read_matches((dir + "/matches_" + s + ".txt").c_str(), m[k]) || !read_edges((dir + "/edges_" + s + ".bin").c_str(), ws[k], hs[k], e1[k])) {
            fprintf(stderr, "matches / edges of scene %d unreadable\n", k);
            return 2;
        }
        e2[k] = e1[k];
        image_t **all[4] = {&fx[k], &fy[k], &bx[k], &by[k]};
        for (image_t **im : all) { *im = image_new(ws[k], hs[k]); image_erase(*im); }
        rc1[k] = epic(ctx, fx[k], fy[k], lab[k], m[k], e1[k], &p);
        if (rc1[k] < 0) { fprintf(stderr, "epic: %s\n", sfa_last_error(ctx)); return 3; }
    }
    std::vector<const color_image_t *> labs(lab.begin(), lab.end());
    std::vector<const epic_matches *> ms(count);
    std::vector<epic_edges *> es(count);
    for (int k = 0; k < count; k++) { ms[k] = &m[k]; es[k] = &e2[k]; }
    epic_batch(ctx, count, bx.data(), by.data(), labs.data(), ms.data(), es.data(), &p, rc2.data(), budget);
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
    if (argc > 1 && (!strcmp(argv[1], "seeds") || (!strcmp(argv[1], "time") && argc > 6))) rc = run_seeds(argc, argv);
    else if (argc > 1 && !strcmp(argv[1], "epic")) rc = run_epic(argc, argv);
    if (rc == 2) fprintf(stderr, "usage: epic_nn_tool seeds dir w h nn | epic_nn_tool time dir w h nn reps | epic_nn_tool epic dir count method saliency_th pref_nn pref_th nn coef_kernel euc [workspace_bytes]\n");
    return rc;
}
