// Host side of tests/test_epic_fill.py and tools/bench_epic_fill.py: dense_tracking's fill-in of the rates of one start_jet, twice.
//   epic_fill_tool <dir> <w> <h> <skip_pixel> <epic_skip> <euc> <r_Jets of rate 0> [<r_Jets of rate 1> ...]
//       <dir>/rgb.bin (3 planes of h * stride floats, 8-bit values), edges.bin (w * h floats), and per rate r: acc_u_r.bin, acc_v_r.bin ([r_Jets][h][w] doubles),
//       tracked_r.bin ([h][w] ints).
//   The plain chain, all on the host and in the reference's order: region growing in column-major scan order with a done list and in-place zeroing, the match
//   loop with its float step, ONE epic() call per step on ONE shared edge map (so that euc accumulates by itself, over the steps and over the rates), the
//   scaling -> chain_u_r.bin, chain_v_r.bin, chain_tracked_r.bin.  Then epic_fill_rate per rate with call_index carried across the rates -> fill_u_r.bin,
//   fill_v_r.bin, fill_tracked_r.bin.  Outputs start out as -7 and stay so where a rate is not filled.  Per rate one line
//   "rate r chain <filled> <kept> <matches> fill <filled> <kept> <matches> index <call_index after>" and one line "ms r grow <> regions <> chain <> fill <>":
//   the milliseconds of the region growing, of sfa_consistent_regions (the call, copies included), of the chain's r_Jets epic() calls and of epic_fill_rate.
//   Needs the GPU (epic()'s saliency filter runs there).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "epic_fill.h"

template <class T>
static void wr(const std::string &p, const std::vector<T> &d) { std::ofstream f(p.c_str(), std::ios::binary); f.write(reinterpret_cast<const char *>(d.data()), (std::streamsize)(d.size() * sizeof(T))); }
template <class T>
static bool rd(const std::string &p, std::vector<T> &out, size_t want) {
    std::ifstream f(p.c_str(), std::ios::binary | std::ios::ate);
    if (!f) return false;
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    out.resize((size_t)bytes / sizeof(T));
    f.read(reinterpret_cast<char *>(out.data()), bytes);
    return (bool)f && out.size() == want;
}
static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// removeSmallSegments(F, 0.1, min_size) restated: seeds in column-major order, a list grown over left, right, up, down neighbours that are not done and
// differ by at most 0.1 from the current pixel, everything reached marked done, short lists zeroed in place.  Returns the 1s left.
static int grow_segments(std::vector<int> &F, int w, int h, int min_size) {
    std::vector<int> done((size_t)w * h, 0), list((size_t)w * h);
    for (int u = 0; u < w; u++)
        for (int v = 0; v < h; v++) {
            if (done[(size_t)v * w + u]) continue;
            int count = 1, curr = 0;
            list[0] = v * w + u;
            while (curr < count) {
                const int a = list[(size_t)curr], cu = a % w, cv = a / w;
                const int nu[4] = {cu - 1, cu + 1, cu, cu}, nv[4] = {cv, cv, cv - 1, cv + 1};
                for (int i = 0; i < 4; i++) {
                    if (nu[i] < 0 || nv[i] < 0 || nu[i] >= w || nv[i] >= h) continue;
                    const int b = nv[i] * w + nu[i];
                    if (!done[(size_t)b] && std::abs(F[(size_t)a] - F[(size_t)b]) <= 0.1f) { list[(size_t)count++] = b; done[(size_t)b] = 1; }
                }
                curr++;
                done[(size_t)a] = 1;
            }
            if (count < min_size)
                for (int i = 0; i < count; i++) F[(size_t)list[(size_t)i]] = 0;
        }
    int ones = 0;
    for (int v : F) ones += v == 1;
    return ones;
}

int main(int argc, char **argv) {
    if (argc < 8) {
        fprintf(stderr, "usage: epic_fill_tool dir w h skip_pixel epic_skip euc r_Jets [r_Jets ...]\n");
        return 2;
    }
    const std::string dir = argv[1];
    const int w = atoi(argv[2]), h = atoi(argv[3]), skip_pixel = atoi(argv[4]);
    const float epic_skip = (float)atof(argv[5]);
    epic_params_t p;
    epic_fill_params(&p);
    p.euc = (float)atof(argv[6]);
    std::vector<int> rJ;
    for (int i = 7; i < argc; i++) rJ.push_back(atoi(argv[i]));
    const size_t pl = (size_t)w * h;
    sfa_ctx *ctx = nullptr;
    if (sfa_ctx_create(0, &ctx) != SFA_OK) { fprintf(stderr, "%s\n", sfa_last_error(nullptr)); return 3; }
    color_image_t *rgb = color_image_new(w, h);
    std::vector<float> planes;
    epic_edges edges;
    if (!rd(dir + "/rgb.bin", planes, (size_t)3 * rgb->stride * h) || !read_edges((dir + "/edges.bin").c_str(), w, h, edges)) { fprintf(stderr, "rgb.bin / edges.bin unreadable\n"); return 2; }
    memcpy(rgb->c1, planes.data(), planes.size() * sizeof(float));
    color_image_t *lab = rgb_to_lab(rgb);
    color_image_delete(rgb);
    epic_edges shared = edges;                                               // the chain's one edge map: every epic() call adds euc to it
    int call_index = 0;
    for (size_t r = 0; r < rJ.size(); r++) {
        const int J = rJ[r];
        const std::string s = std::to_string(r);
        std::vector<double> au, av;
        std::vector<int> tracked;
        if (!rd(dir + "/acc_u_" + s + ".bin", au, J * pl) || !rd(dir + "/acc_v_" + s + ".bin", av, J * pl) || !rd(dir + "/tracked_" + s + ".bin", tracked, pl)) {
            fprintf(stderr, "inputs of rate %zu unreadable\n", r);
            return 2;
        }
        // ---- the plain chain ----
        std::vector<int> cons(pl);
        for (size_t i = 0; i < pl; i++) cons[i] = tracked[i] == J ? 1 : 0;                                  // :1223-1226
        auto t0 = std::chrono::steady_clock::now();
        const int c_kept = grow_segments(cons, w, h, EPIC_FILL_MIN_SEGMENT);                                 // :1265
        const double grow_ms = ms_since(t0);
        std::vector<double> cu(J * pl, -7.0), cv(J * pl, -7.0), hu(J * pl, -7.0), hv(J * pl, -7.0);
        std::vector<int> ct(pl, -7), ht(pl, -7);
        int c_matches = 0, c_filled = 1;
        t0 = std::chrono::steady_clock::now();
        for (int j = 0; j < J; j++) {
            epic_matches m;
            for (int y = floor(0.5f * epic_skip); y < h; y += epic_skip)                                     // :1278-1289
                for (int x = floor(0.5f * epic_skip); x < w; x += epic_skip)
                    if (cons[(size_t)y * w + x] == 1) {
                        const float row[4] = {(float)x, (float)y, (float)(x + au[j * pl + (size_t)y * w + x] / (skip_pixel + 1)),
                                              (float)(y + av[j * pl + (size_t)y * w + x] / (skip_pixel + 1))};
                        m.m.insert(m.m.end(), row, row + 4);
                    }
            c_matches = m.count();
            image_t *wx = image_new(w, h), *wy = image_new(w, h);
            const int rc = epic(ctx, wx, wy, lab, m, shared, &p);                                             // :1294
            if (rc < 0) { fprintf(stderr, "epic: %s\n", sfa_last_error(ctx)); return 3; }
            if (rc > 0) c_filled = 0;
            if (c_filled)
                for (int y = 0; y < h; y++)
                    for (int x = 0; x < w; x++) {                                                            // :1304-1305
                        cu[j * pl + (size_t)y * w + x] = wx->data[(size_t)y * wx->stride + x] * (skip_pixel + 1);
                        cv[j * pl + (size_t)y * w + x] = wy->data[(size_t)y * wy->stride + x] * (skip_pixel + 1);
                    }
            image_delete(wx);
            image_delete(wy);
        }
        const double chain_ms = ms_since(t0);
        if (c_filled) ct.assign(pl, J);
        else { cu.assign(J * pl, -7.0); cv.assign(J * pl, -7.0); }
        // ---- sfa_consistent_regions alone, for its time ----
        std::vector<unsigned char> mask(pl);
        int kept = 0;
        t0 = std::chrono::steady_clock::now();
        if (sfa_consistent_regions(ctx, 1, w, h, tracked.data(), &J, EPIC_FILL_MIN_SEGMENT, mask.data(), &kept) != SFA_OK) { fprintf(stderr, "%s\n", sfa_last_error(ctx)); return 3; }
        const double regions_ms = ms_since(t0);
        // ---- epic_fill_rate ----
        epic_fill_stats st;
        t0 = std::chrono::steady_clock::now();
        const int next = epic_fill_rate(ctx, w, h, J, skip_pixel, epic_skip, au.data(), av.data(), tracked.data(), lab, edges, &p, call_index, hu.data(), hv.data(),
                                        ht.data(), &st);
        const double fill_ms = ms_since(t0);
        if (next < 0) { fprintf(stderr, "epic_fill_rate: %d %s\n", next, sfa_last_error(ctx)); return 3; }
        call_index = next;
        wr(dir + "/chain_u_" + s + ".bin", cu); wr(dir + "/chain_v_" + s + ".bin", cv); wr(dir + "/chain_tracked_" + s + ".bin", ct);
        wr(dir + "/fill_u_" + s + ".bin", hu); wr(dir + "/fill_v_" + s + ".bin", hv); wr(dir + "/fill_tracked_" + s + ".bin", ht);
        printf("rate %zu chain %d %d %d fill %d %d %d index %d\n", r, c_filled, c_kept, c_matches, st.filled, st.kept_pixels, st.matches, call_index);
        printf("ms %zu grow %.3f regions %.3f chain %.3f fill %.3f\n", r, grow_ms, regions_ms, chain_ms, fill_ms);
    }
    color_image_delete(lab);
    sfa_ctx_destroy(ctx);
    return 0;
}
