// Host side of tools/bench_ref_image.py: the route sfa_reference_lab_device replaces at acc_skip_pixel 0, as accumulate -fill ran it before -- rgb8_to_lab on
// the host (host/epic.cpp), then the upload of the three Lab planes -- timed per frame.
//   ref_image_route <w> <h> <frames> <repetitions>      prints one line per repetition: "route_ms <host function> <upload and wait> <both>", per frame
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "epic.h"                       // host/; brings include/slowflow_amd.h

static double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: ref_image_route w h frames repetitions\n"); return 2; }
    const int w = atoi(argv[1]), h = atoi(argv[2]), n = atoi(argv[3]), reps = atoi(argv[4]);
    sfa_ctx *ctx = nullptr;
    sfa_sequence *seq = nullptr;
    if (sfa_ctx_create(0, &ctx) != SFA_OK || sfa_sequence_create(ctx, w, h, 1, &seq) != SFA_OK) { fprintf(stderr, "%s\n", sfa_last_error(ctx)); return 3; }
    std::vector<color_image_t *> frames;
    unsigned state = 12345u;
    for (int i = 0; i < n; i++) {
        color_image_t *f = color_image_new(w, h);
        for (size_t k = 0; k < (size_t)3 * f->stride * h; k++) { state = state * 1664525u + 1013904223u; f->c1[k] = (float)(state >> 24); }
        frames.push_back(f);
    }
    for (int r = 0; r <= reps; r++) {                                          // repetition 0 warms up and is not printed
        double t_host = 0, t_up = 0;
        for (int i = 0; i < n; i++) {
            auto t0 = std::chrono::steady_clock::now();
            color_image_t *lab = rgb8_to_lab(frames[i], 1.0f);
            t_host += ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            if (sfa_sequence_upload(seq, 0, lab->c1, lab->stride) != SFA_OK || sfa_ctx_sync(ctx) != SFA_OK) { fprintf(stderr, "%s\n", sfa_last_error(ctx)); return 3; }
            t_up += ms_since(t0);
            color_image_delete(lab);
        }
        if (r) printf("route_ms %.4f %.4f %.4f\n", t_host / n, t_up / n, (t_host + t_up) / n);
    }
    for (color_image_t *f : frames) color_image_delete(f);
    sfa_sequence_destroy(seq);
    sfa_ctx_destroy(ctx);
    return 0;
}
