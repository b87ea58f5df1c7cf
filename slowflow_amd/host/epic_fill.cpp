// epic_fill.cpp -- see epic_fill.h.
#include "epic_fill.h"

#include <cstring>

void epic_fill_params(epic_params_t *p) {                                    // dense_tracking.cpp:652-656
    epic_params_default(p);
    p->pref_nn = 25;
    p->nn = 160;
    p->coef_kernel = 1.1f;
}

namespace {
struct Planes {                                                             // r_Jets flow planes that free themselves
    std::vector<image_t *> im;
    Planes(int n, int w, int h) : im((size_t)n, nullptr) { for (image_t *&p : im) p = image_new(w, h); }
    ~Planes() { for (image_t *p : im) if (p) image_delete(p); }
    Planes(const Planes &) = delete;
    Planes &operator=(const Planes &) = delete;
};
}  // namespace

int epic_fill_rate(sfa_ctx *ctx, int w, int h, int r_Jets, int skip_pixel, float epic_skip, const double *acc_u, const double *acc_v, const int *tracked,
                   const color_image_t *im_lab, const epic_edges &edges, const epic_params_t *params, int call_index, double *fill_u, double *fill_v,
                   int *fill_tracked, epic_fill_stats *stats) {
    if (!ctx || !acc_u || !acc_v || !tracked || !im_lab || !params || !fill_u || !fill_v || !fill_tracked || !stats) return -1;
    if (w < 1 || h < 1 || r_Jets < 1 || skip_pixel < 0 || call_index < 0) return -2;
    if (im_lab->width != w || im_lab->height != h || edges.width != w || edges.height != h || edges.cost.size() != (size_t)w * h) return -2;
    stats->kept_pixels = stats->matches = stats->filled = 0;
    const int next_index = call_index + r_Jets;
    // r_consistent after removeSmallSegments (:1223-1226, 1265)
    std::vector<unsigned char> mask((size_t)w * h);
    if (sfa_consistent_regions(ctx, 1, w, h, tracked, &r_Jets, EPIC_FILL_MIN_SEGMENT, mask.data(), &stats->kept_pixels) != SFA_OK) return -1;
    // the matches of every step (:1274-1289)
    std::vector<int> xs((size_t)w), ys((size_t)h);
    int nx = 0, ny = 0;
    if (sfa_fill_samples(w, epic_skip, xs.data(), &nx) != SFA_OK || sfa_fill_samples(h, epic_skip, ys.data(), &ny) != SFA_OK) return -1;
    if (nx < 1 || ny < 1) return next_index;                                 // no sample on the grid: no match
    const size_t ns = (size_t)nx * ny;
    std::vector<float> rows((size_t)r_Jets * ns * 4);
    if (sfa_fill_matches(ctx, 1, r_Jets, w, h, acc_u, acc_v, mask.data(), xs.data(), nx, ys.data(), ny, skip_pixel + 1, rows.data(), &stats->matches) != SFA_OK)
        return -1;
    if (stats->matches < 1) return next_index;
    // one epic_batch of r_Jets images (:1294): the same image, step j's matches, the edge map as the reference's call call_index + j finds it
    std::vector<epic_matches> matches((size_t)r_Jets);
    std::vector<epic_edges> step_edges((size_t)r_Jets);
    epic_edges advanced = edges;
    if (params->euc)
        for (int c = 0; c < call_index; c++)
            for (float &v : advanced.cost) v += params->euc;
    for (int j = 0; j < r_Jets; j++) {
        const float *r = rows.data() + (size_t)j * ns * 4;
        matches[(size_t)j].m.assign(r, r + (size_t)stats->matches * 4);
        step_edges[(size_t)j] = advanced;
        if (params->euc) for (float &v : advanced.cost) v += params->euc;
    }
    Planes fx(r_Jets, w, h), fy(r_Jets, w, h);
    std::vector<const color_image_t *> labs((size_t)r_Jets, im_lab);
    std::vector<const epic_matches *> mp((size_t)r_Jets);
    std::vector<epic_edges *> ep((size_t)r_Jets);
    std::vector<int> rc((size_t)r_Jets, 0);
    for (int j = 0; j < r_Jets; j++) { mp[(size_t)j] = &matches[(size_t)j]; ep[(size_t)j] = &step_edges[(size_t)j]; }
    epic_batch(ctx, r_Jets, fx.im.data(), fy.im.data(), labs.data(), mp.data(), ep.data(), params, rc.data());
    for (int j = 0; j < r_Jets; j++)
        if (rc[(size_t)j] < 0) return -1;
    for (int j = 0; j < r_Jets; j++)
        if (rc[(size_t)j] > 0) return next_index;                            // a step without a usable match: no fill-in hypothesis for the rate
    // the planes as trajectories (:1299-1310)
    std::vector<const float *> px((size_t)r_Jets), py((size_t)r_Jets);
    for (int j = 0; j < r_Jets; j++) { px[(size_t)j] = fx.im[(size_t)j]->data; py[(size_t)j] = fy.im[(size_t)j]->data; }
    if (sfa_fill_trajectories(ctx, 1, r_Jets, w, h, fx.im[0]->stride, px.data(), py.data(), skip_pixel + 1, fill_u, fill_v, fill_tracked) != SFA_OK) return -1;
    stats->filled = 1;
    return next_index;
}
