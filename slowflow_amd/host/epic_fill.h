// epic_fill.h -- dense_tracking's EpicFlow fill-in of one rate (dense_tracking.cpp:1265-1310): the consistent trajectories of the rate, interpolated to
// every pixel at every step, as the trajectory of a second hypothesis per pixel.  One call composes the library's three fill entry points
// (sfa_consistent_regions, sfa_fill_matches, sfa_fill_trajectories) around ONE epic_batch of r_Jets images, where the reference calls epic() r_Jets times.
#ifndef SLOWFLOW_AMD_HOST_EPIC_FILL_H
#define SLOWFLOW_AMD_HOST_EPIC_FILL_H

#include "epic.h"

/* the reference's parameters of the fill-in (dense_tracking.cpp:652-656): epic_params_default, then pref_nn 25, nn 160, coef_kernel 1.1f; method LA */
void epic_fill_params(epic_params_t *params);

/* removeSmallSegments' min_segment_size at :1265 */
enum { EPIC_FILL_MIN_SEGMENT = 100 };

struct epic_fill_stats {
    int kept_pixels;      /* the 1s of r_consistent after removeSmallSegments */
    int matches;          /* the sampled ones among them: the rows of every step's matches */
    int filled;           /* 1: fill_u, fill_v, fill_tracked were written; 0: the rate has no fill-in hypothesis and they are untouched */
};

/* One rate of one start_jet.  w x h: the accumulation grid, which is im_lab's and edges' size (acc_skip_pixel = skip_pixel; the reference resizes its
 * image by 1 / (skip_pixel + 1), :932-936).  acc_u, acc_v: [r_Jets][h][w] doubles and tracked [h][w] as sfa_accumulate_consistent* returns them with
 * all_steps 1.  epic_skip: the float of acc_epic_skip (:651).  Out: fill_u, fill_v [r_Jets][h][w], fill_tracked [h][w] = r_Jets -- the input of
 * sfa_hypothesis_energies* for the fill-in hypothesis.
 *
 * The edge costs.  epic() adds params->euc to the edge map it is given, and the reference hands the SAME forward_edges to every call of a start_jet
 * (:945, 1294), so its c-th call (counted over the rates as :1102 loops them, the steps ascending) sees the file's costs after c + 1 sequential fp32
 * additions.  `edges` here is the file's map and is not modified; call_index is the number of calls before this rate (0 for the first rate of a
 * start_jet).  Step j's image gets a copy advanced by call_index + j additions, so that epic_batch's own addition is the last one.  Returns the advanced
 * index, call_index + r_Jets, for the next rate: every step counts as a call whether or not it found matches, because epic() adds before it looks.
 *
 * A rate that keeps no match -- no consistent region of EPIC_FILL_MIN_SEGMENT pixels on a sample, or a step whose matches the consistency filter drops
 * entirely (epic's rc > 0) -- gets no fill-in hypothesis: stats->filled = 0, nothing is written, the index still advances.  This behaviour is ours: the
 * reference reads the flow planes epic() left unwritten in that case.
 * Returns < 0 on an error: -1 a GPU / argument error (sfa_last_error(ctx)), -2 sizes that do not agree. */
int epic_fill_rate(sfa_ctx *ctx, int w, int h, int r_Jets, int skip_pixel, float epic_skip, const double *acc_u, const double *acc_v, const int *tracked,
                   const color_image_t *im_lab, const epic_edges &edges, const epic_params_t *params, int call_index, double *fill_u, double *fill_v,
                   int *fill_tracked, epic_fill_stats *stats);

#endif
