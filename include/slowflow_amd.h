/*
 * slowflow_amd.h -- C-ABI of the MI355X-native (gfx950 HIP) implementation of slowflow's variational
 * optical-flow refinement hot path.  Plain pointers and sizes only; every entry point names the
 * reference interface it replaces (file:line relative to the reference root).
 *
 * Conventions (identical to the reference, epic_flow_extended/image.h:17-43):
 *   - planes are fp32, row-major, `stride` floats per row (stride >= width); a colour image is 3 planes
 *     of height*stride floats each; only the `width` valid columns of a row are read or written,
 *   - all pointers below are HOST pointers unless a function says "device-resident"; the library owns
 *     every device buffer (through the context),
 *   - functions return 0 (SFA_OK) or a negative sfa_status; they never exit() (the reference does:
 *     image.c:19-30, solver.c:75-78); sfa_last_error() gives the message,
 *   - a context is bound to one GPU and one HIP stream; it is thread-compatible, not thread-safe: use one
 *     context per host thread (the reference runs one Variational_MT per OpenMP thread, slow_flow.cpp:706).
 * There is NO CPU fallback: without a HIP device every compute entry point fails with SFA_ERR_NO_DEVICE.
 */
#ifndef SLOWFLOW_AMD_H
#define SLOWFLOW_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFA_VERSION 1
#define SFA_MAX_REF 8          /* slow_flow_S - 1 <= 8: windows of up to 17 frames (4 until round 5) */

typedef enum {
    SFA_OK = 0,
    SFA_ERR_ARG = -1,          /* bad argument (null pointer, size, unsupported S) */
    SFA_ERR_HIP = -2,          /* a HIP runtime call failed */
    SFA_ERR_NO_DEVICE = -3,    /* no usable GPU */
    SFA_ERR_REF_FRAME = -4,    /* "Frame compared to reference frame is the reference frame itself" (variational_aux_mt.cpp:419) */
    SFA_ERR_TIMEOUT = -5,      /* a bounded in-kernel wait gave up (solver pipeline) */
    SFA_ERR_UNSUPPORTED = -6   /* a path that needs the absent third-party hook (occlusion graph cut) */
} sfa_status;

/* layout-compatible with image_t / color_image_t (epic_flow_extended/image.h:17-33) */
typedef struct sfa_image { int width, height, stride; float *data; } sfa_image;
typedef struct sfa_color_image { int width, height, stride; float *c1, *c2, *c3; } sfa_color_image;

/* penalty ids as Variational_AUX_MT::select_robust_function (variational_aux_mt.cpp:909-925):
 * 0 quadratic, 2 lorentzian, 3 truncated modified L1, 4 geman-mcclure, anything else modified L1 */
typedef struct sfa_penalty { int id; float eps; float trunc; } sfa_penalty;

/* the cfg keys Variational_MT reads (variational_mt.cpp:173-192, 533-568), already parsed */
typedef struct sfa_params {
    int   S;                    /* slow_flow_S */
    int   one_direction;        /* slow_flow_method == "forward" */
    int   smoothing;            /* slow_flow_smoothing */
    int   dataterm_norm;        /* slow_flow_dataterm */
    int   niter_alter, niter_outer, niter_inner, niter_solver;
    float thres_outer, thres_inner;
    float sor_omega;
    float alpha, gamma, delta;
    sfa_penalty robust_color, robust_grad, robust_reg;
    float rho[SFA_MAX_REF], omega[SFA_MAX_REF];      /* slow_flow_rho_<a>, slow_flow_omega_<a> */
    int   hbit;                 /* 16bit */
    float norm_avg[3], norm_std[3];                  /* slow_flow_img_norm_{avg,std}_{1,2,3} */
    int   occlusion_reasoning;  /* slow_flow_occlusion_reasoning */
    int   layers;               /* slow_flow_layers */
    float p_scale;              /* slow_flow_p_scale */
    float presmooth_sigma;      /* > 0 when cfg `sigma` > 0: value of slow_flow_sigma */
    /* discrete occlusion step between alternations (optimizeOcc, variational_aux_mt.cpp:758-887) */
    float occlusion_penalty;    /* slow_flow_occlusion_penalty ("1.0"): cost of the label "occluded in the future" */
    float occlusion_alpha;      /* slow_flow_occlusion_alpha ("0.5"): Potts weight between 4-neighbours */
    int   niter_graphc;         /* slow_flow_niter_graphc ("10"): expansion iterations; a two-label cut is exact after one */
    /* ADDITIVE key slow_flow_sor_order: 0 = "lexicographic" (default; the reference's raster order, results identical to sor_coupled), 1 = "red_black":
     * a DIFFERENT ALGORITHM (two-colour sweeps of the same point update) that does not reproduce the reference -- after 30 sweeps its increment is 1e-2..1e-1
     * away -- kept as a labelled low-latency mode for a single frame pair; every result produced with it is to be labelled as such */
    int   sor_order;
} sfa_params;

/* variational_params_t (epic_flow_extended/variational.h:16-25), same layout */
typedef struct sfa_params_2frame {
    float alpha, gamma, delta, sigma;
    int niter_outer, niter_inner, niter_solver;
    float sor_omega;
} sfa_params_2frame;

typedef struct sfa_ctx sfa_ctx;

/* ---- context ------------------------------------------------------------------------------------ */
int  sfa_device_count(void);
int  sfa_ctx_create(int device, sfa_ctx **out);
void sfa_ctx_destroy(sfa_ctx *ctx);
const char *sfa_last_error(const sfa_ctx *ctx);     /* ctx may be NULL: last error of the calling thread */
int  sfa_ctx_sync(sfa_ctx *ctx);
void sfa_params_default(sfa_params *p);             /* driver defaults, slow_flow.cpp:64-128 */

/* ---- the path itself ---------------------------------------------------------------------------- */

/* Replaces Variational_MT::variational (variational_mt.cpp:526-784): coarse-to-fine refinement of (wx,wy),
 * in place.  frames[f] = first plane of colour frame f (3 consecutive planes), f = 0 .. 2*(S-1), reference
 * frame in the middle; chw = channel weights (setChannelWeights, :521) or NULL for all ones;
 * occlusions_out (h*stride floats) or NULL; change[2] = returned Point2f (mean |du|, mean |dv| of the last
 * outer iteration of level 0). */
int sfa_variational(sfa_ctx *ctx, const sfa_params *p, float *wx, float *wy, int w, int h, int stride,
                    const float *const *frames, int n_frames, const float *const chw[3],
                    float *occlusions_out, float change[2]);

/* The reference's ORIGINAL two-frame refinement, `variational(wx, wy, im1, im2, params)` (epic_flow_extended/variational.c:101-143
 * with variational_aux.c): one level, fixed modified-L1 penalties, weights halved; wx, wy refined in place.  im1, im2: first
 * plane of 3.  Pinned end to end, bit for bit, against the compiled reference.  p == NULL: variational_params_default. */
int sfa_variational_2frame(sfa_ctx *ctx, float *wx, float *wy, int w, int h, int stride, const float *im1, const float *im2, const sfa_params_2frame *p);
void sfa_params_2frame_default(sfa_params_2frame *p);          /* variational.c:86-98 */
/* n independent pairs of one size (1 <= n <= 128), one parameter set, refined in place in one launch sequence on the context's stream: pair i
 * (wx[i], wy[i], im1[i], im2[i], each laid out as for sfa_variational_2frame) comes out bit-identical to sfa_variational_2frame on that pair alone,
 * whatever n and its position.  The adaptiveFR program refines its samples through this.  (csrc/two_frame.hip: the single call is this one with n = 1, and
 * both run the launch sequence of the resident pair jobs below on a pair job that lives for the call, with the stored derivative stack.) */
int sfa_variational_2frame_batch(sfa_ctx *ctx, int n, float *const *wx, float *const *wy, int w, int h, int stride, const float *const *im1,
                                 const float *const *im2, const sfa_params_2frame *p);
/* EpicFlow's geodesic k nearest seeds (epic_aux.cpp:44-380; host/epic.cpp: epic_nearest_seeds) for n images of one size w x h in one call, on the GPU
 * (csrc/epic_nn.hip): the distance transform of the seeds over the cost map with label propagation, the graph of the label regions, and for every seed its
 * nn nearest seeds on that graph.  Image i: cost[i] = w * h floats, row-major, the constant `euc` already added; seeds_xy[i] = 2 * ns[i] ints (x, y), a later
 * seed on the same pixel wins; labels[i] (out) = w * h ints, the closest seed of every pixel, -1 where none reaches; nn_index[i], nn_dist[i] (out) =
 * ns[i] * nn entries, seed q's neighbours in the order the reference's search finds them and their raw geodesic distances (no kernel applied), -1 /
 * 0x7F7F7F7F where fewer than nn exist.  Every output equals the host function's bit for bit, whatever n and the image's position.
 * THE DOMAIN of a cost is +0 ... +Inf, subnormals, FLT_MAX and +Inf included (a pixel of cost +Inf is never reached; a seed on one has every distance +Inf); -0.0
 * counts as +0.0 and gives the bits +0.0 gives.  A NaN or a cost below 0 is refused (the host function itself is undefined there: its sort of the border lengths
 * loses its ordering, and the search the bound its heap is sized by).  tests/test_epic_value_ranges.py walks the domain.
 * Host pointers; the call waits for its results.  The batch runs in sub-batches whose device memory (planes, the border table, the search's visited
 * sets and heaps, the heaps sized from the counted graph: 1 + min((nn - 1) * largest degree, 2 * edges) entries per seed) stays within workspace_bytes (0:
 * half of the GPU's free memory); status[i] = 0: computed, 1: image i does not fit the budget even alone -- its outputs are untouched and the caller
 * computes it on the host.  In the default mode the visited sets of an image are ns * ns floats, held for all its seeds at once; in the compact mode
 * (sfa_ctx_set_epic_search) an image is flagged only if its planes, table, rows and the search of one 64-seed workgroup exceed the budget.
 * Refused with SFA_ERR_ARG, the argument named and nothing launched: n < 1, w or h < 1, nn < 1, an ns[i] < 1, a null pointer, a seed outside the image,
 * a cost that is NaN or below 0 (image and pixel named), w * h > 2^29 or ns[i] * nn > 2^31 - 1 (32-bit indices), min(w, h) > 4000 (two diagonals of the sweep
 * live in LDS). */
int sfa_epic_nearest_seeds_batch(sfa_ctx *ctx, int n, int w, int h, const float *const *cost, const int *const *seeds_xy, const int *ns, int nn,
                                 int *const *labels, int *const *nn_index, float *const *nn_dist, size_t workspace_bytes, int *status);
/* The kernel time of the context's last sfa_epic_nearest_seeds_batch in milliseconds, from HIP events around the launches, summed over its sub-batches:
 * ms[0] initial state and seeds, ms[1] the sweeps, ms[2] the region graph (border count, table, rows), ms[3] the graph search, ms[4] the lists.
 * Copies, allocations and the waits between the stages are not in it (tools/bench_epic_nn.py). */
int sfa_epic_nn_stage_ms(sfa_ctx *ctx, float ms[5]);
/* How the graph search of the nearest-seeds stage holds its state, per context; it applies to sfa_epic_nearest_seeds_batch and sfa_epic_batch and so to
 * everything above them, and never changes a bit of any output.
 *   SFA_EPIC_SEARCH_DENSE (the default)  every seed of an image owns a row of ns floats, and an image is computed only if all its rows and heaps fit the
 *     budget at once.
 *   SFA_EPIC_SEARCH_COMPACT  the seeds of an image are searched in slices -- runs of whole 64-seed workgroups, in (image, seed) order -- that share one
 *     workspace as large as the largest slice, and an image takes the smaller of two forms of visited set: the dense row, 4 * ns bytes per seed, or an
 *     open-addressing map of node -> distance, 8 bytes per slot, its slots the smallest power of two >= twice the heap's bound (dense on a tie).  An image
 *     whose whole search fits is one slice.  ms[3] of sfa_epic_nn_stage_ms sums the slices, the clearing of their workspace included.
 * Any other mode: SFA_ERR_ARG, `mode` named, nothing changed. */
#define SFA_EPIC_SEARCH_DENSE 0
#define SFA_EPIC_SEARCH_COMPACT 1
int sfa_ctx_set_epic_search(sfa_ctx *ctx, int mode);
/* The graph search of the context's last nearest-seeds stage (the last sfa_epic_nearest_seeds_batch, or the interpolation's search of the last
 * sfa_epic_batch), summed over its sub-batches: info[0] slices launched (the default mode: one per image), info[1] images searched with the dense set,
 * info[2] images searched with the sparse set, info[3] the largest search workspace in bytes (visited sets and heaps). */
int sfa_epic_nn_search_info(sfa_ctx *ctx, long long info[4]);
/* EpicFlow's per-seed model fit and its dense application (epic_aux.cpp:386-497; host/epic.cpp: epic_fit_localaffine, epic_fit_nadarayawatson and the apply
 * loops of epic()) for n images of one size w x h in one call, on the GPU (csrc/epic_fit.hip).  method 0: locally-weighted affine (LA), 1: Nadaraya-Watson
 * (NW).  Image i: seeds_xy[i] = 2 * ns[i] ints (x, y); vects[i] = 2 * ns[i] floats; nn_index[i], nn_weight[i] = ns[i] * nn entries, the lists of
 * sfa_epic_nearest_seeds_batch AFTER the kernel function has been applied to the distances (the epic_nn that epic_fit_localaffine takes: the library forms no
 * exp, the weights are the caller's bits); labels[i] = w * h ints.  Out: model[i] = ns[i] * 6 (LA) or ns[i] * 2 (NW) floats, or model == NULL; flow_x[i],
 * flow_y[i] = h rows of `stride` floats, of which columns >= w are not written.  flow_x == flow_y == NULL: only the models are computed, labels may be NULL
 * and w, h are checked but not used.  Models and flows equal the host code's bit for bit (one lane sums one seed's list in list order; fp64 normal equations;
 * no fused multiply-add); where NW's weights sum to 0 both give a NaN, whose sign is the platform's.
 * List entries with an index < 0 are skipped as on the host; entries with an index >= ns[i] are skipped too, and a pixel whose label lies outside
 * [0, ns[i]) gets 0.0f in both planes: the host code indexes out of bounds in both cases, the values are this library's choice.
 * Sub-batches, workspace_bytes and status as for sfa_epic_nearest_seeds_batch: everything allocated for a sub-batch stays within workspace_bytes (0: half of
 * the GPU's free memory); status[i] = 1: image i does not fit even alone, its outputs are untouched and the caller computes it on the host.
 * Refused with SFA_ERR_ARG, the argument named and nothing launched: n < 1, w or h < 1, nn < 1, an ns[i] < 1, a method other than 0 or 1, stride < w, a null
 * pointer that is needed (only one of flow_x / flow_y, labels with flows, model without them, any image's own pointer), w * h > 2^29, ns[i] * nn > 2^31 - 1. */
int sfa_epic_interpolate_batch(sfa_ctx *ctx, int n, int w, int h, int method, const int *const *labels, const int *const *seeds_xy, const float *const *vects,
                               const int *ns, int nn, const int *const *nn_index, const float *const *nn_weight, float *const *flow_x, float *const *flow_y,
                               int stride, float *const *model, size_t workspace_bytes, int *status);
/* The kernel time of the context's last sfa_epic_interpolate_batch in milliseconds, from HIP events, summed over its sub-batches: ms[0] the fit, ms[1] the
 * dense application.  Copies and allocations are not in it (tools/bench_epic_fit.py). */
int sfa_epic_fit_stage_ms(sfa_ctx *ctx, float ms[2]);
/* epic_params_t's numeric fields (host/epic.h, epic_flow_extended/epic.h:6-15); method 0: locally-weighted affine (LA), 1: Nadaraya-Watson (NW).  euc is
 * carried for completeness: sfa_epic_batch takes cost maps that already hold it. */
typedef struct sfa_epic_params {
    int method;
    float saliency_th;
    int pref_nn;
    float pref_th;
    int nn;
    float coef_kernel;
    float euc;
} sfa_epic_params;
/* epic() (epic_flow_extended/epic.cpp:147-235; host/epic.cpp) for n images of one size w x h as one chain on the GPU (csrc/epic_batch.hip,
 * csrc/epic_filter.hip): nothing but the inputs goes up, nothing but the two flow planes (and the survivors, if asked for) comes down, and the planes equal
 * epic()'s bit for bit.  Image i: lab[i] = 3 planes of h * lab_stride floats (read only when saliency_th != 0; lab may be NULL otherwise); cost[i] = w * h
 * floats, euc already added; matches[i] = 4 * nm[i] floats (x1 y1 x2 y2), nm[i] may be 0; flow_x[i], flow_y[i] (out) = h rows of flow_stride floats,
 * columns >= w are not written.  Per sub-batch, in epic()'s order: the clamp of the matches to the image; if saliency_th != 0 the saliency
 * (image.c:729-791, sigma 0.8 and 1.0) and its filter, whose index is the host's float expression (int)(y1 * stride + x1) with stride = ceil(w / 4) * 4;
 * if pref_nn != 0 the nearest seeds with min(pref_nn + 1, count) neighbours, the kernel weights expf(-coef_kernel * d) + 1e-08, the Nadaraya-Watson
 * estimate and the consistency filter |estimate - vector|^2 < pref_th^2; then for the images with matches left the nearest seeds with min(nn, count)
 * neighbours, the weights, the fit of `method` and its dense application.  The neighbour count is per image.
 * rc[i] (out) = epic()'s return value: 0, or 1 = no match (left): the flow planes of such an image are untouched and it takes no further part.  counts
 * (or NULL): per image the matches that came in, that passed the saliency filter, that passed the consistency filter (a filter that is off passes all).
 * kept_matches (or NULL): kept_matches[i] receives the 4 * counts[i][2] floats of the survivors in list order (room for 4 * nm[i]).
 * Sub-batches, workspace_bytes and status as for sfa_epic_nearest_seeds_batch: nothing allocated exceeds workspace_bytes (0: half of the GPU's free memory);
 * both searches run in the context's mode (sfa_ctx_set_epic_search: the ns * ns floats per image are the default mode's only);
 * status[i] = 1: image i does not fit even alone -- rc[i], counts[i] and its outputs are untouched and the caller computes it on the host.  No result depends
 * on the sub-batch cut or on an image's place in the batch.
 * Refused with SFA_ERR_ARG, the argument named and nothing launched: n < 1, w or h < 1, nn < 1, pref_nn < 0, a method other than 0 or 1, flow_stride < w,
 * with the saliency filter lab_stride < w or w or h <= 8 (its Gaussian), nm[i] < 0, a null pointer that is needed, a match coordinate that is not finite,
 * a cost that is NaN or below 0 (image and pixel named; the domain of cost[i] is sfa_epic_nearest_seeds_batch's: +0 ... +Inf, -0.0 counts as +0.0),
 * w * h > 2^29, nm[i] * nn > 2^31 - 1, min(w, h) > 4000. */
int sfa_epic_batch(sfa_ctx *ctx, int n, int w, int h, const sfa_epic_params *p, const float *const *lab, int lab_stride, const float *const *cost,
                   const float *const *matches, const int *nm, float *const *flow_x, float *const *flow_y, int flow_stride, int *rc, int (*counts)[3],
                   float *const *kept_matches, size_t workspace_bytes, int *status);
/* The saliency of n Lab images of one size (image.c:729-791; host/epic.cpp: saliency()) in one call, every step on the GPU: out[i] = h * stride floats, the
 * smallest eigenvalue of the smoothed autocorrelation matrix, columns >= w zero.  lab[i] = 3 planes of h * stride floats.  Refused: n outside 1 .. 4096, an
 * image not larger than either Gaussian (sfa_gaussian_presmooth's rule), h < 2, stride < w, a sigma that is not positive, a null pointer. */
int sfa_epic_saliency_batch(sfa_ctx *ctx, int n, int w, int h, const float *const *lab, int stride, float sigma_image, float sigma_matrix, float *const *out);
/* The kernel time of the context's last sfa_epic_batch in milliseconds, from HIP events, summed over its sub-batches: ms[0] saliency, ms[1] clamp, filters,
 * compactions, seeds and vectors, ms[2] the first nearest-seeds stage, ms[3] its weights and estimate, ms[4] the second nearest-seeds stage, ms[5] its
 * weights, ms[6] the fit, ms[7] the dense application.  A refused call leaves them as they were. */
int sfa_epic_batch_stage_ms(sfa_ctx *ctx, float ms[8]);
/* adaptiveFR's flow-magnitude quantile (adaptiveFR.cpp:644-668) on the GPU.  n host fields (u[i], v[i]: w x h, row stride `stride`); every value is scaled
 * by flow_scale first (one fp32 multiply, image_mul_scalar), m = sqrtf(u*u + v*v) in IEEE fp32; the order statistics are found by an exact radix select
 * over the bit patterns of m.  NaN magnitudes sort above +Inf (their bit order; std::sort has no defined order for them), Inf where it belongs.
 * *quantile = the rank rule below on the sorted m (as doubles), *max_magnitude = the largest m.  Same bits on every run. */
int sfa_flow_magnitude_quantile(sfa_ctx *ctx, int n, const float *const *u, const float *const *v, int w, int h, int stride, float flow_scale, float q,
                                double *quantile, double *max_magnitude);
/* The rank rule of adaptiveFR.cpp:660-666 for N sorted values, host only: np = q * (float)N - 1 (N goes through float: exact up to 2^24);
 * np < (float)(N - 1) and fmodf(np, 2) == 0 -> *average = 1, the mean of ranks *k0 = (int)np and *k1 = *k0 + 1; else *average = 0, *k0 = *k1 = (int)ceilf(np).
 * SFA_ERR_ARG for N == 0, q outside (0, 1] and an N, q whose rank falls outside the N values (the reference reads past its array there). */
int sfa_quantile_ranks(size_t N, float q, size_t *k0, size_t *k1, int *average);
/* The same quantile and maximum (adaptiveFR.cpp:644-668) for G groups of flow fields that already live in GPU memory, in one launch sequence on the
 * context's stream; nothing is copied from or to the host and the call does not wait for the GPU (pair it with sfa_ctx_wait_stream /
 * sfa_ctx_signal_stream like the other device entry points).  Element (group g, field f, row y, column x) of u is u_dev[g strides[0] + f strides[1] +
 * y strides[2] + x strides[3]] (element strides), the same for v_dev: planar [G][n][2][h][w] (v_dev = u_dev + the plane stride), channels-last
 * [G][n][h][w][2] (v_dev = u_dev + 1), padded rows and slices are read in place.  Group g takes its first counts[g] fields (counts: host, G entries;
 * NULL = all n).  out_dev[g][0] = the quantile of group g under sfa_quantile_ranks' rule over its counts[g] w h magnitudes, out_dev[g][1] their maximum:
 * the bits sfa_flow_magnitude_quantile returns for the same values.  The scratch (4 bytes per value, the histograms) stays on the context from call
 * to call; a call that needs more than any before it waits for the stream once, to replace it.
 * SFA_ERR_ARG, naming the argument, before anything is launched: G outside 1..64, n < 1, w or h < 1, a count outside 1..n, u_dev / v_dev / out_dev that
 * are not device memory of the context's GPU (or views that leave their allocation), a row or column stride < 1, a negative group or field stride,
 * strides under which two elements of one group share an address, out_dev overlapping the flows, more than 2^32 - 1 values in a group, and whatever
 * sfa_quantile_ranks refuses for a group (the group is named). */
int sfa_flow_magnitude_quantiles_device(sfa_ctx *ctx, int G, int n, const int *counts, const float *u_dev, const float *v_dev, const long long strides[4],
                                        int w, int h, float flow_scale, float q, double *out_dev);
/* dense_tracking's first stage, accumulateConsistentBatches (utils/utils.cpp:517-617, with bilinearInterp<double>, utils/utils.h:182-217), for n
 * independent segments of FF steps in one launch.  Segment s, step f reads the host planes fwd_u/fwd_v/bwd_u/bwd_v[s * FF + f] (w x h, row stride
 * `stride` floats; widened to double exactly, as readGTMiddlebury's CV_64FC2) and, where masks != NULL, masks[s * FF + f] (uint8, row stride `stride`
 * bytes; 0 = occluded, the reference's value after 255 - x).  The grid is sfa_accumulate_grid(w, h, skip).  Outputs (host, packed): acc_u, acc_v
 * [n][S][gh][gw] doubles with S = FF (all_steps != 0) or 1 (the last step only), tracked [n][gh][gw] (FF = fully tracked; else the first inconsistent
 * step + 1, or 0 with discard).  IEEE fp64 without contraction: bit-identical to a plain restatement of the reference's statements. */
int sfa_accumulate_consistent(sfa_ctx *ctx, int n, int FF, int w, int h, int stride, const float *const *fwd_u, const float *const *fwd_v,
                              const float *const *bwd_u, const float *const *bwd_v, const unsigned char *const *masks, double epsilon, int skip, int discard,
                              int all_steps, double *acc_u, double *acc_v, int *tracked);
/* The accumulation grid of utils.cpp:522-526, host only: xy_incr = skip + 1, xy_start = (int)(0.5f * skip), *gh = floor((1.0f * h) / xy_incr),
 * *gw = floor((1.0f * w) / xy_incr); grid pixel (x, y) sits on image pixel (x * xy_incr + xy_start, y * xy_incr + xy_start).
 * SFA_ERR_ARG for w, h < 1, skip < 0 and an empty grid. */
int sfa_accumulate_grid(int w, int h, int skip, int *gw, int *gh);
/* Where a rate's jet files sit relative to the tracking frames (dense_tracking.cpp:1134-1146, :1171-1177): the planes as read, the crop of
 * utils.cpp:308-318 and the factor the reference resizes by.  The target is lrint(cw * (double)rescale) x lrint(ch * (double)rescale) (cvRound:
 * halves to even) and must be the w x h of the call.  A source without a crop, of the target's size and with rescale 1 is the identity: it is not
 * resampled (the reference's identity resize can only turn -0.0 into +0.0).  sfa_jet_source_default fills the identity of a w x h plane. */
typedef struct sfa_jet_source {
    int sw, sh, stride;     /* the planes as read; row stride in elements */
    int x0, y0, cw, ch;     /* crop: columns x0 .. x0+cw-1, rows y0 .. y0+ch-1 (utils.cpp:308-318); 0, 0, sw, sh = none */
    float rescale;          /* (1.0f * w) / cw, dense_tracking.cpp:1142 */
} sfa_jet_source;
void sfa_jet_source_default(sfa_jet_source *src, int w, int h, int stride);
/* Stage binding: n flow fields u[k], v[k] (host float planes as src describes them; stride padding is never read) cropped, resized as
 * cv::resize(src, dst, Size(0, 0), rescale, rescale, INTER_LINEAR) resizes CV_64FC2 and multiplied by (double)rescale (:1143-1146), on the GPU.
 * The source coordinate is (float)((d + 0.5) * (1.0 / (double)rescale) - 0.5), its floor the left tap, taps clamped at the border with weight 0; the
 * weights 1.f - f and f are floats, samples, products and sums fp64 without contraction, rows first, then columns (OpenCV's
 * HResizeLinear<double, double, float>).  OpenCV is not in the tree: parity unpinned, pinned to tests/jet_resample_ref.py.  Always resamples, the
 * identity included.  out_u, out_v: packed [n][h][w] doubles.  SFA_ERR_ARG, naming the argument: a target other than w x h (both sizes are named), a
 * crop outside the planes, rescale <= 0. */
int sfa_jet_flow_resample(sfa_ctx *ctx, int n, const sfa_jet_source *src, const float *const *u, const float *const *v, int w, int h, double *out_u,
                          double *out_v);
/* Stage binding: n raw 8-bit occlusion images (row stride src->stride bytes) -> packed [n][h][w] masks, 0 = occluded: cv::resize(..., INTER_CUBIC) on
 * 8-bit (taps floor(f) - 1 .. floor(f) + 2 with clamped indices, Keys' cubic with A = -0.75 in fp32, each coefficient rounded to a 16-bit integer at 11
 * fractional bits, integer row sums, columns ending in (sum + 2^21) >> 22 saturated to 0 .. 255), the 3 x 3 median with a replicated border, 255 - x
 * (:1177-1189).  With rescale 1 the cubic is the identity.  Parity unpinned, as the median: OpenCV's SIMD build rounds the column pass in float, which can
 * differ by one grey level within two source pixels of a label edge.  A crop is refused by name (the reference's crop() reads the 8-bit Mat through
 * at<Vec2d>: undefined). */
int sfa_jet_occlusion_decode(sfa_ctx *ctx, int n, const sfa_jet_source *src, const unsigned char *const *occ, int w, int h, unsigned char *mask);
/* sfa_accumulate_consistent for jets of another size: the flows are the planes src describes and are brought to w x h on the GPU as
 * sfa_jet_flow_resample does it; occ (or NULL) are the RAW occlusion images as read, decoded on the GPU as sfa_jet_occlusion_decode does it.  The
 * resampled flows are doubles, and the kernel gathers them as such.  An identity source runs sfa_accumulate_consistent's float path: the same kernel,
 * the same bits.  stage_ms: NULL or 2 floats, the milliseconds of the resampling / interleaving kernels and of the accumulation kernel (HIP events). */
int sfa_accumulate_consistent_scaled(sfa_ctx *ctx, int n, int FF, int w, int h, const sfa_jet_source *src, const float *const *fwd_u,
                                     const float *const *fwd_v, const float *const *bwd_u, const float *const *bwd_v, const unsigned char *const *occ,
                                     double epsilon, int skip, int discard, int all_steps, double *acc_u, double *acc_v, int *tracked, float *stage_ms);
/* dense_tracking's unary energies (dense_tracking.cpp:1219-1257): the cfg keys of setDefault (:118-165) with the C types the reference reads them in
 * (:606-623, :489-495, :661-675).  sfa_energy_params_default fills setDefault's values, weight 0 and skip 1. */
typedef struct sfa_energy_params {
    float  acc_jc;                  /* acc_jet_consistency ("1.0") */
    float  acc_bc;                  /* acc_brightness_constancy ("0.1") */
    float  acc_gc;                  /* acc_gradient_constancy ("1.0") */
    float  acc_occ;                 /* acc_occlusion_penalty ("500.0") */
    double acc_cv;                  /* acc_cv ("0.0") */
    double acc_temporal_occ;        /* acc_temporal_occ ("10.0") */
    float  occlusion_threshold;     /* acc_occlusion_threshold ("5.0") */
    float  occlusion_fb_threshold;  /* acc_occlusion_fb_threshold ("5.0") */
    int    penalty;                 /* acc_penalty_fct_data ("1"): 0 quadratic, 1 modified L1, anything else Lorentzian */
    double penalty_eps;             /* acc_penalty_fct_data_eps ("0.001"); the penalty's constructor takes it as float */
    float  weight;                  /* weight_jet_estimation[r]: jet_weight[r], or r where none is given */
    int    skip;                    /* acc_skip_pixel: the grid of sfa_accumulate_grid and addBCGC's radius (int)(0.5f * (skip + 1)) */
} sfa_energy_params;
void sfa_energy_params_default(sfa_energy_params *p);
/* The energy of every hypothesis of n segments of one rate: adaptFPS(Jets), setOcclusions, addJC + addBCGC + addOC + weight (utils/hypothesis.h:136-175,
 * utils/hypothesis.cpp:172-215, dense_tracking.cpp:176-365).  acc_u, acc_v, tracked: as sfa_accumulate_consistent returns them for FF = r_Jets and
 * all_steps = 1 ([n][r_Jets][gh][gw] doubles, [n][gh][gw]); a hypothesis exists where tracked == r_Jets.  frames[s * (Jets + 1) + f]: the first plane of
 * 3 (c1, c2, c3, each h * stride floats) of normalised colour frame f of segment s; dx, dy are derived on the GPU.  fwd_u .. bwd_v[s * Jets + t]: rate
 * acc_min_fps's flows (w x h, row stride `stride`), or all four NULL for the empty Mats a rate before acc_min_fps sees (every step t >= 1 occluded).
 * Outputs [n][gh][gw]: energy (the fp32 sum as a double; +Inf where there is no hypothesis) and occ_bits (bit t = occluded(t), t = 0 .. Jets; 0 where
 * there is no hypothesis).  1 <= Jets <= 32, h >= 4 (the reference's vertical 5-tap derivative is undefined below), n (Jets + 1) <= 21845.  IEEE fp64
 * without contraction: bit-identical to a plain restatement (the Lorentzian's fp64 log is the device's, not glibc's; equal after the fp32 rounding
 * wherever it has been compared). */
int sfa_hypothesis_energies(sfa_ctx *ctx, const sfa_energy_params *p, int n, int r_Jets, int Jets, int w, int h, int stride, const double *acc_u,
                            const double *acc_v, const int *tracked, const float *const *frames, const float *const *fwd_u, const float *const *fwd_v,
                            const float *const *bwd_u, const float *const *bwd_v, double *energy, unsigned long long *occ_bits);
/* The same, and where adapted_u, adapted_v are given (both or neither) every hypothesis' flows after adaptFPS(Jets), the flows the energy was computed
 * from, as [n][Jets][gh][gw] doubles (0 where there is no hypothesis).  sfa_hypothesis_energies is this call with both NULL. */
int sfa_hypothesis_energies_ex(sfa_ctx *ctx, const sfa_energy_params *p, int n, int r_Jets, int Jets, int w, int h, int stride, const double *acc_u,
                               const double *acc_v, const int *tracked, const float *const *frames, const float *const *fwd_u, const float *const *fwd_v,
                               const float *const *bwd_u, const float *const *bwd_v, double *energy, unsigned long long *occ_bits, double *adapted_u,
                               double *adapted_v);
/* sfa_hypothesis_energies_ex with rate acc_min_fps's flows described by flow_src (the planes of fwd_u .. bwd_v; `stride` stays the frames') and
 * brought to w x h on the GPU as sfa_jet_flow_resample does it: forward_flow[f] = r_forward_flow[f] (dense_tracking.cpp:1148-1151) are the rescaled
 * doubles.  flow_src is ignored where the four flow arrays are NULL; an identity source runs sfa_hypothesis_energies_ex's float path. */
int sfa_hypothesis_energies_scaled(sfa_ctx *ctx, const sfa_energy_params *p, int n, int r_Jets, int Jets, int w, int h, int stride, const double *acc_u,
                                   const double *acc_v, const int *tracked, const float *const *frames, const sfa_jet_source *flow_src,
                                   const float *const *fwd_u, const float *const *fwd_v, const float *const *bwd_u, const float *const *bwd_v,
                                   double *energy, unsigned long long *occ_bits, double *adapted_u, double *adapted_v);
/* dense_tracking's computeSmoothnessWeight (dense_tracking.cpp:367-405, called at :969-981 with coef 5.0): the luminance
 * (0.299f (c1 std_1 + avg_1) + 0.587f (...) + 0.114f (...)) / 255.0f (/ 65535.0f with hbit), its 5-tap {0, -8/12, 1/12} derivatives, then
 * 0.5f * expf(-coef * sqrtf(lx^2 + ly^2)), all in fp32 without contraction.  The formula is the first output of Variational_AUX_MT::compute_dpsis_weight
 * (sfa_dpsis_weight) and runs through the same pinned kernel; expf is glibc's algorithm restated on the device (see sfa_dpsis_weight).  frame0: the first
 * of 3 planes of h * stride floats; out: a PACKED [h][w] plane.  h >= 4 (the vertical 5-tap). */
int sfa_dt_smoothness_weight(sfa_ctx *ctx, int w, int h, int stride, const float *frame0, float coef, const float avg[3], const float std_dev[3], int hbit,
                             float *out);
/* dense_tracking's fusion of the hypotheses (dense_tracking.cpp:1588-1905): non-maximum suppression, the pairwise MRF and TRW-S.  The cfg keys with the
 * C types the reference reads them in (:605-625, :660-661); sfa_fuse_params_default fills setDefault's values (:136-152) and skip 1. */
typedef struct sfa_fuse_params {
    double acc_beta;                /* acc_beta ("10.0") */
    double acc_spatial_occ;         /* acc_spatial_occ (10.0; setDefault's key is misspelt acc_satial_occ and never read) */
    int    traj_sim_method;         /* acc_traj_sim_method ("1"): 0 ADJ, 1 ACC; 2 FINAL is refused (it reads flow_y[Jets], past the array) */
    int    pin_first;               /* 0 (the default: every slot is sorted).  1: slot 0, where present, stays the first label whatever its energy -- the
                                     * alternation's rounds p > 0, whose sort covers positions 1 onward (:1601-1602); the NMS then measures the others
                                     * against it.  The field takes the four bytes of padding the struct had here: sizes and offsets are unchanged.
                                     * A CALLER THAT FILLS THE STRUCT FIELD BY FIELD WITHOUT sfa_fuse_params_default now passes indeterminate bytes
                                     * here: call the default first, or set the field.  The track jobs refuse pin_first != 0 at creation */
    double traj_sim_thres;          /* acc_traj_sim_thres ("0.1") */
    double trws_eps;                /* acc_trws_eps ("1e-5") */
    int    trws_max_iter;           /* acc_trws_max_iter ("10") */
    int    skip;                    /* acc_skip_pixel: the grid of sfa_accumulate_grid, xy_incr = skip + 1, xy_start = (int)(0.5f * skip) */
} sfa_fuse_params;
void sfa_fuse_params_default(sfa_fuse_params *p);
/* n segments (start_jets) of gw x gh grid pixels with K label slots each (1 <= K <= 16, the rates), 1 <= Jets <= 32.  Inputs: U, V [n][K][Jets][gh][gw]
 * adapted flows (sfa_hypothesis_energies_ex), energy [n][K][gh][gw] (+Inf: no hypothesis in that slot), occ_bits [n][K][gh][gw] (bit t = occluded(t)),
 * weight [n][h][w] packed smoothness weights (sfa_dt_smoothness_weight).  Per pixel: the present slots sorted by (float) energy, ties to the lower slot,
 * then the NMS of :1592-1630 with its `break`; a pixel left without a hypothesis is no node and its edges are dropped.  Right and down edges cost
 * P = (w[o1] + w[o2]) * (acc_beta * (float) distance + acc_spatial_occ * smooth_occ) (:1716-1797).  TRW-S in sequential raster order, fp64 without
 * contraction (INTEGRATION.md 4c defines it; the bound is the reparametrisation bound, not the MRF library's tree bound).  Outputs [n][gh][gw]: slot (-1 =
 * none), flow_u, flow_v = u(Jets - 1) / xy_incr, v(Jets - 1) / xy_incr (:1856-1857; 1e10 = UNKNOWN_FLOW where there is no node), occ = max_t occluded(t),
 * t = 0 .. Jets (:1859-1863); per segment: seg_energy (of the labelling returned, the lowest over the iterations), seg_bound (after the last iteration),
 * seg_iters.  stage_ms: NULL or 4 floats, the milliseconds of the label, pairwise, TRW-S and output kernels of the call (HIP events). */
int sfa_fuse_hypotheses(sfa_ctx *ctx, const sfa_fuse_params *p, int n, int K, int Jets, int w, int h, const double *U, const double *V, const double *energy,
                        const unsigned long long *occ_bits, const float *weight, int *slot, double *flow_u, double *flow_v, unsigned char *occ,
                        double *seg_energy, double *seg_bound, int *seg_iters, float *stage_ms);
/* ---- dense_tracking's alternation around the fusion (dense_tracking.cpp:1381-1583) on the GPU (csrc/neigh.hip), as INTEGRATION.md 4d defines it: the
 * reference's own result depends on FLANN's result order, on one random engine consumed pixel after pixel and on an out-of-bounds read, so the stage is
 * pinned to a restatement (tests/neigh_ref.py), like the fusion.  Host pointers; each call waits for its results.
 * A pixel's hypothesis list has 16 positions: U, V [n][16][Jets][gh][gw] adapted flows, energy [n][16][gh][gw] (+Inf or NaN: no hypothesis at that
 * position), occ_bits [n][16][gh][gw], origin [n][16][gh][gw]: the slot the hypothesis was born in, | 0x80 once it has arrived as a neighbour's proposal. */
typedef struct sfa_hyp_lists {
    double *U, *V, *energy;
    unsigned long long *occ_bits;
    unsigned char *origin;
} sfa_hyp_lists;
/* The keys of the neighbour proposals with setDefault's values (:136-159); seed: the reference takes the clock, here 0. */
typedef struct sfa_neigh_params {
    double traj_sim_thres;          /* acc_traj_sim_thres ("0.1") */
    int    traj_sim_method;         /* acc_traj_sim_method ("1"): 0 ADJ, 1 ACC */
    int    neigh_hyp;               /* acc_neigh_hyp ("5"): set t may bring the round's proposals to (t + 1) * acc_neigh_hyp */
    float  neigh_hyp_radius;        /* acc_neigh_hyp_radius ("100.0", read as an int into a float, :631): FLANN's L2 radius, a SQUARED distance */
    int    neigh_skip1, neigh_skip2;/* acc_neigh_skip1 ("2"), acc_neigh_skip2 ("4"): the candidate lattices */
    int    hyp_neigh_tryouts;       /* acc_hyp_neigh_tryouts ("20") per set */
    unsigned seed;                  /* seed: round p draws with the Philox key (seed + p, sequence_start) */
    int    slots;                   /* (4) round 0: the lists hold hypotheses at positions 0 .. slots - 1 only (2 K under -fill) */
    int    perturb_keep;            /* acc_perturb_keep (no default: -1 = not set, refused from round 1 on): later rounds' lists end at position perturb_keep */
} sfa_neigh_params;
void sfa_neigh_params_default(sfa_neigh_params *p);
/* The prune of rounds p > 0 (:1384-1416): position 0 of `out` is the position `selected` [n][gh][gw] names (the fusion's slot; -1 or an absent position:
 * none), then the other present positions by (float) energy, ties to the lower position, while the list holds at most perturb_keep entries -- at most
 * perturb_keep + 1 in all; every later position is absent (+Inf, zeros).  in and out must not overlap.  stage_ms: NULL or 2 floats, the milliseconds of
 * the map and the gather kernel (HIP events).  Refused: perturb_keep + 1 outside 1 .. 16. */
int sfa_prune_hypotheses(sfa_ctx *ctx, int n, int Jets, int gw, int gh, int perturb_keep, const int *selected, const sfa_hyp_lists *in,
                         const sfa_hyp_lists *out, float *stage_ms);
/* The neighbour proposals of round `round` (:1432-1583).  out = in with the accepted proposals at the lowest absent positions.  A proposal is a copy of
 * the drawn candidate pixel's source hypothesis in `in` (round 0: the lowest (float) energy, ties to the lower position; later: position 0): its flows,
 * its origin | 0x80 and, until the caller has scored it at its new place, the source's energy and occlusion word.  It is discarded when
 * !(distance(h, proposal) > traj_sim_thres) for a hypothesis h of the list as it stands.  consistent [n][gh][gw] (1 = some rate is tracked over its
 * whole length) is read in round 0 only and may be NULL later.  sequence_start [n]: the second key word of the segment's draws.  src_pixel, src_position
 * [n][16][gh][gw]: for a position filled in this call the source's pixel index y * gw + x and position, -1 / 0 elsewhere; accepted [n]: their count;
 * stage_ms: NULL or 3 floats, the milliseconds of the flag, the search-draw-accept and the gather kernel (HIP events).
 * Refused by the key's name, before anything is copied: acc_neigh_hyp_radius <= 0 or NaN, acc_neigh_skip1/2 < 1, acc_hyp_neigh_tryouts < 0,
 * acc_neigh_hyp < 0, acc_traj_sim_method other than 0 or 1; round 0: slots + 2 * acc_neigh_hyp > 16; later rounds: acc_perturb_keep not set,
 * acc_perturb_keep + 1 + 2 * acc_neigh_hyp > 16; a hypothesis at a position beyond those the round's limit counts (so no list can fill up); a grid side beyond 2896 (d^2 would no longer be exact in fp32). */
int sfa_neighbour_proposals(sfa_ctx *ctx, const sfa_neigh_params *p, int n, int Jets, int gw, int gh, int round, const unsigned *sequence_start,
                            const unsigned char *consistent, const sfa_hyp_lists *in, const sfa_hyp_lists *out, int *src_pixel,
                            unsigned char *src_position, int *accepted, float *stage_ms);
/* The rescoring of a round's accepted proposals (:1549-1553): each is a trajectory of Jets steps at its new pixel; its occlusions are set from rate
 * acc_min_fps's flows and its energy is JC + BC/GC + OC + slot_weight[origin & 0x7f] in fp32 -- sfa_hypothesis_energies' kernels on the lists' own flow
 * planes (r_Jets = Jets, where adaptFPS is the identity), p->weight ignored.  frames, fwd_u .. bwd_v, w, h, stride: as sfa_hypothesis_energies takes
 * them (flows of the frames' size); the lists are on the grid of (w, h, p->skip).  slot_weight: 16 floats, weight_jet_estimation of the rate each slot
 * belongs to.  src_pixel: as sfa_neighbour_proposals returned it; positions with src_pixel >= 0 get their energy and occ_bits replaced in `lists`, every
 * other value is left as it is.  stage_ms: NULL or 1 float, the milliseconds of the scoring launches (the frames' records and the uploads are not in
 * it).  Refused: what sfa_hypothesis_energies refuses of the sizes; a proposal whose origin names no slot below 16. */
int sfa_rescore_proposals(sfa_ctx *ctx, const sfa_energy_params *p, int n, int Jets, int w, int h, int stride, const float *const *frames,
                          const float *const *fwd_u, const float *const *fwd_v, const float *const *bwd_u, const float *const *bwd_v,
                          const float *slot_weight, const int *src_pixel, const sfa_hyp_lists *lists, float *stage_ms);
/* Philox4x32-10 (Salmon et al., SC'11) as the draws use it: on the host, and n (counter, key) pairs through the device function the kernel calls. */
void sfa_philox4x32_10(const unsigned ctr[4], const unsigned key[2], unsigned out[4]);
int sfa_philox4x32_10_device(sfa_ctx *ctx, int n, const unsigned *ctr, const unsigned *key, unsigned *out);
/* ---- the steps around dense_tracking's EpicFlow fill-in (dense_tracking.cpp:1265-1310) for n maps of one size w x h in one call, on the GPU
 * (csrc/fill.hip).  Host pointers; each call waits for its results.  Each refuses with SFA_ERR_ARG, the argument named and nothing launched: n, w or h < 1,
 * a null pointer, w * h > 2^29 (32-bit pixel indices), more than 65535 maps (planes) in a call, and what is listed with it. -------------------------------
 * removeSmallSegments(r_consistent, 0.1, 100) (utils/utils.cpp:169-284) on r_consistent = (tracked == r_Jets) (dense_tracking.cpp:1223-1226, 1265).
 * tracked: [n][h][w] ints (sfa_accumulate_consistent*); full[n]: map i's r_Jets; mask (out): [n][h][w] bytes, 1 where tracked == full[i] and the pixel's
 * 4-connected component of such pixels has at least min_size pixels, else 0; kept[n] (out): the number of 1s.  The reference's scan order does not matter
 * (csrc/fill.hip says why), and the mask does not depend on the order of the kernels' atomics.  Also refused: min_size < 1. */
int sfa_consistent_regions(sfa_ctx *ctx, int n, int w, int h, const int *tracked, const int *full, int min_size, unsigned char *mask, int *kept);
/* The sample columns (rows) of the fill-in's matches: `for (int x = floor(0.5f * epic_skip); x < extent; x += epic_skip)` with the float epic_skip as the
 * reference writes it (dense_tracking.cpp:1278-1279), so a non-integer step truncates after every addition.  Host only, no GPU.  out: extent ints or NULL
 * (count only); *count: the number of samples.  Refused: extent outside 1 .. 2^23 (beyond 2^24 the fp32 sum no
 * longer advances x), epic_skip outside 1 .. 1e6 (or NaN), count NULL. */
int sfa_fill_samples(int extent, float epic_skip, int *out, int *count);
/* The matches of the consistent trajectories (dense_tracking.cpp:1274-1289).  acc_u, acc_v: [n][J][h][w] doubles (sfa_accumulate_consistent* with
 * all_steps 1; acc_u is the reference's Vec2d[1]); mask: [n][h][w] (sfa_consistent_regions); xs[nx], ys[ny]: the sample columns and rows
 * (sfa_fill_samples); divisor: acc_skip_pixel + 1.  For map i and step j the samples (ys outer, xs inner) with a non-zero mask become the rows
 * (float) x, (float) y, (float) (x + acc_u / divisor), (float) (y + acc_v / divisor) of matches[i][j], sum and division in fp64; count[i] (out): the rows,
 * the same for every j.  matches: [n][J][nx * ny][4] floats, of which only the first count[i] rows of each [i][j] are written.
 * Also refused: J < 1, nx outside 1 .. w, ny outside 1 .. h, a sample outside the map, divisor < 1. */
int sfa_fill_matches(sfa_ctx *ctx, int n, int J, int w, int h, const double *acc_u, const double *acc_v, const unsigned char *mask, const int *xs, int nx,
                     const int *ys, int ny, int divisor, float *matches, int *count);
/* The interpolated planes as the trajectories of every pixel (dense_tracking.cpp:1299-1310): flow_x[i * J + j], flow_y[i * J + j] = h rows of `stride`
 * floats, step j of map i (sfa_epic_interpolate_batch); scale: acc_skip_pixel + 1.  Out: acc_u, acc_v [n][J][h][w] = (double) (plane * (float) scale),
 * tracked [n][h][w] = J -- the input of sfa_hypothesis_energies*.  Also refused: J < 1, n * J > 65535, stride < w, stride * h > 2^29, scale < 1. */
int sfa_fill_trajectories(sfa_ctx *ctx, int n, int J, int w, int h, int stride, const float *const *flow_x, const float *const *flow_y, int scale,
                          double *acc_u, double *acc_v, int *tracked);
/* ---- resident track jobs: dense_tracking's accumulation, energies and fusion of start_jets that stay in GPU memory (csrc/track.hip) -----------
 * A track job owns the device planes of up to n start_jets (segments) x K rates: the flows in the kernels' layout, the frames and their records, the
 * accumulated trajectories, the energies, adapted flows and occlusion words in the fusion's [n][K] layout, the MRF and the fused result.  It takes the
 * inputs once, from host planes or from GPU memory, and sfa_track_job_run enqueues frame records -> accumulation (all steps) of every rate -> energies
 * and adapted flows of every rate, best / occluded -> smoothness weight -> labels -> pairwise -> TRW-S -> output for segments 0 .. ns-1 on the context's
 * stream and RETURNS WITHOUT WAITING: no stage reads or writes host memory, and TRW-S's stopping rule runs inside its kernel.  The stages are the
 * launches of sfa_accumulate_consistent_scaled (all_steps), sfa_hypothesis_energies_scaled and sfa_fuse_hypotheses over the same planes, so segment s
 * comes out with the bits of those calls on that segment alone, whatever n, ns and s.  Slot k of the fusion is rate k.
 * The parameters: n start_jets of capacity (1 .. 64), K rates (1 .. 16), Jets (1 .. 32), the tracking frames' w x h (h >= 4), min_fps_idx (rates before
 * it see no flows in their energies: every step t >= 1 occluded; r_Jets[min_fps_idx] must be Jets, its flows being the Jets steps the energies read),
 * do_fuse (0: the job stops after the energies and holds no fused result), use_occlusions (the accumulation reads the rates' occlusion images); per rate
 * r_Jets (its steps), source (where its jet planes sit, sfa_jet_source) and weight (weight_jet_estimation[r]); the accumulation's epsilon
 * (acc_consistency_threshold), skip (acc_skip_pixel: the one grid of all stages; energy.skip and fuse.skip are ignored) and discard; the energies' keys
 * (energy.weight is ignored) and the fusion's; the smoothness weight's coef, avg, std_dev, hbit (sfa_dt_smoothness_weight).
 * sfa_track_params_default: n = K = Jets = 1, do_fuse 1, epsilon 1.0, skip 1, discard 1, r_Jets 1, weight[r] = r, coef 5, avg 0, std_dev 1 and the
 * defaults of sfa_energy_params_default / sfa_fuse_params_default; the sources are left zero and must be set. */
typedef struct sfa_track_params {
    int n, K, Jets, w, h, min_fps_idx, do_fuse, use_occlusions;
    int r_Jets[16];
    sfa_jet_source source[16];
    float weight[16];
    double epsilon;
    int skip, discard;
    sfa_energy_params energy;
    sfa_fuse_params fuse;
    float coef, avg[3], std_dev[3];
    int hbit;
} sfa_track_params;
void sfa_track_params_default(sfa_track_params *p);
typedef struct sfa_track_job sfa_track_job;
/* Host only: the device bytes a job of these parameters allocates (one allocation).  Refuses what sfa_track_job_create refuses. */
int  sfa_track_job_bytes(const sfa_track_params *p, size_t *bytes);
/* Allocates once.  Refused with SFA_ERR_ARG, naming the argument: everything the three stages refuse (K, Jets, h < 4, an empty grid, a source whose
 * rescaled crop is not w x h, occlusions together with a crop, adaptFPS reading past a rate's steps, fuse.traj_sim_method 2, fuse.trws_max_iter < 1), n
 * outside 1 .. 64, min_fps_idx outside the rates, r_Jets[min_fps_idx] != Jets. */
int  sfa_track_job_create(sfa_ctx *ctx, const sfa_track_params *p, sfa_track_job **out);
void sfa_track_job_destroy(sfa_track_job *job);
/* The flows of rate r of segment s: r_Jets[r] host planes per array, as source[r] describes them (identity: packed and interleaved; else cropped, resized
 * and multiplied by rescale on the GPU, as sfa_accumulate_consistent_scaled does it).  occ: the r_Jets[r] RAW 8-bit occlusion images (decoded on the GPU)
 * on a job with use_occlusions, else ignored (NULL).  Waits for its copies. */
int  sfa_track_job_upload_flows(sfa_track_job *job, int s, int r, const float *const *fwd_u, const float *const *fwd_v, const float *const *bwd_u,
                                const float *const *bwd_v, const unsigned char *const *occ);
/* The Jets + 1 normalised colour frames of segment s: frames[f] the first plane of 3 (c1, c2, c3, each h * stride floats), as sfa_hypothesis_energies
 * takes them.  Waits for its copies. */
int  sfa_track_job_upload_frames(sfa_track_job *job, int s, const float *const *frames, int stride);
/* The same from GPU memory, for segments s0 .. s0+ns-1: fwd_dev, bwd_dev fp32 [ns][r_Jets[r]][2 (u, v)][sh][sw] and frames_dev fp32
 * [ns][Jets+1][3][h][w], element (i0, .., i4) at p + sum i_k strides[k] (64-bit element strides, >= 0, the column stride >= 1).  Read in stream order on
 * the context's stream and without a host wait: with sfa_ctx_wait_stream / sfa_ctx_signal_stream around them the caller needs none either.  On a job
 * with use_occlusions the device flows leave the rate's masks as they are: the occlusion images are an upload of their own
 * (sfa_track_job_upload_occlusions_device, or occ of sfa_track_job_upload_flows), in any order with the flows.  Refused: memory that is not the
 * context's GPU's, a view that leaves its allocation, segments outside the job. */
int  sfa_track_job_upload_flows_device(sfa_track_job *job, int s0, int ns, int r, const float *fwd_dev, const float *bwd_dev, const long long strides[5]);
int  sfa_track_job_upload_frames_device(sfa_track_job *job, int s0, int ns, const float *frames_dev, const long long strides[5]);
/* The occlusion images of rate r of segments s0 .. s0+ns-1 from GPU memory: occ_dev [ns][r_Jets[r]][sh][sw] (sh x sw of source[r]) at strides[4], of
 * dtype (sfa_dev_dtype) SFA_DEV_U8, the RAW 8-bit images that sfa_track_job_upload_flows takes as occ, or SFA_DEV_F32, the labels as
 * sfa_job_download_device leaves them in occ_dev, turned into the grey image the driver writes by its own expression: v = (x + 1) * 0.5f * 255.0f in
 * fp32 without contraction, nearbyint (halves to even), max(0.0f, min(255.0f, .)): -1 -> 0, 0 -> 128, +1 -> 255, NaN -> 255, -Inf -> 0, +Inf -> 255.  The
 * images are decoded into the rate's masks like the host's (cubic resize, 3 x 3 median, 255 - x), segment by segment, in stream order on the context's
 * stream and without a host wait.  Refused by name, with nothing launched: a job without use_occlusions, r or segments outside the job, any other
 * dtype, memory that is not the context's GPU's, a view that leaves its allocation. */
int  sfa_track_job_upload_occlusions_device(sfa_track_job *job, int s0, int ns, int r, const void *occ_dev, int dtype, const long long strides[4]);
/* Tracks, scores and (do_fuse) fuses segments 0 .. ns-1 (1 <= ns <= n) from what the job holds and returns without waiting.  Everything a run reads that
 * an earlier run wrote (the messages, the labellings, the per-segment records) is initialised again: a job serves any number of groups. */
int  sfa_track_job_run(sfa_track_job *job, int ns);
/* Rate r of segment s after a run, [gh][gw] each: the last accumulated step, tracked, the energy (+Inf: no hypothesis), the occlusion word and its
 * popcount.  NULL skips an output.  Waits for the run. */
int  sfa_track_job_download_rate(sfa_track_job *job, int s, int r, double *acc_u_last, double *acc_v_last, int *tracked, double *energy,
                                 unsigned long long *occ_bits, unsigned char *occluded);
/* The fused result of segment s, [gh][gw] each, as sfa_fuse_hypotheses returns it (slot = rate, -1 none), best = the rate of the lowest fp32 energy (ties
 * to the lower rate, 255 none), and the segment's energy, bound and iterations.  NULL skips an output.  Waits for the run.  Refused on a job with
 * do_fuse 0. */
int  sfa_track_job_download_fused(sfa_track_job *job, int s, int *slot, double *flow_u, double *flow_v, unsigned char *occ, unsigned char *best,
                                  double *energy, double *bound, int *iters);
/* best [gh][gw] of segment s alone, also on a job with do_fuse 0.  Waits for the run. */
int  sfa_track_job_download_best(sfa_track_job *job, int s, unsigned char *best);
/* The bytes of device memory that are free on the context's GPU now (hipMemGetInfo): what the accumulate program sizes its track job by. */
int  sfa_ctx_free_bytes(sfa_ctx *ctx, size_t *free_bytes);
/* The fused results of segments s0 .. s0+ns-1 into GPU memory, in stream order and without a host wait: flow_dev fp64 [ns][2 (u, v)][gh][gw] at
 * strides[4]; packed slot_dev int32 [ns][gh][gw], occ_dev uint8 [ns][gh][gw] and stats_dev fp64 [ns][3] (energy, bound, iterations), each or NULL.
 * Refused: strides that let two elements of the flow share an address (a zero u|v stride ...), destinations that overlap one another. */
int  sfa_track_job_download_device(sfa_track_job *job, int s0, int ns, double *flow_dev, const long long strides[4], int *slot_dev, unsigned char *occ_dev,
                                   double *stats_dev);
/* Rate r of segments s0 .. s0+ns-1 after a run into GPU memory, with the values of sfa_track_job_download_rate, in stream order and without a host wait,
 * also on a job with do_fuse 0: acc_dev fp64 [ns][2 (u, v)][gh][gw] at strides[4], the last accumulated step; packed [ns][gh][gw] tracked_dev int32,
 * energy_dev fp64 (the fp32 sum; +Inf: no hypothesis), occ_bits_dev uint64 and occluded_dev uint8 (its popcount).  NULL skips an output (strides may be
 * NULL with acc_dev).  sfa_track_job_download_best_device: best uint8 [ns][gh][gw], as sfa_track_job_download_best gives it.  Refused: strides that let
 * two elements of acc_dev share an address (a zero u|v stride ...), destinations that overlap one another, r or segments outside the job. */
int  sfa_track_job_download_rate_device(sfa_track_job *job, int s0, int ns, int r, double *acc_dev, const long long strides[4], int *tracked_dev,
                                        double *energy_dev, unsigned long long *occ_bits_dev, unsigned char *occluded_dev);
int  sfa_track_job_download_best_device(sfa_track_job *job, int s0, int ns, unsigned char *best_dev);
/* The last run's kernel times in ms (HIP events; waits for the run): frame derivatives and records, accumulation, energies (with best / occluded), smoothness
 * weight (its kernel alone), labels, pairwise, TRW-S, output; the last five are 0 on a job with do_fuse 0.  Slot 0 is NOT a pack + resample time: the flows are packed
 * and resampled by the uploads, outside the run. */
int  sfa_track_job_stage_ms(sfa_track_job *job, float ms[8]);
/* ---- a track job that fills in: dense_tracking's EpicFlow fill-in hypothesis of every rate (dense_tracking.cpp:1265-1350), resident ----------
 * A job made by sfa_track_job_create_fill holds, beside the planes of a plain job, each start_jet's edge cost map and the saliency of its Lab image, and
 * its fusion runs over S = 2 K slots: slot 2 r is rate r's accumulated hypothesis, slot 2 r + 1 its fill-in (the reference's push order), and that is the
 * index sfa_track_job_download_fused returns as `slot`.  best, occluded and sfa_track_job_download_rate keep describing the accumulated hypotheses only.
 * sfa_track_job_run, after the accumulation of every rate, does rate by rate: removeSmallSegments on tracked == r_Jets[r] and the matches at the sampled
 * pixels (sfa_consistent_regions, sfa_fill_matches with divisor skip + 1 on the positions of sfa_fill_samples(epic_skip)); the edge costs of every step
 * (start_jet s, step j of rate r reads the uploaded map after c_r + j + 1 sequential fp32 additions of epic.euc, c_r = r_Jets[0] + .. + r_Jets[r - 1]:
 * the map is shared by all epic() calls of a start_jet in the reference, each of which adds euc on entry, filled or not; euc == 0 adds nothing); the
 * interpolation of all ns * r_Jets[r] images by sfa_epic_batch's chain on these device planes, the saliency shared; sfa_fill_trajectories with scale
 * skip + 1.  Then the energies of both kinds with the rate's weight, and the fusion.  A start_jet without a sample, without a match, or with a step whose
 * matches the filters remove entirely is not filled for that rate: its odd slot holds energy +Inf, occlusion word 0 and adapted flows 0.
 * A RUN WITH FILL WAITS FOR THE STREAM where the fill-in does: once per rate for the ns match counts, and wherever the interpolation reads its
 * survivors.  An image that does not fit the interpolation's workspace even alone fails the run with an error naming start_jet, rate and step; there
 * is no host path.  The match targets are not tested for finite values (sfa_epic_batch refuses those on the host).
 * sfa_track_fill_params_default: epic_skip 2, min_size 100, epic = epic_fill_params (epic_params_default with pref_nn 25, nn 160, coef_kernel 1.1,
 * LA), workspace_bytes 0 = half of what is free at run time. */
typedef struct sfa_track_fill_params {
    float epic_skip;            /* acc_epic_skip: the sampling step of the matches, >= 1 */
    int min_size;               /* removeSmallSegments' smallest region */
    sfa_epic_params epic;
    size_t workspace_bytes;     /* the interpolation's workspace (not part of the job's allocation); 0: half of the free device memory at run time */
} sfa_track_fill_params;
void sfa_track_fill_params_default(sfa_track_fill_params *fill);
/* Host only: the fixed allocation of a fill job.  Both refuse, by the argument's name, what sfa_track_job_create refuses and: K > 8; epic.nn < 1,
 * epic.pref_nn < 0, epic.method outside 0 and 1; epic_skip not finite or < 1; min_size < 1; a grid of 8 columns or rows or fewer with
 * epic.saliency_th != 0; a grid the nearest-seeds stage cannot index. */
int  sfa_track_job_bytes_fill(const sfa_track_params *p, const sfa_track_fill_params *fill, size_t *bytes);
int  sfa_track_job_create_fill(sfa_ctx *ctx, const sfa_track_params *p, const sfa_track_fill_params *fill, sfa_track_job **out);
/* start_jet s of a fill job: lab = the Lab image at the grid's size, 3 planes of gh rows of lab_stride floats (NULL where epic.saliency_th == 0);
 * edges = gh * gw floats, the cost map as the edge file holds it (euc not added), every cost +0 ... +Inf (-0.0 counts as +0.0; sfa_epic_nearest_seeds_batch's domain): a NaN
 * or a cost below 0 is refused with SFA_ERR_ARG, start_jet and pixel named, before anything is copied or launched.  Waits: the caller's planes are free on return. */
int  sfa_track_job_upload_fill(sfa_track_job *job, int s, const float *lab, int lab_stride, const float *edges);
/* The same for start_jets s0 .. s0+ns-1 from GPU memory, in stream order and without a host wait: lab_dev fp32 [ns][3][gh][gw] at lab_strides[4] (NULL
 * where epic.saliency_th == 0), edges_dev fp32 [ns][gh][gw] at edge_strides[3].  The planes are not read on the host, so nothing here can
 * test them: THE CALLER GUARANTEES that every cost is +0 ... +Inf or -0.0, never NaN or below 0 (outside it a run may end in SFA_ERR_HIP, "the search's heap met
 * its capacity", or in lists the reference does not define). */
int  sfa_track_job_upload_fill_device(sfa_track_job *job, int s0, int ns, const float *lab_dev, const long long lab_strides[4], const float *edges_dev,
                                      const long long edge_strides[3]);
/* The same two uploads from frame 0 itself (dense_tracking.cpp:931-955): rgb = the frame as read, before the normalisation, at the FRAMES' size -- 3
 * planes of h rows of `stride` floats (rgb_dev: fp32 [ns][3][h][w] at strides[4]) -- and norm as sfa_reference_lab_device takes it.  The Lab image at the
 * grid's size is formed in GPU memory by that stage's kernel, straight into the job's plane; nothing of it passes through the host.  Refused beside what
 * the forms above refuse: a job whose skip the stage does not serve, a size OpenCV's resize rounds to another grid (sfa_reference_grid), a NaN norm.  The
 * edge-cost checks are those of the forms above.  The host form keeps a device copy of one frame (3 w h floats) beside the job's allocation. */
int  sfa_track_job_upload_fill_reference(sfa_track_job *job, int s, const float *rgb, int stride, float norm, const float *edges);
int  sfa_track_job_upload_fill_reference_device(sfa_track_job *job, int s0, int ns, const float *rgb_dev, const long long strides[4], float norm,
                                                const float *edges_dev, const long long edge_strides[3]);
/* Rate r's fill-in of segment s after a run: the trajectories fill_u, fill_v [r_Jets[r]][gh][gw] (0 where not filled), energy and occ_bits [gh][gw] (slot
 * 2 r + 1), stats[3] = {kept_pixels, matches, filled}.  NULL skips an output.  Waits for the run. */
int  sfa_track_job_download_fill(sfa_track_job *job, int s, int r, double *fill_u, double *fill_v, double *energy, unsigned long long *occ_bits, int *stats);
/* The last run's fill-in times in ms (HIP events, summed over the rates; waits for the run): regions and matches, the edge costs, the interpolation chain
 * (with its host reads), trajectories.  On a fill job sfa_track_job_stage_ms' energies slot begins where the last rate's fill-in ends. */
int  sfa_track_job_fill_ms(sfa_track_job *job, float ms[4]);
/* How the last run's interpolation was cut, summed over the rates: info[0] the sub-batches that ran to their end, info[1] those that were cut short by the
 * workspace and run again with the images that fit.  No result depends on the cut. */
int  sfa_track_job_fill_info(sfa_track_job *job, int info[2]);
/* ---- A track job that ALTERNATES (csrc/track_alt.hip): in place of the one fusion it runs `rounds` (acc_alternate) rounds of prune (rounds
 * p > 0) -> neighbour proposals -> rescoring -> fusion (position 0 pinned in rounds p > 0) on lists of 16 positions made of the job's slots (K, or 2 K with
 * fill-in), all enqueued by sfa_track_job_run without a host wait between the rounds.  Each step is the stage call's own device function, so start_jet s has the
 * bits of sfa_prune_hypotheses / sfa_neighbour_proposals / sfa_rescore_proposals / sfa_fuse_hypotheses chained on that start_jet alone, whatever the group.
 * neigh: the proposals' keys; its slots and traj_sim_* are taken from the job (slots, fuse.traj_sim_*), perturb_keep is needed when rounds > 1.  fill: NULL, or
 * the parameters of a job that also fills in.  consistent (round 0) = some rate's accumulated hypothesis is tracked over its whole length.  The existing
 * creators, their byte counts and results are unchanged.  Refused by name, before anything is allocated: rounds < 1, do_fuse 0, what the creators refuse, and
 * the proposals' limits -- slots + 2 * acc_neigh_hyp > 16, acc_perturb_keep not set or acc_perturb_keep + 1 + 2 * acc_neigh_hyp > 16 with rounds > 1,
 * acc_neigh_skip1/2 < 1, acc_hyp_neigh_tryouts < 0, acc_neigh_hyp_radius <= 0. */
typedef struct sfa_track_alt_params {
    int rounds;                     /* acc_alternate ("5") */
    sfa_neigh_params neigh;
} sfa_track_alt_params;
void sfa_track_alt_params_default(sfa_track_alt_params *a);
int  sfa_track_job_bytes_alternate(const sfa_track_params *p, const sfa_track_fill_params *fill, const sfa_track_alt_params *alt, size_t *bytes);
int  sfa_track_job_create_alternate(sfa_ctx *ctx, const sfa_track_params *p, const sfa_track_fill_params *fill, const sfa_track_alt_params *alt,
                                    sfa_track_job **job);
/* sequence_start of start_jets 0 .. n-1, the second key word of their draws (0 until set); copied before the call returns. */
int  sfa_track_job_set_sequence_starts(sfa_track_job *job, const unsigned *sequence_start);
/* Start_jet s of the last run: sfa_track_job_download_fused gives the last round's flow, occlusions, energy, bound and iterations, with slot = the chosen
 * POSITION; this call gives origin [gh][gw]: the slot the chosen hypothesis was born in, | 0x80 if it arrived as a proposal (255: no node), and per round
 * [rounds]: energy, bound, iterations, node count and accepted proposals.  NULL skips an output.  Waits. */
int  sfa_track_job_download_alternation(sfa_track_job *job, int s, unsigned char *origin, double *energy, double *bound, int *iters, int *nodes, int *accepted);
/* ---- resident pair jobs: the two-frame refinement of pairs that stay in GPU memory (csrc/two_frame.hip) -------------------------------
 * A pair job owns the planes of n pairs of one size (24 per pair: those of sfa_variational_2frame without its 24-plane derivative stack) and one solver
 * workspace, across any number of uploads and runs.  sfa_pair_job_run enqueues variational()'s launch sequence (variational.c:19-82) for all n pairs on the
 * context's stream and RETURNS WITHOUT WAITING -- the two-frame path has no break decision, so nothing needs the host: the one refinement entry point of
 * the library that is fully asynchronous.  sfa_pair_job_download and sfa_ctx_sync are the waits (and report a solver wait that gave up).  The derivatives
 * and the data term are formed in one kernel (k_data_2f_fused); pair b comes out bit-identical to sfa_variational_2frame on that pair alone, whatever n and
 * b.  A run refines the flow the job holds: after a run without a new upload the next run refines the result further.
 * Refused with SFA_ERR_ARG: w < 2, h < 5, n outside 1 .. 128, n x width beyond the change norms' scratch, a null plane, stride < w, b outside the job.
 * p == NULL: sfa_params_2frame_default.  upload: host planes as for sfa_variational_2frame (im1, im2: first plane of 3); it waits for its copies. */
typedef struct sfa_pair_job sfa_pair_job;
int  sfa_pair_job_create(sfa_ctx *ctx, const sfa_params_2frame *p, int w, int h, int n, sfa_pair_job **out);
void sfa_pair_job_destroy(sfa_pair_job *job);
int  sfa_pair_job_upload(sfa_pair_job *job, int b, const float *wx, const float *wy, int stride, const float *im1, const float *im2);
int  sfa_pair_job_run(sfa_pair_job *job);
int  sfa_pair_job_download(sfa_pair_job *job, int b, float *wx, float *wy, int stride);
/* The reference's own symbol and signature (variational.h:34), for relinking callers such as adaptiveFR / EpicFlow's refinement
 * step: runs on device 0 with a process-wide context; aborts with a message on error like the reference does. */
void variational(sfa_image *wx, sfa_image *wy, const sfa_color_image *im1, const sfa_color_image *im2, sfa_params_2frame *params);

/* Replaces Variational_MT::compute_one_level (variational_mt.cpp:169-493): one pyramid level. */
int sfa_compute_one_level(sfa_ctx *ctx, const sfa_params *p, float *wx, float *wy, int w, int h, int stride,
                          const float *const *frames, int n_frames, const float *const chw[3],
                          float *occlusions_out, float change[2]);

/* Replaces normalize() (variational_mt.cpp:17-85): in-place (I-avg)/std over F colour frames; avg/std are the
 * doubles the reference publishes as slow_flow_img_norm_* params. */
int sfa_normalize(sfa_ctx *ctx, float *const *frames, int n_frames, int w, int h, int stride,
                  double avg[3], double std_dev[3]);

/* Replaces sor_coupled (solver.h:11, solver.c:63-399) on host planes: K lexicographic SOR sweeps, results
 * numerically identical to the reference's raster order (hyperplane-pipelined on the GPU).  a11/a12/a22 are
 * overwritten with the inverted 2x2 blocks exactly as the reference does. */
int sfa_sor_coupled(sfa_ctx *ctx, sfa_image *du, sfa_image *dv, sfa_image *a11, sfa_image *a12, sfa_image *a22,
                    sfa_image *b1, sfa_image *b2, sfa_image *dpsis_horiz, sfa_image *dpsis_vert,
                    int iterations, float omega);
/* LABELLED MODE, not a replacement of anything in the reference: K red-black sweeps of the same per-point update on host planes (a11/a12/a22 are overwritten
 * with the inverted blocks).  Bit-identical to the test checker's red-black restatement, NOT to sor_coupled. */
int sfa_sor_red_black(sfa_ctx *ctx, sfa_image *du, sfa_image *dv, sfa_image *a11, sfa_image *a12, sfa_image *a22,
                      sfa_image *b1, sfa_image *b2, sfa_image *dpsis_horiz, sfa_image *dpsis_vert, int iterations, float omega);
/* the reference's own symbol and signature (solver.h:11); uses a process-wide default context on device 0 and
 * aborts with a message if no GPU is usable (the reference's error style, solver.c:75-78) */
void sor_coupled(sfa_image *du, sfa_image *dv, sfa_image *a11, sfa_image *a12, sfa_image *a22, sfa_image *b1,
                 sfa_image *b2, sfa_image *dpsis_horiz, sfa_image *dpsis_vert, const int iterations, const float omega);

/* ---- stage entry points (host planes; used by the parity tests and by partial integrations) ------ */

/* optimizeOcc, first half (variational_aux_mt.cpp:783-866): the data costs of the labels "occluded in the past" (d0) and
 * "occluded in the future" (d1).  masks[s]: raw warp mask of slot s; succ1/succ2[s], ref1/ref2[s]: the colour image pairs
 * (first plane of 3) whose difference is Iz of the slot's successive-frames / reference-frame derivative stack. */
int sfa_occlusion_costs(sfa_ctx *ctx, const sfa_params *p, float *d0, float *d1, const float *const *masks, const float *const *succ1,
                        const float *const *succ2, const float *const *ref1, const float *const *ref2, int w, int h, int stride);
/* optimizeOcc, second half (:868-880): occ[p] = 2*l_p - 1 for the labelling that minimises sum_p D_{l_p}(p) + alpha * #{4-neighbour
 * pairs with different labels} -- what GCO's two-label expansion computes; exact s-t minimum cut on the GPU. */
int sfa_grid_cut(sfa_ctx *ctx, float *occ, const float *d0, const float *d1, int w, int h, int stride, float alpha);
/* the same cut (variational_aux_mt.cpp:868-880) of nb independent windows in the launches a lockstep batch of jobs shares: occ, d0, d1 are nb planes of
 * h x stride each, window after window; 1 <= nb <= 128.  Each window gets the labels sfa_grid_cut gives it alone.  A refusal (SFA_ERR_ARG) names the
 * argument and launches nothing. */
int sfa_grid_cut_batch(sfa_ctx *ctx, float *occ, const float *d0, const float *d1, int nb, int w, int h, int stride, float alpha);

/* Variational_AUX_MT::image_warp (variational_aux_mt.cpp:722-756); mask may be NULL */
int sfa_image_warp(sfa_ctx *ctx, float *dst3, float *mask, const float *src3, const float *wx, const float *wy,
                   int w, int h, int stride, int factor);
/* one derivative stack of get_derivatives (variational_mt.cpp:113-133): out = Ix,Iy,Iz,Ixx,Ixy,Iyy,Ixz,Iyz,
 * each a colour image (3*h*stride floats), from I1 (im1p) and I2 (im2p) */
int sfa_derivative_stack(sfa_ctx *ctx, float *out8x3, const float *I1, const float *I2, int w, int h, int stride);
/* convolve_horiz / convolve_vert with the path's derivative filters (image.c:400-526); order 1 or 2 */
int sfa_convolve(sfa_ctx *ctx, float *dst, const float *src, int w, int h, int stride, int order, int horizontal);
/* Variational_AUX_MT::compute_dpsis_weight, first output (variational_aux_mt.cpp:673-719) */
int sfa_dpsis_weight(sfa_ctx *ctx, float *dst, const float *im3, int w, int h, int stride, float coef,
                     const float avg[3], const float std_dev[3], int hbit);
/* Variational_AUX_MT::compute_smoothness (variational_aux_mt.cpp:18-127) */
int sfa_smoothness(sfa_ctx *ctx, int method, float *dst_horiz, float *dst_vert, const float *uu, const float *vv,
                   const float *dpsis, int w, int h, int stride, float alpha, const sfa_penalty *reg);
/* Variational_AUX_MT::sub_laplacian (variational_aux_mt.cpp:130-161): dst += div(w grad src) */
int sfa_sub_laplacian(sfa_ctx *ctx, float *dst, const float *src, const float *wh, const float *wv, int w, int h, int stride);
/* Variational_AUX_MT::add_data_and_match / add_data_and_match_ref (variational_aux_mt.cpp:166-403, 408-634):
 * accumulate one data term into a11,a12,a22,b1,b2.  D8x3 as sfa_derivative_stack's output. */
int sfa_add_data_and_match(sfa_ctx *ctx, float *a11, float *a12, float *a22, float *b1, float *b2, const float *mask,
                           const float *du, const float *dv, const float *D8x3, const float *const chw[3],
                           int w, int h, int stride, float delta_over3, float gamma_over3, float s, int ref_term,
                           int dt_norm, const sfa_penalty *color, const sfa_penalty *grad);
/* pyramid arithmetic (cv::GaussianBlur / cv::resize as used at variational_mt.cpp:607,611,672,711); sfa_gaussian_blur: sigma * 8 + 1 < 33 (at most 33 taps,
 * radius 16), SFA_ERR_ARG beyond */
int sfa_gaussian_blur(sfa_ctx *ctx, float *dst, const float *src, int w, int h, int stride, float sigma);
int sfa_resize_linear(sfa_ctx *ctx, float *dst, int dw, int dh, int dstride, const float *src, int sw, int sh, int sstride);
/* optional presmoothing of level 0 (cfg `sigma` > 0, variational_mt.cpp:590-597): gaussian_filter (image.c:310-348) through
 * convolve_horiz / convolve_vert (image.c:529-644; orders 1 and 2 take the 3 / 5-tap routines) */
int sfa_gaussian_presmooth(sfa_ctx *ctx, float *dst, const float *src, int w, int h, int stride, float sigma);
/* cv::resize(src, dst, Size(0,0), fx, fy, INTER_LINEAR) as the driver's input rescaling uses it (slow_flow.cpp:552): the caller
 * passes dw = cvRound(sw*fx), dh = cvRound(sh*fy); source coordinate = (dst + 0.5) / fx - 0.5 */
int sfa_resize_linear_fx(sfa_ctx *ctx, float *dst, int dw, int dh, int dstride, const float *src, int sw, int sh, int sstride, double fx, double fy);
int sfa_pyramid_sizes(int w, int h, int layers, float p_scale, int *ws, int *hs);

/* ---- a sequence's frames resident in HBM (the multi-pair driver) ----------------------------------------------------------------------
 * The reference keeps the whole sequence in host memory (slow_flow.cpp:447-592), normalises it in place (:673) and hands windows of it to the solver
 * (:721-724).  Here the frames cross PCIe once: uploaded, normalised on the GPU (same arithmetic as sfa_normalize, which is built on this), and copied
 * device-to-device into the jobs that need them. */
typedef struct sfa_sequence sfa_sequence;
int  sfa_sequence_create(sfa_ctx *ctx, int w, int h, int n_frames, sfa_sequence **out);
void sfa_sequence_destroy(sfa_sequence *seq);
int  sfa_sequence_upload(sfa_sequence *seq, int f, const float *frame3, int stride);      /* asynchronous on the context's stream */
int  sfa_sequence_download(sfa_sequence *seq, int f, float *frame3, int stride);
/* normalize() (variational_mt.cpp:17-85) over the frames [f0, f0 + n) in place on the GPU; avg / std as sfa_normalize */
int  sfa_sequence_normalize(sfa_sequence *seq, int f0, int n, double avg[3], double std_dev[3]);
/* The same in its three parts, for a sequence whose frames are spread over several GPUs (each GPU holds the frames its windows read) and must still be
 * normalised with the statistics of ALL loaded frames (slow_flow.cpp:673): (1) the six fp64 sums of the raw frames [f0, f0 + n), sums[6 f + 2 k] = sum of
 * channel k, sums[6 f + 2 k + 1] = sum of its squares -- a deterministic kernel, the same bits on whichever GPU holds a frame; (2) avg / std from per-frame sums
 * in frame order (host arithmetic, variational_mt.cpp:41-52); (3) I <- (I - avg) / std on resident frames. */
int  sfa_sequence_frame_sums(sfa_sequence *seq, int f0, int n, double *sums /* n x 6 */);
int  sfa_normalize_statistics(const double *sums /* n_frames x 6 */, int n_frames, int w, int h, double avg[3], double std_dev[3]);
int  sfa_sequence_apply_normalization(sfa_sequence *seq, int f0, int n, const double avg[3], const double std_dev[3]);

/* ---- device-resident batches (measurement and the multi-pair driver) ------------------------------
 * A job = `batch` independent frame windows of identical size solved in lockstep by the same launches
 * (forward + backward of a jet, several jets ...), all inputs resident in HBM.
 * sfa_job_create refuses (SFA_ERR_ARG, naming p_scale) a p_scale that is NaN, <= 0 or > 1, or whose pyramid blur sigma = 1 / sqrt(2 p_scale) needs more
 * than the 33 taps the blur kernels carry (p_scale below about 0.03). */
typedef struct sfa_job sfa_job;
int  sfa_job_create(sfa_ctx *ctx, const sfa_params *p, int w, int h, int batch, sfa_job **out);
void sfa_job_destroy(sfa_job *job);
/* frames / initial flow of batch element b (host -> HBM); chw NULL = ones */
int  sfa_job_upload(sfa_job *job, int b, const float *const *frames, int n_frames, const float *wx, const float *wy,
                    int stride, const float *const chw[3]);
/* the same with the frames of the window taken from a resident sequence on the same GPU: frame f of the window = sequence frame frame_index[f] */
int  sfa_job_upload_resident(sfa_job *job, int b, const sfa_sequence *seq, const int *frame_index, int n_frames, const float *wx, const float *wy,
                             int stride, const float *const chw[3]);
int  sfa_job_reset_flow(sfa_job *job);               /* re-arm every element with the uploaded initial flow */
int  sfa_job_run(sfa_job *job);                      /* the whole coarse-to-fine path on the ctx stream; may be called again on the same uploads
                                                        (same result: presmoothing, cfg sigma > 0, is applied once per upload) */
int  sfa_job_download(sfa_job *job, int b, float *wx, float *wy, int stride, float change[2]);
/* Variational_MT::getOcclusions() of window b after the run: -1 occluded in the past / forward terms only, +1 in the future, 0 none */
int  sfa_job_download_occlusions(sfa_job *job, int b, float *occ, int stride);
/* Per-alternation labels (key slow_flow_occlusions_output: the reference writes <prefix><alter>.png after the discrete step of every alternation
 * alter >= 1, variational_mt.cpp:275-285; every pyramid level overwrites the file, the finest level's survives).  Enable before the run; after it
 * download the finest level's labels of alternation 1 <= alter < niter_alter of window b. */
int  sfa_job_keep_alternation_occlusions(sfa_job *job, int on);
int  sfa_job_download_alternation_occlusions(sfa_job *job, int b, int alter, float *occ, int stride);
double sfa_job_mpix_iters(const sfa_job *job);       /* sum over the job's SOR solves of w*h*K / 1e6, per run */
double sfa_job_device_bytes(const sfa_job *job);     /* device memory the job holds right now (arena + solver workspaces shaped so far) */

/* ---- the device seam: frames, initial flow and results that already live in the job's GPU memory ---------------------------------
 * Everything above takes HOST planes: sfa_job_upload / sfa_sequence_upload copy pageable host memory at a host stride and wait for the stream,
 * sfa_job_upload_resident still takes the initial flow from the host, sfa_job_download* copy plane by plane and wait.  The entry points below take
 * DEVICE pointers of the context's GPU (a decoder's output, a network's flow, a torch tensor's data_ptr) and move the data with one kernel launch per
 * call (csrc/device_io.hip).  They are asynchronous on the context's stream and never wait for it; order them against the caller's own stream with
 * sfa_ctx_wait_stream / sfa_ctx_signal_stream.  They only convert ((float) of the element, no scaling) and move: a job filled through them gives the
 * bits of the same job filled through the host entry points.
 * Refused with SFA_ERR_ARG, by the argument's name and before anything is launched: a pointer that hipPointerGetAttributes does not report as
 * device memory of the context's GPU (host and managed memory, other GPUs) or whose view leaves its allocation, an unknown element type, a column
 * stride < 1, any negative stride, windows outside the batch, and download destinations that the checks below cannot prove free of overlap.
 * sfa_job_run takes its break decisions on the host, so none of this can be captured into a HIP graph; nothing here attempts it. */
typedef enum { SFA_DEV_F32 = 0, SFA_DEV_U8 = 1, SFA_DEV_U16 = 2 } sfa_dev_dtype;
/* Where element (window, frame, channel, row, column) of the caller's frames lies: strides in ELEMENTS of `dtype`, 64-bit.  Planar [B,F,3,H,W],
 * interleaved [B,F,H,W,3] (channel 1, column 3), a crop of a larger tensor (row > width) and frames shared by windows (window < F frames, or 0)
 * are all this one description. */
typedef struct sfa_dev_layout { int dtype; long long window, frame, channel, row, column; } sfa_dev_layout;
/* contiguous planar fp32 [n][n_frames][3][h][w] */
void sfa_dev_layout_default(sfa_dev_layout *l, int w, int h, int n_frames);
/* Replaces sfa_job_upload's frame copies (3 F hipMemcpy2DAsync per window + hipStreamSynchronize) for the windows [b0, b0 + n): one launch of
 * k_pack_frames.  Columns >= width of the job's planes are not written.  chw: NULL (ones) or 3 HOST planes of h * stride floats,
 * stride = 4 * ceil(w / 4) as color_image_new lays them out, attached to every window of the call (they go through a pinned staging copy).
 * Unlike sfa_job_upload with wx = wy = NULL this call leaves the windows' initial flow as it is: on a job that held other windows before, follow it
 * with sfa_job_set_flow_device (NULL for zeros), or the run starts from the flow uploaded for the previous windows. */
int  sfa_job_upload_device(sfa_job *job, int b0, int n, const void *frames_dev, const sfa_dev_layout *layout, const float *const chw[3]);
/* Replaces the wx / wy arguments of sfa_job_upload and sfa_job_upload_resident (which may be called with NULL, NULL before): the initial flow of
 * the windows [b0, b0 + n) from fp32 device memory, strides[4] = element strides of (window, u|v, row, column); flow_dev NULL = zeros (strides
 * ignored).  One launch of k_pack_flow. */
int  sfa_job_set_flow_device(sfa_job *job, int b0, int n, const float *flow_dev, const long long strides[4]);
/* Replaces sfa_job_download + sfa_job_download_occlusions (2 + 1 hipMemcpy2DAsync per window + a stream wait each): (u, v) of the windows
 * [b0, b0 + n) into flow_dev (strides[4] as above) and, where occ_dev != NULL, getOcclusions() into occ_dev (occ_strides[3] = window, row, column),
 * one launch of k_unpack_planes.  Accepted destinations: every (window, plane) occupies a byte range of its own, or flow and occlusions lie apart and
 * each is a layout whose strides, sorted, each exceed the extent of the smaller ones (a slice of a larger tensor, channels-last ...). */
int  sfa_job_download_device(sfa_job *job, int b0, int n, float *flow_dev, const long long strides[4], float *occ_dev, const long long occ_strides[3]);
/* The change norms sfa_job_download returns, for the windows [b0, b0 + n) of the last run: out[2 i], out[2 i + 1].  Host record, no copy, no wait. */
int  sfa_job_changes(const sfa_job *job, int b0, int n, float *out);
/* Replaces sfa_sequence_upload for the frames [f0, f0 + n): frame i at frames_dev + i * layout->frame (layout->window is not used). */
int  sfa_sequence_upload_device(sfa_sequence *seq, int f0, int n, const void *frames_dev, const sfa_dev_layout *layout);
/* The same seam for resident pair jobs (csrc/two_frame.hip), the pairs [b0, b0 + n): the same kernels, one launch per call, no host copy, no wait, columns >= width never
 * written, and the same refusals by the same checks.  frames_dev holds two frames per pair: the layout's frame index 0 is im1, 1 is im2 (layout->window
 * steps from pair to pair).  flow_dev NULL in set_flow: zeros.  upload_device leaves the pairs' flow as it is, like sfa_job_upload_device. */
int  sfa_pair_job_upload_device(sfa_pair_job *job, int b0, int n, const void *frames_dev, const sfa_dev_layout *layout);
int  sfa_pair_job_set_flow_device(sfa_pair_job *job, int b0, int n, const float *flow_dev, const long long strides[4]);
int  sfa_pair_job_download_device(sfa_pair_job *job, int b0, int n, float *flow_dev, const long long strides[4]);
/* ---- raw Bayer ingest on the GPU (csrc/mosaic.hip) -----------------------------------------------------------------------------------------
 * The driver's camera path (cfg raw 1): a frame arrives as a one-channel Bayer mosaic, is demosaiced (raw_demosaicing 0: bayer2rgbGR, utils/utils.cpp:
 * 1242-1334; 2: cv::cvtColor(CV_Bayer*2RGB) on 8-bit data, slow_flow.cpp:502-520), cropped (center / extent) and rescaled (scale).  The calls below do
 * that on mosaics in GPU memory, in the arithmetic of the host routines (slowflow_amd/host/ingest.cpp): the frames hold the same bits as frames demosaiced
 * on the host and uploaded.  method = the cfg's raw_demosaicing (0 or 2; 1, Hamilton-Adams, is third-party code the reference does not ship: refused),
 * (red_x, red_y) = raw_red_loc, each 0 or 1.
 * A mosaic descriptor: element type, 64-bit ELEMENT strides of (frame, row, column), the size W x H of the full mosaic and the origin (x0, y0) of the crop
 * to produce; the crop's size is the destination's w x h.  Without a crop x0 = y0 = 0 and W, H = w, h.  The colour of a site follows from its
 * coordinates in the full mosaic, and so do the mirrored borders of method 0 and the repeated outer ring of method 2: a crop is the full result, sliced.
 * Refused with SFA_ERR_ARG, by the argument's name and before anything is launched: method other than 0 or 2, red_x / red_y outside {0, 1}, W < 2 or H < 2
 * with method 0 (the reference reads outside the image there), a crop that leaves the mosaic, every pointer or view the seam above refuses (the view of
 * mosaic_dev is the whole W x H of its n frames), a destination that overlaps itself or the source. */
typedef struct sfa_mosaic_desc { int dtype; long long frame, row, column; int W, H, x0, y0; } sfa_mosaic_desc;
/* n mosaics -> fp32 RGB at dst_dev, dst_strides[4] = element strides of (frame, channel, row, column); one launch of k_demosaic_gr / k_demosaic_cv8u per
 * 32768 frames; asynchronous on the context's stream, never waits. */
int  sfa_demosaic_device(sfa_ctx *ctx, int n, const void *mosaic_dev, const sfa_mosaic_desc *desc, int method, int red_x, int red_y, float *dst_dev,
                         const long long dst_strides[4], int w, int h);
/* The same kernel with the sequence's frames [f0, f0 + n) as the destination (w, h = the sequence's size). */
int  sfa_sequence_upload_mosaic_device(sfa_sequence *seq, int f0, int n, const void *mosaic_dev, const sfa_mosaic_desc *desc, int method, int red_x, int red_y);
/* The host-pointer form (the driver's, cfg gpu_ingest 1): a W x H mosaic of `dtype` elements, `host_stride` elements per row, goes through a pinned
 * staging copy to the GPU as it is (1, 2 or 4 bytes per pixel instead of 12) and through the same kernel into frame f.  Asynchronous on the context's
 * stream: the caller's buffer is free on return, the call waits only for the copy of the previous call out of the staging buffer. */
int  sfa_sequence_upload_mosaic(sfa_sequence *seq, int f, const void *mosaic_host, int dtype, long long host_stride, int W, int H, int x0, int y0, int method,
                                int red_x, int red_y);
/* rawWeighting (utils.cpp:1336-1374) of the windows [b0, b0 + n), formed on the GPU in the job's channel-weight planes (allocated at the first use, as by a
 * chw argument): the bits of passing rawWeighting's planes as chw to sfa_job_upload* -- which this call FOLLOWS: an upload with chw == NULL sets the
 * window's weights back to ones.  The planes take the stride of that upload (any stride >= w), as chw planes given to it would; a job that already holds
 * weights of another stride refuses.  Asynchronous. */
int  sfa_job_set_raw_weights(sfa_job *job, int b0, int n, int red_x, int red_y, float weight);
/* The driver's input rescaling (slow_flow.cpp:550-553; host form: color_image_rescale of ingest.cpp) of resident frames: src_seq's frames [f_src, f_src + n),
 * blurred with sigma = 1 / sqrt(2 scale) and resized by `scale`, become dst_seq's frames [f_dst, f_dst + n).  The kernels behind sfa_gaussian_blur and
 * sfa_resize_linear_fx, device to device: bit-equal to those two calls per channel.  Both sequences on one context; dst_seq of lrint(w scale) x lrint(h scale)
 * (SFA_ERR_ARG naming dst_seq otherwise); scale > 0 with a blur of at most 17 taps (scale >= 0.125).  Asynchronous. */
int  sfa_sequence_rescale(sfa_sequence *dst_seq, int f_dst, sfa_sequence *src_seq, int f_src, int n, float scale);
/* ---- EpicFlow's initialisation on resident data (csrc/epic_init.hip, csrc/lab_math.h) -------------------------------------------------------
 * deep_matching 1 starts every window from EpicFlow's interpolation of its matches (slow_flow.cpp:744-863).  The calls below keep that stage's planes in
 * GPU memory: the L*a*b* image, the chain of sfa_epic_batch, and the step from its field to a job's initial flow.
 * The Lab image of the driver (slow_flow.cpp:472-474, 578-586 + image.c:694-726; host/epic.cpp: rgb8_to_lab): every sample times `norm`, rounded to
 * nearest (ties to even) and saturated to 0 .. 255, then rgb_to_lab; out: L, a c, b c.  The arithmetic is csrc/lab_math.h, one function for host and device
 * code whose cube root and exponential are written from IEEE fp64 operations; tests/host/test_lab_math.cpp walks all 2^24 8-bit triples through it against the
 * host function, and the kernel is that function: the planes equal rgb8_to_lab's bit for bit.  +Inf saturates to 255, -Inf to 0, a NaN sample gives NaN
 * in all three planes of its pixel.
 * n fp32 images [n][3][h][w] at rgb_strides[4] = element strides of (image, channel, row, column) -> lab_dev at lab_strides[4]; columns >= w of the
 * destination are not written.  One thread per pixel; asynchronous on the context's stream, never waits.  Refused with SFA_ERR_ARG, the argument named,
 * nothing launched: n, w or h < 1, a NaN norm, every pointer or view the device seam refuses, a destination whose strides let two of its elements share
 * memory, a destination that overlaps the source. */
int  sfa_rgb8_to_lab_device(sfa_ctx *ctx, int n, int w, int h, const float *rgb_dev, const long long rgb_strides[4], float norm, float *lab_dev,
                            const long long lab_strides[4]);
/* ---- dense_tracking's reduced reference image (dense_tracking.cpp:931-955; csrc/ref_image.hip, csrc/ref_image.h) --------------------------------
 * With acc_skip_pixel > 0 the reference converts frame 0 to 8 bits, blurs it with OpenCV's 8-bit GaussianBlur (sigma = 1 / sqrt(2 / (skip + 1))) and
 * reduces it with resize(INTER_LINEAR) to the accumulation grid; EpicFlow's Lab image (:947-955) and the file its edge detector reads
 * (tmp/frame_epic_<start>.png, :944, 960) come from that image.  OpenCV is not in this tree: INTEGRATION.md 4c' defines the stage's integer arithmetic,
 * restated from OpenCV 2.4's x86-64 source, and the stage is PARITY-UNPINNED against OpenCV itself.  Served: skip 0 (the 8-bit step
 * alone: sfa_rgb8_to_lab_device bit for bit), 1 (7 taps) and 3 (9 taps); every other skip is refused by name.
 * sfa_reference_grid (dense_tracking.cpp:931-955; host only): the grid of sfa_accumulate_grid, refused with SFA_ERR_ARG where skip is not served or
 * where OpenCV's own size, cvRound(w / (skip + 1)) x cvRound(h / (skip + 1)) with ties to even, is another (w = 7 at skip 1).
 * sfa_reference_taps (dense_tracking.cpp:931-955; host only): the blur's taps in 8 fractional bits, *n of them (at most 9; skip 0: none); taps may
 * be NULL. */
int  sfa_reference_grid(int w, int h, int skip, int *gw, int *gh);
int  sfa_reference_taps(int skip, int *taps, int *n);
/* dense_tracking.cpp:931-955 for n frames in GPU memory: rgb_dev fp32 [n][3][h][w] at rgb_strides[4] (the samples as read; norm 1/255 for 16-bit
 * input, else 1) -> lab_dev fp32 [n][3][gh][gw] at lab_strides[4] and, where rgb8_dev is not NULL, the reduced 8-bit RGB image [n][3][gh][gw] at
 * rgb8_strides[4] (in bytes).  One kernel from the samples to the Lab planes, no plane in memory in between; asynchronous on the context's stream.  A
 * NaN sample counts as 0 where skip > 0.  Refused with SFA_ERR_ARG, the argument named, nothing launched: what sfa_reference_grid refuses, n < 1, a NaN
 * norm, every pointer or view the device seam refuses, destinations whose strides let two elements share memory, views that overlap. */
int  sfa_reference_lab_device(sfa_ctx *ctx, int n, int w, int h, int skip, const float *rgb_dev, const long long rgb_strides[4], float norm, float *lab_dev,
                              const long long lab_strides[4], unsigned char *rgb8_dev, const long long rgb8_strides[4]);
/* dense_tracking.cpp:931-955 for one frame in host memory: rgb = 3 planes of h rows of `stride` floats -> lab = 3 planes of gh rows of lab_stride floats
 * and, where not NULL, rgb8 = [3][gh][gw] bytes.  Allocates, uploads, launches, downloads and waits. */
int  sfa_reference_lab(sfa_ctx *ctx, int w, int h, int skip, const float *rgb, int stride, float norm, float *lab, int lab_stride, unsigned char *rgb8);
/* sfa_rgb8_to_lab_device's kernel between two resident sequences of one size and one context: src_seq's frames [f_src, f_src + n) -> dst_seq's [f_dst, f_dst + n).  The
 * source frames must still hold the samples as they were read: the caller orders this call before sfa_sequence_apply_normalization.  src_seq == dst_seq
 * is taken where the two frame ranges lie apart. */
int  sfa_sequence_lab(sfa_sequence *dst_seq, int f_dst, sfa_sequence *src_seq, int f_src, int n, float norm);
/* A resident EpicFlow batch: the inputs of epic() (epic_flow_extended/epic.cpp:147-235) for n images of one size w x h, and the fields it leaves, in GPU
 * memory.  params as for sfa_epic_batch, with one difference: the job adds params->euc to the cost maps itself, once and in fp32, as epic() does on entry
 * (epic.cpp:160).  Refused at creation: what sfa_epic_batch refuses of n, w, h and params (n at most 4096). */
typedef struct sfa_epic_job sfa_epic_job;
int  sfa_epic_job_create(sfa_ctx *ctx, const sfa_epic_params *params, int w, int h, int n, sfa_epic_job **out);
void sfa_epic_job_destroy(sfa_epic_job *job);
/* Image i from host memory, as the match and edge files hold it: matches = 4 * nm floats (x1 y1 x2 y2), nm may be 0; edges = w * h floats WITHOUT euc,
 * which is added on the device.  Refused: a coordinate that is not finite, an edge cost that is NaN or below 0 (sfa_epic_nearest_seeds_batch's domain;
 * image and pixel named), nm * nn beyond 2^31 - 1.  Waits for its copies: the buffers are free on return. */
int  sfa_epic_job_upload(sfa_epic_job *job, int i, const float *matches, int nm, const float *edges);
/* The Lab images of [i0, i0 + n) from a resident sequence of the job's size on the job's GPU (slow_flow.cpp:809: un_seq[ref]): frame_index[k] is image
 * i0 + k's frame.  Device to device on the JOB's stream; a sequence of another context is ordered by the caller (its frames are final before the call, as
 * for sfa_job_upload_resident).  What the job keeps is the image's saliency (image.c:729-791, sigma 0.8 and 1.0), the only reader of the Lab image; with
 * saliency_th == 0 nothing is read.  Asynchronous. */
int  sfa_epic_job_set_lab(sfa_epic_job *job, int i0, int n, const sfa_sequence *lab_seq, const int *frame_index);
/* Lab images and / or cost maps of [i0, i0 + n) from fp32 device memory: lab_dev [n][3][h][w] at lab_strides[4] (or NULL: not set by this call), cost_dev
 * [n][h][w] at cost_strides[3] (or NULL).  cost_has_euc 0: euc is added on the device, as for the host upload; 1: the maps hold it already.
 * THE DOMAIN of a cost that arrives in device memory is the caller's responsibility: +0 ... +Inf (sfa_epic_nearest_seeds_batch); a NaN or a negative cost is
 * not looked for -- there is no read-back -- and the search has no defined result on one.  Asynchronous. */
int  sfa_epic_job_upload_device(sfa_epic_job *job, int i0, int n, const float *lab_dev, const long long lab_strides[4], const float *cost_dev,
                                const long long cost_strides[3], int cost_has_euc);
/* Image i's matches from device memory: nm contiguous rows of x1 y1 x2 y2, copied on the stream.  The coordinates are not tested for finite values
 * (sfa_epic_job_upload does that on the host).  Asynchronous: matches_dev must stay valid, and unchanged, until the context's stream has passed the copy
 * (sfa_ctx_signal_stream, or the wait of sfa_epic_job_run). */
int  sfa_epic_job_set_matches_device(sfa_epic_job *job, int i, const float *matches_dev, int nm);
/* epic() for the images [0, n): the saliency filter on the planes the job holds, then sfa_epic_batch's chain on its device planes -- the same sub-batches
 * within workspace_bytes (0: half of the GPU's free memory), the context's search mode (sfa_ctx_set_epic_search), rc[n], counts[n][3] (or NULL) and
 * status[n] as sfa_epic_batch has them, and fields that equal its planes bit for bit.  An image with rc 1 (no match, or none left) holds a field of zeros
 * afterwards, which is what the driver starts such a window from (slow_flow.cpp:529 of the host program); an image with status 1 holds no field.
 * LIKE THE CHAIN THIS CALL WAITS FOR THE STREAM: the chain reads the survivors of its filters on the host.  Refused: an image of [0, n) without matches,
 * cost map or (saliency_th != 0) Lab image. */
int  sfa_epic_job_run(sfa_epic_job *job, int n, int *rc, int (*counts)[3], size_t workspace_bytes, int *status);
/* Image i's field to host planes of `stride` floats per row (columns >= w not written; waits).  Refused: an image without a field (not run, or status 1). */
int  sfa_epic_job_download(sfa_epic_job *job, int i, float *fx, float *fy, int stride);
/* The fields of [i0, i0 + n) to flow_dev [n][2][h][w] at strides[4] = element strides of (image, u|v, row, column); asynchronous.  Refused: an image
 * without a field, a destination the device seam refuses or whose strides let two of its elements share memory. */
int  sfa_epic_job_download_device(sfa_epic_job *job, int i0, int n, float *flow_dev, const long long strides[4]);
/* Image i's field from host planes of `stride` floats per row, in place of a run's: what the driver does with an image the run flagged (status 1), after
 * epic() of the host program has computed it.  The image holds a field afterwards (rc 0).  Waits for its copies.  (This entry and sfa_sequence_lab's
 * Python form are what the driver needs beyond the list of create / upload / set_lab / upload_device / set_matches_device / run / download.) */
int  sfa_epic_job_upload_flow(sfa_epic_job *job, int i, const float *fx, const float *fy, int stride);
/* epic_to_initial_flow of the driver (slow_flow.cpp:826-843) on the GPU: the fields of the epic job's images [i0, i0 + n) become the initial flow of the
 * job's windows [b0, b0 + n), written where sfa_job_set_flow_device writes.  Fields of the job's size: one fp32 multiplication by mul_u / mul_v
 * (image_mul_scalar; the driver passes fx / steps, fy / steps).  Fields of a size that divides the job's in both directions: sfa_resize_linear's arithmetic
 * per plane, then that multiplication.  Any other size is refused: the reference keeps a field of the reduced size there (:538-544 of the host program).
 * Both jobs on ONE context (one stream orders the run before this call); refused otherwise, and for an image without a field.  One launch; asynchronous. */
int  sfa_job_set_flow_epic(sfa_job *job, int b0, int n, const sfa_epic_job *epic_job, int i0, float mul_u, float mul_v);

/* Ordering against a stream of the caller (a hipStream_t; NULL = the device's null stream, which is torch's default stream).  wait: the context's
 * stream waits for everything submitted to `stream` so far; signal: `stream` waits for everything submitted to the context's stream so far.  Both
 * record an event and return at once.  With wait before the first and signal after the last call that touches a buffer, work the caller submits to
 * its stream afterwards -- a free or reuse by a stream-ordered allocator included -- is ordered after the library's last access.  The context keeps
 * its own stream; one context per host thread, as before.  `stream` must be a stream of the context's GPU: the handle is not checked. */
int  sfa_ctx_wait_stream(sfa_ctx *ctx, void *stream);
int  sfa_ctx_signal_stream(sfa_ctx *ctx, void *stream);

/* SOR-only resident batch: `batch` independent systems of one size */
typedef struct sfa_sor_batch sfa_sor_batch;
int  sfa_sor_batch_create(sfa_ctx *ctx, int w, int h, int batch, sfa_sor_batch **out);
void sfa_sor_batch_destroy(sfa_sor_batch *sb);
int  sfa_sor_batch_upload(sfa_sor_batch *sb, int b, const float *du, const float *dv, const float *a11, const float *a12,
                          const float *a22, const float *b1, const float *b2, const float *sh, const float *sv, int stride);
int  sfa_sor_batch_run(sfa_sor_batch *sb, int iterations, float omega);   /* prepare + solve + finish, async */
int  sfa_sor_batch_download(sfa_sor_batch *sb, int b, float *du, float *dv, int stride);

/* ---- test hook: the bound of the solver's in-kernel waits --------------------------------------------------------------------------
 * Every wait of one workgroup for another inside the SOR kernels is bounded (2^22 polls); a wait that gives up poisons the launch, every other wait
 * of the launch gives up at its next look at the error word, the kernel drains, and the entry point returns SFA_ERR_TIMEOUT.  `spins` > 0 shortens
 * that bound for this context (1: any wait that is not satisfied at once gives up) so that the path can be exercised; 0 restores the default.
 * A context that has returned SFA_ERR_TIMEOUT stays usable: progress words, tickets and the error word are reset by the next launch. */
int  sfa_ctx_set_wait_bound(sfa_ctx *ctx, unsigned spins);

/* ---- test / tooling hooks: the library's cross-check and what-if paths ------------------------------------------------------------
 * sfa_debug_set: one switch ("SFA_UNFUSED", "SFA_SOR_CHAIN", ... -- the names tools/README.md lists); value NULL = back to the default.  The library reads
 * these names from the ENVIRONMENT only when SFA_DEBUG=1 is set at the first sfa_ctx_create of the process: a drop-in caller's environment cannot otherwise
 * select other kernels.  Process-wide; not to be called while a refinement runs.
 * sfa_ctx_set_verbose: the reference's "inner it / outer it ... avg change" lines (variational_mt.cpp:404-405, 431-432) on stdout for this context; costs a
 * host round trip per iteration. */
int  sfa_debug_set(const char *name, const char *value);
int  sfa_ctx_set_verbose(sfa_ctx *ctx, int on);

/* ---- test hook: the linear system of a pair job --------------------------------------------------------------------------------------
 * a11, a12, a22, b1, b2 of pair b as the last data-term launch of the last run left them (host planes, row stride `stride`); waits for the stream.  The
 * switch SFA_PAIR_UNFUSED=1 (sfa_debug_set) makes a pair job run the stored derivative stack and k_data_2f instead of k_data_2f_fused, on a stack it
 * allocates at the first such run: the parity test compares the two systems plane by plane. */
int  sfa_pair_job_download_system(sfa_pair_job *job, int b, float *a11, float *a12, float *a22, float *b1, float *b2, int stride);

/* ---- test hooks: the pyramid, stage by stage ------------------------------------------------------------------------------------------
 * sfa_pyramid_down: one pyramid step (cv::GaussianBlur(sigma) then cv::resize to dw x dh, variational_mt.cpp:607,611) of nb windows of nplanes planes each,
 * host planes src[nb][nplanes][sh][sstride] -> dst[nb][nplanes][dh][dstride], through the function sfa_job_run's pyramid calls per level: k_pyr_down where
 * its footprint fits LDS and the radius is at most 8, else k_gauss_h / k_gauss_v + k_resize; SFA_PYRAMID_UNFUSED=1 (sfa_debug_set) forces the latter.
 * info (may be NULL) = {1 if k_pyr_down ran else 0, its tile height td, its LDS bytes}.  sigma as for sfa_gaussian_blur: at most 33 taps.
 * sfa_resize_flow: the flow's hand-over between two levels (variational_mt.cpp:672-680, 711-717; k_resize_flow): nb fields, host planes swx, swy
 * [nb][sh][sstride] -> dwx, dwy [nb][dh][dstride], resized like sfa_resize_linear and multiplied by post_x / post_y.
 * sfa_job_download_level_frame: the 3 planes of frame f (0 .. 2 (S - 1)) of window b at pyramid level `level` as the last sfa_job_run left them
 * (level 0: the uploaded frame, presmoothed if the cfg's sigma > 0), host rows of `stride` >= the level's width floats; waits for the stream. */
int  sfa_pyramid_down(sfa_ctx *ctx, float *dst, int dw, int dh, int dstride, const float *src, int sw, int sh, int sstride, int nplanes, int nb, float sigma,
                      int info[3]);
int  sfa_resize_flow(sfa_ctx *ctx, float *dwx, float *dwy, int dw, int dh, int dstride, const float *swx, const float *swy, int sw, int sh, int sstride, int nb,
                     float post_x, float post_y);
int  sfa_job_download_level_frame(sfa_job *job, int b, int level, int f, float *frame3, int stride);

/* ---- test hook: the division of the normalised data terms --------------------------------------------------------------------
 * The cfg-default instance of the fused assembly kernel forms the quotients r^2 / n and t / n of variational_aux_mt.cpp:240-250, 333-347, 479-490, 556-572
 * with the hardware's correctly-rounded chain and ONE refined reciprocal per denominator, behind range guards (kernels.hip: recip_of / div_by / num_ok).
 * Per element: q_chain = that chain without any guard, q_exact = the IEEE division, admitted = 1 where the guards let the chain be used.  The parity test
 * asserts q_chain == q_exact bit for bit wherever admitted == 1. */
int  sfa_division_chain(sfa_ctx *ctx, const float *numerators, const float *denominators, float *q_chain, float *q_exact, unsigned char *admitted, size_t n);

/* ---- in-library kernel timing (HIP events on the context's stream) ---------------------------------
 * While enabled every SOR solve kernel launch is bracketed by an event pair on the launch stream. */
int  sfa_profile_enable(sfa_ctx *ctx, int on);
int  sfa_profile_read(sfa_ctx *ctx, int *n_sor_launches, double *sor_ms_total, double *sor_bytes_total);
/* the same for the data-term assembly kernel (pixels x data terms of the bracketed launches), and the name of the solver kernel shape the last
 * solve was launched with (so that a measurement can be matched to the kernel it was taken from) */
int  sfa_profile_read_kernels(sfa_ctx *ctx, int *n_assembly_launches, double *assembly_ms_total, double *assembly_pixel_terms, char *sor_kernel, int sor_kernel_len);
/* wall bracket on the stream: start/stop an event pair around arbitrary enqueued work */
int  sfa_timer_start(sfa_ctx *ctx);
int  sfa_timer_stop(sfa_ctx *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif
