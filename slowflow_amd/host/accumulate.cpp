// accumulate.cpp -- the first stage of dense_tracking (step 3 of the reference's pipeline, README "Run Pipeline"): chains the jets that slow_flow wrote
// into trajectories at the final frame rate.  Same command line as dense_tracking (dense_tracking.cpp:408-476: <cfg> [-select k] [-resume]), the same
// derivation of steps, Jets, skip and r_Jets from the cfg (:482-571, :1102-1108), the same flow file names (:1118-1119), and accumulateConsistentBatches
// (utils/utils.cpp:517-617) for every start_jet and rate on the GPU: sfa_accumulate_consistent, all segments that share FF in one call (up to a memory
// bound).  It writes, per rate r and start_jet:
//   <output>/accumulated/<r>/<flow_format % sequence_start>.flo   the last step's accumulated flow on the grid (what the fully tracked pixels' hypotheses
//                                                                 end at), rounded to fp32 as writeFlowMiddlebury rounds it (utils.cpp:333)
//   <output>/accumulated/<r>/tracked_<sequence_start>.pgm         255 where tracked == FF, else 255 * tracked / FF
// and <output>/accumulated/run.json: per segment the created and rejected hypotheses (:1353), plus timings.
// With -energies it also scores every hypothesis as dense_tracking does before its fusion (:1219-1257; sfa_hypothesis_energies) and writes
//   <output>/accumulated/<r>/energy_<sequence_start>.pfm          the energy per grid pixel, fp32 (exact: the reference sums four floats), +Inf without one
//   <output>/accumulated/<r>/occluded_<sequence_start>.pgm        the number of occluded frames of the hypothesis (0 without one)
//   <output>/accumulated/best_<sequence_start>.pgm                the rate of lowest energy (ties: the lower r; 255: none) -- the first element of the
//                                                                 reference's sort by compareHypotheses (:1401), NOT the TRW-S result
//
// With -fuse (implies -energies) it fuses every start_jet's rates as dense_tracking does (:1588-1905): the smoothness weight of normalised frame 0, NMS,
// the pairwise MRF and TRW-S in raster order.  Both flags run through one resident track job (sfa_track_job): the start_jets to do
// are uploaded in groups of acc_gpu_batch (absent: chosen from the free device memory, at most 16) and each group is tracked, scored and fused by one
// launch sequence on the GPU.  -fuse writes
//   <output>/accumulated/<flow_format % sequence_start>.flo       the fused flow on the grid, u(Jets - 1) / xy_incr; UNKNOWN_FLOW (1e10) without a node
//   <output>/accumulated/<...>_vis.png                            its colour coding
//   <output>/accumulated/occlusions/frame_<sequence_start>.pgm    max_t occluded(t) of the chosen hypothesis, 0 / 255
//   <output>/accumulated/labels_<sequence_start>.pgm              the chosen rate (255: none)
//
// Jets of another size than the tracking frames (slow_flow.cfg estimates at scale 0.25, dense_tracking.cfg tracks at scale 1.0) are cropped (center /
// extent, utils.cpp:308-318), resized by rescale = (1.0f * W) / cw and multiplied by it on the GPU, their occlusion images resized with the cubic
// (:1134-1146, :1171-1189; sfa_accumulate_consistent_scaled, sfa_hypothesis_energies_scaled).  The target W x H is the ingested frames' size with
// -energies / -fuse (after center / extent and scale); in the plain mode the jets' common size, or, where the rates differ, the size of the ingested
// frame at sequence_start.  Refused: a rate whose rescaled size is not the target, a crop outside a flow, occlusions together with center.
//
// With -fill (implies -fuse) every rate also gets dense_tracking's EpicFlow fill-in hypothesis (:1265-1350): the rate's consistent trajectories,
// interpolated to every pixel at every step (epic_fill_rate, host/epic_fill.h), scored like any other hypothesis and fused with the accumulated ones in
// the reference's push order (slot 2 r: rate r accumulated, slot 2 r + 1: rate r filled in), so that the fused flow has no holes.  It reads
// <output>/accumulated/tmp/edges_<sequence_start>.dat (the reference's name, :945; read_edges' format) and runs through the same track job, created with
// sfa_track_job_create_fill, in the same groups of acc_gpu_batch: the Lab image of the 8-bit frame 0 and the edge map go up with each start_jet, and
// the fill-in of a whole group is one launch sequence per rate.  acc_skip_pixel 0; with acc_gpu_reference_image 1 also 1 and 3 (the reference's blurred
// and resized 8-bit image of frame 0, :931-936, is formed on the GPU as INTEGRATION.md 4c' defines it: sfa_track_job_upload_fill_reference; the
// restatement is parity-unpinned against OpenCV, hence the key); at most 8 rates.
//
// With -reference the program writes <output>/accumulated/tmp/frame_epic_<sequence_start>.png (the reference's name, :944) for every start_jet and exits:
// the reduced 8-bit RGB image of frame 0 on the grid, the image an edge detector has to see to produce the edges_<sequence_start>.dat that -fill reads.
//
// With -alternate (implies -fill) the job alternates (sfa_track_job_create_alternate): acc_alternate rounds of prune, neighbour proposals, rescoring and
// fusion as INTEGRATION.md 4d defines them (FLANN and GSL are not in this tree); labels hold origin slots, proposed_<sequence_start>.pgm is written.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "epic_fill.h"
#include "flow_vis.h"
#include "image.h"
#include "ingest.h"
#include "io.h"
#include "parameter_list.h"
#include "png.h"
#include "util.h"
#include "../../include/slowflow_amd.h"

using std::string;
using std::vector;

static void usage() {
    printf("usage:\n");
    printf("    ./accumulate [cfg] -select [estimation for one specific final pair] -resume -energies -fuse -fill -alternate -reference\n");
    printf("    ./accumulate -decode_occlusion [occlusion .pgm / .pbm] [mask .pgm]   (the mask this program uses: median 3x3, 255 - x; 0 = occluded)\n");
    printf("\n");
    printf("Runs dense_tracking's first stage only: consistent accumulation of the jets (accumulateConsistentBatches).  cfg keys read: jet_estimation\n");
    printf("(repeated), jet_S, jet_fps, jet_weight, flow_format, start, ref_fps, ref_fps_F, max_fps, acc_min_fps, acc_skip_pixel, acc_use_jet_occlusions\n");
    printf("(or acc_occlusion), acc_discard_inconsistent, acc_consistency_threshold, output, sintel, subframes, center, extent.  A missing input file exits\n");
    printf("with status 2.\n");
    printf("\n");
    printf("Jets of another size than the target are cropped (center / extent), resized by (1.0f * W) / cw and multiplied by it on the GPU, as dense_tracking\n");
    printf("does.  The target W x H: with -energies / -fuse the ingested frames' size; else the jets' common size, or where the rates differ the size of the\n");
    printf("frame at `start` (cfg `file`, scale, center / extent).  Refused: a rate whose rescaled size is not the target, a crop outside a flow,\n");
    printf("occlusions together with center.\n");
    printf("\n");
    printf("-energies: also reads the Jets + 1 frames of each start_jet (cfg `file`, the driver's ingest: scale, raw, raw_demosaicing 0 / 2), normalises\n");
    printf("them and writes each hypothesis' unary energy (energy_<start>.pfm), its occluded frames (occluded_<start>.pgm) and the lowest-energy rate\n");
    printf("(best_<start>.pgm).  Keys: acc_jet_consistency, acc_brightness_constancy, acc_gradient_constancy, acc_occlusion_penalty, acc_temporal_occ,\n");
    printf("acc_cv, acc_occlusion_threshold, acc_occlusion_fb_threshold, acc_penalty_fct_data, acc_penalty_fct_data_eps.  Refused: acc_occlusion 1,\n");
    printf("grayscale 1, raw_demosaicing 1, Jets > 32.  acc_gpu_batch: the start_jets of one run on the GPU (1 .. 64; absent: chosen from the free device\n");
    printf("memory, at most 16); outside 1 .. 64, or too large for the device, the program exits with status 1.\n");
    printf("\n");
    printf("-fuse: implies -energies, then fuses all rates of each start_jet with TRW-S (raster order) into <flow_format %% start>.flo, _vis.png,\n");
    printf("occlusions/frame_<start>.pgm and labels_<start>.pgm.  Keys: acc_beta, acc_spatial_occ, acc_traj_sim_method, acc_traj_sim_thres, acc_trws_eps,\n");
    printf("acc_trws_max_iter, 16bit, img_norm_avg_*, img_norm_std_*.  Refused: acc_approach 1, acc_traj_sim_method 2, a width that is not a multiple\n");
    printf("of 4, more than 16 rates.  EpicFlow's fill-in and the neighbour proposals (acc_epic_interpolation) are not run.\n");
    printf("\n");
    printf("-fill: implies -fuse, and adds EpicFlow's fill-in hypothesis of every rate (removeSmallSegments on the consistent pixels, their matches at\n");
    printf("every acc_epic_skip-th pixel, one batch of EpicFlow interpolations per rate) to the fusion: slot 2 r is rate r's accumulated hypothesis, slot\n");
    printf("2 r + 1 its fill-in; labels_<start>.pgm holds the slot.  Reads <output>/accumulated/tmp/edges_<start>.dat (w * h floats; a missing one exits\n");
    printf("with status 2), so the output folder exists beforehand: run it with -resume.  Key: acc_epic_skip (2).  acc_skip_pixel 0 is served; with\n");
    printf("acc_gpu_reference_image 1 (default 0) also 1 and 3: the reference's 8-bit, blurred and resized image of frame 0 is then formed on the GPU\n");
    printf("(INTEGRATION.md 4c'; OpenCV's arithmetic restated, parity-unpinned against OpenCV).  Refused: acc_skip_pixel other than 0 without that key,\n");
    printf("any other acc_skip_pixel with it, a frame size OpenCV's resize rounds to another grid (width 7 at acc_skip_pixel 1), more than 8 rates,\n");
    printf("acc_epic_interpolation 0.  The neighbour proposals are not run.  acc_gpu_epic_search (0): 1 runs the fill-in's graph searches in\n");
    printf("the library's compact mode (slices of seeds in one shared workspace: the same bits, and match counts whose ns * ns table would not fit, such as\n");
    printf("acc_epic_skip 2 on a full frame, stay on the GPU); any other value exits with status 1.\n");
    printf("\n");
    printf("-reference: writes <output>/accumulated/tmp/frame_epic_<start>.png for every start_jet (with -select: that one) and exits with status 0: the\n");
    printf("reduced 8-bit RGB image of frame 0 on the grid (acc_skip_pixel 0, 1, 3), what an edge detector has to read to write the edges_<start>.dat of\n");
    printf("-fill.  Keys: file, start, 16bit, scale, center / extent, raw.  Every other flag but -select and -resume is ignored.\n");
    printf("\n");
    printf("-alternate: implies -fill, and runs acc_alternate (5) rounds of prune (to the last selection plus acc_perturb_keep), neighbour proposals, their\n");
    printf("rescoring and the fusion in place of the one fusion (the track job that alternates; INTEGRATION.md 4d defines the rounds).  Keys: acc_perturb_keep\n");
    printf("(no default: needed when acc_alternate > 1), acc_neigh_hyp (5), acc_neigh_hyp_radius (100), acc_neigh_skip1 (2), acc_neigh_skip2 (4),\n");
    printf("acc_hyp_neigh_tryouts (20), seed (0, recorded in run.json; the reference takes the clock).  labels_<start>.pgm holds the slot the chosen hypothesis\n");
    printf("was born in, the new proposed_<start>.pgm 255 where it arrived from a neighbour; run.json gains the rounds.  Refused by name with status 1:\n");
    printf("slots + 2 acc_neigh_hyp > 16, acc_perturb_keep + 1 + 2 acc_neigh_hyp > 16, acc_neigh_skip1/2 < 1, acc_hyp_neigh_tryouts < 0, acc_neigh_hyp_radius <= 0.\n");
}

// dense_tracking.cpp:1183-1193 for a file of the flows' size: medianBlur(3) with OpenCV's border for ksize 3 (replicate; OpenCV is absent here, so this
// median is parity-unpinned), then 255 - x.  0 = occluded.  The slow_flow drivers write grey 255 where the occlusion label is +1 (slow_flow.cpp:896-898:
// 0.5 (occ + 1) * 255; this project's writePGM(offset 1, scale 127.5)), and that is what comes out as 0.  out: row stride `stride` bytes.
static void decode_occlusion(const vector<unsigned char> &g, int w, int h, int stride, unsigned char *out) {
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            unsigned char v[9];
            int k = 0;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int yy = std::min(std::max(y + dy, 0), h - 1), xx = std::min(std::max(x + dx, 0), w - 1);
                    v[k++] = g[(size_t)yy * w + xx];
                }
            std::nth_element(v, v + 4, v + 9);
            out[(size_t)y * stride + x] = (unsigned char)(255 - v[4]);
        }
}

// everything main() derives from the cfg (:479-594, :716-746) and the mode
struct Run {
    string cfg;
    vector<string> jets;                     // jet_estimation lines, each ending in '/': one per rate
    vector<int> jet_S, jet_fps;              // per rate, from the cfg or each jet folder's config.cfg
    vector<double> jet_weight;               // as the cfg gives them (the rate where it does not)
    unsigned rates = 0, Jets = 0, sequence_start = 0, start_jets = 1;   // start_jets: ref_fps_F
    int steps = 0, skip = 0, max_fps = 0, skip_pixel = 1, min_fps_idx = 0;
    double threshold = 1;
    bool discard = true, use_occ = false, sintel = false;
    bool energies = false, fuse = false;     // -energies, -fuse (implies -energies)
    bool fill = false;                       // -fill (implies -fuse)
    bool alternate = false;                  // -alternate (implies -fill): the reference's rounds of prune, neighbour proposals and fusion
    bool reference = false;                  // -reference: write each start_jet's reduced 8-bit image and exit
    string flow_format, acc_dir;             // flow_format without its extension; <output>/accumulated/
    bool crop_flows = false, crop_frames = false;   // center.x > 0 (:1135); extent.x > 0 || extent.y > 0 (:876)
    int cx = 0, cy = 0, ex = 0, ey = 0;      // center, extent
    string size_frame;                       // the plain mode with rates of different sizes: the frame whose ingested size is the target
};

struct Segment {
    int r = 0;                   // rate (index of its jet_estimation line)
    unsigned start_jet = 0, seq_start = 0;
    int FF = 0;
    string out_flo, out_tracked;
    vector<string> fwd, bwd, occ;   // input files, FF each (occ: empty without occlusions)
    int created = 0, rejected = 0;
};

// rc == SFA_OK; otherwise the library's message on stderr
static bool sfa_ok(sfa_ctx *ctx, int rc) {
    if (rc != SFA_OK) std::cerr << sfa_last_error(ctx) << std::endl;
    return rc == SFA_OK;
}

// the fused flow's name without its extension (:1895-1898)
static string fused_base(const Run &run, unsigned seq_start) {
    return run.acc_dir + (run.sintel ? fmt2(run.flow_format, (int)seq_start, 0) : fmt1(run.flow_format, (int)seq_start));
}

// the size in a .flo's header; false where the file is none
static bool flo_size(const string &file, int &w, int &h) {
    FILE *f = fopen(file.c_str(), "rb");
    if (!f) return false;
    float tag = 0;
    int wh[2] = {0, 0};
    const bool ok = fread(&tag, 4, 1, f) == 1 && fread(wh, 4, 2, f) == 2 && tag == 202021.25f && wh[0] >= 1 && wh[1] >= 1;
    fclose(f);
    w = wh[0]; h = wh[1];
    return ok;
}

// where each rate's files sit relative to the target: the size of the rate's first flow and the crop of utils.cpp:308-318 (center.x > 0, :1135).
// rescale and stride are filled later (fit_rates, read_segment).  1 with a message where a file is no .flo or the crop leaves the flow
static int read_geometry(const Run &run, const vector<Segment> &segs, vector<sfa_jet_source> &geo) {
    geo.assign(run.rates, sfa_jet_source{0, 0, 0, 0, 0, 0, 0, 1.0f});
    for (const Segment &s : segs) {
        sfa_jet_source &g = geo[s.r];
        if (g.sw) continue;
        if (!flo_size(s.fwd[0], g.sw, g.sh)) { std::cerr << "cannot read " << s.fwd[0] << " as a .flo" << std::endl; return 1; }
        g.cw = g.sw; g.ch = g.sh;
        if (!run.crop_flows) continue;
        g.x0 = run.cx - run.ex / 2; g.y0 = run.cy - run.ey / 2; g.cw = run.ex; g.ch = run.ey;   // off = x - extent / 2 + center
        if (g.x0 < 0 || g.y0 < 0 || g.cw < 1 || g.ch < 1 || g.x0 + g.cw > g.sw || g.y0 + g.ch > g.sh) {
            std::cerr << "center " << run.cx << "," << run.cy << " / extent " << run.ex << "," << run.ey << ": the crop leaves the " << g.sw << " x " << g.sh
                      << " flows of rate " << s.r << " (" << s.fwd[0] << "); the reference reads outside its Mat there" << std::endl;
            return 1;
        }
    }
    return 0;
}

// rescale = (1.0f * W) / cw per rate (:1142); false with a message where a rate's rescaled size, cvRound(cw * rescale) x cvRound(ch * rescale), is not W x H
static bool fit_rates(vector<sfa_jet_source> &geo, int W, int H) {
    for (size_t r = 0; r < geo.size(); r++) {
        sfa_jet_source &g = geo[r];
        if (!g.sw) continue;                                              // no segment of this rate
        g.rescale = (1.0f * W) / g.cw;
        const long tw = lrint((double)g.cw * (double)g.rescale), th = lrint((double)g.ch * (double)g.rescale);
        if (tw != W || th != H) {
            std::cerr << "rate " << r << ": its " << g.cw << " x " << g.ch << " flows rescaled by " << g.rescale << " are " << tw << " x " << th << ", not the target "
                      << W << " x " << H << std::endl;
            return false;
        }
    }
    return true;
}

static bool same_geometry(const sfa_jet_source &a, const sfa_jet_source &b) {
    return a.sw == b.sw && a.sh == b.sh && a.x0 == b.x0 && a.y0 == b.y0 && a.cw == b.cw && a.ch == b.ch;
}

// segments' flows (and raw occlusion images) read into host images, appended to `in`; false with a message on failure
struct SegmentInput {
    vector<image_t **> fl;                                                // forward, backward per step
    vector<const float *> fu, fv, bu, bv;
    vector<vector<unsigned char>> mbuf;                                   // the occlusion images as read, rows of the flows' stride
    vector<const unsigned char *> mp;
    ~SegmentInput() { for (image_t **c : fl) { image_delete(c[0]); image_delete(c[1]); free(c); } }
};
static bool read_segment(const Segment &s, bool use_occ, sfa_jet_source &g, SegmentInput &in) {
    for (int f = 0; f < s.FF; f++) {
        image_t **a = readFlowFile(s.fwd[f].c_str()), **b = readFlowFile(s.bwd[f].c_str());
        if (a) in.fl.push_back(a);
        if (b) in.fl.push_back(b);
        if (!a || !b) { std::cerr << "cannot read " << (a ? s.bwd[f] : s.fwd[f]) << " as a .flo" << std::endl; return false; }
        for (image_t **c : {a, b})
            if (c[0]->width != g.sw || c[0]->height != g.sh) {
                std::cerr << (c == a ? s.fwd[f] : s.bwd[f]) << " is " << c[0]->width << " x " << c[0]->height << ", not " << g.sw << " x " << g.sh
                          << " like the first flow of rate " << s.r << std::endl;
                return false;
            }
        g.stride = a[0]->stride;
        in.fu.push_back(a[0]->data); in.fv.push_back(a[1]->data); in.bu.push_back(b[0]->data); in.bv.push_back(b[1]->data);
        if (use_occ) {
            int ow, oh;
            vector<unsigned char> px;
            if (!read_pnm8(s.occ[f], ow, oh, px)) { std::cerr << s.occ[f] << ": not a binary PGM (maxval 255) or PBM" << std::endl; return false; }
            if (ow != g.sw || oh != g.sh) { std::cerr << s.occ[f] << " is not " << g.sw << " x " << g.sh << std::endl; return false; }
            in.mbuf.emplace_back((size_t)g.stride * g.sh, 0);
            for (int y = 0; y < oh; y++) memcpy(in.mbuf.back().data() + (size_t)y * g.stride, px.data() + (size_t)y * ow, (size_t)ow);
        }
    }
    in.mp.clear();
    for (auto &m : in.mbuf) in.mp.push_back(m.data());
    return true;
}

// one frame as dense_tracking ingests it (:793-905): decoded, demosaiced (raw_demosaicing 0 / 2) or taken as RGB, cropped (center / extent), rescaled
// where scale != 1
static color_image_t *ingest_frame(ParameterList &params, const Run &run, sfa_ctx *ctx, const string &name) {
    vector<int> red_loc;
    std::stringstream ss(params.parameter<string>("raw_red_loc", "0,0"));
    for (string t; std::getline(ss, t, ',');) red_loc.push_back(atoi(t.c_str()));
    int maxval = 255;
    string error;
    color_image_t *img = load_frame(name, params.exists("raw") && params.parameter<bool>("raw"), params.parameter<int>("raw_demosaicing", "0"),
                                    red_loc.size() > 0 ? red_loc[0] : 0, red_loc.size() > 1 ? red_loc[1] : 0, &maxval, &error);
    if (!img) { std::cerr << error << std::endl; return nullptr; }
    if (run.crop_frames) {                                                // use only a part of the images, before the rescaling (:875-886)
        color_image_t *part = color_image_crop(img, run.cx, run.cy, run.ex, run.ey);
        if (!part) std::cerr << "center / extent do not fit the " << img->width << " x " << img->height << " frame " << name << std::endl;
        color_image_delete(img);
        if (!part) return nullptr;
        img = part;
    }
    const float scale = (float)params.parameter<double>("scale", "1.0");
    if (scale != 1) {                                                     // GaussianBlur + resize against aliasing (:863-868)
        color_image_t *small = color_image_rescale(ctx, img, scale);
        color_image_delete(img);
        if (!small) std::cerr << "rescaling " << name << " failed: " << sfa_last_error(ctx) << std::endl;
        img = small;
    }
    return img;
}

// a segment's last step: the accumulated flow on the grid as <flow_format % start>.flo (convertTo(CV_32F), utils.cpp:333; channel 1 = u) and
// tracked_<start>.pgm (255 where tracked == FF, else 255 * tracked / FF), its created and rejected hypotheses (:1225-1257) and the line of :1353.
// u, v, tracked: gw x gh planes.  false where a file cannot be written
static bool write_last_step(Segment &s, const double *u, const double *v, const int *tracked, int gw, int gh) {
    image_t *fu = image_new(gw, gh), *fv = image_new(gw, gh);
    vector<unsigned char> tp((size_t)gw * gh);
    for (int y = 0; y < gh; y++)
        for (int x = 0; x < gw; x++) {
            const size_t i = (size_t)y * gw + x;
            fu->data[(size_t)y * fu->stride + x] = (float)u[i];
            fv->data[(size_t)y * fv->stride + x] = (float)v[i];
            const int t = tracked[i];
            if (t == s.FF) s.created++; else s.rejected++;
            tp[i] = (unsigned char)(t == s.FF ? 255 : 255 * t / s.FF);
        }
    const bool ok = writeFlowFile(s.out_flo.c_str(), fu, fv) == 0 && write_pgm8(s.out_tracked, gw, gh, tp.data(), gw);
    image_delete(fu); image_delete(fv);
    std::cout << "rate " << s.r << ", start " << s.seq_start << ": " << s.created << " trajectory hypotheses generated! (" << s.rejected << " rejected)"
              << std::endl;
    return ok;
}

// run.json: the cfg's figures, the rates, the segments and the skipped outputs, then `tail` (the mode's own fields, each after ",\n  ").
// -energies writes 17 digits, jet_weight as the float it scores with and each segment's hypotheses; the plain run the stream's defaults
static bool write_run_json(const Run &run, const vector<Segment> &segs, const vector<string> &skipped, const vector<sfa_jet_source> &geo, int width, int height,
                           const string &tail) {
    std::ofstream js((run.acc_dir + "run.json").c_str());
    if (run.energies) js.precision(17);
    js << "{\n  \"cfg\": \"" << run.cfg << "\",\n  " << (run.energies ? "\"energies\": true, " : "") << "\"Jets\": " << run.Jets << ", \"steps\": "
       << run.steps << ", \"skip\": " << run.skip << ", \"acc_skip_pixel\": " << run.skip_pixel << ", \"width\": " << width << ", \"height\": " << height
       << ",\n  \"rates\": [";
    for (unsigned r = 0; r < run.rates; r++) {
        const double weight = run.jet_weight.size() > r ? run.jet_weight[r] : (double)r;
        js << (r ? ", " : "") << "{\"jet_estimation\": \"" << run.jets[r] << "\", \"jet_S\": " << run.jet_S[r] << ", \"jet_fps\": " << run.jet_fps[r]
           << ", \"jet_weight\": " << (run.energies ? (double)(float)weight : weight) << ", \"source_width\": " << geo[r].sw << ", \"source_height\": " << geo[r].sh
           << ", \"rescale\": " << (double)geo[r].rescale << "}";
    }
    js << "],\n  \"segments\": [";
    for (size_t i = 0; i < segs.size(); i++) {
        js << (i ? ",\n    " : "\n    ") << "{\"rate\": " << segs[i].r << ", \"start_jet\": " << segs[i].start_jet << ", \"sequence_start\": " << segs[i].seq_start
           << ", \"FF\": " << segs[i].FF << ", \"created\": " << segs[i].created << ", \"rejected\": " << segs[i].rejected;
        if (run.energies) js << ", \"hypotheses\": " << segs[i].created;
        js << ", \"flo\": \"" << segs[i].out_flo << "\"}";
    }
    js << "],\n  \"skipped\": [";
    for (size_t i = 0; i < skipped.size(); i++) js << (i ? ", " : "") << "\"" << skipped[i] << "\"";
    js << "]" << tail << "\n}\n";
    return js.good();
}

// the plain run: accumulateConsistentBatches for every segment, those that share FF and the geometry of their files in one call of up to 2 GiB of
// device planes.  The target is the jets' common size, or the ingested size of run.size_frame where the rates differ
static int run_accumulate(ParameterList &params, const Run &run, vector<Segment> &segs, const vector<string> &skipped, vector<sfa_jet_source> &geo) {
    sfa_ctx *ctx = nullptr;
    if (!segs.empty() && !sfa_ok(nullptr, sfa_ctx_create(0, &ctx))) return 1;
    double t_read = 0, t_gpu = 0, t_write = 0;
    const double t0 = now_s();
    int width = 0, height = 0, calls = 0, status = 0;
    if (!run.size_frame.empty()) {
        color_image_t *img = ingest_frame(params, run, ctx, run.size_frame);
        if (!img) status = 1;
        else { width = img->width; height = img->height; color_image_delete(img); }
    } else if (!segs.empty()) {
        width = geo[segs[0].r].cw; height = geo[segs[0].r].ch;
    }
    if (status == 0 && !segs.empty() && !fit_rates(geo, width, height)) status = 1;
    std::map<std::pair<int, int>, vector<size_t>> groups;                 // (FF, the first rate of the same geometry)
    for (size_t i = 0; i < segs.size(); i++) {
        int gi = segs[i].r;
        for (int r = 0; r < gi; r++)
            if (geo[r].sw && same_geometry(geo[r], geo[gi])) { gi = r; break; }
        groups[std::make_pair(segs[i].FF, gi)].push_back(i);
    }
    for (auto &grp : groups) {
        if (status) break;
        const int FF = grp.first.first;
        const vector<size_t> &idx = grp.second;
        sfa_jet_source &g = geo[grp.first.second];
        const bool identity = g.x0 == 0 && g.y0 == 0 && g.cw == g.sw && g.ch == g.sh && g.sw == width && g.sh == height;
        for (size_t lo = 0, hi; lo < idx.size() && status == 0; lo = hi) {
            double ta = now_s();
            SegmentInput in;                                              // [k * FF + f]: segment k's step f
            size_t bytes = 0;
            for (hi = lo; hi < idx.size() && status == 0 && (hi == lo || bytes < (size_t)2 << 30); hi++) {
                if (!read_segment(segs[idx[hi]], run.use_occ, g, in)) status = 1;
                // what the device holds per step: the planes as read (4 floats and a byte per source pixel) and, where they are resampled, two
                // double2 planes of the target
                bytes += (size_t)FF * ((size_t)g.sw * g.sh * 17 + (identity ? 0 : (size_t)width * height * 32));
            }
            double tb = now_s();
            t_read += tb - ta;
            if (status) break;
            const int n = (int)(hi - lo);
            int gw = 0, gh = 0;
            if (!sfa_ok(nullptr, sfa_accumulate_grid(width, height, run.skip_pixel, &gw, &gh))) { status = 1; break; }
            const size_t gpl = (size_t)gw * gh;
            vector<double> au(n * gpl), av(au.size());
            vector<int> tracked(au.size());
            calls++;
            if (!sfa_ok(ctx, sfa_accumulate_consistent_scaled(ctx, n, FF, width, height, &g, in.fu.data(), in.fv.data(), in.bu.data(), in.bv.data(),
                                                              run.use_occ ? in.mp.data() : nullptr, run.threshold, run.skip_pixel, run.discard, 0, au.data(),
                                                              av.data(), tracked.data(), nullptr))) { status = 1; break; }
            double tc = now_s();
            t_gpu += tc - tb;
            for (int k = 0; k < n && status == 0; k++) {
                Segment &s = segs[idx[lo + k]];
                if (!write_last_step(s, au.data() + k * gpl, av.data() + k * gpl, tracked.data() + k * gpl, gw, gh)) {
                    std::cerr << "cannot write " << s.out_flo << std::endl;
                    status = 1;
                }
            }
            t_write += now_s() - tc;
        }
    }
    if (ctx) sfa_ctx_destroy(ctx);
    if (status) return status;
    std::ostringstream tail;
    tail << ",\n  \"calls\": " << calls << ",\n  \"timings_s\": {\"read\": " << t_read << ", \"gpu_call\": " << t_gpu << ", \"write\": " << t_write
         << ", \"total\": " << now_s() - t0 << "}";
    const bool ok = write_run_json(run, segs, skipped, geo, width, height, tail.str());
    std::cout << "wrote " << segs.size() << " segment(s) to " << run.acc_dir << std::endl;
    return ok ? 0 : 1;
}

// -fuse: the settings (setDefault :136-152, read as at :605-625, :660-661) and the record of every fused start_jet
struct Fusion {
    sfa_fuse_params fup;
    float nav[3], nsd[3];                    // the statistics the smoothness weight de-normalises with (img_norm_avg_* / img_norm_std_*)
    int hbit = 0;
    // t_weight, t_fuse and stage_ms exist per group of start_jets only: each of its start_jets carries the group's value
    struct Round { double energy, bound; int iters, nodes, accepted; };
    struct Record { unsigned seq_start; int nodes, iters, group, group_size; double energy, bound, t_weight, t_fuse; float stage_ms[4]; vector<Round> rounds; };
    vector<Record> done;
};

// one start_jet's fused result out of the track job (:1588-1905 ran on the GPU): writes the fused flow (u(Jets - 1) / xy_incr, 1e10 without a node), its
// colour coding, the occlusions and the labels.  fu: the record with the group's figures filled in
// the fused planes of one start_jet as files; slots: the label slots of the fusion (the rates; with -fill two per rate)
static bool write_fused_planes(const Run &run, Fusion &fz, Fusion::Record fu, int gw, int gh, int slots, const vector<int> &slot, const vector<double> &flu,
                               const vector<double> &flv, const vector<unsigned char> &oc) {
    const size_t gpl = (size_t)gw * gh;
    image_t *u = image_new(gw, gh), *v = image_new(gw, gh);
    vector<unsigned char> lp(gpl), op(gpl);
    for (int y = 0; y < gh; y++)
        for (int x = 0; x < gw; x++) {
            const size_t i = (size_t)y * gw + x;
            u->data[(size_t)y * u->stride + x] = (float)flu[i];   // writeFlowMiddlebury's fp32 (utils.cpp:333); 1e10 without a node
            v->data[(size_t)y * v->stride + x] = (float)flv[i];
            lp[i] = slot[i] < 0 ? 255 : (unsigned char)slot[i];     // slot k is rate k; with -fill rate k / 2, accumulated (even) or filled in (odd)
            op[i] = oc[i] ? 255 : 0;                                // convertTo(CV_8UC1, 255) (:1893)
            fu.nodes += slot[i] >= 0;
        }
    const string base = fused_base(run, fu.seq_start);
    mkdirs(run.acc_dir + "occlusions/");
    const bool ok = writeFlowFile((base + ".flo").c_str(), u, v) == 0 && png_write((base + "_vis.png").c_str(), flowColorImg(u, v, 0)) &&
                    write_pgm8(run.acc_dir + "occlusions/frame_" + std::to_string(fu.seq_start) + ".pgm", gw, gh, op.data(), gw) &&
                    write_pgm8(run.acc_dir + "labels_" + std::to_string(fu.seq_start) + ".pgm", gw, gh, lp.data(), gw);
    if (!ok) std::cerr << "cannot write the fused outputs of start " << fu.seq_start << " under " << run.acc_dir << std::endl;
    image_delete(u); image_delete(v);
    std::cout << "start " << fu.seq_start << ": fused " << slots << (run.fill ? " slot(s) over " : " rate(s) over ") << fu.nodes << " nodes, energy " << fu.energy << ", lower bound "
              << fu.bound << ", " << fu.iters << " TRW-S iteration(s)" << std::endl;
    fz.done.push_back(fu);
    return ok;
}

static bool write_fused(sfa_ctx *ctx, sfa_track_job *job, int k, const Run &run, Fusion &fz, Fusion::Record fu, int gw, int gh, int rounds) {
    const size_t gpl = (size_t)gw * gh;
    vector<int> slot(gpl);
    vector<double> flu(gpl), flv(gpl);
    vector<unsigned char> oc(gpl);
    if (!sfa_ok(ctx, sfa_track_job_download_fused(job, k, slot.data(), flu.data(), flv.data(), oc.data(), nullptr, &fu.energy, &fu.bound, &fu.iters))) return false;
    if (run.alternate) {
        // the job's slot is a position of the last round's list: labels_<n>.pgm takes the slot the chosen hypothesis was born in, proposed_<n>.pgm whether it
        // arrived from a neighbour (0 / 255)
        const int R = rounds;
        vector<unsigned char> origin(gpl), prop(gpl);
        vector<double> e(R), b(R);
        vector<int> it(R), nd(R), ac(R);
        if (!sfa_ok(ctx, sfa_track_job_download_alternation(job, k, origin.data(), e.data(), b.data(), it.data(), nd.data(), ac.data()))) return false;
        for (size_t i = 0; i < gpl; i++) {
            prop[i] = slot[i] >= 0 && (origin[i] & 0x80) ? 255 : 0;
            slot[i] = slot[i] < 0 ? -1 : (origin[i] & 0x7f);
        }
        for (int r = 0; r < R; r++) fu.rounds.push_back(Fusion::Round{e[r], b[r], it[r], nd[r], ac[r]});
        if (!write_pgm8(run.acc_dir + "proposed_" + std::to_string(fu.seq_start) + ".pgm", gw, gh, prop.data(), gw)) {
            std::cerr << "cannot write " << run.acc_dir << "proposed_" << fu.seq_start << ".pgm" << std::endl;
            return false;
        }
    }
    return write_fused_planes(run, fz, fu, gw, gh, (int)run.rates * (run.fill ? 2 : 1), slot, flu, flv, oc);
}

// the energies' keys: setDefault (:118-165), in the types of :606-623 and :661-675
static void read_energy_params(ParameterList &params, sfa_energy_params &ep) {
    ep.acc_jc = params.parameter<float>("acc_jet_consistency", "1.0");
    ep.acc_bc = params.parameter<float>("acc_brightness_constancy", "0.1");
    ep.acc_gc = params.parameter<float>("acc_gradient_constancy", "1.0");
    ep.acc_occ = params.parameter<float>("acc_occlusion_penalty", "500.0");
    ep.acc_temporal_occ = params.parameter<double>("acc_temporal_occ", "10.0");
    ep.acc_cv = params.parameter<double>("acc_cv", "0.0");
    ep.occlusion_threshold = params.parameter<float>("acc_occlusion_threshold", "5.0");
    ep.occlusion_fb_threshold = params.parameter<float>("acc_occlusion_fb_threshold", "5.0");
    ep.penalty = params.parameter<int>("acc_penalty_fct_data", "1");
    ep.penalty_eps = params.parameter<double>("acc_penalty_fct_data_eps", "0.001");
}

// the fusion's keys and the smoothness weight's statistics
static void read_fusion(ParameterList &params, const Run &run, Fusion &fz) {
    sfa_fuse_params_default(&fz.fup);
    fz.fup.acc_beta = params.parameter<double>("acc_beta", "10.0");
    fz.fup.acc_spatial_occ = params.parameter<double>("acc_spatial_occ", "10.0");   // setDefault's "acc_satial_occ" never reaches this key
    fz.fup.traj_sim_method = params.parameter<int>("acc_traj_sim_method", "1");
    fz.fup.traj_sim_thres = params.parameter<double>("acc_traj_sim_thres", "0.1");
    fz.fup.trws_eps = params.parameter<double>("acc_trws_eps", "1e-5");
    fz.fup.trws_max_iter = params.parameter<int>("acc_trws_max_iter", "10");
    fz.fup.skip = run.skip_pixel;
    // the reference reads img_norm_* (defaults 0 / 1, :971-972), keys normalize() does not publish (it writes slow_flow_img_norm_*), so by default
    // the weight is taken from the normalised frame itself
    for (int k = 0; k < 3; k++) {
        fz.nav[k] = (float)params.parameter<double>("img_norm_avg_" + std::to_string(k + 1), "0");
        fz.nsd[k] = (float)params.parameter<double>("img_norm_std_" + std::to_string(k + 1), "1");
    }
    fz.hbit = params.parameter<bool>("16bit", "0") ? 1 : 0;
}

// -alternate: acc_alternate and the proposals' keys (setDefault :153-159, read as at :626-637); seed: the reference takes the clock, here the key or 0
static void read_alternation(ParameterList &params, sfa_track_alt_params &alt) {
    sfa_track_alt_params_default(&alt);
    alt.rounds = params.parameter<int>("acc_alternate", "5");
    alt.neigh.perturb_keep = params.exists("acc_perturb_keep") ? params.parameter<int>("acc_perturb_keep") : -1;   // no default in setDefault
    alt.neigh.neigh_hyp = params.parameter<int>("acc_neigh_hyp", "5");
    alt.neigh.neigh_hyp_radius = (float)params.parameter<int>("acc_neigh_hyp_radius", "100");   // parameter<int> into a float (:631)
    alt.neigh.neigh_skip1 = params.parameter<int>("acc_neigh_skip1", "2");
    alt.neigh.neigh_skip2 = params.parameter<int>("acc_neigh_skip2", "4");
    alt.neigh.hyp_neigh_tryouts = params.parameter<int>("acc_hyp_neigh_tryouts", "20");
    alt.neigh.seed = (unsigned)params.parameter<int>("seed", "0");
}

// the track job of the run: B start_jets x all rates.  acc_gpu_batch given: that B or status 1; absent: the largest B <= 16 and <= todo whose job takes at most
// half of the device memory that is free now.  fill: null, or the parameters of a job that fills in -- its bytes count the fill planes, and the half
// that stays free is what the interpolation takes its workspace from at run time
static sfa_track_job *create_job(ParameterList &params, sfa_ctx *ctx, sfa_track_params tp, const sfa_track_fill_params *fill, const sfa_track_alt_params *alt,
                                 size_t todo, int &B) {
    sfa_track_job *job = nullptr;
    size_t bytes = 0;
    auto job_bytes = [&](size_t *b) {
        return alt ? sfa_track_job_bytes_alternate(&tp, fill, alt, b) : fill ? sfa_track_job_bytes_fill(&tp, fill, b) : sfa_track_job_bytes(&tp, b);
    };
    auto job_create = [&]() {
        return alt ? sfa_track_job_create_alternate(ctx, &tp, fill, alt, &job) : fill ? sfa_track_job_create_fill(ctx, &tp, fill, &job) : sfa_track_job_create(ctx, &tp, &job);
    };
    if (params.exists("acc_gpu_batch")) {
        tp.n = B = params.parameter<int>("acc_gpu_batch");
        const bool sized = job_bytes(&bytes) == SFA_OK;
        if (!sized || job_create() != SFA_OK) {
            std::cerr << "acc_gpu_batch " << B << ": the track job cannot be created";
            if (sized) std::cerr << " (" << bytes << " bytes of device memory needed)";
            std::cerr << ": " << sfa_last_error(sized ? ctx : nullptr) << std::endl;
            return nullptr;
        }
    } else {
        size_t free_bytes = 0;
        if (!sfa_ok(ctx, sfa_ctx_free_bytes(ctx, &free_bytes))) return nullptr;
        for (B = (int)std::min<size_t>(16, todo); B >= 1; B--) {
            tp.n = B;
            if (job_bytes(&bytes) != SFA_OK) { std::cerr << sfa_last_error(nullptr) << std::endl; return nullptr; }
            if (bytes <= free_bytes / 2 || B == 1) break;
        }
        if (!sfa_ok(ctx, job_create())) return nullptr;
    }
    std::cout << "gpu batch: " << B << " start_jet(s) per run (" << bytes << " bytes of device memory" << (params.exists("acc_gpu_batch") ? ", acc_gpu_batch" : ", chosen")
              << ")" << std::endl;
    return job;
}

// the edge map of a start_jet (:945)
static string edges_file(const Run &run, unsigned seq_start) { return run.acc_dir + "tmp/edges_" + std::to_string(seq_start) + ".dat"; }

// -energies / -fuse: the start_jets in groups of B through one resident track job (sfa_track_job): per start_jet the frames are ingested and normalised and
// every rate's jets read and uploaded; one run accumulates (all steps), scores (:1219-1257) and, with -fuse, fuses the whole group on the GPU; then the
// outputs of each start_jet are written in cfg order.  -fill: the job fills in (sfa_track_job_create_fill); each start_jet also uploads the Lab image of its
// 8-bit frame 0 and its edge map, the fusion runs over 2 x rates slots, and the fill-in's figures go into run.json
static int run_energies(ParameterList &params, const Run &run, vector<Segment> &segs, const vector<string> &skipped,
                        const std::map<unsigned, vector<string>> &frame_files, vector<sfa_jet_source> &geo) {
    sfa_track_params tp;
    sfa_track_params_default(&tp);
    read_energy_params(params, tp.energy);
    Fusion fz;
    read_fusion(params, run, fz);
    for (int k = 0; k < 3; k++) { tp.avg[k] = fz.nav[k]; tp.std_dev[k] = fz.nsd[k]; }
    tp.hbit = fz.hbit;
    tp.fuse = fz.fup;
    tp.K = (int)run.rates; tp.Jets = (int)run.Jets; tp.min_fps_idx = run.min_fps_idx; tp.do_fuse = run.fuse ? 1 : 0; tp.use_occlusions = run.use_occ ? 1 : 0;
    tp.epsilon = run.threshold; tp.skip = run.skip_pixel; tp.discard = run.discard ? 1 : 0;
    tp.coef = 5.0f;                                                       // :969-981
    sfa_ctx *ctx = nullptr;
    if (!segs.empty() && !sfa_ok(nullptr, sfa_ctx_create(0, &ctx))) return 1;
    sfa_track_fill_params fill;
    sfa_track_fill_params_default(&fill);                                  // epic_fill_params (:652-656), removeSmallSegments' 100 (:1265)
    fill.epic_skip = params.parameter<float>("acc_epic_skip", "2");        // :651
    sfa_track_alt_params alt;
    read_alternation(params, alt);
    const int epic_search = run.fill ? params.parameter<int>("acc_gpu_epic_search", "0") : 0;   // 0 or 1 (refusal()): the graph searches of the fill-in, compact
    if (ctx && epic_search && !sfa_ok(ctx, sfa_ctx_set_epic_search(ctx, SFA_EPIC_SEARCH_COMPACT))) { sfa_ctx_destroy(ctx); return 1; }
    struct RateFill { unsigned seq_start; int r; int st[3]; };              // kept_pixels, matches, filled
    vector<RateFill> fills;
    sfa_track_job *job = nullptr;
    double t_frames = 0, t_acc = 0, t_energy = 0, t_io = 0, t_fuse = 0, t_fill = 0;
    const double t0 = now_s();
    int width = 0, height = 0, status = 0, B = 0, gw = 0, gh = 0;
    vector<unsigned> starts;                                              // the start_jets to do, in order; each has a segment of every rate
    for (auto it = frame_files.begin(); it != frame_files.end(); ++it) starts.push_back(it->first);
    struct Group { int size; float ms[8]; float fill_ms[4]; };
    vector<Group> groups;
    for (size_t g0 = 0; g0 < starts.size() && status == 0; g0 += (size_t)B) {
        int ng = 0;
        // ---- the group's inputs, one start_jet after another: ingest, normalise, read, upload
        for (size_t q = g0; q < starts.size() && (B == 0 ? q == g0 : q < g0 + (size_t)B) && status == 0; q++, ng++) {
            const unsigned seq_start = starts[q];
            vector<size_t> mine;                                          // this start_jet's segments, in rate order
            for (size_t i = 0; i < segs.size(); i++)
                if (segs[i].seq_start == seq_start) mine.push_back(i);
            // the frames set the target size (sequence[0].cols, :1142)
            double ta = now_s();
            vector<color_image_t *> fr;
            for (const string &name : frame_files.at(seq_start)) {
                color_image_t *img = ingest_frame(params, run, ctx, name);
                if (!img) { status = 1; break; }
                fr.push_back(img);
                if (fr.size() == 1 && width == 0) { width = img->width; height = img->height; }
                if (img->width != width || img->height != height) {
                    std::cerr << name << " is " << img->width << " x " << img->height << ", not " << width << " x " << height << " like the first frame" << std::endl;
                    status = 1;
                    break;
                }
            }
            if (status == 0 && !fit_rates(geo, width, height)) status = 1;
            if (status == 0 && mine.size() != run.rates) { std::cerr << "start " << seq_start << ": " << mine.size() << " of " << run.rates << " rates to do" << std::endl; status = 1; }
            const int stride = fr.empty() ? 0 : fr[0]->stride;
            vector<float *> fp;
            for (color_image_t *c : fr) fp.push_back(c->c1);
            // :931-955: frame 0 as read, before the normalisation: its 8-bit, blurred and resized copy and the Lab image of that are formed on the GPU
            struct Raw { color_image_t *im; ~Raw() { if (im) color_image_delete(im); } } raw{status == 0 && run.fill ? color_image_cpy(fr[0]) : nullptr};
            double avg[3], sd[3];
            if (status == 0 && !sfa_ok(ctx, sfa_normalize(ctx, fp.data(), (int)fp.size(), width, height, stride, avg, sd))) status = 1;   // normalize(data, Jets + 1) (:916)
            if (status == 0 && !sfa_ok(nullptr, sfa_accumulate_grid(width, height, run.skip_pixel, &gw, &gh))) status = 1;
            if (status == 0 && run.fill && sfa_reference_grid(width, height, run.skip_pixel, &gw, &gh) != SFA_OK) {
                std::cerr << "-fill: acc_skip_pixel " << run.skip_pixel << " on " << width << " x " << height << " frames is not supported: " << sfa_last_error(nullptr) << std::endl;
                status = 1;
            }
            if (status == 0 && run.fuse && width % 4 != 0) {
                // the reference indexes its stride-pitched weight image as (y * xy_incr + xy_start) * owidth + ... (:1722, 1733, 1737): exact only where
                // stride == width
                std::cerr << "-fuse: width " << width << " is not a multiple of 4 (the reference's smoothness-weight index reads padding)" << std::endl;
                status = 1;
            }
            epic_edges edges;
            if (status == 0 && run.fill && !read_edges(edges_file(run, seq_start).c_str(), gw, gh, edges)) {
                std::cerr << edges_file(run, seq_start) << " does not hold " << gw << " x " << gh << " floats" << std::endl;
                status = 2;
            }
            t_frames += now_s() - ta;
            // every rate of the start_jet is read before anything is uploaded: read_segment fills the rates' row strides, which the job's sources carry
            vector<SegmentInput> in(mine.size());
            double tb = now_s();
            for (size_t k = 0; k < mine.size() && status == 0; k++) {
                const Segment &s = segs[mine[k]];
                if (!read_segment(s, run.use_occ, geo[s.r], in[k]) || in[k].fu.empty()) status = 1;
            }
            t_io += now_s() - tb;
            if (status == 0 && !job) {
                tp.w = width; tp.h = height;
                for (unsigned r = 0; r < run.rates; r++) {
                    tp.source[r] = geo[r];
                    tp.weight[r] = run.jet_weight.size() > r ? (float)run.jet_weight[r] : (float)r;   // weight_jet_estimation, vector<float> (:489-495)
                }
                for (size_t m = 0; m < mine.size(); m++) tp.r_Jets[segs[mine[m]].r] = segs[mine[m]].FF;
                job = create_job(params, ctx, tp, run.fill ? &fill : nullptr, run.alternate ? &alt : nullptr, starts.size(), B);
                if (!job) status = 1;
            }
            for (size_t k = 0; k < mine.size() && status == 0; k++)
                if (!sfa_ok(ctx, sfa_track_job_upload_flows(job, ng, segs[mine[k]].r, in[k].fu.data(), in[k].fv.data(), in[k].bu.data(), in[k].bv.data(),
                                                            run.use_occ ? in[k].mp.data() : nullptr)))
                    status = 1;
            vector<const float *> cfp(fp.begin(), fp.end());
            if (status == 0 && !sfa_ok(ctx, sfa_track_job_upload_frames(job, ng, cfp.data(), stride))) status = 1;
            if (status == 0 && run.fill &&
                !sfa_ok(ctx, sfa_track_job_upload_fill_reference(job, ng, raw.im->c1, raw.im->stride, fz.hbit ? 1.0f / 255 : 1.0f, edges.cost.data())))
                status = 1;
            for (color_image_t *c : fr) color_image_delete(c);
        }
        if (status) break;
        // ---- one run for the group
        Group grp{ng, {}, {}};
        if (run.alternate) {                                              // the second key word of each start_jet's draws
            vector<unsigned> seq((size_t)B, 0u);
            for (int k = 0; k < ng; k++) seq[k] = starts[g0 + k];
            if (!sfa_ok(ctx, sfa_track_job_set_sequence_starts(job, seq.data()))) { status = 1; break; }
        }
        if (!sfa_ok(ctx, sfa_track_job_run(job, ng)) || !sfa_ok(ctx, sfa_track_job_stage_ms(job, grp.ms))) { status = 1; break; }
        if (run.fill && !sfa_ok(ctx, sfa_track_job_fill_ms(job, grp.fill_ms))) { status = 1; break; }
        groups.push_back(grp);
        for (float v : grp.fill_ms) t_fill += 1e-3 * v;
        t_acc += 1e-3 * grp.ms[1];
        t_energy += 1e-3 * (grp.ms[0] + grp.ms[2]);
        t_fuse += 1e-3 * (grp.ms[3] + grp.ms[4] + grp.ms[5] + grp.ms[6] + grp.ms[7]);
        // ---- the group's outputs, start_jet by start_jet in the order of the staged program
        const size_t gpl = (size_t)gw * gh;
        for (int k = 0; k < ng && status == 0; k++) {
            const unsigned seq_start = starts[g0 + k];
            double td = now_s();
            for (size_t i = 0; i < segs.size() && status == 0; i++) {
                Segment &s = segs[i];
                if (s.seq_start != seq_start) continue;
                vector<double> au(gpl), av(gpl), energy(gpl);
                vector<int> tracked(gpl);
                vector<unsigned char> oc(gpl);
                if (!sfa_ok(ctx, sfa_track_job_download_rate(job, k, s.r, au.data(), av.data(), tracked.data(), energy.data(), nullptr, oc.data()))) { status = 1; break; }
                vector<float> ef(gpl);
                for (size_t p = 0; p < gpl; p++) ef[p] = (float)energy[p];   // an fp32 sum stored in a double: exact
                const string dir = run.acc_dir + std::to_string(s.r) + "/";
                if (!write_last_step(s, au.data(), av.data(), tracked.data(), gw, gh) ||
                    !write_pfm(dir + "energy_" + std::to_string(seq_start) + ".pfm", gw, gh, ef.data()) ||
                    !write_pgm8(dir + "occluded_" + std::to_string(seq_start) + ".pgm", gw, gh, oc.data(), gw)) {
                    std::cerr << "cannot write the outputs of rate " << s.r << " under " << dir << std::endl;
                    status = 1;
                }
                if (status || !run.fill) continue;
                RateFill rf{seq_start, s.r, {0, 0, 0}};
                if (!sfa_ok(ctx, sfa_track_job_download_fill(job, k, s.r, nullptr, nullptr, nullptr, nullptr, rf.st))) { status = 1; break; }
                fills.push_back(rf);
                std::cout << "rate " << s.r << ", start " << seq_start << ": fill-in from " << rf.st[0] << " consistent pixels, " << rf.st[1] << " matches per step"
                          << (rf.st[2] ? "" : ": no fill-in hypothesis") << std::endl;
            }
            if (status == 0 && run.fuse) {
                Fusion::Record fu{};
                fu.seq_start = seq_start; fu.group = (int)groups.size() - 1; fu.group_size = ng;
                fu.t_weight = 1e-3 * grp.ms[3];
                fu.t_fuse = 1e-3 * (grp.ms[4] + grp.ms[5] + grp.ms[6] + grp.ms[7]);
                for (int m = 0; m < 4; m++) fu.stage_ms[m] = grp.ms[4 + m];
                if (!write_fused(ctx, job, k, run, fz, fu, gw, gh, alt.rounds)) status = 1;
            }
            vector<unsigned char> best(gpl);                              // the rate of the lowest fp32 energy, ties to the lower rate, formed on the GPU
            if (status == 0 && !sfa_ok(ctx, sfa_track_job_download_best(job, k, best.data()))) status = 1;
            if (status == 0 && !write_pgm8(run.acc_dir + "best_" + std::to_string(seq_start) + ".pgm", gw, gh, best.data(), gw)) {
                std::cerr << "cannot write " << run.acc_dir << "best_" << seq_start << ".pgm" << std::endl;
                status = 1;
            }
            t_io += now_s() - td;
        }
    }
    if (job) sfa_track_job_destroy(job);
    if (ctx) sfa_ctx_destroy(ctx);
    if (status) return status;
    std::ostringstream tail;
    tail.precision(17);
    tail << ",\n  \"gpu_batch\": " << B << ", \"groups\": [";
    for (size_t i = 0; i < groups.size(); i++) {
        tail << (i ? ", " : "") << "{\"group\": " << i << ", \"group_size\": " << groups[i].size << ", \"stage_ms\": [";
        for (int m = 0; m < 8; m++) tail << (m ? ", " : "") << groups[i].ms[m];
        tail << "]";
        if (run.fill) {                                                   // regions and matches, edge costs, the interpolation chain, trajectories
            tail << ", \"fill_ms\": [";
            for (int m = 0; m < 4; m++) tail << (m ? ", " : "") << groups[i].fill_ms[m];
            tail << "]";
        }
        tail << "}";
    }
    tail << "]";
    if (run.fuse) {
        const sfa_fuse_params &fup = fz.fup;
        tail << ",\n  \"fused\": true, ";
        if (run.fill)
            tail << "\"epic_fill\": true, \"fill_path\": \"track_job\", \"epic_interpolation\": true, \"neighbour_proposals\": " << (run.alternate ? "true" : "false")
                 << ", \"acc_epic_skip\": " << (double)fill.epic_skip << ", \"acc_gpu_epic_search\": " << epic_search;
        else
            tail << "\"epic_interpolation\": false, \"neighbour_proposals\": false";
        if (run.alternate)
            tail << ", \"acc_alternate\": " << alt.rounds << ", \"acc_perturb_keep\": " << alt.neigh.perturb_keep << ", \"acc_neigh_hyp\": " << alt.neigh.neigh_hyp
                 << ", \"acc_neigh_hyp_radius\": " << (double)alt.neigh.neigh_hyp_radius << ", \"acc_neigh_skip1\": " << alt.neigh.neigh_skip1
                 << ", \"acc_neigh_skip2\": " << alt.neigh.neigh_skip2 << ", \"acc_hyp_neigh_tryouts\": " << alt.neigh.hyp_neigh_tryouts << ", \"seed\": "
                 << alt.neigh.seed;
        tail << ", \"acc_beta\": " << fup.acc_beta << ", \"acc_spatial_occ\": "
             << fup.acc_spatial_occ << ", \"acc_traj_sim_method\": " << fup.traj_sim_method << ", \"acc_traj_sim_thres\": " << fup.traj_sim_thres
             << ", \"acc_trws_eps\": " << fup.trws_eps << ", \"acc_trws_max_iter\": " << fup.trws_max_iter;
        if (run.fill) {
            int taps[16], ntaps = 0;
            sfa_reference_taps(run.skip_pixel, taps, &ntaps);             // (refusal() passed: the skip is served)
            tail << ",\n  \"reference_image\": {\"skip\": " << run.skip_pixel << ", \"taps\": [";
            for (int i = 0; i < ntaps; i++) tail << (i ? ", " : "") << taps[i];
            tail << "], \"size\": [" << gw << ", " << gh << "]}";
            tail << ",\n  \"slots\": [";
            for (unsigned k = 0; k < 2 * run.rates; k++)
                tail << (k ? ", " : "") << "{\"slot\": " << k << ", \"rate\": " << k / 2 << ", \"kind\": \"" << (k % 2 ? "epic_fill" : "accumulated") << "\"}";
            tail << "],\n  \"fill\": [";
            for (size_t i = 0; i < fills.size(); i++)
                tail << (i ? ",\n    " : "\n    ") << "{\"sequence_start\": " << fills[i].seq_start << ", \"rate\": " << fills[i].r << ", \"kept_pixels\": " << fills[i].st[0]
                     << ", \"matches\": " << fills[i].st[1] << ", \"filled\": " << (fills[i].st[2] ? "true" : "false") << "}";
            tail << "]";
        }
        tail << ",\n  \"fusion\": [";
        for (size_t i = 0; i < fz.done.size(); i++) {
            const Fusion::Record &f = fz.done[i];
            tail << (i ? ",\n    " : "\n    ") << "{\"sequence_start\": " << f.seq_start << ", \"nodes\": " << f.nodes << ", \"energy\": " << f.energy
                 << ", \"lower_bound\": " << f.bound << ", \"iterations\": " << f.iters << ", \"group\": " << f.group << ", \"group_size\": " << f.group_size
                 << ", \"weight_s\": " << f.t_weight << ", \"fuse_call_s\": " << f.t_fuse
                 << ", \"kernels_ms\": {\"labels\": " << f.stage_ms[0] << ", \"pairwise\": " << f.stage_ms[1] << ", \"trws\": " << f.stage_ms[2]
                 << ", \"output\": " << f.stage_ms[3] << "}";
            if (run.alternate) {                                          // per round: the fusion's figures and the proposals accepted before it
                tail << ", \"rounds\": [";
                for (size_t r = 0; r < f.rounds.size(); r++)
                    tail << (r ? ", " : "") << "{\"round\": " << r << ", \"energy\": " << f.rounds[r].energy << ", \"lower_bound\": " << f.rounds[r].bound
                         << ", \"iterations\": " << f.rounds[r].iters << ", \"nodes\": " << f.rounds[r].nodes << ", \"accepted_proposals\": " << f.rounds[r].accepted << "}";
                tail << "]";
            }
            tail << "}";
        }
        tail << "]";
    }
    tail << ",\n  \"timings_s\": {\"frames\": " << t_frames << ", \"accumulate\": " << t_acc;
    if (run.fill) tail << ", \"epic_fill\": " << t_fill;
    tail << ", \"energy_call\": " << t_energy << ", \"write\": " << t_io;
    if (run.fuse) tail << ", \"fuse\": " << t_fuse;
    tail << ", \"total\": " << now_s() - t0 << "}";
    const bool ok = write_run_json(run, segs, skipped, geo, width, height, tail.str());
    if (run.alternate) std::cout << "wrote the flows of " << alt.rounds << " round(s) of proposals and fusion of " << fz.done.size() << " start_jet(s) to " << run.acc_dir << std::endl;
    else if (run.fill) std::cout << "wrote the fused flows with fill-in of " << fz.done.size() << " start_jet(s) to " << run.acc_dir << std::endl;
    else std::cout << "wrote the energies of " << segs.size() << " segment(s) to " << run.acc_dir << std::endl;
    return ok ? 0 : 1;
}

// the cfg as dense_tracking reads it (:479-571, :716-746); a non-zero exit status, with a message, where it cannot be used
static int read_run(ParameterList &params, Run &run) {
    run.jets = repeated(run.cfg, "jet_estimation");
    for (const string &v : repeated(run.cfg, "jet_S")) run.jet_S.push_back(atoi(v.c_str()));
    for (const string &v : repeated(run.cfg, "jet_fps")) run.jet_fps.push_back(atoi(v.c_str()));
    for (const string &v : repeated(run.cfg, "jet_weight")) run.jet_weight.push_back(atof(v.c_str()));
    for (string &j : run.jets)
        if (j.back() != '/') j += "/";                                   // :479-480
    run.rates = (unsigned)run.jets.size();
    if (run.rates == 0) { std::cerr << "No Jet estimation specified!" << std::endl; return 1; }
    run.sintel = params.parameter<bool>("sintel", "0");
    run.skip_pixel = params.parameter<int>("acc_skip_pixel", "1");       // setDefault: "1" (:122)
    run.start_jets = (unsigned)params.parameter<int>("ref_fps_F", "1");
    run.min_fps_idx = params.parameter<int>("acc_min_fps", "0");
    run.max_fps = params.parameter<int>("max_fps", "0");
    run.threshold = params.parameter<double>("acc_consistency_threshold", "1.0");
    run.discard = params.parameter<bool>("acc_discard_inconsistent", "1");
    // the reference gates the jets' occlusion masks on acc_use_jet_occlusions (:628, :1158); its sample cfg sets only acc_occlusion, read where the first is absent
    run.use_occ = params.exists("acc_use_jet_occlusions") ? params.parameter<bool>("acc_use_jet_occlusions") : params.parameter<bool>("acc_occlusion", "0");
    const int mfi = run.min_fps_idx;
    if (mfi < 0 || mfi >= (int)run.rates) { std::cerr << "acc_min_fps " << mfi << " names no jet estimation" << std::endl; return 1; }
    // slow_flow_S and jet_fps from each jet folder's config.cfg where the cfg does not give one per rate (:502-556)
    for (int pass = 0; pass < 2; pass++) {
        vector<int> &dst = pass ? run.jet_fps : run.jet_S;
        const char *key = pass ? "jet_fps" : "slow_flow_S";
        if (dst.size() == run.rates) continue;
        dst.assign(run.rates, 0);
        for (unsigned r = 0; r < run.rates; r++) {
            const string jc = run.jets[r] + "config.cfg";
            if (!file_exists(jc)) { std::cerr << "Error reading " << jc << " (does not exist)" << std::endl; return 2; }
            ParameterList tmp(jc);
            if (!tmp.exists(key)) { std::cerr << "Error reading " << key << " from " << jc << std::endl; return 1; }
            dst[r] = tmp.parameter<int>(key);
        }
    }
    run.steps = run.jet_S[mfi] - 1;                                      // :527
    if (!params.exists("ref_fps")) { std::cerr << "ref_fps missing from " << run.cfg << std::endl; return 1; }
    const int ref_fps = params.parameter<int>("ref_fps");
    if (run.steps < 1 || ref_fps < 1 || run.jet_fps[mfi] < 1) { std::cerr << "slow_flow_S, ref_fps and jet_fps must be positive" << std::endl; return 1; }
    run.Jets = (unsigned)(run.jet_fps[mfi] / (1.0f * ref_fps * run.steps));   // :564, float -> u_int32_t
    run.skip = (int)((1.0f * run.max_fps) / run.jet_fps[mfi]);          // :571
    if (run.Jets < 1) { std::cerr << "Jets = jet_fps / (ref_fps * steps) is 0" << std::endl; return 1; }
    run.sequence_start = params.sequence_start;
    if (run.sintel && !params.parameter<bool>("subframes", "0")) run.sequence_start *= 1000;   // :716-717
    run.flow_format = params.parameter<string>("flow_format", "frame_%i");
    run.flow_format = run.flow_format.substr(0, run.flow_format.find_last_of('.'));   // :745-746
    run.crop_flows = params.center.x > 0;                                // :1135
    run.crop_frames = params.extent.x > 0 || params.extent.y > 0;        // :876
    run.cx = params.center.x; run.cy = params.center.y; run.ex = params.extent.x; run.ey = params.extent.y;
    return 0;
}

// what -energies and -fuse do not support; 1 with a message
static int refusal(ParameterList &params, const Run &run) {
    if (run.use_occ && run.crop_flows) {
        // crop() reads its argument through at<Vec2d> (utils.cpp:314): on the 8-bit occlusion Mat that is undefined in the reference
        std::cerr << "the jets' occlusions (acc_use_jet_occlusions / acc_occlusion) together with center are not supported: the reference's crop() reads "
                     "the 8-bit image as pairs of doubles" << std::endl;
        return 1;
    }
    if (run.energies) {
        // acc_occlusion 1 makes addBCGC read occlusion_masks[Jets], one past the Mat[Jets] array (:784, :289): undefined in the reference
        const char *refused = params.parameter<bool>("acc_occlusion", "0") ? "acc_occlusion 1 (addBCGC reads occlusion_masks[Jets], past the array)"
                              : params.parameter<bool>("grayscale", "0") ? "grayscale 1"
                              : (params.exists("raw") && params.parameter<bool>("raw") && params.parameter<int>("raw_demosaicing", "0") == 1)
                                  ? "raw_demosaicing 1 (Hamilton-Adams, third-party, not here)"
                              : run.Jets > 32 ? "Jets > 32" : nullptr;
        if (refused) { std::cerr << "-energies: " << refused << " is not supported" << std::endl; return 1; }
        if (params.file.empty()) { std::cerr << "-energies: `file` (the frames) missing from " << run.cfg << std::endl; return 1; }
        if (params.exists("acc_gpu_batch")) {                             // the start_jets of one run of the track job; never clamped
            const int b = params.parameter<int>("acc_gpu_batch");
            if (b < 1 || b > 64) { std::cerr << "acc_gpu_batch " << b << " is outside 1 .. 64" << std::endl; return 1; }
        }
    }
    if (run.fuse) {
        const int method = params.parameter<int>("acc_traj_sim_method", "1");
        const char *refused = params.parameter<int>("acc_approach", "0") == 1 ? "acc_approach 1 (BP)"
                              : method == 2 ? "acc_traj_sim_method 2 (FINAL reads flow_y[Jets], past the adapted array)"
                              : (method != 0 && method != 1) ? "an acc_traj_sim_method other than 0 or 1"
                              : run.rates > 16 ? "more than 16 rates" : nullptr;
        if (refused) { std::cerr << "-fuse: " << refused << " is not supported" << std::endl; return 1; }
        if (run.fill) {
            // the reference blurs and resizes its 8-bit image with OpenCV for acc_skip_pixel > 0 (:932-936): restated for 1 and 3 (INTEGRATION.md 4c')
            // The restatement is parity-unpinned against OpenCV, so it is the cfg's choice: acc_gpu_reference_image 1.  Without the key -fill serves what it
            // served before the restatement existed, acc_skip_pixel 0, and refuses the rest as it did
            const bool restated = params.parameter<bool>("acc_gpu_reference_image", "0");
            if (run.skip_pixel != 0 && !restated) {
                std::cerr << "-fill: acc_skip_pixel other than 0 (the reference's resized reference image is OpenCV's; acc_gpu_reference_image 1 takes its restatement, "
                             "INTEGRATION.md 4c', for acc_skip_pixel 1 and 3) is not supported" << std::endl;
                return 1;
            }
            int ntaps = 0;
            if (sfa_reference_taps(run.skip_pixel, nullptr, &ntaps) != SFA_OK) {
                std::cerr << "-fill: acc_skip_pixel other than 0, 1 and 3 (the reference's resized reference image is not restated: " << sfa_last_error(nullptr)
                          << ") is not supported" << std::endl;
                return 1;
            }
            refused = run.rates > 8 ? "more than 8 rates (jet_estimation lines; two of the 16 slots each)"   // 16 slots = 8 rates x 2
                      : !params.parameter<bool>("acc_epic_interpolation", "1") ? "acc_epic_interpolation 0" : nullptr;
            if (refused) { std::cerr << "-fill: " << refused << " is not supported" << std::endl; return 1; }
            const int search = params.parameter<int>("acc_gpu_epic_search", "0");
            if (search != 0 && search != 1) { std::cerr << "-fill: acc_gpu_epic_search " << search << " is neither 0 (the default search) nor 1 (the compact search)" << std::endl; return 1; }
            if (run.alternate) {                                          // the library's limits, named here before anything is read or written
                sfa_track_alt_params alt;
                read_alternation(params, alt);
                const int slots = 2 * (int)run.rates, hyp = alt.neigh.neigh_hyp, keep = alt.neigh.perturb_keep;
                std::ostringstream why;
                if (alt.rounds < 1) why << "acc_alternate " << alt.rounds << " < 1";
                else if (alt.rounds > 1 && !params.exists("acc_perturb_keep")) why << "acc_perturb_keep is not set (it has no default; acc_alternate > 1 needs it)";
                else if (alt.rounds > 1 && keep < 0) why << "acc_perturb_keep " << keep << " < 0";
                else if (hyp < 0) why << "acc_neigh_hyp " << hyp << " < 0";
                else if (slots + 2 * hyp > 16) why << "slots + 2 * acc_neigh_hyp = " << slots << " + 2 * " << hyp << " > 16";
                else if (alt.rounds > 1 && keep + 1 + 2 * hyp > 16) why << "acc_perturb_keep + 1 + 2 * acc_neigh_hyp = " << keep << " + 1 + 2 * " << hyp << " > 16";
                else if (alt.neigh.neigh_skip1 < 1) why << "acc_neigh_skip1 " << alt.neigh.neigh_skip1 << " < 1";
                else if (alt.neigh.neigh_skip2 < 1) why << "acc_neigh_skip2 " << alt.neigh.neigh_skip2 << " < 1";
                else if (alt.neigh.hyp_neigh_tryouts < 0) why << "acc_hyp_neigh_tryouts " << alt.neigh.hyp_neigh_tryouts << " < 0";
                else if (!(alt.neigh.neigh_hyp_radius > 0)) why << "acc_neigh_hyp_radius " << alt.neigh.neigh_hyp_radius << " <= 0 (the knnSearch(acc_neigh_draws) branch)";
                if (!why.str().empty()) { std::cerr << "-alternate: " << why.str() << " is not supported" << std::endl; return 1; }
            }
        } else if (params.parameter<bool>("acc_epic_interpolation", "1"))
            std::cout << "-fuse: acc_epic_interpolation 1, but EpicFlow's fill-in and the neighbour proposals are not run (pixels without a hypothesis "
                         "stay UNKNOWN_FLOW)" << std::endl;
    }
    return 0;
}

// the output folder: never an existing one without -resume (:582-594)
static int choose_output(const ParameterList &params, bool resume, Run &run) {
    string output = params.output;
    if (output.empty()) { std::cerr << "output missing from " << run.cfg << std::endl; return 1; }
    if (!resume) {
        if (output.back() == '/') output.pop_back();
        string np = output;
        for (int num = 1; file_exists(np); num++) { std::cerr << np << " already exists!" << std::endl; np = output + "_" + std::to_string(num); }
        output = np;
    }
    if (output.back() != '/') output += "/";
    run.acc_dir = output + "accumulated/";
    return 0;
}

// every start_jet x rate whose output is not there yet (:722-735, :1100-1119); the outputs that are, in `skipped`
static int build_segments(const Run &run, unsigned selected, unsigned selected_end, vector<Segment> &segs, vector<string> &skipped) {
    for (unsigned start_jet = selected; start_jet < selected_end; start_jet++) {
        const unsigned seq_start = run.sequence_start + start_jet * run.Jets * run.steps * run.skip;   // :735
        if (run.fuse) {                                                  // the fused flow is the start_jet's product
            const string flo = fused_base(run, seq_start) + ".flo";
            if (file_exists(flo)) { std::cout << "Flow file " << flo << " already exists!" << std::endl; skipped.push_back(flo); continue; }
        } else if (run.energies) {                                       // with the energies a start_jet is done as a whole: all its rates are compared
            const string best = run.acc_dir + "best_" + std::to_string(seq_start) + ".pgm";
            if (file_exists(best)) { std::cout << "Energy file " << best << " already exists!" << std::endl; skipped.push_back(best); continue; }
        }
        for (unsigned r = 0; r < run.rates; r++) {
            Segment s;
            s.r = (int)r; s.start_jet = start_jet; s.seq_start = seq_start;
            const int r_steps = run.jet_S[r] - 1;                                                // :1101
            const float ratio = (1.0f * run.jet_fps[r]) / run.jet_fps[run.min_fps_idx];          // :1103
            s.FF = (int)(unsigned)(ratio * run.Jets);                                            // :1104
            const int r_skip = (int)((1.0f * run.max_fps) / run.jet_fps[r]);                     // :1105
            const string dir = run.acc_dir + std::to_string(r) + "/";
            s.out_flo = dir + (run.sintel ? fmt2("s" + run.flow_format, (int)seq_start, 0) : fmt1(run.flow_format, (int)seq_start)) + ".flo";
            s.out_tracked = dir + "tracked_" + std::to_string(seq_start) + ".pgm";
            if (!run.energies && file_exists(s.out_flo)) { std::cout << "Flow file " << s.out_flo << " already exists!" << std::endl; skipped.push_back(s.out_flo); continue; }
            if (s.FF < 1) { std::cerr << "rate " << r << ": r_Jets = " << s.FF << ", nothing to accumulate" << std::endl; return 1; }
            for (int f = 0; f < s.FF; f++) {
                const int a = (int)seq_start + f * r_steps * r_skip;
                s.fwd.push_back(run.jets[r] + fmt1(run.flow_format, a) + ".flo");                                     // :1118
                s.bwd.push_back(run.jets[r] + fmt1(run.flow_format, a + r_steps * r_skip) + "_back.flo");              // :1119
                if (run.use_occ) s.occ.push_back(run.jets[r] + "/occlusion/frame_" + std::to_string(a));               // :1161, extension below
            }
            segs.push_back(s);
        }
    }
    return 0;
}

// every input must exist before anything runs (the reference breaks out of its read loop and goes on with empty flows, :1121-1128); with
// -energies the frames of each start_jet (:793-810): sequence_start + f * steps * skip, f = 0 .. Jets.  2 with a message where one is missing
static int check_inputs(const ParameterList &params, const Run &run, vector<Segment> &segs, std::map<unsigned, vector<string>> &frame_files) {
    for (Segment &s : segs)
        for (int f = 0; f < s.FF; f++) {
            for (const string &file : {s.fwd[f], s.bwd[f]})
                if (!file_exists(file)) { std::cerr << file << " does not exist!" << std::endl; return 2; }
            if (run.use_occ) {
                if (file_exists(s.occ[f] + ".pgm")) s.occ[f] += ".pgm";      // what this project's driver writes
                else if (file_exists(s.occ[f] + ".pbm")) s.occ[f] += ".pbm"; // the reference's name
                else { std::cerr << s.occ[f] << ".pgm does not exist (nor " << s.occ[f] << ".pbm)!" << std::endl; return 2; }
            }
        }
    if (run.fill)
        for (const Segment &s : segs)
            if (!file_exists(edges_file(run, s.seq_start))) { std::cerr << edges_file(run, s.seq_start) << " does not exist!" << std::endl; return 2; }
    if (!run.energies) return 0;
    const size_t sf = params.file.find_last_of('/') + 1;                 // :740-751 (npos + 1 == 0: no folder)
    string sequence_path = params.file.substr(0, sf);
    if (!sequence_path.empty() && sequence_path.back() != '/') sequence_path += "/";
    const string format = sequence_path + params.file.substr(sf);
    for (const Segment &s : segs) {
        vector<string> &names = frame_files[s.seq_start];
        if (!names.empty()) continue;
        for (unsigned f = 0; f <= run.Jets; f++) {
            names.push_back(sequence_frame_name(format, (int)s.seq_start, (int)(f * run.steps * run.skip), run.sintel));
            if (!file_exists(names.back())) { std::cerr << names.back() << " does not exist!" << std::endl; return 2; }
        }
    }
    return 0;
}

// -reference: the reduced 8-bit image of frame 0 of every start_jet (:931-936) as <output>/accumulated/tmp/frame_epic_<sequence_start>.png (:944, 960), the
// file the reference hands to its edge detector.  sfa_reference_lab forms it on the GPU
static int run_reference(ParameterList &params, const Run &run, unsigned selected, unsigned selected_end) {
    int ntaps = 0;
    if (sfa_reference_taps(run.skip_pixel, nullptr, &ntaps) != SFA_OK) {
        std::cerr << "-reference: acc_skip_pixel other than 0, 1 and 3 is not supported: " << sfa_last_error(nullptr) << std::endl;
        return 1;
    }
    if (params.file.empty()) { std::cerr << "-reference: `file` (the frames) missing from " << run.cfg << std::endl; return 1; }
    const size_t sf = params.file.find_last_of('/') + 1;                 // :740-751, as check_inputs
    string sequence_path = params.file.substr(0, sf);
    if (!sequence_path.empty() && sequence_path.back() != '/') sequence_path += "/";
    const string format = sequence_path + params.file.substr(sf);
    vector<std::pair<unsigned, string>> todo;
    for (unsigned start_jet = selected; start_jet < selected_end; start_jet++) {
        const unsigned seq_start = run.sequence_start + start_jet * run.Jets * run.steps * run.skip;   // :735
        todo.emplace_back(seq_start, sequence_frame_name(format, (int)seq_start, 0, run.sintel));
        if (!file_exists(todo.back().second)) { std::cerr << todo.back().second << " does not exist!" << std::endl; return 2; }
    }
    sfa_ctx *ctx = nullptr;
    if (!sfa_ok(nullptr, sfa_ctx_create(0, &ctx))) return 1;
    mkdirs(run.acc_dir + "tmp/");
    const float norm = params.parameter<bool>("16bit", "0") ? 1.0f / 255 : 1.0f;
    int status = 0;
    for (size_t i = 0; i < todo.size() && status == 0; i++) {
        color_image_t *img = ingest_frame(params, run, ctx, todo[i].second);
        if (!img) { status = 1; break; }
        int gw = 0, gh = 0;
        if (sfa_reference_grid(img->width, img->height, run.skip_pixel, &gw, &gh) != SFA_OK) {
            std::cerr << "-reference: acc_skip_pixel " << run.skip_pixel << " on " << img->width << " x " << img->height << " frames is not supported: "
                      << sfa_last_error(nullptr) << std::endl;
            status = 1;
        }
        const size_t gpl = (size_t)gw * gh;
        vector<float> lab(3 * gpl);
        vector<unsigned char> rgb8(3 * gpl);
        if (status == 0 && !sfa_ok(ctx, sfa_reference_lab(ctx, img->width, img->height, run.skip_pixel, img->c1, img->stride, norm, lab.data(), gw, rgb8.data()))) status = 1;
        color_image_delete(img);
        if (status) break;
        png_image png;
        png.width = gw; png.height = gh; png.channels = 3; png.depth = 8;
        png.samples.resize(3 * gpl);
        for (size_t k = 0; k < gpl; k++)
            for (int c = 0; c < 3; c++) png.samples[3 * k + c] = rgb8[c * gpl + k];
        const string out = run.acc_dir + "tmp/frame_epic_" + std::to_string(todo[i].first) + ".png";
        if (!png_write(out.c_str(), png)) { std::cerr << "cannot write " << out << std::endl; status = 1; break; }
        std::cout << "start " << todo[i].first << ": wrote the " << gw << " x " << gh << " reference image " << out << std::endl;
    }
    sfa_ctx_destroy(ctx);
    return status;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "-decode_occlusion")) {
        if (argc != 4) { usage(); return 1; }
        int w, h;
        vector<unsigned char> g;
        if (!read_pnm8(argv[2], w, h, g)) { std::cerr << argv[2] << ": not a binary PGM (maxval 255) or PBM" << std::endl; return file_exists(argv[2]) ? 1 : 2; }
        vector<unsigned char> m((size_t)w * h);
        decode_occlusion(g, w, h, w, m.data());
        return write_pgm8(argv[3], w, h, m.data(), w) ? 0 : 1;
    }
    if (argc < 2) { usage(); return 1; }
    Run run;
    run.cfg = argv[1];
    if (!file_exists(run.cfg)) { usage(); return 1; }
    printf("using parameters %s\n", run.cfg.c_str());
    unsigned selected = 0, selected_end = 0;
    bool resume = false;
    for (int i = 2; i < argc; i++) {                                     // :449-476
        const char *a = argv[i];
        if (a[0] != '-') continue;
        if (!strcmp(a, "-h") || !strcmp(a, "-help")) usage();
        else if (!strcmp(a, "-resume")) resume = true;
        else if (!strcmp(a, "-energies")) run.energies = true;
        else if (!strcmp(a, "-fuse")) run.fuse = run.energies = true;
        else if (!strcmp(a, "-fill")) run.fill = run.fuse = run.energies = true;
        else if (!strcmp(a, "-alternate")) run.alternate = run.fill = run.fuse = run.energies = true;
        else if (!strcmp(a, "-reference")) run.reference = true;
        else if (!strcmp(a, "-select") && i + 1 < argc) { selected = (unsigned)atoi(argv[++i]); selected_end = selected + 1; }
        else { fprintf(stderr, "unknown argument %s\n", a); usage(); return 1; }
    }
    ParameterList params;
    params.read(run.cfg);
    if (int status = read_run(params, run)) return status;
    if (run.reference) {
        if (int status = choose_output(params, resume, run)) return status;
        return run_reference(params, run, selected, selected_end ? selected_end : run.start_jets);
    }
    if (int status = refusal(params, run)) return status;
    if (int status = choose_output(params, resume, run)) return status;
    vector<Segment> segs;
    vector<string> skipped;
    if (int status = build_segments(run, selected, selected_end ? selected_end : run.start_jets, segs, skipped)) return status;   // :722-723
    std::map<unsigned, vector<string>> frame_files;
    if (int status = check_inputs(params, run, segs, frame_files)) return status;
    vector<sfa_jet_source> geo;
    if (int status = read_geometry(run, segs, geo)) return status;
    if (!run.energies) {                                                 // rates of different sizes: the frame at sequence_start gives the target
        bool differ = false;
        for (const Segment &s : segs) differ = differ || geo[s.r].cw != geo[segs[0].r].cw || geo[s.r].ch != geo[segs[0].r].ch;
        if (differ) {
            if (params.file.empty()) { std::cerr << "the jets differ in size and `file` (the frames, whose size they are brought to) is missing from " << run.cfg << std::endl; return 1; }
            run.size_frame = sequence_frame_name(params.file, (int)run.sequence_start, 0, run.sintel);
            if (!file_exists(run.size_frame)) { std::cerr << run.size_frame << " does not exist!" << std::endl; return 2; }
        }
    }
    mkdirs(run.acc_dir);
    for (unsigned r = 0; r < run.rates; r++) mkdirs(run.acc_dir + std::to_string(r) + "/");
    return run.energies ? run_energies(params, run, segs, skipped, frame_files, geo) : run_accumulate(params, run, segs, skipped, geo);
}
