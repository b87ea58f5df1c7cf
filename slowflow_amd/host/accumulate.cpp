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
// With -fuse (implies -energies) it fuses every start_jet's rates as dense_tracking does (:1588-1905): the smoothness weight of normalised frame 0
// (sfa_dt_smoothness_weight), NMS, the pairwise MRF and TRW-S in raster order (sfa_fuse_hypotheses), and writes
//   <output>/accumulated/<flow_format % sequence_start>.flo       the fused flow on the grid, u(Jets - 1) / xy_incr; UNKNOWN_FLOW (1e10) without a node
//   <output>/accumulated/<...>_vis.png                            its colour coding
//   <output>/accumulated/occlusions/frame_<sequence_start>.pgm    max_t occluded(t) of the chosen hypothesis, 0 / 255
//   <output>/accumulated/labels_<sequence_start>.pgm              the chosen rate (255: none)
//
// Out of scope (FLANN, GSL, OpenCV are not in this tree): EpicFlow's fill-in and the neighbour proposals, removeSmallSegments, cropping and the
// rescaling of flows of another size (:1131-1146; such flows are refused).
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "flow_vis.h"
#include "image.h"
#include "ingest.h"
#include "io.h"
#include "parameter_list.h"
#include "../../include/slowflow_amd.h"

using std::string;
using std::vector;

static void usage() {
    printf("usage:\n");
    printf("    ./accumulate [cfg] -select [estimation for one specific final pair] -resume -energies -fuse\n");
    printf("    ./accumulate -decode_occlusion [occlusion .pgm / .pbm] [mask .pgm]   (the mask this program uses: median 3x3, 255 - x; 0 = occluded)\n");
    printf("\n");
    printf("Runs dense_tracking's first stage only: consistent accumulation of the jets (accumulateConsistentBatches).  cfg keys read: jet_estimation\n");
    printf("(repeated), jet_S, jet_fps, jet_weight, flow_format, start, ref_fps, ref_fps_F, max_fps, acc_min_fps, acc_skip_pixel, acc_use_jet_occlusions\n");
    printf("(or acc_occlusion), acc_discard_inconsistent, acc_consistency_threshold, output, sintel, subframes.  Not done: flows of a size other than\n");
    printf("the first flow's are refused (no rescaling), and the TRW-S fusion, EpicFlow fill-in and removeSmallSegments are left out.\n");
    printf("A missing input file exits with status 2.\n");
    printf("\n");
    printf("-energies: also reads the Jets + 1 frames of each start_jet (cfg `file`, the driver's ingest: scale, raw, raw_demosaicing 0 / 2), normalises\n");
    printf("them and writes each hypothesis' unary energy (energy_<start>.pfm), its occluded frames (occluded_<start>.pgm) and the lowest-energy rate\n");
    printf("(best_<start>.pgm).  Keys: acc_jet_consistency, acc_brightness_constancy, acc_gradient_constancy, acc_occlusion_penalty, acc_temporal_occ,\n");
    printf("acc_cv, acc_occlusion_threshold, acc_occlusion_fb_threshold, acc_penalty_fct_data, acc_penalty_fct_data_eps.  Refused: acc_occlusion 1,\n");
    printf("grayscale 1, raw_demosaicing 1, center / extent, Jets > 32.\n");
    printf("\n");
    printf("-fuse: implies -energies, then fuses all rates of each start_jet with TRW-S (raster order) into <flow_format %% start>.flo, _vis.png,\n");
    printf("occlusions/frame_<start>.pgm and labels_<start>.pgm.  Keys: acc_beta, acc_spatial_occ, acc_traj_sim_method, acc_traj_sim_thres, acc_trws_eps,\n");
    printf("acc_trws_max_iter, 16bit, img_norm_avg_*, img_norm_std_*.  Refused: acc_approach 1, acc_traj_sim_method 2, a width that is not a multiple\n");
    printf("of 4, more than 16 rates.  EpicFlow's fill-in and the neighbour proposals (acc_epic_interpolation) are not run.\n");
}

// little-endian PFM (Pf, scale -1), rows bottom to top: what io.cpp's reader expects
static bool write_pfm(const string &file, int w, int h, const float *px) {
    FILE *f = fopen(file.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "Pf\n%d %d\n-1.0\n", w, h);
    for (int y = h - 1; y >= 0; y--) fwrite(px + (size_t)y * w, sizeof(float), (size_t)w, f);
    return fclose(f) == 0;
}

static bool file_exists(const string &f) { return access(f.c_str(), F_OK) != -1; }
static void mkdirs(const string &path) {
    string cur;
    for (size_t i = 0; i <= path.size(); i++) {
        if ((i == path.size() || path[i] == '/') && !cur.empty()) mkdir(cur.c_str(), 0777);
        if (i < path.size()) cur.push_back(path[i]);
    }
}
static string fmt1(const string &format, int a) { char b[1024]; snprintf(b, sizeof b, format.c_str(), a); return b; }
static string fmt2(const string &format, int a, int c) { char b[1024]; snprintf(b, sizeof b, format.c_str(), a, c); return b; }
static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the keys the host ParameterList keeps one value of but the reference collects (utils/parameter_list.cpp:113-130): every line "key<TAB>value", in order
static vector<string> repeated(const string &cfg, const string &key) {
    vector<string> out;
    std::ifstream f(cfg.c_str(), std::ios::binary);
    string line;
    while (std::getline(f, line)) {
        while (!line.empty() && (line.back() == '\r' || line.back() == '\n')) line.pop_back();
        vector<string> tok;
        size_t pos = 0;
        while (pos <= line.size()) {                                     // tabs separate, consecutive tabs collapse (parameter_list.cpp split_tabs)
            size_t next = line.find('\t', pos);
            if (next == string::npos) next = line.size();
            if (next > pos) tok.push_back(line.substr(pos, next - pos));
            pos = next + 1;
        }
        if (tok.size() >= 2 && tok[0] == key && tok[1][0] != '#') out.push_back(tok[1]);
    }
    return out;
}

// binary PGM (P5, maxval 255) or PBM (P4: bit 1 = black = 0, bit 0 = white = 255, as OpenCV reads it); 8-bit grey values, w x h; false on failure
static bool read_pnm8(const string &file, int &w, int &h, vector<unsigned char> &px) {
    FILE *f = fopen(file.c_str(), "rb");
    if (!f) return false;
    auto token = [&](string &t) {
        t.clear();
        int c;
        for (;;) {
            c = fgetc(f);
            if (c == EOF) return false;
            if (c == '#') { while (c != '\n' && c != EOF) c = fgetc(f); continue; }
            if (!isspace(c)) break;
        }
        while (c != EOF && !isspace(c)) { t.push_back((char)c); c = fgetc(f); }
        return true;                                                     // the one whitespace after the token is consumed
    };
    string magic, sw, sh, smax;
    bool ok = token(magic) && (magic == "P5" || magic == "P4") && token(sw) && token(sh) && (magic == "P4" || token(smax));
    if (ok) { w = atoi(sw.c_str()); h = atoi(sh.c_str()); ok = w > 0 && h > 0 && w <= 65535 && h <= 65535 && (magic == "P4" || atoi(smax.c_str()) == 255); }
    if (ok) {
        px.assign((size_t)w * h, 0);
        if (magic == "P5") ok = fread(px.data(), 1, px.size(), f) == px.size();
        else {
            const size_t rb = (size_t)(w + 7) / 8;
            vector<unsigned char> row(rb);
            for (int y = 0; ok && y < h; y++) {
                ok = fread(row.data(), 1, rb, f) == rb;
                for (int x = 0; ok && x < w; x++) px[(size_t)y * w + x] = ((row[x >> 3] >> (7 - (x & 7))) & 1) ? 0 : 255;
            }
        }
    }
    fclose(f);
    return ok;
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

static bool write_pgm8(const string &file, int w, int h, const unsigned char *px, int stride) {
    FILE *f = fopen(file.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "P5\n%d %d\n255\n", w, h);
    for (int y = 0; y < h; y++) fwrite(px + (size_t)y * stride, 1, w, f);
    return fclose(f) == 0;
}

struct Segment {
    int r = 0;                   // rate (index of its jet_estimation line)
    unsigned start_jet = 0, seq_start = 0;
    int FF = 0;
    string out_flo, out_tracked;
    vector<string> fwd, bwd, occ;   // input files, FF each (occ: empty without occlusions)
    int created = 0, rejected = 0;
};

// read a segment's flows (and masks) into host images; false with a message on failure
struct SegmentInput {
    vector<image_t **> fl;                                                // forward, backward per step
    vector<const float *> fu, fv, bu, bv;
    vector<vector<unsigned char>> mbuf;
    vector<const unsigned char *> mp;
    ~SegmentInput() { for (image_t **c : fl) { image_delete(c[0]); image_delete(c[1]); free(c); } }
};
static bool read_segment(const Segment &s, bool use_occ, int &width, int &height, SegmentInput &in) {
    for (int f = 0; f < s.FF; f++) {
        image_t **a = readFlowFile(s.fwd[f].c_str()), **b = readFlowFile(s.bwd[f].c_str());
        if (a) in.fl.push_back(a);
        if (b) in.fl.push_back(b);
        if (!a || !b) { std::cerr << "cannot read " << (a ? s.bwd[f] : s.fwd[f]) << " as a .flo" << std::endl; return false; }
        if (width == 0) { width = a[0]->width; height = a[0]->height; }
        for (image_t **c : {a, b})
            if (c[0]->width != width || c[0]->height != height) {
                std::cerr << (c == a ? s.fwd[f] : s.bwd[f]) << " is " << c[0]->width << " x " << c[0]->height << ", not " << width << " x " << height
                          << ": rescaling is not implemented" << std::endl;
                return false;
            }
        in.fu.push_back(a[0]->data); in.fv.push_back(a[1]->data); in.bu.push_back(b[0]->data); in.bv.push_back(b[1]->data);
        if (use_occ) {
            int ow, oh;
            vector<unsigned char> g;
            if (!read_pnm8(s.occ[f], ow, oh, g)) { std::cerr << s.occ[f] << ": not a binary PGM (maxval 255) or PBM" << std::endl; return false; }
            if (ow != width || oh != height) { std::cerr << s.occ[f] << " is not " << width << " x " << height << std::endl; return false; }
            in.mbuf.emplace_back((size_t)a[0]->stride * height, 0);
            decode_occlusion(g, width, height, a[0]->stride, in.mbuf.back().data());
        }
    }
    for (auto &m : in.mbuf) in.mp.push_back(m.data());
    return true;
}

// one frame as dense_tracking ingests it (:793-905): decoded, demosaiced (raw_demosaicing 0 / 2) or taken as RGB, rescaled where scale != 1
static color_image_t *ingest_frame(ParameterList &params, sfa_ctx *ctx, const string &name) {
    int maxval = 255;
    color_image_t *img = color_image_load(name.c_str(), &maxval);
    if (!img) { std::cerr << "cannot read frame " << name << " (PNG, TIFF or binary PPM/PGM/PFM expected)" << std::endl; return nullptr; }
    if (params.exists("raw") && params.parameter<bool>("raw")) {
        vector<int> red_loc;
        std::stringstream ss(params.parameter<string>("raw_red_loc", "0,0"));
        for (string t; std::getline(ss, t, ',');) red_loc.push_back(atoi(t.c_str()));
        image_t mosaic = {img->width, img->height, img->stride, img->c1};
        color_image_t *rgb = color_image_new(img->width, img->height);
        color_image_erase(rgb);
        const int rx = red_loc.size() > 0 ? red_loc[0] : 0, ry = red_loc.size() > 1 ? red_loc[1] : 0;
        if (params.parameter<int>("raw_demosaicing", "0") == 2) bayer2rgb_cv8u(&mosaic, rgb, rx, ry);
        else bayer2rgbGR(&mosaic, rgb, rx, ry);
        color_image_delete(img);
        img = rgb;
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

// -energies: per start_jet the frames, then for every rate in cfg order the accumulation (all steps) and the hypotheses' energies (:1100-1257)
static int run_energies(ParameterList &params, const string &cfg, const string &acc_dir, vector<Segment> &segs, const vector<string> &skipped,
                        const std::map<unsigned, vector<string>> &frame_files, unsigned rates, int min_fps_idx, unsigned Jets, int steps, int skip,
                        int skip_pixel, double threshold, bool discard, bool use_occ, const vector<string> &jets, const vector<int> &jet_S,
                        const vector<int> &jet_fps, const vector<double> &jet_weight, bool fuse, const string &flow_format, bool sintel) {
    sfa_energy_params ep;
    sfa_energy_params_default(&ep);                                       // setDefault (:118-165), in the types of :606-623 and :661-675
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
    ep.skip = skip_pixel;
    sfa_fuse_params fup;
    sfa_fuse_params_default(&fup);                                         // setDefault (:136-152), read as at :605-625, :660-661
    fup.acc_beta = params.parameter<double>("acc_beta", "10.0");
    fup.acc_spatial_occ = params.parameter<double>("acc_spatial_occ", "10.0");   // setDefault's "acc_satial_occ" never reaches this key
    fup.traj_sim_method = params.parameter<int>("acc_traj_sim_method", "1");
    fup.traj_sim_thres = params.parameter<double>("acc_traj_sim_thres", "0.1");
    fup.trws_eps = params.parameter<double>("acc_trws_eps", "1e-5");
    fup.trws_max_iter = params.parameter<int>("acc_trws_max_iter", "10");
    fup.skip = skip_pixel;
    // the statistics the smoothness weight de-normalises with: the reference reads img_norm_* (defaults 0 / 1, :971-972), keys normalize() does not
    // publish (it writes slow_flow_img_norm_*), so by default the weight is taken from the normalised frame itself
    float nav[3], nsd[3];
    for (int k = 0; k < 3; k++) {
        nav[k] = (float)params.parameter<double>("img_norm_avg_" + std::to_string(k + 1), "0");
        nsd[k] = (float)params.parameter<double>("img_norm_std_" + std::to_string(k + 1), "1");
    }
    const int hbit = params.parameter<bool>("16bit", "0") ? 1 : 0;
    struct Fused { unsigned seq_start; int nodes, iters; double energy, bound, t_weight, t_fuse; float stage_ms[4]; };
    vector<Fused> fused;
    double t_fuse = 0;
    sfa_ctx *ctx = nullptr;
    if (!segs.empty() && sfa_ctx_create(0, &ctx) != SFA_OK) { std::cerr << sfa_last_error(nullptr) << std::endl; return 1; }
    double t_frames = 0, t_acc = 0, t_energy = 0, t_io = 0;
    const double t0 = now_s();
    int width = 0, height = 0, status = 0;
    vector<int> hyps(segs.size(), 0);
    for (auto it = frame_files.begin(); it != frame_files.end() && status == 0; ++it) {
        const unsigned seq_start = it->first;
        vector<size_t> mine;                                              // this start_jet's segments, in rate order
        for (size_t i = 0; i < segs.size(); i++)
            if (segs[i].seq_start == seq_start) mine.push_back(i);
        // rate acc_min_fps's flows: forward_flow / backward_flow of the reference (:1148-1151)
        double ta = now_s();
        SegmentInput minf;
        size_t mi = mine.size();
        for (size_t k = 0; k < mine.size(); k++)
            if (segs[mine[k]].r == min_fps_idx) mi = k;
        if (mi == mine.size() || !read_segment(segs[mine[mi]], false, width, height, minf)) { status = 1; break; }
        vector<color_image_t *> fr;
        for (const string &name : it->second) {
            color_image_t *img = ingest_frame(params, ctx, name);
            if (!img) { status = 1; break; }
            fr.push_back(img);
            if (img->width != width || img->height != height) {
                std::cerr << name << " is " << img->width << " x " << img->height << ", the flows " << width << " x " << height << std::endl;
                status = 1;
                break;
            }
        }
        const int stride = fr.empty() ? 0 : fr[0]->stride;
        vector<float *> fp;
        for (color_image_t *c : fr) fp.push_back(c->c1);
        double avg[3], sd[3];
        if (status == 0 && sfa_normalize(ctx, fp.data(), (int)fp.size(), width, height, stride, avg, sd) != SFA_OK) {   // normalize(data, Jets + 1) (:916)
            std::cerr << sfa_last_error(ctx) << std::endl;
            status = 1;
        }
        t_frames += now_s() - ta;
        int gw = 0, gh = 0;
        if (status == 0 && sfa_accumulate_grid(width, height, skip_pixel, &gw, &gh) != SFA_OK) { std::cerr << sfa_last_error(nullptr) << std::endl; status = 1; }
        const size_t gpl = (size_t)gw * gh;
        vector<float> best_e(gpl, INFINITY);
        vector<unsigned char> best(gpl, 255);
        vector<const float *> cfp(fp.begin(), fp.end());
        if (status == 0 && fuse && width % 4 != 0) {
            // the reference indexes its stride-pitched weight image as (y * xy_incr + xy_start) * owidth + ... (:1722, 1733, 1737): exact only where
            // stride == width
            std::cerr << "-fuse: width " << width << " is not a multiple of 4 (the reference's smoothness-weight index reads padding)" << std::endl;
            status = 1;
        }
        const size_t K = mine.size();
        vector<double> fU, fV, fE;                                        // [K][Jets][gpl], [K][gpl]: the fusion's inputs, slot k = rate mine[k]
        vector<unsigned long long> fO;
        if (fuse) { fU.assign(K * Jets * gpl, 0); fV.assign(fU.size(), 0); fE.assign(K * gpl, 0); fO.assign(K * gpl, 0); }
        for (size_t k = 0; k < mine.size() && status == 0; k++) {
            Segment &s = segs[mine[k]];
            double tb = now_s();
            SegmentInput in;
            if (!read_segment(s, use_occ, width, height, in) || in.fu.empty()) { status = 1; break; }
            if (in.fl[0][0]->stride != stride || minf.fl[0][0]->stride != stride) { std::cerr << "frames and flows differ in row stride" << std::endl; status = 1; break; }
            const int fstride = in.fl[0][0]->stride;
            vector<double> au((size_t)s.FF * gpl), av(au.size());
            vector<int> tracked(gpl);
            if (sfa_accumulate_consistent(ctx, 1, s.FF, width, height, fstride, in.fu.data(), in.fv.data(), in.bu.data(), in.bv.data(),
                                          use_occ ? in.mp.data() : nullptr, threshold, skip_pixel, discard, 1, au.data(), av.data(), tracked.data()) != SFA_OK) {
                std::cerr << sfa_last_error(ctx) << std::endl;
                status = 1;
                break;
            }
            double tc = now_s();
            t_acc += tc - tb;
            // a rate before acc_min_fps sees empty flow Mats (:786, :1148-1151)
            const bool flows = s.r >= min_fps_idx;
            ep.weight = jet_weight.size() > (size_t)s.r ? (float)jet_weight[s.r] : (float)s.r;   // weight_jet_estimation, vector<float> (:489-495)
            vector<double> energy(gpl);
            vector<unsigned long long> occ(gpl);
            if (sfa_hypothesis_energies_ex(ctx, &ep, 1, s.FF, (int)Jets, width, height, stride, au.data(), av.data(), tracked.data(), cfp.data(),
                                           flows ? minf.fu.data() : nullptr, flows ? minf.fv.data() : nullptr, flows ? minf.bu.data() : nullptr,
                                           flows ? minf.bv.data() : nullptr, energy.data(), occ.data(), fuse ? fU.data() + k * Jets * gpl : nullptr,
                                           fuse ? fV.data() + k * Jets * gpl : nullptr) != SFA_OK) {
                std::cerr << sfa_last_error(ctx) << std::endl;
                status = 1;
                break;
            }
            double td = now_s();
            t_energy += td - tc;
            if (fuse) {
                std::copy(energy.begin(), energy.end(), fE.begin() + k * gpl);
                std::copy(occ.begin(), occ.end(), fO.begin() + k * gpl);
            }
            image_t *u = image_new(gw, gh), *v = image_new(gw, gh);
            vector<unsigned char> tp(gpl), oc(gpl);
            vector<float> ef(gpl);
            for (int y = 0; y < gh; y++)
                for (int x = 0; x < gw; x++) {
                    const size_t i = (size_t)y * gw + x, last = (size_t)(s.FF - 1) * gpl + i;
                    u->data[(size_t)y * u->stride + x] = (float)au[last];
                    v->data[(size_t)y * v->stride + x] = (float)av[last];
                    const int t = tracked[i];
                    if (t == s.FF) s.created++; else s.rejected++;
                    tp[i] = (unsigned char)(t == s.FF ? 255 : 255 * t / s.FF);
                    ef[i] = (float)energy[i];                                 // an fp32 sum stored in a double: exact
                    oc[i] = (unsigned char)__builtin_popcountll(occ[i]);
                    if (ef[i] < best_e[i]) { best_e[i] = ef[i]; best[i] = (unsigned char)s.r; }   // strict: ties keep the lower r
                }
            hyps[mine[k]] = s.created;
            const string dir = acc_dir + std::to_string(s.r) + "/";
            if (writeFlowFile(s.out_flo.c_str(), u, v) != 0 || !write_pgm8(s.out_tracked, gw, gh, tp.data(), gw) ||
                !write_pfm(dir + "energy_" + std::to_string(seq_start) + ".pfm", gw, gh, ef.data()) ||
                !write_pgm8(dir + "occluded_" + std::to_string(seq_start) + ".pgm", gw, gh, oc.data(), gw)) {
                std::cerr << "cannot write the outputs of rate " << s.r << " under " << dir << std::endl;
                status = 1;
            }
            image_delete(u); image_delete(v);
            t_io += now_s() - td;
            std::cout << "rate " << s.r << ", start " << s.seq_start << ": " << s.created << " trajectory hypotheses generated! (" << s.rejected
                      << " rejected)" << std::endl;                                               // :1353
        }
        if (status == 0 && fuse) {
            // ---- the fusion of all rates (:1588-1905): the smoothness weight of normalised frame 0 (:969-981), then NMS, pairwise terms, TRW-S
            const double te = now_s();
            Fused fu{};
            fu.seq_start = seq_start;
            vector<float> weight((size_t)width * height);
            if (sfa_dt_smoothness_weight(ctx, width, height, stride, fp[0], 5.0f, nav, nsd, hbit, weight.data()) != SFA_OK) {
                std::cerr << sfa_last_error(ctx) << std::endl;
                status = 1;
            }
            const double tf = now_s();
            vector<int> slot(gpl);
            vector<double> flu(gpl), flv(gpl);
            vector<unsigned char> oc(gpl);
            if (status == 0 && sfa_fuse_hypotheses(ctx, &fup, 1, (int)K, (int)Jets, width, height, fU.data(), fV.data(), fE.data(), fO.data(), weight.data(),
                                                   slot.data(), flu.data(), flv.data(), oc.data(), &fu.energy, &fu.bound, &fu.iters, fu.stage_ms) != SFA_OK) {
                std::cerr << sfa_last_error(ctx) << std::endl;
                status = 1;
            }
            const double tg = now_s();
            fu.t_weight = tf - te;
            fu.t_fuse = tg - tf;
            t_fuse += tg - te;
            if (status == 0) {
                image_t *u = image_new(gw, gh), *v = image_new(gw, gh);
                vector<unsigned char> lp(gpl), op(gpl);
                for (int y = 0; y < gh; y++)
                    for (int x = 0; x < gw; x++) {
                        const size_t i = (size_t)y * gw + x;
                        u->data[(size_t)y * u->stride + x] = (float)flu[i];   // writeFlowMiddlebury's fp32 (utils.cpp:333); 1e10 without a node
                        v->data[(size_t)y * v->stride + x] = (float)flv[i];
                        lp[i] = slot[i] < 0 ? 255 : (unsigned char)segs[mine[slot[i]]].r;
                        op[i] = oc[i] ? 255 : 0;                                // convertTo(CV_8UC1, 255) (:1893)
                        fu.nodes += slot[i] >= 0;
                    }
                const string base = acc_dir + (sintel ? fmt2(flow_format, (int)seq_start, 0) : fmt1(flow_format, (int)seq_start));   // :1895-1898
                mkdirs(acc_dir + "occlusions/");
                if (writeFlowFile((base + ".flo").c_str(), u, v) != 0 || !png_write((base + "_vis.png").c_str(), flowColorImg(u, v, 0)) ||
                    !write_pgm8(acc_dir + "occlusions/frame_" + std::to_string(seq_start) + ".pgm", gw, gh, op.data(), gw) ||
                    !write_pgm8(acc_dir + "labels_" + std::to_string(seq_start) + ".pgm", gw, gh, lp.data(), gw)) {
                    std::cerr << "cannot write the fused outputs of start " << seq_start << " under " << acc_dir << std::endl;
                    status = 1;
                }
                image_delete(u); image_delete(v);
                std::cout << "start " << seq_start << ": fused " << K << " rate(s) over " << fu.nodes << " nodes, energy " << fu.energy << ", lower bound "
                          << fu.bound << ", " << fu.iters << " TRW-S iteration(s)" << std::endl;
                fused.push_back(fu);
            }
        }
        for (color_image_t *c : fr) color_image_delete(c);
        if (status == 0 && !write_pgm8(acc_dir + "best_" + std::to_string(seq_start) + ".pgm", gw, gh, best.data(), gw)) {
            std::cerr << "cannot write " << acc_dir << "best_" << seq_start << ".pgm" << std::endl;
            status = 1;
        }
    }
    if (ctx) sfa_ctx_destroy(ctx);
    if (status) return status;
    std::ofstream js((acc_dir + "run.json").c_str());
    js.precision(17);
    js << "{\n  \"cfg\": \"" << cfg << "\",\n  \"energies\": true, \"Jets\": " << Jets << ", \"steps\": " << steps << ", \"skip\": " << skip
       << ", \"acc_skip_pixel\": " << skip_pixel << ", \"width\": " << width << ", \"height\": " << height << ",\n  \"rates\": [";
    for (unsigned r = 0; r < rates; r++)
        js << (r ? ", " : "") << "{\"jet_estimation\": \"" << jets[r] << "\", \"jet_S\": " << jet_S[r] << ", \"jet_fps\": " << jet_fps[r]
           << ", \"jet_weight\": " << (jet_weight.size() > r ? (double)(float)jet_weight[r] : (double)r) << "}";
    js << "],\n  \"segments\": [";
    for (size_t i = 0; i < segs.size(); i++)
        js << (i ? ",\n    " : "\n    ") << "{\"rate\": " << segs[i].r << ", \"start_jet\": " << segs[i].start_jet << ", \"sequence_start\": " << segs[i].seq_start
           << ", \"FF\": " << segs[i].FF << ", \"created\": " << segs[i].created << ", \"rejected\": " << segs[i].rejected << ", \"hypotheses\": " << hyps[i]
           << ", \"flo\": \"" << segs[i].out_flo << "\"}";
    js << "],\n  \"skipped\": [";
    for (size_t i = 0; i < skipped.size(); i++) js << (i ? ", " : "") << "\"" << skipped[i] << "\"";
    js << "]";
    if (fuse) {
        js << ",\n  \"fused\": true, \"epic_interpolation\": false, \"neighbour_proposals\": false, \"acc_beta\": " << fup.acc_beta << ", \"acc_spatial_occ\": "
           << fup.acc_spatial_occ << ", \"acc_traj_sim_method\": " << fup.traj_sim_method << ", \"acc_traj_sim_thres\": " << fup.traj_sim_thres
           << ", \"acc_trws_eps\": " << fup.trws_eps << ", \"acc_trws_max_iter\": " << fup.trws_max_iter << ",\n  \"fusion\": [";
        for (size_t i = 0; i < fused.size(); i++)
            js << (i ? ",\n    " : "\n    ") << "{\"sequence_start\": " << fused[i].seq_start << ", \"nodes\": " << fused[i].nodes << ", \"energy\": " << fused[i].energy
               << ", \"lower_bound\": " << fused[i].bound << ", \"iterations\": " << fused[i].iters << ", \"weight_s\": " << fused[i].t_weight
               << ", \"fuse_call_s\": " << fused[i].t_fuse << ", \"kernels_ms\": {\"labels\": " << fused[i].stage_ms[0] << ", \"pairwise\": "
               << fused[i].stage_ms[1] << ", \"trws\": " << fused[i].stage_ms[2] << ", \"output\": " << fused[i].stage_ms[3] << "}}";
        js << "]";
    }
    js << ",\n  \"timings_s\": {\"frames\": " << t_frames << ", \"accumulate\": " << t_acc << ", \"energy_call\": " << t_energy << ", \"write\": " << t_io;
    if (fuse) js << ", \"fuse\": " << t_fuse;
    js << ", \"total\": " << now_s() - t0 << "}\n}\n";
    std::cout << "wrote the energies of " << segs.size() << " segment(s) to " << acc_dir << std::endl;
    return js.good() ? 0 : 1;
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
    const string cfg = argv[1];
    if (!file_exists(cfg)) { usage(); return 1; }
    printf("using parameters %s\n", cfg.c_str());
    unsigned selected = 0, selected_end = 0;
    bool resume = false, energies = false, fuse = false;
    for (int i = 2; i < argc; i++) {                                     // :449-476
        const char *a = argv[i];
        if (a[0] != '-') continue;
        if (!strcmp(a, "-h") || !strcmp(a, "-help")) usage();
        else if (!strcmp(a, "-resume")) resume = true;
        else if (!strcmp(a, "-energies")) energies = true;
        else if (!strcmp(a, "-fuse")) fuse = energies = true;
        else if (!strcmp(a, "-select") && i + 1 < argc) { selected = (unsigned)atoi(argv[++i]); selected_end = selected + 1; }
        else { fprintf(stderr, "unknown argument %s\n", a); usage(); return 1; }
    }
    ParameterList params;
    params.read(cfg);
    vector<string> jets = repeated(cfg, "jet_estimation");
    vector<int> jet_S, jet_fps;
    for (const string &v : repeated(cfg, "jet_S")) jet_S.push_back(atoi(v.c_str()));
    for (const string &v : repeated(cfg, "jet_fps")) jet_fps.push_back(atoi(v.c_str()));
    vector<double> jet_weight;
    for (const string &v : repeated(cfg, "jet_weight")) jet_weight.push_back(atof(v.c_str()));
    for (string &j : jets)
        if (j.back() != '/') j += "/";                                   // :479-480
    const unsigned rates = (unsigned)jets.size();
    if (rates == 0) { std::cerr << "No Jet estimation specified!" << std::endl; return 1; }
    const bool sintel = params.parameter<bool>("sintel", "0"), subframes = params.parameter<bool>("subframes", "0");
    const int skip_pixel = params.parameter<int>("acc_skip_pixel", "1");        // setDefault: "1" (:122)
    const int ref_fps_F = params.parameter<int>("ref_fps_F", "1");
    const int min_fps_idx = params.parameter<int>("acc_min_fps", "0");
    const int max_fps = params.parameter<int>("max_fps", "0");
    const double threshold = params.parameter<double>("acc_consistency_threshold", "1.0");
    const bool discard = params.parameter<bool>("acc_discard_inconsistent", "1");
    // the reference gates the jets' occlusion masks on acc_use_jet_occlusions (:628, :1158); its sample cfg sets only acc_occlusion, read where the first is absent
    const bool use_occ = params.exists("acc_use_jet_occlusions") ? params.parameter<bool>("acc_use_jet_occlusions")
                                                                 : params.parameter<bool>("acc_occlusion", "0");
    if (min_fps_idx < 0 || min_fps_idx >= (int)rates) { std::cerr << "acc_min_fps " << min_fps_idx << " names no jet estimation" << std::endl; return 1; }
    // slow_flow_S and jet_fps from each jet folder's config.cfg where the cfg does not give one per rate (:502-556)
    for (int pass = 0; pass < 2; pass++) {
        vector<int> &dst = pass ? jet_fps : jet_S;
        const char *key = pass ? "jet_fps" : "slow_flow_S";
        if (dst.size() == rates) continue;
        dst.assign(rates, 0);
        for (unsigned r = 0; r < rates; r++) {
            const string jc = jets[r] + "config.cfg";
            if (!file_exists(jc)) { std::cerr << "Error reading " << jc << " (does not exist)" << std::endl; return 2; }
            ParameterList tmp(jc);
            if (!tmp.exists(key)) { std::cerr << "Error reading " << key << " from " << jc << std::endl; return 1; }
            dst[r] = tmp.parameter<int>(key);
        }
    }
    const int steps = jet_S[min_fps_idx] - 1;                            // :527
    if (!params.exists("ref_fps")) { std::cerr << "ref_fps missing from " << cfg << std::endl; return 1; }
    const int ref_fps = params.parameter<int>("ref_fps");
    if (steps < 1 || ref_fps < 1 || jet_fps[min_fps_idx] < 1) { std::cerr << "slow_flow_S, ref_fps and jet_fps must be positive" << std::endl; return 1; }
    const unsigned Jets = (unsigned)(jet_fps[min_fps_idx] / (1.0f * ref_fps * steps));     // :564, float -> u_int32_t
    const int skip = (int)((1.0f * max_fps) / jet_fps[min_fps_idx]);    // :571
    if (Jets < 1) { std::cerr << "Jets = jet_fps / (ref_fps * steps) is 0" << std::endl; return 1; }
    if (energies) {
        // acc_occlusion 1 makes addBCGC read occlusion_masks[Jets], one past the Mat[Jets] array (:784, :289): undefined in the reference
        const char *refused = params.parameter<bool>("acc_occlusion", "0") ? "acc_occlusion 1 (addBCGC reads occlusion_masks[Jets], past the array)"
                              : params.parameter<bool>("grayscale", "0") ? "grayscale 1"
                              : (params.exists("raw") && params.parameter<bool>("raw") && params.parameter<int>("raw_demosaicing", "0") == 1)
                                  ? "raw_demosaicing 1 (Hamilton-Adams, third-party, not here)"
                              : (params.extent.x > 0 || params.extent.y > 0 || params.center.x > 0) ? "cropping (center / extent)"
                              : Jets > 32 ? "Jets > 32" : nullptr;
        if (refused) { std::cerr << "-energies: " << refused << " is not supported" << std::endl; return 1; }
        if (params.file.empty()) { std::cerr << "-energies: `file` (the frames) missing from " << cfg << std::endl; return 1; }
    }
    if (fuse) {
        const int method = params.parameter<int>("acc_traj_sim_method", "1");
        const char *refused = params.parameter<int>("acc_approach", "0") == 1 ? "acc_approach 1 (BP)"
                              : method == 2 ? "acc_traj_sim_method 2 (FINAL reads flow_y[Jets], past the adapted array)"
                              : (method != 0 && method != 1) ? "an acc_traj_sim_method other than 0 or 1"
                              : rates > 16 ? "more than 16 rates" : nullptr;
        if (refused) { std::cerr << "-fuse: " << refused << " is not supported" << std::endl; return 1; }
        if (params.parameter<bool>("acc_epic_interpolation", "1"))
            std::cout << "-fuse: acc_epic_interpolation 1, but EpicFlow's fill-in and the neighbour proposals are not run (pixels without a hypothesis "
                         "stay UNKNOWN_FLOW)" << std::endl;
    }
    if (selected_end == 0) selected_end = (unsigned)ref_fps_F;           // :722-723
    unsigned sequence_start = params.sequence_start;
    if (sintel && !subframes) sequence_start *= 1000;                    // :716-717
    string flow_format = params.parameter<string>("flow_format", "frame_%i");
    flow_format = flow_format.substr(0, flow_format.find_last_of('.'));  // :745-746
    // the output folder: never an existing one without -resume (:582-594)
    string output = params.output;
    if (output.empty()) { std::cerr << "output missing from " << cfg << std::endl; return 1; }
    if (!resume) {
        if (output.back() == '/') output.pop_back();
        string np = output;
        for (int num = 1; file_exists(np); num++) { std::cerr << np << " already exists!" << std::endl; np = output + "_" + std::to_string(num); }
        output = np;
    }
    if (output.back() != '/') output += "/";
    const string acc_dir = output + "accumulated/";

    // ---- the segments: every start_jet x rate whose output is not there yet ----------------------------------------------------------------------
    vector<Segment> segs;
    vector<string> skipped;
    for (unsigned start_jet = selected; start_jet < selected_end; start_jet++) {
        const unsigned seq_start = sequence_start + start_jet * Jets * steps * skip;   // :735
        if (fuse) {                                                      // the fused flow is the start_jet's product
            const string flo = acc_dir + (sintel ? fmt2(flow_format, (int)seq_start, 0) : fmt1(flow_format, (int)seq_start)) + ".flo";
            if (file_exists(flo)) { std::cout << "Flow file " << flo << " already exists!" << std::endl; skipped.push_back(flo); continue; }
        } else if (energies) {                                           // with the energies a start_jet is done as a whole: all its rates are compared
            const string best = acc_dir + "best_" + std::to_string(seq_start) + ".pgm";
            if (file_exists(best)) { std::cout << "Energy file " << best << " already exists!" << std::endl; skipped.push_back(best); continue; }
        }
        for (unsigned r = 0; r < rates; r++) {
            Segment s;
            s.r = (int)r; s.start_jet = start_jet; s.seq_start = seq_start;
            const int r_steps = jet_S[r] - 1;                                            // :1101
            const float ratio = (1.0f * jet_fps[r]) / jet_fps[min_fps_idx];              // :1103
            s.FF = (int)(unsigned)(ratio * Jets);                                        // :1104
            const int r_skip = (int)((1.0f * max_fps) / jet_fps[r]);                     // :1105
            const string dir = acc_dir + std::to_string(r) + "/";
            s.out_flo = dir + (sintel ? fmt2("s" + flow_format, (int)seq_start, 0) : fmt1(flow_format, (int)seq_start)) + ".flo";
            s.out_tracked = dir + "tracked_" + std::to_string(seq_start) + ".pgm";
            if (!energies && file_exists(s.out_flo)) { std::cout << "Flow file " << s.out_flo << " already exists!" << std::endl; skipped.push_back(s.out_flo); continue; }
            if (s.FF < 1) { std::cerr << "rate " << r << ": r_Jets = " << s.FF << ", nothing to accumulate" << std::endl; return 1; }
            for (int f = 0; f < s.FF; f++) {
                const int a = (int)seq_start + f * r_steps * r_skip;
                s.fwd.push_back(jets[r] + fmt1(flow_format, a) + ".flo");                                         // :1118
                s.bwd.push_back(jets[r] + fmt1(flow_format, a + r_steps * r_skip) + "_back.flo");                                  // :1119
                if (use_occ) s.occ.push_back(jets[r] + "/occlusion/frame_" + std::to_string(a));                                  // :1161, extension below
            }
            segs.push_back(s);
        }
    }
    // every input must exist before anything runs (the reference breaks out of its read loop and goes on with empty flows, :1121-1128)
    for (Segment &s : segs)
        for (int f = 0; f < s.FF; f++) {
            for (const string &file : {s.fwd[f], s.bwd[f]})
                if (!file_exists(file)) { std::cerr << file << " does not exist!" << std::endl; return 2; }
            if (use_occ) {
                if (file_exists(s.occ[f] + ".pgm")) s.occ[f] += ".pgm";      // what this project's driver writes
                else if (file_exists(s.occ[f] + ".pbm")) s.occ[f] += ".pbm"; // the reference's name
                else { std::cerr << s.occ[f] << ".pgm does not exist (nor " << s.occ[f] << ".pbm)!" << std::endl; return 2; }
            }
        }
    // the frames of each start_jet (:793-810): sequence_start + f * steps * skip, f = 0 .. Jets
    std::map<unsigned, vector<string>> frame_files;
    if (energies) {
        const size_t sf = params.file.find_last_of('/') + 1;             // :740-751 (npos + 1 == 0: no folder)
        string sequence_path = params.file.substr(0, sf);
        const string format = params.file.substr(sf);
        if (!sequence_path.empty() && sequence_path.back() != '/') sequence_path += "/";
        for (const Segment &s : segs) {
            vector<string> &names = frame_files[s.seq_start];
            if (!names.empty()) continue;
            for (unsigned f = 0; f <= Jets; f++) {
                if (!sintel) names.push_back(fmt1(sequence_path + format, (int)(s.seq_start + f * steps * skip)));
                else {
                    int sintel_frame = (int)s.seq_start / 1000, hfr = (int)(f * steps * skip) + (int)(s.seq_start % 1000);
                    while (hfr < 0) { sintel_frame--; hfr += 42; }
                    while (hfr > 41) { sintel_frame++; hfr -= 42; }
                    names.push_back(fmt2(sequence_path + format, sintel_frame, hfr));
                }
                if (!file_exists(names.back())) { std::cerr << names.back() << " does not exist!" << std::endl; return 2; }
            }
        }
    }
    mkdirs(acc_dir);
    for (unsigned r = 0; r < rates; r++) mkdirs(acc_dir + std::to_string(r) + "/");
    if (energies) return run_energies(params, cfg, acc_dir, segs, skipped, frame_files, rates, min_fps_idx, Jets, steps, skip, skip_pixel, threshold, discard,
                                      use_occ, jets, jet_S, jet_fps, jet_weight, fuse, flow_format, sintel);

    sfa_ctx *ctx = nullptr;
    if (!segs.empty() && sfa_ctx_create(0, &ctx) != SFA_OK) { std::cerr << sfa_last_error(nullptr) << std::endl; return 1; }
    double t_read = 0, t_gpu = 0, t_write = 0;
    const double t0 = now_s();
    int width = 0, height = 0, calls = 0;
    std::map<int, vector<size_t>> by_ff;                                 // segments that share FF go through one call
    for (size_t i = 0; i < segs.size(); i++) by_ff[segs[i].FF].push_back(i);
    int status = 0;
    for (auto &grp : by_ff) {
        const int FF = grp.first;
        const vector<size_t> &idx = grp.second;
        size_t lo = 0;
        while (lo < idx.size() && status == 0) {
            double ta = now_s();
            // read one chunk: up to 2 GiB of input planes per call
            vector<image_t **> fl;                                       // [k * FF + f]: forward, then backward (2 per plane pair)
            vector<const float *> fu, fv, bu, bv;
            vector<vector<unsigned char>> mbuf;
            vector<const unsigned char *> mp;
            size_t hi = lo, bytes = 0;
            while (hi < idx.size() && status == 0 && (hi == lo || bytes < (size_t)2 << 30)) {
                Segment &s = segs[idx[hi]];
                for (int f = 0; f < FF && status == 0; f++) {
                    image_t **a = readFlowFile(s.fwd[f].c_str()), **b = readFlowFile(s.bwd[f].c_str());
                    if (a) fl.push_back(a);
                    if (b) fl.push_back(b);
                    if (!a || !b) { std::cerr << "cannot read " << (a ? s.bwd[f] : s.fwd[f]) << " as a .flo" << std::endl; status = 1; break; }
                    if (width == 0) { width = a[0]->width; height = a[0]->height; }
                    for (image_t **c : {a, b})
                        if (c[0]->width != width || c[0]->height != height) {
                            std::cerr << (c == a ? s.fwd[f] : s.bwd[f]) << " is " << c[0]->width << " x " << c[0]->height << ", the first flow " << width << " x "
                                      << height << ": rescaling is not implemented" << std::endl;
                            status = 1;
                        }
                    if (status) break;
                    fu.push_back(a[0]->data); fv.push_back(a[1]->data); bu.push_back(b[0]->data); bv.push_back(b[1]->data);
                    if (use_occ) {
                        int ow, oh;
                        vector<unsigned char> g;
                        if (!read_pnm8(s.occ[f], ow, oh, g)) { std::cerr << s.occ[f] << ": not a binary PGM (maxval 255) or PBM" << std::endl; status = 1; break; }
                        if (ow != width || oh != height) { std::cerr << s.occ[f] << " is not " << width << " x " << height << std::endl; status = 1; break; }
                        mbuf.emplace_back((size_t)a[0]->stride * height, 0);
                        decode_occlusion(g, width, height, a[0]->stride, mbuf.back().data());
                    }
                }
                bytes += (size_t)FF * width * height * 17;
                hi++;
            }
            for (auto &m : mbuf) mp.push_back(m.data());
            double tb = now_s();
            t_read += tb - ta;
            if (status == 0) {
                const int n = (int)(hi - lo), stride = fl[0][0]->stride;
                int gw = 0, gh = 0;
                if (sfa_accumulate_grid(width, height, skip_pixel, &gw, &gh) != SFA_OK) { std::cerr << sfa_last_error(nullptr) << std::endl; status = 1; }
                vector<double> au, av;
                vector<int> tracked;
                if (status == 0) {
                    au.resize((size_t)n * gw * gh); av.resize(au.size()); tracked.resize(au.size());
                    if (sfa_accumulate_consistent(ctx, n, FF, width, height, stride, fu.data(), fv.data(), bu.data(), bv.data(), use_occ ? mp.data() : nullptr,
                                                  threshold, skip_pixel, discard, 0, au.data(), av.data(), tracked.data()) != SFA_OK) {
                        std::cerr << sfa_last_error(ctx) << std::endl;
                        status = 1;
                    }
                    calls++;
                }
                double tc = now_s();
                t_gpu += tc - tb;
                for (int k = 0; k < n && status == 0; k++) {
                    Segment &s = segs[idx[lo + k]];
                    const size_t off = (size_t)k * gw * gh;
                    image_t *u = image_new(gw, gh), *v = image_new(gw, gh);
                    vector<unsigned char> tp((size_t)gw * gh);
                    for (int y = 0; y < gh; y++)
                        for (int x = 0; x < gw; x++) {
                            const size_t i = off + (size_t)y * gw + x;
                            u->data[(size_t)y * u->stride + x] = (float)au[i];           // convertTo(CV_32F) (utils.cpp:333), channel 1 = u
                            v->data[(size_t)y * v->stride + x] = (float)av[i];
                            const int t = tracked[i];
                            if (t == FF) s.created++; else s.rejected++;                  // :1225-1257
                            tp[(size_t)y * gw + x] = (unsigned char)(t == FF ? 255 : 255 * t / FF);
                        }
                    if (writeFlowFile(s.out_flo.c_str(), u, v) != 0 || !write_pgm8(s.out_tracked, gw, gh, tp.data(), gw)) {
                        std::cerr << "cannot write " << s.out_flo << std::endl;
                        status = 1;
                    }
                    image_delete(u); image_delete(v);
                    std::cout << "rate " << s.r << ", start " << s.seq_start << ": " << s.created << " trajectory hypotheses generated! (" << s.rejected
                              << " rejected)" << std::endl;                                           // :1353
                }
                t_write += now_s() - tc;
            }
            for (image_t **c : fl) { image_delete(c[0]); image_delete(c[1]); free(c); }
            lo = hi;
        }
    }
    if (ctx) sfa_ctx_destroy(ctx);
    if (status) return status;
    // run.json
    std::ofstream js((acc_dir + "run.json").c_str());
    js << "{\n  \"cfg\": \"" << cfg << "\",\n  \"Jets\": " << Jets << ", \"steps\": " << steps << ", \"skip\": " << skip << ", \"acc_skip_pixel\": " << skip_pixel
       << ", \"width\": " << width << ", \"height\": " << height << ",\n  \"rates\": [";
    for (unsigned r = 0; r < rates; r++)
        js << (r ? ", " : "") << "{\"jet_estimation\": \"" << jets[r] << "\", \"jet_S\": " << jet_S[r] << ", \"jet_fps\": " << jet_fps[r]
           << ", \"jet_weight\": " << (jet_weight.size() > r ? jet_weight[r] : (double)r) << "}";
    js << "],\n  \"segments\": [";
    for (size_t i = 0; i < segs.size(); i++)
        js << (i ? ",\n    " : "\n    ") << "{\"rate\": " << segs[i].r << ", \"start_jet\": " << segs[i].start_jet << ", \"sequence_start\": " << segs[i].seq_start
           << ", \"FF\": " << segs[i].FF << ", \"created\": " << segs[i].created << ", \"rejected\": " << segs[i].rejected << ", \"flo\": \"" << segs[i].out_flo << "\"}";
    js << "],\n  \"skipped\": [";
    for (size_t i = 0; i < skipped.size(); i++) js << (i ? ", " : "") << "\"" << skipped[i] << "\"";
    js << "],\n  \"calls\": " << calls << ",\n  \"timings_s\": {\"read\": " << t_read << ", \"gpu_call\": " << t_gpu << ", \"write\": " << t_write
       << ", \"total\": " << now_s() - t0 << "}\n}\n";
    std::cout << "wrote " << segs.size() << " segment(s) to " << acc_dir << std::endl;
    return js.good() ? 0 : 1;
}
