// slow_flow.cpp -- the slow_flow driver of the drop-in: same cfg keys, command line and outputs as the reference's
// slow_flow.cpp (usage :58-62, defaults :64-128, adaptive frame rates :277-357, frame indexing :411-465, jet loop :706-1047,
// .flo outputs :908-911, :1027-1030, resume :794,958, config.cfg :684-688) for the path this repository implements:
//   frames -> normalize -> per jet: forward / backward Variational_MT::variational -> flow * steps -> .flo
// The jets of a sequence are independent; they are sharded over the node's GPUs (shard.h: `gpu_streams` host threads per
// GPU, each with its own context = HIP stream) and each worker refines `gpu_batch` frame windows in lockstep.  The driver is
// a pipeline: frames are decoded by a pool of host threads, sent to every GPU once and normalised there (sfa_sequence), every worker
// keeps ONE resident job for all its batches (device-to-device window copies / run / download), and results go to the output pool (.flo, colour PNG, occlusion images) while the worker
// already refines its next batch; with two workers per GPU the uploads of one overlap the kernels of the other.
// deep_matching 1 initialises the flow with EpicFlow's interpolation (epic.h) of match and edge files found at the reference's locations; producing those files
// (DeepMatching, the MATLAB SED detector) and the third-party Hamilton-Adams demosaicer (raw_demosaicing 1) are outside this build and reported as such.
//
// New, additive keys: gpus (default: all visible; gpu_oversubscribe 1 lets it exceed them: a rehearsal of the multi-GPU path), gpu_batch (windows refined in lockstep per job, default 32), gpu_streams
// (default 2), gpu_device (first device, default 0), io_threads (decode / output pool, default min(16, cores)), gpu_ingest (default 0; 1 with raw 1: the
// mosaics go to the GPU as they are and are demosaiced, cropped and rescaled there, sfa_sequence_upload_mosaic / sfa_sequence_rescale; same output files),
// adaptive_fr_file (default: adaptiveFR.dat next to the executable, the reference's SOURCE_PATH).
#include <unistd.h>

#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <mutex>
#include <string>
#include <future>
#include <thread>
#include <vector>

#include "epic.h"
#include "flow_vis.h"
#include "image.h"
#include "ingest.h"
#include "io.h"
#include "parameter_list.h"
#include "shard.h"
#include "util.h"
#include "variational_mt.h"

using std::string;

static void usage() {
    printf("usage:\n    ./slow_flow [cfg] -overwrite -resume -deep_settings [settings] -threads -fr [select one specific adaptive frame rate] "
           "-jet [select one specific high speed flow]\n\n"
           "    -deep_settings is accepted and ignored: the reference passes it to the DeepMatching binary it starts (slow_flow.cpp:180-181, :768); this build does\n"
           "    not start DeepMatching or the MATLAB edge detector -- with deep_matching 1 it reads their outputs from <output>tmp/ (matches_<a>_<b>.dat, edges_<n>.dat).\n"
           "    raw_demosaicing 1 (Hamilton-Adams, third-party code absent from the reference tree) is rejected; 0 (bilinear) and 2 (OpenCV's 8-bit conversion) work.\n"
           "    cfg keys of this build: gpu_epic 1 interpolates a batch's matches on the GPU (deep_matching 1); with it, gpu_epic_search 1 runs EpicFlow's graph searches\n"
           "    in the library's compact mode (slices of seeds in one shared workspace; the same bits).  gpu_epic_search other than 0 or 1 exits with status 1.\n\n");
}

static void setDefault(ParameterList &p) {        // slow_flow.cpp:64-128
    const char *kv[][2] = {
        {"verbose", "0"}, {"threads", "1"}, {"16bit", "1"}, {"raw", "1"}, {"raw_weight", "1"}, {"raw_demosaicing", "1"}, {"raw_red_loc", "1,0"},
        {"Jets", "1"}, {"adaptive", "1"}, {"max_fps", "200"}, {"ref_fps", "20"}, {"scale", "1.0f"}, {"sigma", "0.0f"}, {"deep_matching", "1"},
        {"dm_scale", "1.0f"}, {"slow_flow_method", "symmetric"}, {"slow_flow_S", "2"}, {"slow_flow_dataterm", "1"}, {"slow_flow_smoothing", "1"},
        {"slow_flow_alpha", "4.0f"}, {"slow_flow_gamma", "6.0f"}, {"slow_flow_delta", "1.0f"}, {"slow_flow_rho_0", "1"}, {"slow_flow_rho_1", "1"},
        {"slow_flow_omega_0", "0"}, {"slow_flow_omega_1", "2"}, {"slow_flow_layers", "1"}, {"slow_flow_p_scale", "0.9f"}, {"slow_flow_niter_alter", "10"},
        {"slow_flow_niter_graphc", "10"}, {"slow_flow_niter_outer", "10"}, {"slow_flow_thres_outer", "1e-5"}, {"slow_flow_niter_inner", "1"},
        {"slow_flow_thres_inner", "1e-5"}, {"slow_flow_niter_solver", "30"}, {"slow_flow_sor_omega", "1.9f"}, {"slow_flow_occlusion_reasoning", "1"},
        {"slow_flow_occlusion_penalty", "0.1"}, {"slow_flow_occlusion_alpha", "0.1"}, {"slow_flow_output_occlusions", "1"}, {"slow_flow_robust_color", "1"},
        {"slow_flow_robust_color_eps", "0.001"}, {"slow_flow_robust_color_truncation", "0.5"}, {"slow_flow_robust_reg", "1"},
        {"slow_flow_robust_reg_eps", "0.001"}, {"slow_flow_robust_reg_truncation", "0.5"}};
    for (auto &e : kv) p.insert(e[0], e[1], true);
}

static string exe_dir() {
    char buf[4096];
    const ssize_t n = readlink("/proc/self/exe", buf, sizeof buf - 1);
    if (n <= 0) return ".";
    buf[n] = 0;
    string s(buf);
    return s.substr(0, s.find_last_of('/'));
}

// owners of the library's and the image module's objects: every exit releases what it holds
template <typename T, void (*Free)(T *)> struct Release { void operator()(T *p) const { Free(p); } };
typedef std::unique_ptr<image_t, Release<image_t, image_delete>> Image;
typedef std::unique_ptr<color_image_t, Release<color_image_t, color_image_delete>> ColorImage;
typedef std::unique_ptr<sfa_ctx, Release<sfa_ctx, sfa_ctx_destroy>> Ctx;
typedef std::unique_ptr<sfa_job, Release<sfa_job, sfa_job_destroy>> Job;
typedef std::unique_ptr<sfa_sequence, Release<sfa_sequence, sfa_sequence_destroy>> DeviceSequence;
typedef std::unique_ptr<sfa_epic_job, Release<sfa_epic_job, sfa_epic_job_destroy>> EpicJob;
typedef std::pair<Image, Image> Flow;

static Image zero_image(int w, int h) {
    Image im(image_new(w, h));
    image_erase(im.get());
    return im;
}
static Ctx new_ctx(int device) {                 // null on failure (sfa_last_error(nullptr))
    sfa_ctx *c = nullptr;
    sfa_ctx_create(device, &c);
    return Ctx(c);
}

struct Window {
    unsigned jet; bool backward; string out; double seconds; int gpu; double epe, aae;   // epe/aae < 0: no ground truth
    Window(unsigned j, bool b, const string &o) : jet(j), backward(b), out(o), seconds(0), gpu(-1), epe(-1), aae(-1) {}
};

// the labels of optimizeOcc as an 8-bit image, (occ + 1) / 2 * 255 (variational_mt.cpp:277-279, slow_flow.cpp:895-896)
static png_image occlusion_image(const image_t *occ) {
    png_image im;
    im.width = occ->width; im.height = occ->height; im.channels = 1; im.depth = 8;
    im.samples.resize((size_t)occ->width * occ->height);
    for (int y = 0; y < occ->height; y++)
        for (int x = 0; x < occ->width; x++) {
            const float v = (occ->data[(size_t)y * occ->stride + x] + 1) * 0.5f * 255.0f;
            im.samples[(size_t)y * occ->width + x] = (uint16_t)std::max(0.0f, std::min(255.0f, std::nearbyint(v)));
        }
    return im;
}

struct RunOptions {
    bool resume_frame = false;
    int selected_jet = -1;
};

// the settings of one pass, read once from the cfg (the body of the reference's adFR loop, slow_flow.cpp:367-1060)
struct Run {
    Run(const ParameterList &params, const string &format, int skip_, const RunOptions &opt)
        : p(params), format_flow(format.substr(0, format.find_last_of('.'))), skip(skip_), layout(plan_sequence(params.Jets, steps, opt.resume_frame, opt.selected_jet)) {}
    const ParameterList &p;                                                         // (the members below are read from it in this order)
    const string output = p.output, format_flow, file_gt = p.file_gt;
    const bool raw = p.exists("raw") && p.parameter<bool>("raw");
    const std::vector<int> red_loc = p.splitParameter<int>("raw_red_loc", "0,0");   // :439
    const int red_x = red_loc.size() > 0 ? red_loc[0] : 0, red_y = red_loc.size() > 1 ? red_loc[1] : 0;
    const int demosaicing = p.parameter<int>("raw_demosaicing", "0");
    const float raw_weight = p.parameter<float>("raw_weight", "1.0"), scale = p.parameter<float>("scale", "1.0");
    const bool preprocess = !p.exists("raw") || raw_weight == 1.0f;                 // :531
    const bool rescale = preprocess && scale != 1;
    const bool crop = preprocess && (p.extent.x > 0 || p.extent.y > 0);             // :533-536
    const bool gpu_ingest = p.parameter<bool>("gpu_ingest", "0");                   // additive: raw frames are demosaiced, cropped and rescaled on the GPU
    const int steps = p.parameter<int>("slow_flow_S") - 1, skip;                    // :208-209 (ref = steps)
    const bool sintel = p.parameter<bool>("sintel", "0");
    const unsigned start = p.sequence_start;
    const Point center = p.center, extent = p.extent;
    const int io_threads = std::max(1, std::min(64, p.parameter<int>("io_threads", std::to_string(std::max(1u, std::min(16u, std::thread::hardware_concurrency()))))));
    const SequenceLayout layout;
    // gpu_oversubscribe 1: `gpus` may exceed the devices of the box, GPU g then runs on device g mod devices -- the multi-GPU code path (one resident
    // sequence, one set of workers and one statistics slot per GPU) rehearsed on fewer cards than it is written for; never a way to get speed
    const bool oversubscribe = p.parameter<bool>("gpu_oversubscribe", "0");
    const int dev0 = p.parameter<int>("gpu_device", "0"), batch = p.parameter<int>("gpu_batch", "32");
    // the GPUs, chosen before anything is read so that the HIP runtime starts up -- 0.35 s for the first context of a process -- beside the decoding
    const int ndev = sfa_device_count();
    const int gpus = !p.exists("gpus") ? ndev : std::max(1, oversubscribe ? std::min(16, p.parameter<int>("gpus")) : std::min(ndev, p.parameter<int>("gpus")));
    const int ngpu = oversubscribe ? gpus : std::max(1, std::min(gpus, ndev - dev0));   // devices dev0 .. ndev-1 exist; asking for more would only fail after all frames are decoded
    // `gpu_streams` workers per GPU (default 2), each with its own context = HIP stream: two lockstep groups fill each other's
    // ramp-up / drain phases (the reference runs its windows from `threads` OpenMP threads the same way, slow_flow.cpp:706)
    const int streams = std::max(1, std::min(4, p.parameter<int>("gpu_streams", "2")));
    const bool deep_matching = p.parameter<bool>("deep_matching");
    const bool gpu_epic = p.parameter<bool>("gpu_epic", "0");                       // additive: deep_matching 1 interpolates a batch's matches through epic_batch (the graph searches on the GPU)
    const int gpu_epic_search = p.parameter<int>("gpu_epic_search", "0");          // additive, with gpu_epic 1: 1 = those searches in the library's compact mode (main() refuses other values)
    // gpu_ingest 1 + deep_matching 1 + gpu_epic 1: the initialisation stays on the GPU from the frames to the job's initial flow (sfa_sequence_lab, sfa_epic_job,
    // sfa_job_set_flow_epic); only the match and edge files are read on the host
    const bool resident_epic = gpu_ingest && deep_matching && gpu_epic;
    // dm_scale (:396-402, :571-586, :801-843): DeepMatching and the edge detector ran on frames blurred (sigma = 1 / sqrt(2 dm_scale)) and resized by dm_scale; the
    // interpolation then runs at that resolution (the saliency image, the edge map, the matches' coordinates) and its flow is resized to the frames and multiplied by the
    // INTEGER ratio of the widths (:827-828: `float fx = im[ref]->width / wx->width` divides two ints).  dm_scale_run = dm_scale, halved by main() when max_flow > 150
    const double dm_scale = p.exists("dm_scale_run") ? p.parameter<double>("dm_scale_run") : (double)p.parameter<float>("dm_scale", "1.0");
    const bool verbose_changes = p.verbosity(VER_CMD);  // the library prints the reference's "inner it / outer it ... avg change" lines (variational_mt.cpp:404-405, 431-432): per worker context
    const bool write_files = p.verbosity(WRITE_FILES);
    const bool forward_only = p.exists("method") && p.parameter("method") == "forward";              // :1019-1020
    const bool out_occ = p.parameter<bool>("slow_flow_output_occlusions", "0");                      // :892
    // the per-alternation labels (:878-884: <output>tmp/frame_<n>_<alter>.png), with WRITE_FILES verbosity only
    const bool out_alt_occ = out_occ && p.parameter<bool>("slow_flow_occlusion_reasoning", "0") && write_files && p.parameter<int>("slow_flow_niter_alter", "1") > 1;
    int device_of(int g) const { return oversubscribe ? (dev0 + g) % ndev : dev0 + g; }
};

static string flow_file(const Run &run, unsigned jet, bool backward) {
    const JetFrames n = jet_frames(run.start, jet, run.steps, run.skip);
    const string pattern = run.output + run.format_flow + (backward ? "_back.flo" : ".flo");
    return run.sintel ? fmt2(pattern, backward ? n.to : n.from, 0) : fmt1(pattern, backward ? n.to : n.from);
}
static string edges_file(const Run &run, int frame_number) { return run.output + "tmp/edges_" + std::to_string(frame_number) + ".dat"; }              // :740-741
static string matches_file(const Run &run, int a, int b) { return run.output + "tmp/matches_" + std::to_string(a) + "_" + std::to_string(b) + ".dat"; }   // :742-743

// the windows to refine: forward and backward of every jet (:706-1047); -resume skips existing flows (:712-716 / :934-938)
static std::vector<Window> windows_to_refine(const Run &run, bool resume) {
    std::vector<Window> todo;
    for (unsigned j = run.layout.start_j; j < run.layout.end_j; j++) {
        const JetFrames n = jet_frames(run.start, j, run.steps, run.skip);
        for (int backward = 0; backward < 2; backward++) {
            const string out = flow_file(run, j, backward);
            if (!resume || !file_exists(out)) todo.push_back(Window(j, backward, out));
            else std::cout << (backward ? "Backward" : "Forward") << " flow from frame " << (backward ? n.from : n.listed_from) << " to " << n.to << " already exist!" << std::endl;
        }
    }
    return todo;
}

// ---- deep_matching 1 (:744-863): the flow is initialised by EpicFlow's interpolation (epic.h) of DeepMatching matches along SED edges.  The reference starts
//      both tools with system() (MATLAB + a binary, third-party); this build reads their outputs from the reference's own locations and says so if they are missing.
static bool deep_matching_inputs_exist(const Run &run, bool resume) {
    for (unsigned j = run.layout.start_j; j < run.layout.end_j; j++) {
        if (resume && file_exists(flow_file(run, j, false)) && file_exists(flow_file(run, j, true))) continue;   // -resume: a jet whose two flows exist is skipped and needs no inputs
        const JetFrames n = jet_frames(run.start, j, run.steps, run.skip);
        const string need[4] = {edges_file(run, n.from), edges_file(run, n.to), matches_file(run, n.from, n.to), matches_file(run, n.to, n.from)};
        for (const string &f : need)
            if (!file_exists(f)) {
                std::cerr << "deep_matching 1: " << f << " is missing. The matches come from DeepMatching and the edge maps from the SED detector (matlab/detect_edges.m), "
                             "third-party programs this build does not start; place their outputs there (raw float edge map of the frame size; one match 'x1 y1 x2 y2 ...' per line) "
                             "and run with -resume or -overwrite, or set deep_matching 0" << std::endl;
                return false;
            }
    }
    return true;
}

// The loaded sequence and its way onto the GPUs.  The frames go to the GPUs once and are normalised there (:673; the three parts of sfa_sequence_normalize: same kernels,
// same statistics as the host-plane normalize() of variational_mt.h).  GPU g holds the frames gpu_frames[g] of its own windows (+ the halo its boundary jets share with
// the neighbour): about 1 / N of the sequence.  The statistics are those of ALL loaded frames: every GPU forms the six fp64 sums of the frames it holds (a deterministic
// kernel: a frame two GPUs hold gets the same bits from both), the sums are collected per frame on the host, and the moment the last frame's sums are in, the statistics
// are formed from them in frame order -- one set of doubles for every GPU.  One thread per GPU: it creates the context while the io pool decodes, uploads each of its
// frames the moment it is published, normalises its frames once the statistics are known and releases that GPU's workers; no GPU waits for another GPU's uploads beyond
// the sums of the frames it does not hold itself.  A GPU without windows only creates its context: with nothing to refine nobody waits for statistics.
class Sequence {
public:
    struct Gpu { Ctx ctx; DeviceSequence resident, lab; string err; bool ready = false; double upload_bytes = 0, upload_done_s = 0, ready_s = 0, first_refine_s = -1; };   // (resident and lab go before ctx; s since the run began; lab: the L*a*b* images of the reference frames of the GPU's windows at the interpolation's size, one frame each (lab_slot; resident_epic))
    std::vector<ColorImage> frames;              // by frame of the pass (only [start_f, end_f) is loaded); width x height: published with the first frame
    std::vector<int> maxval;                     // 255 / 65535 per frame: the 8-bit copy EpicFlow's saliency works on divides 16-bit samples by 255 (:472-474, :578)
    std::vector<Mosaic> mosaics;                 // gpu_ingest 1: the decoded mosaics instead of `frames`; the GPUs demosaic, crop and rescale them
    int width = 0, height = 0, stride = 0;       // the frames the solver sees (after crop and rescale), and the row stride of their host images
    const std::vector<FrameRange> &gpu_frames;
    const std::vector<std::vector<char>> &lab_frames_;
    // lab_frames[g][f] (resident_epic; else empty): loaded frame f is the reference frame of one of GPU g's windows
    Sequence(const Run &run, const std::vector<FrameRange> &gpu_frames_, const std::vector<std::vector<char>> &lab_frames, double t_begin)
        : frames(run.layout.frames), maxval(run.layout.frames, 255), mosaics(run.gpu_ingest ? run.layout.frames : 0), gpu_frames(gpu_frames_), lab_frames_(lab_frames), run_(run), t_begin_(t_begin), n_loaded_((int)(run.layout.end_f - run.layout.start_f)),
          frame_ready_(run.layout.frames, 0), have_sums_(n_loaded_, 0), frame_sums_((size_t)6 * n_loaded_, 0.0), gpus_(run.ngpu) {
        for (int g = 0; g < run.ngpu; g++) up_.emplace_back(&Sequence::upload, this, g);
    }
    ~Sequence() { abort(); join(); }
    // frames [f0, f1) are final: publish the size once, then the frames.  Every frame is held against the published size BEFORE it is marked ready: the uploaders copy
    // width x height of the published size out of each frame's buffer, so a smaller frame in the middle of the sequence would be read beyond its end; it is
    // left unpublished and reported through size_mismatch() instead
    void publish(unsigned f0, unsigned f1) {
        {
            std::lock_guard<std::mutex> l(mu_);
            for (unsigned f = f0; f < f1; f++) {
                const color_image_t *im = frames[f].get();
                if (!size_known_) { width = im->width; height = im->height; stride = im->stride; size_known_ = true; }
                if (im->width != width || im->height != height) {
                    if (size_mismatch_.empty())
                        size_mismatch_ = "frames of different sizes: frame " + std::to_string(f) + " of the sequence is " + std::to_string(im->width) + "x" + std::to_string(im->height) +
                                         ", the sequence " + std::to_string(width) + "x" + std::to_string(height);
                    continue;
                }
                frame_ready_[f] = 1;
            }
        }
        cv_.notify_all();
    }
    // gpu_ingest 1: mosaic f is final.  The first one fixes the geometry of the pass: the crop (color_image_crop's ranges) and the rescaled size
    // (color_image_rescale's) follow from the mosaic's size as they do on the host; a mosaic of another size is left unpublished like a frame of another size
    void publish_mosaic(unsigned f) {
        {
            std::lock_guard<std::mutex> l(mu_);
            const Mosaic &m = mosaics[f];
            if (!size_known_ && size_mismatch_.empty()) {
                int cw = m.width, ch = m.height;
                if (run_.crop) {
                    const int x0 = run_.center.x - run_.extent.x / 2, x1 = run_.center.x + run_.extent.x / 2, y0 = run_.center.y - run_.extent.y / 2, y1 = run_.center.y + run_.extent.y / 2;
                    if (x0 < 0 || y0 < 0 || x1 > m.width || y1 > m.height || x1 <= x0 || y1 <= y0)
                        size_mismatch_ = "center / extent do not fit the " + std::to_string(m.width) + "x" + std::to_string(m.height) + " frames";
                    crop_x0_ = x0; crop_y0_ = y0; cw = x1 - x0; ch = y1 - y0;
                }
                src_width_ = cw; src_height_ = ch;
                if (run_.rescale) { cw = (int)lrint((double)cw * run_.scale); ch = (int)lrint((double)ch * run_.scale); }
                if (size_mismatch_.empty() && (cw < 1 || ch < 1)) size_mismatch_ = "scale " + std::to_string(run_.scale) + " leaves no pixel of the frames";
                if (size_mismatch_.empty()) { mosaic_width_ = m.width; mosaic_height_ = m.height; width = cw; height = ch; stride = ((cw + 3) / 4) * 4; size_known_ = true; }
            }
            if (size_known_ && (m.width != mosaic_width_ || m.height != mosaic_height_)) {
                if (size_mismatch_.empty())
                    size_mismatch_ = "frames of different sizes: frame " + std::to_string(f) + " of the sequence is " + std::to_string(m.width) + "x" + std::to_string(m.height) +
                                     ", the sequence " + std::to_string(mosaic_width_) + "x" + std::to_string(mosaic_height_);
            } else if (size_known_) frame_ready_[f] = 1;
        }
        cv_.notify_all();
    }
    string size_mismatch() { std::lock_guard<std::mutex> l(mu_); return size_mismatch_; }
    bool wait_statistics(double avg[3], double sd[3]) {
        const bool ok = wait([&] { return stats_known_; });
        std::copy(avg_, avg_ + 3, avg); std::copy(std_, std_ + 3, sd);
        return ok;
    }
    bool wait_gpu(int g) {                                                           // GPU g's frames are resident and normalised; false if aborted first
        if (!wait([&] { return gpus_[g].ready; })) return false;
        std::lock_guard<std::mutex> l(mu_);
        if (gpus_[g].first_refine_s < 0) gpus_[g].first_refine_s = now_s() - t_begin_;
        return true;
    }
    const Gpu &gpu(int g) const { return gpus_[g]; }                              // resident: after wait_gpu(g); times: once the threads have ended
    // resident_epic: where GPU g's Lab sequence holds the Lab image of loaded frame f (a reference frame of one of its windows): the sequence has one frame
    // per such frame, in frame order
    int lab_slot(int g, int f) const {
        int slot = 0;
        for (int k = 0; k < f; k++) slot += lab_frames_[g][k] != 0;
        return slot;
    }
    bool report_errors() {                                                           // joins the uploaders, prints each GPU's error; true if there was one
        join();
        bool any = false;
        for (int g = 0; g < run_.ngpu; g++)
            if (!gpus_[g].err.empty()) { std::cerr << "GPU " << run_.device_of(g) << ": " << gpus_[g].err << std::endl; any = true; }
        return any;
    }

private:
    template <typename Ready> bool wait(Ready ready) {                               // false once aborted
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return ready() || aborted_; });
        return !aborted_;
    }
    void abort() {
        { std::lock_guard<std::mutex> l(mu_); aborted_ = true; }
        cv_.notify_all();
    }
    void join() { for (auto &t : up_) if (t.joinable()) t.join(); }
    void fail(int g) {                                                               // nobody may wait for this GPU's sums or readiness
        gpus_[g].err = sfa_last_error(gpus_[g].ctx.get());
        abort();
    }
    // GPU g's thread: context, uploads as frames are published, the frames' sums, then the normalisation with the statistics of all frames
    void upload(int g) {
        const FrameRange fr = gpu_frames[g];
        const int n_mine = fr.hi - fr.lo, start_f = (int)run_.layout.start_f;
        Gpu &gpu = gpus_[g];
        gpu.ctx = new_ctx(run_.device_of(g));
        if (!gpu.ctx) return fail(g);
        if (n_mine <= 0 || !wait([&] { return size_known_; })) return;             // more GPUs than windows, or aborted
        sfa_sequence *s = nullptr;
        int rc = sfa_sequence_create(gpu.ctx.get(), width, height, n_mine, &s);
        gpu.resident.reset(s);
        // gpu_ingest 1: the mosaic as it is, demosaiced into the crop (host order: demosaic, crop, rescale); where the frames are rescaled, into a one-frame
        // sequence of the crop's size that sfa_sequence_rescale reads -- one stream, so the next mosaic overwrites it only after that
        DeviceSequence full;
        if (run_.gpu_ingest && run_.rescale && rc == SFA_OK) {
            sfa_sequence *t = nullptr;
            rc = sfa_sequence_create(gpu.ctx.get(), src_width_, src_height_, 1, &t);
            full.reset(t);
        }
        // resident_epic: the Lab image of every reference frame, from the frame as it was read (before the normalisation), at the interpolation's size
        // (:571-573, 578-586: blur and resize by dm_scale, convertTo(CV_8U, norm), rgb_to_lab)
        DeviceSequence dm;
        const int ew = run_.dm_scale != 1 ? (int)std::lrint(width * run_.dm_scale) : width, eh = run_.dm_scale != 1 ? (int)std::lrint(height * run_.dm_scale) : height;
        if (run_.resident_epic && rc == SFA_OK && ew >= 1 && eh >= 1) {
            sfa_sequence *t = nullptr;
            rc = sfa_sequence_create(gpu.ctx.get(), ew, eh, std::max(1, lab_slot(g, (int)lab_frames_[g].size())), &t);
            gpu.lab.reset(t);
            if (rc == SFA_OK && run_.dm_scale != 1) {
                rc = sfa_sequence_create(gpu.ctx.get(), ew, eh, 1, &t);
                dm.reset(t);
            }
        }
        double sent = 0;
        for (int f = fr.lo; f < fr.hi && rc == SFA_OK; f++) {
            if (!wait([&] { return frame_ready_[start_f + f] != 0; })) return;
            if (run_.gpu_ingest) {
                const Mosaic &m = mosaics[start_f + f];
                rc = sfa_sequence_upload_mosaic(full ? full.get() : s, full ? 0 : f - fr.lo, m.data.data(), m.dtype, m.width, m.width, m.height, crop_x0_, crop_y0_, run_.demosaicing,
                                                run_.red_x, run_.red_y);
                if (rc == SFA_OK && full) rc = sfa_sequence_rescale(s, f - fr.lo, full.get(), 0, 1, run_.scale);
                sent += (double)m.data.size();
            } else {
                rc = sfa_sequence_upload(s, f - fr.lo, frames[start_f + f]->c1, frames[start_f + f]->stride);
                sent += (double)3 * width * height * sizeof(float);
            }
            if (rc == SFA_OK && gpu.lab && lab_frames_[g][start_f + f]) {
                if (dm) rc = sfa_sequence_rescale(dm.get(), 0, s, f - fr.lo, 1, (float)run_.dm_scale);
                if (rc == SFA_OK) rc = sfa_sequence_lab(gpu.lab.get(), lab_slot(g, start_f + f), dm ? dm.get() : s, dm ? 0 : f - fr.lo, 1, maxval[start_f + f] > 255 ? 1.0f / 255 : 1.0f);
            }
        }
        std::vector<double> mine((size_t)6 * n_mine);
        if (rc == SFA_OK) rc = sfa_sequence_frame_sums(s, 0, n_mine, mine.data());  // (waits for the uploads: one stream)
        if (rc != SFA_OK) return fail(g);
        {
            std::lock_guard<std::mutex> l(mu_);
            gpu.upload_bytes = sent;
            gpu.upload_done_s = now_s() - t_begin_;
            for (int f = fr.lo; f < fr.hi; f++)
                if (!have_sums_[f]) {                                                // a halo frame: whoever is first; the other GPU's sums are the same bits
                    std::copy(mine.begin() + 6 * (f - fr.lo), mine.begin() + 6 * (f - fr.lo) + 6, frame_sums_.begin() + 6 * f);
                    have_sums_[f] = 1;
                    n_have_++;
                }
            if (n_have_ == n_loaded_ && !stats_known_) {                             // variational_mt.cpp:41-52 over all loaded frames, in frame order
                (void)sfa_normalize_statistics(frame_sums_.data(), n_loaded_, width, height, avg_, std_);
                stats_known_ = true;
            }
        }
        cv_.notify_all();
        if (!wait([&] { return stats_known_; })) return;
        if (sfa_sequence_apply_normalization(s, 0, n_mine, avg_, std_) != SFA_OK) return fail(g);
        { std::lock_guard<std::mutex> l(mu_); gpu.ready = true; gpu.ready_s = now_s() - t_begin_; }
        cv_.notify_all();
    }

    const Run &run_;
    const double t_begin_;
    const int n_loaded_;
    std::mutex mu_;
    std::condition_variable cv_;
    bool size_known_ = false, stats_known_ = false, aborted_ = false;
    int n_have_ = 0;
    string size_mismatch_;
    int mosaic_width_ = 0, mosaic_height_ = 0, crop_x0_ = 0, crop_y0_ = 0, src_width_ = 0, src_height_ = 0;   // gpu_ingest 1: the mosaics, the crop's origin, the frames before the rescaling
    std::vector<char> frame_ready_, have_sums_;
    std::vector<double> frame_sums_;
    double avg_[3] = {0, 0, 0}, std_[3] = {1, 1, 1};
    std::vector<Gpu> gpus_;
    std::vector<std::thread> up_;
};

// ---- read the image sequence (:447-592, without OpenCV: PNG, binary PPM / PGM / PFM): decoded, demosaiced and cropped by the io pool, one frame per task, each published
//      as it is done unless rescaled (blur + resize against aliasing, :550-553, on the GPU: only once all frames are in).  0 or the exit code; decoded_at: end of decoding
static int read_frames(const Run &run, const string &sequence_path, const string &format, Sequence &seq, double &decoded_at) {
    std::vector<string> names(run.layout.frames);
    for (unsigned f = run.layout.start_f; f < run.layout.end_f; f++) {
        names[f] = sequence_frame_name(sequence_path + format, (int)run.start, (int)f * run.skip - run.steps * run.skip, run.sintel);
        std::cout << "Reading " << names[f] << "..." << std::endl;
    }
    std::mutex err_mu;
    string load_error;
    {
        TaskPool pool(run.io_threads);
        for (unsigned f = run.layout.start_f; f < run.layout.end_f; f++)
            pool.submit([&, f] {
                int maxval = 255;
                string error;                                                        // demosaicing (:482-527): the mosaic is the grey image
                if (run.gpu_ingest) {                                                // ... and goes to the GPUs as it is
                    if (!load_mosaic(names[f], &seq.mosaics[f], &error)) { std::lock_guard<std::mutex> l(err_mu); if (load_error.empty()) load_error = error; return; }
                    seq.maxval[f] = seq.mosaics[f].maxval;
                    seq.publish_mosaic(f);
                    return;
                }
                ColorImage img(load_frame(names[f], run.raw, run.demosaicing, run.red_x, run.red_y, &maxval, &error));
                if (img && run.preprocess && (run.extent.x > 0 || run.extent.y > 0)) {   // use only a part of the images (:533-536)
                    ColorImage part(color_image_crop(img.get(), run.center.x, run.center.y, run.extent.x, run.extent.y));
                    if (!part) error = "center / extent do not fit the " + std::to_string(img->width) + "x" + std::to_string(img->height) + " frames";
                    img = std::move(part);
                }
                if (!img) { std::lock_guard<std::mutex> l(err_mu); if (load_error.empty()) load_error = error; return; }
                seq.frames[f] = std::move(img);
                seq.maxval[f] = maxval;
                if (!run.rescale) seq.publish(f, f + 1);
            });
        pool.wait_all();
    }
    if (load_error.empty()) load_error = seq.size_mismatch();
    if (!load_error.empty()) { std::cerr << load_error << std::endl; return 3; }
    decoded_at = now_s();
    if (!run.rescale || run.gpu_ingest) return 0;
    Ctx ctx = new_ctx(run.dev0);
    if (!ctx) { std::cerr << sfa_last_error(nullptr) << std::endl; return 4; }
    for (unsigned f = run.layout.start_f; f < run.layout.end_f; f++) {
        ColorImage small(color_image_rescale(ctx.get(), seq.frames[f].get(), run.scale));
        if (!small) { std::cerr << "rescaling failed: " << sfa_last_error(ctx.get()) << std::endl; return 4; }
        seq.frames[f] = std::move(small);
    }
    seq.publish(run.layout.start_f, run.layout.end_f);
    load_error = seq.size_mismatch();
    if (!load_error.empty()) { std::cerr << load_error << std::endl; return 3; }
    return 0;
}

// ---- ground truth, if the cfg names it (:603-661): .flo -> crop -> nearest resize * scale -> gt/flow_%05i.{png,flo}; 0 or the exit code
static int load_ground_truth(const Run &run, std::vector<Flow> &gt) {
    mkdirs(run.output + "gt/");
    for (unsigned j = run.layout.start_j; j < run.layout.end_j; j++) {
        const string path = sequence_frame_name(run.file_gt, (int)run.start, (int)j * run.steps, run.sintel);
        std::cout << path << std::endl;
        if (!file_exists(path)) continue;
        image_t **g = readFlowFile(path.c_str());
        if (!g) { std::cout << "No gt flow for frame " << std::endl; continue; }
        gt[j] = Flow(Image(g[0]), Image(g[1]));
        free(g);
        for (Image *c : {&gt[j].first, &gt[j].second}) {
            if (run.center.x > 0) {                                                  // crop like the frames (:634-637)
                const int x0 = run.center.x - run.extent.x / 2, y0 = run.center.y - run.extent.y / 2;
                const int cw = 2 * (run.extent.x / 2), chh = 2 * (run.extent.y / 2);
                if (x0 < 0 || y0 < 0 || x0 + cw > (*c)->width || y0 + chh > (*c)->height) { std::cerr << "center / extent do not fit the ground truth" << std::endl; return 3; }
                Image part = zero_image(cw, chh);
                for (int y = 0; y < chh; y++) memcpy(part->data + (size_t)y * part->stride, (*c)->data + (size_t)(y0 + y) * (*c)->stride + x0, sizeof(float) * cw);
                *c = std::move(part);
            }
            c->reset(flow_resize_nearest(c->get(), run.scale));                      // nearest, not linear: motion discontinuities (:640-641)
        }
        const string base = run.output + "gt/" + fmt1("flow_%05i", (int)run.start + (int)j * run.steps);
        png_write((base + ".png").c_str(), flowColorImg(gt[j].first.get(), gt[j].second.get(), run.verbose_changes));
        writeFlowFile((base + ".flo").c_str(), gt[j].first.get(), gt[j].second.get());
    }
    return 0;
}

struct EpicInit { Image wx, wy; int rc = SFA_OK, er = 0; };     // the initial flow of one window (deep_matching 1); er: what epic() returned for it (1: no match left, zeros)
// what epic() reads for one window: the matches, the edge map and the L*a*b* frame at the interpolation's resolution ew x eh
struct EpicInput { epic_matches mt; epic_edges ed; ColorImage lab; int ew = 0, eh = 0; };
static epic_params_t driver_epic_params() {
    epic_params_t ep;
    epic_params_default(&ep);
    ep.pref_nn = 25; ep.nn = 160; ep.coef_kernel = 1.1f;         // :271-275
    return ep;
}

// the match and edge files of one window, read at the interpolation's size ew x eh; SFA_OK or the error
static int epic_files(const Run &run, const Sequence &seq, const Window &wd, std::mutex &io_mu, epic_matches &mt, epic_edges &ed, int *ew_out, int *eh_out) {
    const int width = seq.width, height = seq.height;
    const double dm_scale = run.dm_scale;
    const JetFrames n = jet_frames(run.start, wd.jet, run.steps, run.skip);
    const int a = n.from, b = n.to;
    // the resolution the interpolation runs at: cv::resize(img, img, Size(0, 0), dm_scale, dm_scale) makes cvRound(cols * dm_scale) x cvRound(rows * dm_scale)
    const int ew = dm_scale != 1 ? (int)std::lrint(width * dm_scale) : width, eh = dm_scale != 1 ? (int)std::lrint(height * dm_scale) : height;
    // ... while the reference allocates un_seq / wx and sizes the edge file with the TRUNCATED product (`color_image_new(width*dm_scale, height*dm_scale)`,
    // slow_flow.cpp:584, :801-806).  Where the two differ (1023 * 0.5: 512 against 511) the reference copies a 512-wide image into a 511-wide one -- no defined
    // result, and edge / match files laid out for either width would be misread by the other: refused by name
    if (dm_scale != 1 && (ew != (int)(width * dm_scale) || eh != (int)(height * dm_scale))) {
        std::lock_guard<std::mutex> l(io_mu);
        std::cerr << "dm_scale " << dm_scale << ": " << width << " x " << height << " frames give a rescaled image of " << ew << " x " << eh << " (cv::resize rounds) but buffers and edge files of "
                  << (int)(width * dm_scale) << " x " << (int)(height * dm_scale) << " (slow_flow.cpp:584 truncates): the reference has no defined result here; crop the frames to a multiple of 1 / dm_scale"
                  << std::endl;
        return SFA_ERR_ARG;
    }
    if (ew < 1 || eh < 1 || !read_matches((wd.backward ? matches_file(run, b, a) : matches_file(run, a, b)).c_str(), mt) ||
        !read_edges((wd.backward ? edges_file(run, b) : edges_file(run, a)).c_str(), ew, eh, ed)) return SFA_ERR_ARG;
    *ew_out = ew; *eh_out = eh;
    return SFA_OK;
}

// the inputs of EpicFlow's interpolation of the matches of one window (:801-863 / :960-1004); SFA_OK or the error
static int epic_inputs(const Run &run, const Sequence &seq, const Window &wd, sfa_ctx *ctx, std::mutex &io_mu, EpicInput &in) {
    const double dm_scale = run.dm_scale;
    const int fi = window_tap(wd.jet, wd.backward, run.steps, run.steps, 0);   // fi: un_im[ref] / un_im_back[ref], the reference frame, not normalised
    const color_image_t *un_ref = seq.frames[fi].get();
    int ew = 0, eh = 0;
    const int frc = epic_files(run, seq, wd, io_mu, in.mt, in.ed, &ew, &eh);
    if (frc != SFA_OK) return frc;
    // the reference hands epic() un_seq: the frame after img.convertTo(CV_8U, norm), i.e. rounded to nearest and saturated to 0..255,
    // 16-bit samples scaled by 1/255 first (slow_flow.cpp:472-474, :578-586) -- not the float frame the refinement reads
    // :571-573: GaussianBlur(sigma = 1 / sqrt(2 dm_scale), BORDER_REPLICATE) then resize by dm_scale, on the float frame (the pyramid's two
    // operators: sfa_gaussian_blur, sfa_resize_linear_fx with cv::resize's fx / fy form of the coordinate scale)
    ColorImage small;
    if (dm_scale != 1) {
        small.reset(color_image_new(ew, eh));
        std::vector<float> tmp((size_t)un_ref->stride * un_ref->height);
        const float sigma = (float)(1 / sqrt(2 * dm_scale));
        float *src3[3] = {un_ref->c1, un_ref->c2, un_ref->c3}, *dst3[3] = {small->c1, small->c2, small->c3};
        for (int ch = 0; ch < 3; ch++) {
            int rc = sfa_gaussian_blur(ctx, tmp.data(), src3[ch], un_ref->width, un_ref->height, un_ref->stride, sigma);
            if (rc == SFA_OK) rc = sfa_resize_linear_fx(ctx, dst3[ch], ew, eh, small->stride, tmp.data(), un_ref->width, un_ref->height, un_ref->stride, dm_scale, dm_scale);
            if (rc != SFA_OK) return rc;
        }
    }
    const color_image_t *un_src = small ? small.get() : un_ref;
    in.lab.reset(rgb8_to_lab(un_src, seq.maxval[fi] > 255 ? 1.0f / 255 : 1.0f));
    in.ew = ew; in.eh = eh;
    return SFA_OK;
}

// a field of ew x eh for frames whose width is less than twice ew: the reference would hand a field of the reduced size to a solver of the frames' size
// (1 < width ratio < 2): it has no defined result, refused by name
static bool reduced_field_kept(const Run &run, const Sequence &seq, int ew, int eh, std::mutex &io_mu) {
    if (seq.width / ew != 1 || (ew == seq.width && eh == seq.height)) return false;
    std::lock_guard<std::mutex> l(io_mu);
    std::cerr << "dm_scale " << run.dm_scale << ": the frames are " << seq.width << " wide, the interpolation " << ew << " -- the reference rescales by the integer ratio "
              << seq.width / ew << " (slow_flow.cpp:827) and would keep the reduced field; use a dm_scale of 1 / n" << std::endl;
    return true;
}

// epic()'s field wx, wy (ew x eh; er: what epic() returned for it) -> the window's initial flow per single frame step; SFA_OK or the error
static int epic_to_initial_flow(const Run &run, const Sequence &seq, const Window &wd, sfa_ctx *ctx, std::mutex &io_mu, int er, Image &wx, Image &wy) {
    const int width = seq.width, height = seq.height, ew = wx->width, eh = wx->height;
    const int a = jet_frames(run.start, wd.jet, run.steps, run.skip).from;
    if (er < 0) return SFA_ERR_HIP;
    if (er > 0) { image_erase(wx.get()); image_erase(wy.get()); }                   // no usable match: start from zero like deep_matching 0
    // :826-843: rescale flow.  fx, fy are quotients of ints; only when fx != 1 is the field resized (cv::resize to the frame's size: the ratio form)
    const float fx = (float)(width / ew), fy = (float)(height / eh);
    if (fx != 1) {
        Image fwx(image_new(width, height)), fwy(image_new(width, height));
        int rc = sfa_resize_linear(ctx, fwx->data, width, height, fwx->stride, wx->data, ew, eh, wx->stride);
        if (rc == SFA_OK) rc = sfa_resize_linear(ctx, fwy->data, width, height, fwy->stride, wy->data, ew, eh, wy->stride);
        if (rc != SFA_OK) return rc;
        wx = std::move(fwx); wy = std::move(fwy);
    } else if (reduced_field_kept(run, seq, ew, eh, io_mu)) {
        return SFA_ERR_ARG;
    }
    image_mul_scalar(wx.get(), fx / run.steps);                                      // :842-843
    image_mul_scalar(wy.get(), fy / run.steps);
    if (run.write_files && !wd.backward)                                             // :845-858
        png_write((run.output + "tmp/frame_" + std::to_string(a) + "_INIT.png").c_str(), flowColorImg(wx.get(), wy.get(), 0));
    return SFA_OK;
}

// EpicFlow's interpolation of the matches of one window, per single frame step, into wx, wy; SFA_OK or the error
static int interpolate_matches(const Run &run, const Sequence &seq, const Window &wd, sfa_ctx *ctx, std::mutex &io_mu, Image &wx, Image &wy, int *er) {
    EpicInput in;
    const int rc = epic_inputs(run, seq, wd, ctx, io_mu, in);
    if (rc != SFA_OK) return rc;
    const epic_params_t ep = driver_epic_params();
    wx = zero_image(in.ew, in.eh); wy = zero_image(in.ew, in.eh);
    *er = epic(ctx, wx.get(), wy.get(), in.lab.get(), in.mt, in.ed, &ep);
    return epic_to_initial_flow(run, seq, wd, ctx, io_mu, *er, wx, wy);
}

// the same for the windows [b0, b0 + v.size()) of `mine` at once, through epic_batch: the graph searches of the whole batch in two GPU calls (gpu_epic 1)
static void interpolate_matches_batch(const Run &run, const Sequence &seq, const std::vector<Window> &todo, const std::vector<size_t> &mine, size_t b0, sfa_ctx *ctx,
                                      std::mutex &io_mu, std::vector<EpicInit> &v) {
    std::vector<EpicInput> in(v.size());
    std::vector<int> use;                                                            // the windows whose inputs are there
    for (size_t e = 0; e < v.size(); e++)
        if ((v[e].rc = epic_inputs(run, seq, todo[mine[b0 + e]], ctx, io_mu, in[e])) == SFA_OK) {
            v[e].wx = zero_image(in[e].ew, in[e].eh); v[e].wy = zero_image(in[e].ew, in[e].eh);
            use.push_back((int)e);
        }
    std::vector<image_t *> fx, fy;
    std::vector<const color_image_t *> lab;
    std::vector<const epic_matches *> mt;
    std::vector<epic_edges *> ed;
    for (int e : use) { fx.push_back(v[e].wx.get()); fy.push_back(v[e].wy.get()); lab.push_back(in[e].lab.get()); mt.push_back(&in[e].mt); ed.push_back(&in[e].ed); }
    std::vector<int> er(use.size());
    const epic_params_t ep = driver_epic_params();
    epic_batch(ctx, (int)use.size(), fx.data(), fy.data(), lab.data(), mt.data(), ed.data(), &ep, er.data());
    for (size_t k = 0; k < use.size(); k++) v[use[k]].er = er[k];
    for (size_t k = 0; k < use.size(); k++) v[use[k]].rc = epic_to_initial_flow(run, seq, todo[mine[b0 + use[k]]], ctx, io_mu, er[k], v[use[k]].wx, v[use[k]].wy);
}

// everything a finished window hands to the output pool
struct WindowResult {
    size_t index = 0;                            // into todo
    Image wx, wy, occ;
    std::vector<Image> alt_occ;                  // labels after alternation 1 .. niter_alter-1 (WRITE_FILES verbosity)
};

// a finished window, off the GPU worker's thread: flow * steps -> .flo, colour PNG, EPE / AAE against a ground truth of the frames' size, occlusion images; false on a write error
static bool emit(const Run &run, Window &wd, WindowResult &r, const Flow &gt, int width, int height) {
    image_mul_scalar(r.wx.get(), (float)run.steps);                                  // :908-909
    image_mul_scalar(r.wy.get(), (float)run.steps);
    bool ok = writeFlowFile(wd.out.c_str(), r.wx.get(), r.wy.get()) == 0;
    const string fnum = std::to_string(jet_frames(run.start, wd.jet, run.steps, run.skip).from);
    if (ok && !wd.backward) {                                                        // the flow as a colour image next to the .flo (:913-925)
        ok = png_write((run.output + "frame_" + fnum + ".png").c_str(), flowColorImg(r.wx.get(), r.wy.get(), 0));
        if (gt.first && gt.first->width == width && gt.first->height == height) {    // additive: error against the ground truth, reported in timings.json
            wd.epe = computeEPE(r.wx.get(), r.wy.get(), gt.first.get(), gt.second.get());
            wd.aae = computeAAE(r.wx.get(), r.wy.get(), gt.first.get(), gt.second.get());
        }
    }
    // the occlusion estimate of the forward window (:892-905; the reference writes a binary PXM named .pbm through OpenCV, here the
    // same 8-bit grey map as PGM) and, with WRITE_FILES verbosity, the labels after every alternation (:878-884 -> variational_mt.cpp:275-285)
    if (ok && r.occ) ok = writePGM((run.output + "occlusion/frame_" + fnum + ".pgm").c_str(), r.occ.get(), 1.0f, 127.5f) == 0;
    for (size_t a = 0; ok && a < r.alt_occ.size(); a++)
        ok = png_write((run.output + "tmp/frame_" + fnum + "_" + std::to_string(a + 1) + ".png").c_str(), occlusion_image(r.alt_occ[a].get()));
    return ok;
}

// what the refinement workers and the output pool share: the pass's inputs, the window list they fill in, and where they report
struct Refinement {
    const Run &run;
    Sequence &seq;
    const color_image_t *channel_weights;
    const std::vector<Flow> &gt;
    std::vector<Window> &todo;
    TaskPool &out_pool;
    std::mutex io_mu;
    std::atomic<bool> failed;
    std::atomic<int> init_from_matches, init_from_zero;   // deep_matching 1: the windows whose interpolation gave a field (epic() returned 0) / had no match left (1)
    int search_mode;                             // resident_epic: the search mode of the contexts the epic jobs ran on (-1: none ran), and sfa_epic_nn_search_info summed over their runs
    long long search_info[4];
    std::mutex lab_mu;                           // resident_epic: a GPU's Lab sequence lives on its uploader's context, which takes one caller at a time
    void fail(const string &message) {           // on stderr; the pass ends with exit code 5
        std::lock_guard<std::mutex> l(io_mu);
        std::cerr << message << std::endl;
        failed = true;
    }
};

// resident_epic: what the match and edge files of one window hold
struct EpicFiles { epic_matches mt; epic_edges ed; int ew = 0, eh = 0, rc = SFA_OK; };
static sfa_epic_params library_epic_params(const epic_params_t &ep) {
    sfa_epic_params p;
    p.method = strcmp(ep.method, "LA") ? 1 : 0; p.saliency_th = ep.saliency_th; p.pref_nn = ep.pref_nn; p.pref_th = ep.pref_th; p.nn = ep.nn;
    p.coef_kernel = ep.coef_kernel; p.euc = ep.euc;
    return p;
}

// resident_epic: the fields of a batch's windows on the worker's context -- the files' matches and edges go up, the Lab frames come from the GPU's Lab
// sequence, sfa_epic_job_run interpolates; an image the run flags takes epic() of the host on its Lab frame, downloaded (the same bits), and its field goes
// back into the epic job.  `lab_index[e]`: window e's reference frame in the Lab sequence.  SFA_OK or the error
static int resident_epic_fields(Refinement &rf, const WorkerPlan &wp, sfa_ctx *ctx, sfa_ctx *ectx, EpicJob &ejob, int &ejob_n, std::vector<EpicFiles> &files,
                                const std::vector<int> &lab_index) {
    const Run &run = rf.run;
    const int nb = (int)files.size(), ew = files[0].ew, eh = files[0].eh;
    for (const EpicFiles &f : files)
        if (f.rc != SFA_OK) return f.rc;
    if (reduced_field_kept(run, rf.seq, ew, eh, rf.io_mu)) return SFA_ERR_ARG;
    const epic_params_t ep = driver_epic_params();
    int rc = SFA_OK;
    if (!ejob || ejob_n != nb) {
        ejob.reset();
        const sfa_epic_params lp = library_epic_params(ep);
        sfa_epic_job *j = nullptr;
        rc = sfa_epic_job_create(ctx, &lp, ew, eh, nb, &j);
        ejob.reset(j);
        ejob_n = nb;
    }
    for (int e = 0; e < nb && rc == SFA_OK; e++) rc = sfa_epic_job_upload(ejob.get(), e, files[e].mt.m.data(), files[e].mt.count(), files[e].ed.cost.data());
    sfa_sequence *lab_seq = rf.seq.gpu(wp.gpu).lab.get();
    if (rc == SFA_OK) rc = sfa_epic_job_set_lab(ejob.get(), 0, nb, lab_seq, lab_index.data());
    std::vector<int> er(nb, 0), status(nb, 0);
    if (rc == SFA_OK) rc = sfa_epic_job_run(ejob.get(), nb, er.data(), nullptr, 0, status.data());
    long long info[4] = {0, 0, 0, 0};                                                // the last search of the run, as the library counted it
    if (rc == SFA_OK) rc = sfa_epic_nn_search_info(ctx, info);
    if (rc == SFA_OK) {
        std::lock_guard<std::mutex> l(rf.lab_mu);
        rf.search_mode = run.gpu_epic_search;                                        // (set on `ctx` by refine_worker before its first batch)
        for (int k = 0; k < 3; k++) rf.search_info[k] += info[k];
        rf.search_info[3] = std::max(rf.search_info[3], info[3]);
    }
    for (int e = 0; e < nb && rc == SFA_OK; e++) {
        if (status[e]) {                                                             // does not fit the interpolation's workspace even alone: the host's epic()
            ColorImage lab(color_image_new(ew, eh));
            {
                std::lock_guard<std::mutex> l(rf.lab_mu);
                rc = sfa_sequence_download(lab_seq, lab_index[e], lab->c1, lab->stride);
            }
            Image wx = zero_image(ew, eh), wy = zero_image(ew, eh);
            if (rc == SFA_OK) er[e] = epic(ectx, wx.get(), wy.get(), lab.get(), files[e].mt, files[e].ed, &ep);
            if (rc == SFA_OK && er[e] < 0) rc = SFA_ERR_HIP;
            if (rc == SFA_OK && er[e] > 0) { image_erase(wx.get()); image_erase(wy.get()); }
            if (rc == SFA_OK) rc = sfa_epic_job_upload_flow(ejob.get(), e, wx->data, wy->data, wx->stride);
        }
        if (rc == SFA_OK) (er[e] == 0 ? rf.init_from_matches : rf.init_from_zero)++;
    }
    return rc;
}

// the windows `mine` of one worker in lockstep batches of gpu_batch on ONE resident job (re-created only for a shorter last batch); with deep_matching 1 the initial flows are
// prepared one batch ahead on a helper thread (ectx: the library's contexts are thread-compatible, not thread-safe); the results go to the output pool meanwhile
static void refine_windows(Refinement &rf, const WorkerPlan &wp, sfa_ctx *ctx, sfa_ctx *ectx, const sfa_params &sp, const std::vector<size_t> &mine) {
    const Run &run = rf.run;
    const int device = run.device_of(wp.gpu), width = rf.seq.width, height = rf.seq.height, F = 2 * run.steps + 1;
    const int first = (int)run.layout.start_f + rf.seq.gpu_frames[wp.gpu].lo;       // the GPU's resident sequence starts at this frame
    Job job;
    int job_nb = 0, rc = SFA_OK;
    auto batch_inits = [&](size_t b0) {
        std::vector<EpicInit> v(std::min((size_t)run.batch, mine.size() - b0));
        if (run.gpu_epic) interpolate_matches_batch(run, rf.seq, rf.todo, mine, b0, ectx, rf.io_mu, v);
        for (size_t e = 0; e < v.size(); e++)
            if ((run.gpu_epic ? v[e].rc : v[e].rc = interpolate_matches(run, rf.seq, rf.todo[mine[b0 + e]], ectx, rf.io_mu, v[e].wx, v[e].wy, &v[e].er)) != SFA_OK) {
                std::lock_guard<std::mutex> l(rf.io_mu);
                std::cerr << "EpicFlow initialisation of jet " << rf.todo[mine[b0 + e]].jet << " failed" << std::endl;
            }
        return v;
    };
    // resident_epic: only the files are read ahead (the helper touches no GPU); the interpolation runs on the worker's own context, whose stream orders it
    // before sfa_job_set_flow_epic
    auto batch_files = [&](size_t b0) {
        std::vector<EpicFiles> v(std::min((size_t)run.batch, mine.size() - b0));
        for (size_t e = 0; e < v.size(); e++)
            if ((v[e].rc = epic_files(run, rf.seq, rf.todo[mine[b0 + e]], rf.io_mu, v[e].mt, v[e].ed, &v[e].ew, &v[e].eh)) != SFA_OK) {
                std::lock_guard<std::mutex> l(rf.io_mu);
                std::cerr << "EpicFlow initialisation of jet " << rf.todo[mine[b0 + e]].jet << " failed" << std::endl;
            }
        return v;
    };
    EpicJob ejob;
    int ejob_n = 0;
    std::future<std::vector<EpicInit>> next_inits;                                   // (a batch prepared ahead and not used is released with it)
    std::future<std::vector<EpicFiles>> next_files;
    if (run.resident_epic) next_files = std::async(std::launch::async, batch_files, (size_t)0);
    else if (run.deep_matching) next_inits = std::async(std::launch::async, batch_inits, (size_t)0);
    for (size_t b0 = 0; b0 < mine.size() && rc == SFA_OK && !rf.failed; b0 += run.batch) {
        const int nb = (int)std::min((size_t)run.batch, mine.size() - b0);
        std::vector<EpicInit> inits;
        std::vector<EpicFiles> files;
        if (run.resident_epic) {
            files = next_files.get();
            if (b0 + run.batch < mine.size()) next_files = std::async(std::launch::async, batch_files, b0 + run.batch);
        } else if (run.deep_matching) {
            inits = next_inits.get();
            if (b0 + run.batch < mine.size()) next_inits = std::async(std::launch::async, batch_inits, b0 + run.batch);
        }
        const double t0 = now_s();
        if (!job || job_nb != nb) {
            job.reset();
            sfa_job *j = nullptr;
            rc = sfa_job_create(ctx, &sp, width, height, nb, &j);
            job.reset(j);
            job_nb = nb;
            if (rc == SFA_OK && run.out_alt_occ) rc = sfa_job_keep_alternation_occlusions(j, 1);
        }
        if (rc == SFA_OK && run.resident_epic) {
            std::vector<int> lab_index(nb);
            for (int e = 0; e < nb; e++) lab_index[e] = rf.seq.lab_slot(wp.gpu, window_tap(rf.todo[mine[b0 + e]].jet, rf.todo[mine[b0 + e]].backward, run.steps, run.steps, 0));
            rc = resident_epic_fields(rf, wp, ctx, ectx, ejob, ejob_n, files, lab_index);
        }
        for (int e = 0; e < nb && rc == SFA_OK; e++) {
            const Window &wd = rf.todo[mine[b0 + e]];
            std::vector<int> idx(F);
            for (int k = 0; k < F; k++) idx[k] = window_tap(wd.jet, wd.backward, run.steps, k, first);
            const color_image_t *cw = rf.channel_weights;                            // (null with gpu_ingest 1)
            const float *chw[3] = {cw ? cw->c1 : nullptr, cw ? cw->c2 : nullptr, cw ? cw->c3 : nullptr};
            const bool host_init = run.deep_matching && !run.resident_epic;          // resident_epic: NULL here, sfa_job_set_flow_epic below
            const image_t *iwx = host_init ? inits[e].wx.get() : nullptr, *iwy = host_init ? inits[e].wy.get() : nullptr;
            if (host_init) rc = inits[e].rc;
            if (host_init && rc == SFA_OK) (inits[e].er == 0 ? rf.init_from_matches : rf.init_from_zero)++;
            // only the forward solver gets the channel weights (:876 vs :1018); without raw weighting they are all ones (:597-598), which is
            // what a NULL pointer means to the library (x * 1.0f is exact: same bits, three planes less to read per pixel)
            if (rc == SFA_OK)
                rc = sfa_job_upload_resident(job.get(), e, rf.seq.gpu(wp.gpu).resident.get(), idx.data(), F, iwx ? iwx->data : nullptr, iwy ? iwy->data : nullptr,
                                             rf.seq.stride, (wd.backward || !run.raw || run.gpu_ingest) ? nullptr : chw);
            // gpu_ingest 1: the same weights, formed on the GPU (after the upload, which sets the window's weights to ones).  raw_weight 1 gives
            // all ones (rawWeighting: weight 1, the others 0.5 * (3 - 1)), which is what the NULL above already means: no planes, same bits
            if (rc == SFA_OK && run.gpu_ingest && !wd.backward && run.raw_weight != 1.0f) rc = sfa_job_set_raw_weights(job.get(), e, 1, run.red_x, run.red_y, run.raw_weight);
        }
        if (rc == SFA_OK && run.resident_epic) {                                     // epic_to_initial_flow on the GPU: fx / steps, fy / steps (:826-843)
            const float fx = (float)(width / files[0].ew), fy = (float)(height / files[0].eh);
            rc = sfa_job_set_flow_epic(job.get(), 0, nb, ejob.get(), 0, fx / run.steps, fy / run.steps);
        }
        if (rc == SFA_OK) rc = sfa_job_run(job.get());
        std::vector<std::shared_ptr<WindowResult>> results;
        for (int e = 0; e < nb && rc == SFA_OK; e++) {
            const bool forward = !rf.todo[mine[b0 + e]].backward;
            std::shared_ptr<WindowResult> r(new WindowResult());
            r->index = mine[b0 + e];
            r->wx = zero_image(width, height); r->wy = zero_image(width, height);
            float change[2];
            rc = sfa_job_download(job.get(), e, r->wx->data, r->wy->data, r->wx->stride, change);
            if (rc == SFA_OK && run.out_occ && forward) {                           // getOcclusions() of the forward solver (:893)
                r->occ = zero_image(width, height);
                rc = sfa_job_download_occlusions(job.get(), e, r->occ->data, r->occ->stride);
            }
            for (int a = 1; a < sp.niter_alter && rc == SFA_OK && run.out_alt_occ && forward; a++) {
                r->alt_occ.push_back(zero_image(width, height));
                rc = sfa_job_download_alternation_occlusions(job.get(), e, a, r->alt_occ.back()->data, r->alt_occ.back()->stride);
            }
            results.push_back(r);
        }
        const double secs = now_s() - t0;
        if (rc != SFA_OK) { rf.fail("GPU " + std::to_string(device) + ": " + sfa_last_error(ctx)); break; }
        for (auto &r : results) {
            Window &wd = rf.todo[r->index];
            wd.seconds = secs / nb;
            wd.gpu = device;
            rf.out_pool.submit([&rf, &wd, r] { if (!emit(rf.run, wd, *r, rf.gt[wd.jet], rf.seq.width, rf.seq.height)) rf.fail("cannot write the results of " + wd.out); });
        }
        std::lock_guard<std::mutex> l(rf.io_mu);
        for (int e = 0; e < nb; e++) {
            const Window &wd = rf.todo[mine[b0 + e]];
            const JetFrames n = jet_frames(run.start, wd.jet, run.steps, run.skip);
            std::cout << (wd.backward ? "Backward" : "Forward") << " flow from frame " << n.from << " to " << n.to
                      << " finished! (GPU " << wp.gpu << " = device " << device << ", " << secs / nb << " s per window in a batch of " << nb << ")" << std::endl;
        }
    }
}

// one worker: its contexts, then its windows once its GPU's frames are resident -- forward and backward windows share one lockstep job (the channel weights
// are per window) unless the backward solver runs with different parameters ("method forward", :1019-1020): then one pass per direction
static void refine_worker(Refinement &rf, const WorkerPlan &wp) {
    if (wp.lo >= wp.hi) return;
    const Run &run = rf.run;
    const Ctx ctx = new_ctx(run.device_of(wp.gpu));
    const Ctx ectx = ctx && run.deep_matching ? new_ctx(run.device_of(wp.gpu)) : Ctx();   // the EpicFlow helper's context (deep_matching 1 only)
    if (!ctx || (run.deep_matching && !ectx)) return rf.fail(sfa_last_error(nullptr));
    (void)sfa_ctx_set_verbose(ctx.get(), run.verbose_changes ? 1 : 0);
    // gpu_epic_search 1: on the context that runs the interpolation's searches -- the helper's, and on the resident route the worker's own (which also keeps
    // the helper's for the host epic() of an image the run flags)
    if (ectx && run.gpu_epic && run.gpu_epic_search && sfa_ctx_set_epic_search(ectx.get(), SFA_EPIC_SEARCH_COMPACT) != SFA_OK) return rf.fail(sfa_last_error(ectx.get()));
    if (run.resident_epic && run.gpu_epic_search && sfa_ctx_set_epic_search(ctx.get(), SFA_EPIC_SEARCH_COMPACT) != SFA_OK) return rf.fail(sfa_last_error(ctx.get()));
    if (!rf.seq.wait_gpu(wp.gpu)) { rf.failed = true; return; }
    ParameterList tp(run.p);                                                         // one copy per thread (:708), with the published normalisation
    for (int dirpass = 0; dirpass < (run.forward_only ? 2 : 1) && !rf.failed; dirpass++) {
        std::vector<size_t> mine;
        for (size_t i = wp.lo; i < wp.hi; i++)
            if (!run.forward_only || (int)rf.todo[i].backward == dirpass) mine.push_back(i);
        if (!mine.empty()) refine_windows(rf, wp, ctx.get(), ectx.get(), sfa_params_from_cfg(tp, dirpass == 1), mine);
    }
}

// the gathered per-window timings (the only cross-GPU exchange of the path) and where the wall time of the run went (seconds)
static void write_timings(const Run &run, const std::vector<Window> &todo, const Sequence &seq, const Refinement &rf, double decode, double normalize, double ingest, double refine, double total) {
    std::ofstream tj((run.output + "timings.json").c_str());
    tj << "[";
    for (size_t i = 0; i < todo.size(); i++)
        tj << (i ? "," : "") << "\n  {\"jet\": " << todo[i].jet << ", \"direction\": \"" << (todo[i].backward ? "backward" : "forward") << "\", \"gpu\": " << todo[i].gpu
           << ", \"seconds\": " << todo[i].seconds << ", \"ingest\": \"" << (run.gpu_ingest ? "gpu" : "host") << "\", \"flo\": \"" << todo[i].out << "\""
           << (todo[i].epe >= 0 ? ", \"epe\": " + std::to_string(todo[i].epe) + ", \"aae\": " + std::to_string(todo[i].aae) : string()) << "}";
    tj << "\n]\n";
    std::ofstream rj((run.output + "run.json").c_str());
    rj << "{\"windows\": " << todo.size() << ", \"gpus\": " << run.ngpu << ", \"streams\": " << run.streams << ", \"batch\": " << run.batch << ", \"io_threads\": " << run.io_threads
       << ", \"ingest_path\": \"" << (run.gpu_ingest ? "gpu" : "host") << "\", \"gpu_epic_search\": " << run.gpu_epic_search << ", \"epic_init_path\": \"" << (run.resident_epic ? "resident" : "host") << "\", \"epic_init_from_matches\": " << rf.init_from_matches
       << ", \"epic_init_from_zero\": " << rf.init_from_zero << ", \"epic_init_search\": {\"mode\": " << rf.search_mode << ", \"slices\": " << rf.search_info[0] << ", \"dense\": " << rf.search_info[1]
       << ", \"sparse\": " << rf.search_info[2] << ", \"workspace_bytes\": " << rf.search_info[3] << "}" << ", \"decode_seconds\": " << decode << ", \"normalize_seconds\": " << normalize << ", \"ingest_seconds\": " << ingest << ", \"refine_seconds\": " << refine << ", \"total_seconds\": " << total;
    // per GPU: the frames it was sent (its windows' frames + halo), when the last of them had arrived, when its frames were normalised and when its first worker
    // began to refine -- all in seconds since the run began.  The whole sequence is "sequence_bytes"
    double last_upload = 0, first_refine = -1;
    rj << ", \"sequence_bytes\": " << (double)(run.layout.end_f - run.layout.start_f) * 3 * seq.width * seq.height * sizeof(float) << ", \"per_gpu\": [";   // (resident; gpu_ingest 1 sends less: upload_bytes)
    for (int g = 0; g < run.ngpu; g++) {
        const Sequence::Gpu &t = seq.gpu(g);
        rj << (g ? ", " : "") << "{\"gpu\": " << g << ", \"device\": " << run.device_of(g) << ", \"frames\": [" << seq.gpu_frames[g].lo << ", " << seq.gpu_frames[g].hi << "], \"upload_bytes\": " << t.upload_bytes
           << ", \"upload_done_s\": " << t.upload_done_s << ", \"ready_s\": " << t.ready_s << ", \"first_refine_s\": " << t.first_refine_s << "}";
        last_upload = std::max(last_upload, t.upload_done_s);
        if (t.first_refine_s >= 0 && (first_refine < 0 || t.first_refine_s < first_refine)) first_refine = t.first_refine_s;
    }
    rj << "], \"first_refine_s\": " << first_refine << ", \"last_upload_done_s\": " << last_upload << "}\n";
}

// One pass over the sequence at one frame rate: the body of the reference's adFR loop (slow_flow.cpp:367-1060), stage by stage
static int run_sequence(ParameterList &params, const string &sequence_path, const string &format, int skip, const RunOptions &opt) {
    const double t_begin = now_s();
    const Run run(params, format, skip, opt);
    if (run.batch < 1 || run.batch > 128) {                                          // a job's windows-still-iterating mask is two 64-bit words: refused by name, not clamped
        std::cerr << "gpu_batch " << run.batch << " is out of range: a lockstep job takes 1 .. 128 windows (more windows run as several jobs: gpu_streams, batches per worker)" << std::endl;
        return 2;
    }
    if (run.gpu_ingest) {                                                            // the runs that need the RGB frames on the host: refused by name, never a silent host path
        const char *why = !run.raw ? "raw 0: the frames are no mosaics, there is nothing to demosaic on the GPU"
                          : run.deep_matching && !run.gpu_epic ? "deep_matching 1: EpicFlow's initialisation reads the RGB frames on the host unless gpu_epic 1 keeps it on the GPU (set gpu_epic 1)"
                          : run.write_files ? "verbose: this verbosity writes sequence/frame_*.png and the tmp/ images from the RGB frames on the host"
                                            : nullptr;
        if (why) { std::cerr << "gpu_ingest 1 is refused with " << why << "; set gpu_ingest 0" << std::endl; return 1; }
    }
    mkdirs(run.output);
    if (run.layout.start_f > run.layout.end_f) return 0;
    if (run.deep_matching && !deep_matching_inputs_exist(run, opt.resume_frame)) return 2;
    if (run.ndev <= 0) { std::cerr << "no HIP device: slowflow_amd has no CPU fallback" << std::endl; return 4; }
    if (!run.oversubscribe && run.dev0 >= run.ndev) { std::cerr << "gpu_device " << run.dev0 << " does not exist (" << run.ndev << " device(s))" << std::endl; return 4; }

    // the windows and who refines them -- known before a frame is read, so that every GPU is sent only the frames ITS windows read
    std::vector<Window> todo = windows_to_refine(run, opt.resume_frame);
    const std::vector<WorkerPlan> plan = plan_workers(todo.size(), run.ngpu, run.streams);
    std::vector<std::pair<int, int>> spans;                                          // relative to the loaded range [start_f, end_f)
    for (const Window &wd : todo) spans.push_back(window_span(wd.jet, wd.backward, run.steps, (int)run.layout.start_f));
    const std::vector<FrameRange> gpu_frames = plan_frames(spans, plan, run.ngpu, (int)(run.layout.end_f - run.layout.start_f));

    // resident_epic: the frames whose Lab image a GPU needs -- the reference frames of its windows (un_seq[ref], :809)
    std::vector<std::vector<char>> lab_frames(run.resident_epic ? run.ngpu : 0, std::vector<char>(run.layout.frames, 0));
    if (run.resident_epic)
        for (const WorkerPlan &wp : plan)
            for (size_t i = wp.lo; i < wp.hi; i++) lab_frames[wp.gpu][window_tap(todo[i].jet, todo[i].backward, run.steps, run.steps, 0)] = 1;
    Sequence seq(run, gpu_frames, lab_frames, t_begin);                                          // one uploader thread per GPU, from now on
    double decoded_at = 0;
    if (const int rc = read_frames(run, sequence_path, format, seq, decoded_at)) return rc;
    if (run.resident_epic && run.dm_scale != 1) {                                    // sfa_job_set_flow_epic takes fields whose size divides the frames' in both directions
        const int ew = (int)std::lrint(seq.width * run.dm_scale), eh = (int)std::lrint(seq.height * run.dm_scale);
        if (ew < 1 || eh < 1 || seq.width % ew != 0 || seq.height % eh != 0) {
            std::cerr << "gpu_ingest 1 is refused with deep_matching 1 and dm_scale " << run.dm_scale << " on " << seq.width << " x " << seq.height << " frames: the interpolation's " << ew << " x " << eh
                      << " does not divide them, and the resident initialisation resizes only by whole factors; crop the frames to a multiple of 1 / dm_scale, or set gpu_ingest 0" << std::endl;
            return 1;
        }
    }
    ColorImage channel_weights(run.gpu_ingest ? nullptr : color_image_new(seq.width, seq.height));   // :597-598 (all ones without raw weighting); gpu_ingest 1: the GPUs form them
    if (channel_weights) {
        std::fill(channel_weights->c1, channel_weights->c1 + (size_t)3 * channel_weights->stride * seq.height, 1.0f);
        if (run.raw) rawWeighting(channel_weights.get(), run.red_x, run.red_y, run.raw_weight);   // :599-600
    }
    std::vector<Flow> gt(params.Jets);
    if (!run.file_gt.empty())
        if (const int rc = load_ground_truth(run, gt)) return rc;

    // the uploaders have been uploading beside the decoding; what is left of the ingest is the normalisation (not needed when -resume left nothing to refine)
    const double t_norm = now_s();
    double avg[3], sd[3];
    if ((todo.empty() || !seq.wait_statistics(avg, sd)) && seq.report_errors()) return 4;
    if (!todo.empty()) publish_normalization(params, avg, sd);                       // the slow_flow_img_norm_* parameters (variational_mt.cpp:71-84)
    const double normalize_seconds = now_s() - t_norm;
    std::ofstream((run.output + "config.cfg").c_str()) << "# SlowFlow variational estimation\n" << params;   // :684-688
    const double ingest_seconds = now_s() - t_begin;

    if (run.out_occ) mkdirs(run.output + "occlusion/");                              // :676-677
    if (run.out_alt_occ || run.deep_matching) mkdirs(run.output + "tmp/");
    TaskPool out_pool(run.io_threads);
    Refinement rf{run, seq, channel_weights.get(), gt, todo, out_pool, {}, {false}, {0}, {0}, -1, {0, 0, 0, 0}, {}};
    const double t_compute = now_s();
    std::vector<std::thread> th;
    for (const WorkerPlan &wp : plan) th.emplace_back(refine_worker, std::ref(rf), wp);
    for (auto &t : th) t.join();
    const double compute_seconds = now_s() - t_compute;
    if (seq.report_errors()) rf.failed = true;
    out_pool.wait_all();
    write_timings(run, todo, seq, rf, decoded_at - t_begin, normalize_seconds, ingest_seconds, compute_seconds, now_s() - t_begin);
    return rf.failed ? 5 : 0;
}

int main(int argc, char **argv) {
    if (argc < 2) { usage(); return 1; }
    ParameterList params;
    setDefault(params);
    if (argv[1][0] != '-' && file_exists(argv[1])) params.read(argv[1]);
    else { std::cerr << "Couldn't find " << argv[1] << "!" << std::endl; return -1; }

    bool overwrite_output = false;
    RunOptions opt;
    int selected_fr = -1;
    for (int i = 1; i < argc; i++) {                                                 // slow_flow.cpp:168-193
        const char *a = argv[i];
        if (a[0] != '-') continue;
        if (!strcmp(a, "-h") || !strcmp(a, "-help")) usage();
        else if (!strcmp(a, "-overwrite")) overwrite_output = true;
        else if (!strcmp(a, "-resume")) opt.resume_frame = true;
        else if (!strcmp(a, "-deep_settings") && i + 1 < argc) i++;
        else if (!strcmp(a, "-threads") && i + 1 < argc) params.insert("threads", argv[++i], true);
        else if (!strcmp(a, "-fr") && i + 1 < argc) selected_fr = atoi(argv[++i]);
        else if (!strcmp(a, "-jet") && i + 1 < argc) { opt.selected_jet = atoi(argv[++i]); opt.resume_frame = true; }
        else { fprintf(stderr, "unknown argument %s", a); usage(); }
    }
    const bool raw = params.exists("raw") && params.parameter<bool>("raw");
    const int demosaicing = params.parameter<int>("raw_demosaicing", "0");
    if (raw && demosaicing != 0 && demosaicing != 2) {
        std::cerr << "raw_demosaicing 1 (Hamilton-Adams, P. Getreuer's dmha) is third-party code absent from the reference tree: use raw_demosaicing 0 "
                     "(the reference's own bilinear / green-ratio routine), 2 (OpenCV's 8-bit bilinear conversion, restated) or provide demosaiced frames with raw 0" << std::endl;
        return 2;
    }
    const int epic_search = params.parameter<int>("gpu_epic_search", "0");
    if (epic_search != 0 && epic_search != 1) {
        std::cerr << "gpu_epic_search " << epic_search << " is neither 0 (the default search) nor 1 (the compact search of the library, with gpu_epic 1)" << std::endl;
        return 1;
    }

    const int steps = params.parameter<int>("slow_flow_S") - 1;                      // :208
    const int max_fps = params.parameter<int>("max_fps", "1");
    const int jet_fps = params.exists("jet_fps") ? params.parameter<int>("jet_fps") : max_fps;
    int skip = (int)((1.0f * max_fps) / jet_fps);                                    // :220
    const bool sintel = params.parameter<bool>("sintel", "0"), subframes = params.parameter<bool>("subframes", "0");
    unsigned start = params.sequence_start;
    const size_t cut = params.file.find_last_of('/') + 1;
    string sequence_path = params.file.substr(0, cut), format = params.file.substr(cut);
    if (sequence_path.empty() || params.output.empty()) { std::cerr << "cfg needs 'file' and 'output'" << std::endl; return -1; }
    if (sintel && !subframes) start *= 1000;
    params.sequence_start = start;

    if (!opt.resume_frame && !overwrite_output) {                                    // never overwrite a results folder (:254-265)
        string np = params.output;
        if (np.back() == '/') np.pop_back();
        const string base = np;
        int num = 1;
        while (file_exists(np)) { std::cerr << np << " already exists!" << std::endl; np = base + "_" + std::to_string(num++); }
        params.output = np;
    }
    if (params.output.back() != '/') params.output += "/";

    // ---- adaptive frame rates (:277-357): adaptiveFR.dat (next to the program: the reference's SOURCE_PATH) names the target quantile and the
    //      low-rate factor, <sequence>/quantil.dat (written by the adaptiveFR program) holds the sequence's flow-magnitude quantile ------------
    bool adaptive = false;
    double quantil = 1.0, hfr_quantil = 2.0;
    int lfr_factor = 4;
    AdaptiveRates rates = {1, 4};
    const string adfr = params.exists("adaptive_fr_file") ? params.parameter("adaptive_fr_file") : exe_dir() + "/adaptiveFR.dat";
    if (file_exists(adfr)) {
        std::ifstream f(adfr.c_str());
        string line;
        while (std::getline(f, line)) {
            const size_t tab = line.find('\t');
            if (tab == string::npos) continue;
            const string key = line.substr(0, tab), val = line.substr(tab + 1);
            if (key == "opt_hfr_quantil") hfr_quantil = atof(val.c_str());
            if (key == "opt_lfr_rate") lfr_factor = (int)atof(val.c_str());
        }
        adaptive = params.parameter<bool>("adaptive", "0");
    }
    // :197-200, :306: the bound on the flow DeepMatching may find -- it restricts the matcher's search (outside this build) and halves dm_scale beyond 150 px (:397-402)
    double max_flow = params.exists("max_flow") ? std::max(5.0f, params.parameter<float>("max_flow")) : 50.0, orig_max_flow = 0;
    const double scale_main = params.parameter<float>("scale", "1.0");
    const string qfstr = sequence_path + "/quantil.dat";
    if (!params.exists("max_flow") && file_exists(qfstr)) {
        std::ifstream f(qfstr.c_str());
        string line;
        std::getline(f, line);
        quantil = atof(line.c_str());
        // :315-319: the flow bound is three times the file's second line (the maximum) if there is one, else three times the quantile
        string line2;
        orig_max_flow = 3.0 * (std::getline(f, line2) ? atof(line2.c_str()) : quantil);
        if (!adaptive) max_flow = std::max(5.0, orig_max_flow * scale_main * steps * skip);   // :354 (ref = steps)
        if (adaptive) {
            const int keyframes = (int)(params.parameter<float>("max_fps") / params.parameter<float>("ref_fps"));   // :324
            rates = adaptive_rates(quantil, hfr_quantil, lfr_factor, keyframes, steps);
            if (keyframes == 0) std::cout << rates.hfr_rate << " " << rates.lfr_rate << std::endl;
            else std::cout << "hfr_rate " << rates.hfr_rate << std::endl << "lfr_rate " << rates.lfr_rate << std::endl;
        }
        // without `adaptive` the quantile only bounds DeepMatching's search radius (:353-355): outside this build
    } else
        adaptive = false;

    int start_fr = 0, end_fr = adaptive ? 2 : 1;                                     // :359-364
    if (selected_fr >= 0) { start_fr = selected_fr; end_fr = selected_fr + 1; }
    int rc_all = 0;
    for (int adFR = start_fr; adFR < end_fr; adFR++) {                               // :367-399
        ParameterList adaptCfg(params);
        if (adaptive) {
            const int rate = adFR == 0 ? rates.hfr_rate : rates.lfr_rate;
            adaptCfg.output += adFR == 0 ? "high_fr/" : "low_fr/";
            adaptCfg.insert("jet_fps", std::to_string(max_fps / rate), true);        // jet estimation fps
            skip = rate;
            max_flow = std::max(5.0, orig_max_flow * scale_main * steps * rate);     // :382, :392
        }
        {   // :396-402: smaller resolution for deep matching
            double dm_scale = params.parameter<float>("dm_scale", "1.0");
            if (params.parameter<bool>("deep_matching") && max_flow > 150) { dm_scale = 0.5 * dm_scale; max_flow = std::max(5.0, 0.5 * max_flow); }   // (:401: the bound at the halved size)
            std::ostringstream o;
            o.precision(17);
            o << dm_scale;
            adaptCfg.insert("dm_scale_run", o.str(), true);
        }
        const int rc = run_sequence(adaptCfg, sequence_path, format, skip, opt);
        if (rc != 0) rc_all = rc;
    }
    std::cout << (rc_all ? "Failed!" : "Done!") << std::endl;
    return rc_all;
}
