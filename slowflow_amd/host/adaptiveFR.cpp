// adaptiveFR.cpp -- step 1 of the reference's pipeline (README "Run Pipeline"; adaptiveFR.cpp of the reference): how fast a sequence moves.  Samples
// `-samples` frame pairs (start + i * step, + skip) at `-scale`, refines EpicFlow's interpolation of their matches with the original two-frame
// variational(), and writes the `-quantil` quantile and the maximum of the flow magnitudes (per recorded frame at full resolution) to
// <sequence>/quantil.dat, which the slow_flow driver reads for `adaptive 1` (slow_flow.cpp).  Same command line (:62-64, :116-186), defaults, file
// names and outputs as the reference; the GPU does the rescaling, EpicFlow's filters, all pending samples' refinements in one launch sequence per 128
// (sfa_variational_2frame_batch) and the quantile as an exact radix select (sfa_flow_magnitude_quantile) instead of std::sort.
//
// Like the driver's `deep_matching 1`, this build starts neither DeepMatching nor the MATLAB edge detector: a first run writes the frames they need
// (adaptiveFR/sequence/frame_epic_<n>.png), lists the match / edge files that are missing and exits with status 2; once the external tools have written
// adaptiveFR/tmp/matches_<a>_<b>.dat and edges_<n>.dat, a second run refines.  The flow of a sample whose .flo exists is read back, not recomputed,
// unless -overwrite is given; it counts toward the quantile either way.
#include <dirent.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "epic.h"
#include "flow_vis.h"
#include "image.h"
#include "ingest.h"
#include "io.h"
#include "parameter_list.h"
#include "png.h"
#include "util.h"

using std::string;

static void usage() {
    printf("usage:\n");
    printf("    ./adaptiveFR -path [path] -folder [one sequence folder | file listing folders] -format [file format] -scale [default 0.25] "
           "-skip [target frame (2)] -samples [number of estimates (40)] -step [frames between estimates (10)] -start [first frame (0)] "
           "-quantil [q (0.9)] -append [file] -overwrite -sintel -subframes -raw -threads -gpu_epic (EpicFlow's graph searches of all pending samples on the GPU)\n");
    printf("\n");
}

// 8-bit RGB planes (values 0..255) -> PNG
static bool write_rgb8(const string &file, const color_image_t *im) {
    png_image p;
    p.width = im->width; p.height = im->height; p.channels = 3; p.depth = 8;
    p.samples.resize((size_t)3 * im->width * im->height);
    const float *c[3] = {im->c1, im->c2, im->c3};
    for (int y = 0; y < im->height; y++)
        for (int x = 0; x < im->width; x++)
            for (int k = 0; k < 3; k++) p.samples[((size_t)y * im->width + x) * 3 + k] = (uint16_t)c[k][(size_t)y * im->stride + x];
    return png_write(file.c_str(), p);
}
// Mat::convertTo(CV_8U, norm): cvRound (to nearest, ties to even) and saturation, in place
static void to_8bit(color_image_t *im, float norm) {
    const size_t n3 = (size_t)3 * im->stride * im->height;
    for (size_t i = 0; i < n3; i++) {
        const float v = nearbyintf(im->c1[i] * norm);
        im->c1[i] = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
    }
}

struct Sample {
    int first = 0;                          // params.sequence_start of the sample: frames first and first + skip
    color_image_t *im[2] = {nullptr, nullptr};
    image_t *wx = nullptr, *wy = nullptr;   // the refined or read-back flow (at the scaled size)
    bool pending = false;                   // refined in this run
    string flo, edges, matches;
    ~Sample() {
        for (auto *i : im) if (i) color_image_delete(i);
        if (wx) image_delete(wx);
        if (wy) image_delete(wy);
    }
};

struct Sequence {
    string name, path, output, format_flow;
    ParameterList params;
    std::vector<Sample *> samples;          // the samples whose frames were found (the reference's wx[it] != NULL)
    ~Sequence() { for (auto *s : samples) delete s; }
};

int main(int argc, char **argv) {
    if (argc < 2) { usage(); exit(1); }
    string format = "%07i.tif", path, folder, append;
    unsigned start = 0;
    bool overwrite = false, sintel = false, subframes = false, raw = false, gpu_epic = false;
    int samples = 40, sample_step = 10, skip = 2, threads = 1;
    const int all_frames = 2;
    float q = 0.90f;
    double scale = 0.25;
    for (int i = 0; i < argc;) {                                                       // :147-192
        const char *a = argv[i++];
        if (a[0] != '-') continue;
        auto next = [&]() -> const char * {
            if (i >= argc) { fprintf(stderr, "missing value of %s\n", a); usage(); exit(1); }
            return argv[i++];
        };
        if (!strcmp(a, "-h") || !strcmp(a, "-help")) usage();
        else if (!strcmp(a, "-path")) path = next();
        else if (!strcmp(a, "-folder")) folder = next();
        else if (!strcmp(a, "-threads")) threads = atoi(next());
        else if (!strcmp(a, "-append")) append = next();
        else if (!strcmp(a, "-scale")) scale = atof(next());
        else if (!strcmp(a, "-skip")) skip = std::max(1, atoi(next()));
        else if (!strcmp(a, "-samples")) samples = atoi(next());
        else if (!strcmp(a, "-step")) sample_step = atoi(next());
        else if (!strcmp(a, "-start")) start = (unsigned)atoi(next());
        else if (!strcmp(a, "-quantil")) q = (float)atof(next());
        else if (!strcmp(a, "-overwrite")) overwrite = true;
        else if (!strcmp(a, "-sintel")) sintel = true;
        else if (!strcmp(a, "-raw")) raw = true;
        else if (!strcmp(a, "-subframes")) subframes = true;
        else if (!strcmp(a, "-format")) format = next();
        else if (!strcmp(a, "-gpu_epic")) gpu_epic = true;
        else { fprintf(stderr, "unknown argument %s", a); usage(); exit(1); }
    }
    (void)threads;          // the reference runs sequences on OpenMP threads (:245); here they run one after the other, each sample batch fills the GPU
    if (!(q > 0.0f && q <= 1.0f)) { std::cerr << "-quantil " << q << ": outside (0, 1] the reference indexes outside its array" << std::endl; return 1; }
    if (samples < 1 || !(scale > 0)) { std::cerr << "-samples must be >= 1 and -scale > 0" << std::endl; return 1; }
    // :381-415: the reference's ParameterList here has no cfg, so raw_demosaicing is its default 0 (bilinear); 1 (Hamilton-Adams, third-party code
    // absent from the reference tree) would be refused as the driver refuses it
    ParameterList defaults;
    defaults.insert("verbose", "0", true);
    const int demosaicing = defaults.parameter<int>("raw_demosaicing", "0");
    if (raw && demosaicing == 1) { std::cerr << "raw_demosaicing 1 (Hamilton-Adams) is third-party code absent from the reference tree" << std::endl; return 2; }

    // ---- sequences (:194-239): one folder, a file listing folders, or every sub-directory of -path; sorted -------------------------------------
    std::vector<string> folders;
    if (folder.empty()) {
        DIR *d = opendir((path + "/").c_str());
        if (!d) { std::cerr << path << ": no such directory" << std::endl; return 1; }
        static const char *const skipped[] = {"$RECYCLE.BIN", "preview", "Rallye", "System Volume Information", "WDApps"};
        while (dirent *e = readdir(d)) {
            const string n = e->d_name;
            if (n.empty() || n[0] == '.' || !is_dir(path + "/" + n)) continue;
            if (std::find(std::begin(skipped), std::end(skipped), n) != std::end(skipped)) continue;
            folders.push_back(n);
        }
        closedir(d);
    } else if (is_dir(path + "/" + folder + "/")) {
        folders.push_back(folder);
    } else if (folder != "-") {
        std::ifstream in(folder.c_str());
        if (!in.is_open()) { std::cerr << folder << ": no such file or directory" << std::endl; return EXIT_FAILURE; }
        string line;
        while (std::getline(in, line)) {
            if (is_dir(path + "/" + line + "/")) folders.push_back(line);
            else std::cerr << path + "/" + line + "/" << ": no such directory" << std::endl;
        }
    }
    std::sort(folders.begin(), folders.end());
    if (sintel && !subframes) start = start * 1000;

    sfa_ctx *ctx = nullptr;
    if (sfa_ctx_create(0, &ctx) != SFA_OK) { std::cerr << sfa_last_error(nullptr) << std::endl; return 4; }

    // ---- pass 1 over every sequence: frames, the images for the external matcher, what each pending sample still needs --------------------------
    std::vector<Sequence *> seqs;
    std::vector<string> missing;
    bool is16 = false;                                 // the reference's "16bit" parameter: once a 16-bit frame was seen, norm = 1/255 from then on (:364-368)
    for (const string &fold : folders) {
        Sequence *S = new Sequence();
        seqs.push_back(S);
        S->name = fold;
        S->path = path + "/" + fold + "/";
        S->output = S->path + "adaptiveFR/";
        S->format_flow = format.substr(0, format.find_last_of('.'));
        S->params.insert("verbose", "0", true);
        S->params.insert("format", format, true);
        S->params.file = S->path;
        S->params.Jets = 1;
        mkdirs(S->output); mkdirs(S->output + "tmp/"); mkdirs(S->output + "sequence/");
        unsigned first = start;
        for (int it = 0; it < samples; it++) {
            if (it > 0) first += sample_step;                                              // :314-319 (Jets = 1)
            Sample *smp = new Sample();
            smp->first = (int)first;
            bool ok = true;
            for (int f = 0; f < all_frames && ok; f++) {
                const string name = sequence_frame_name(S->path + format, (int)first, f * skip, sintel);   // :336-352
                if (!file_exists(name)) { std::cerr << "Could not find " << name << "!" << std::endl; ok = false; break; }
                std::cout << "Reading " << name << "..." << std::endl;
                int maxval = 255;
                string error;                                                               // raw: :376-418, bilinear demosaicing of the mosaic,
                color_image_t *img = load_frame(name, raw, 0, 1, 0, &maxval, &error);       // raw_red_loc default "1,0" (:326)
                if (!img) { std::cerr << error << std::endl; ok = false; break; }
                // The reference takes norm = 1/255 for a single-channel 16-bit image (img.type() == CV_16UC1) and keeps it for every later frame;
                // 16-bit colour frames would be saturated at norm 1 there.  Here every 16-bit frame sets it: the loader replicates grey into 3 planes.
                if (maxval > 255) is16 = true;
                const float norm = is16 ? 1.0f / 255 : 1.0f;
                if (scale != 1) {                                                           // :431-434, on the GPU
                    color_image_t *small = color_image_rescale(ctx, img, (float)scale);
                    color_image_delete(img);
                    if (!small) { std::cerr << "rescaling failed: " << sfa_last_error(ctx) << std::endl; return 4; }
                    img = small;
                }
                if (defaults.verbosity(WRITE_FILES)) {                                      // :442-450
                    color_image_t *out = color_image_cpy(img);
                    to_8bit(out, norm);
                    write_rgb8(S->output + "sequence/frame_" + std::to_string((int)first + f * skip) + ".png", out);
                    color_image_delete(out);
                }
                to_8bit(img, norm);                                                         // :453, the frames refined from here on
                // :466-473: GaussianBlur(sigma 1/sqrt(2 dm_scale)) + resize(dm_scale = 1) -> frame_epic_<n>.png for DeepMatching.  OpenCV blurs 8-bit
                // images in fixed point; this is the float blur rounded back to 8 bit (the file only feeds the external matcher).
                color_image_t *epic_im = color_image_new(img->width, img->height);
                const float sigma = (float)(1 / sqrt(2 * 1.0));
                float *src3[3] = {img->c1, img->c2, img->c3}, *dst3[3] = {epic_im->c1, epic_im->c2, epic_im->c3};
                for (int k = 0; k < 3; k++)
                    if (sfa_gaussian_blur(ctx, dst3[k], src3[k], img->width, img->height, img->stride, sigma) != SFA_OK) {
                        std::cerr << "blur failed: " << sfa_last_error(ctx) << std::endl;
                        return 4;
                    }
                to_8bit(epic_im, 1.0f);
                write_rgb8(S->output + "sequence/frame_epic_" + std::to_string((int)first + f * skip) + ".png", epic_im);
                color_image_delete(epic_im);
                smp->im[f] = img;
            }
            if (!ok) { delete smp; continue; }                                              // :476-477: the sample is left out
            if (smp->im[0]->width != smp->im[1]->width || smp->im[0]->height != smp->im[1]->height) {
                std::cerr << "frames of different sizes in " << S->path << std::endl;
                delete smp;
                continue;
            }
            smp->flo = !sintel ? fmt1(S->output + S->format_flow + ".flo", smp->first) : fmt2(S->output + S->format_flow + ".flo", smp->first, 0);   // :512-515
            smp->edges = S->output + "tmp/edges_" + std::to_string(smp->first) + ".dat";                 // :524 (start + f, f = 0)
            smp->matches = S->output + "tmp/matches_" + std::to_string(smp->first) + "_" + std::to_string(smp->first + skip) + ".dat";   // :538
            smp->pending = overwrite || !file_exists(smp->flo);                                        // :519
            if (smp->pending) {
                for (const string *f : {&smp->edges, &smp->matches})
                    if (!file_exists(*f)) missing.push_back(*f);
            } else {
                image_t **fl = readFlowFile(smp->flo.c_str());                                         // :589-595
                if (!fl) { std::cerr << "cannot read " << smp->flo << std::endl; delete smp; continue; }
                smp->wx = fl[0]; smp->wy = fl[1];
                free(fl);
                std::cout << "Forward flow from frame " << smp->first << " to " << smp->first + skip << " already exist!" << std::endl;
            }
            S->samples.push_back(smp);
        }
        std::ofstream cfg((S->output + "config.cfg").c_str());                                 // :484-488
        cfg << "# Epic Flow estimation\n" << S->params;
    }
    if (!missing.empty()) {
        std::cerr << "DeepMatching and the SED edge detector are not started by this build. Missing for the pending samples:" << std::endl;
        for (const string &m : missing) std::cerr << "  " << m << std::endl;
        std::cerr << "The frames they need are adaptiveFR/sequence/frame_epic_<n>.png; run again once the files exist." << std::endl;
        for (auto *S : seqs) delete S;
        sfa_ctx_destroy(ctx);
        return 2;
    }

    // ---- pass 2: EpicFlow, one batched refinement per 128 pending samples, the quantile ------------------------------------------------------------
    epic_params_t ep;
    epic_params_default(&ep);
    ep.pref_nn = 25; ep.nn = 160; ep.coef_kernel = 1.1f;                                        // :295-297
    sfa_params_2frame fp;
    sfa_params_2frame_default(&fp);
    fp.niter_outer = 5; fp.alpha = 1.0f; fp.gamma = 0.72f; fp.delta = 0.0f; fp.sigma = 1.1f;    // :298-302
    const float flow_scale = (float)(1.0 / (scale * skip));                                     // :612-613: image_mul_scalar takes a float
    std::stringstream overview;
    int rc_all = 0;
    for (Sequence *S : seqs) {
        std::vector<Sample *> todo;
        std::vector<color_image_t *> labs;                                                      // -gpu_epic: the inputs of todo's samples
        std::vector<epic_matches> mts;
        std::vector<epic_edges> eds;
        for (Sample *smp : S->samples) {
            if (!smp->pending) continue;
            const int w = smp->im[0]->width, h = smp->im[0]->height;
            epic_matches mt;
            epic_edges ed;
            if (!read_matches(smp->matches.c_str(), mt) || !read_edges(smp->edges.c_str(), w, h, ed)) {
                std::cerr << "cannot read " << smp->matches << " / " << smp->edges << std::endl;
                return 3;
            }
            color_image_t *lab = rgb_to_lab(smp->im[0]);                                        // :563
            smp->wx = image_new(w, h); smp->wy = image_new(w, h);
            image_erase(smp->wx); image_erase(smp->wy);
            todo.push_back(smp);
            if (gpu_epic) {                                                                     // -gpu_epic: interpolated below, up to 128 samples per epic_batch
                labs.push_back(lab); mts.push_back(std::move(mt)); eds.push_back(std::move(ed));
                continue;
            }
            const int er = epic(ctx, smp->wx, smp->wy, lab, mt, ed, &ep);                       // :568
            color_image_delete(lab);
            if (er < 0) { std::cerr << "EpicFlow interpolation failed: " << sfa_last_error(ctx) << std::endl; return 4; }
            if (er > 0) { image_erase(smp->wx); image_erase(smp->wy); }                         // no usable match: start from zero
        }
        for (size_t b = 0; b < labs.size(); b += 128) {
            const int n = (int)std::min<size_t>(128, labs.size() - b);
            std::vector<image_t *> fx(n), fy(n);
            std::vector<const color_image_t *> lab(n);
            std::vector<const epic_matches *> mt(n);
            std::vector<epic_edges *> ed(n);
            std::vector<int> er(n);
            for (int i = 0; i < n; i++) { fx[i] = todo[b + i]->wx; fy[i] = todo[b + i]->wy; lab[i] = labs[b + i]; mt[i] = &mts[b + i]; ed[i] = &eds[b + i]; }
            epic_batch(ctx, n, fx.data(), fy.data(), lab.data(), mt.data(), ed.data(), &ep, er.data());
            for (int i = 0; i < n; i++) {
                color_image_delete(labs[b + i]);
                if (er[i] < 0) { std::cerr << "EpicFlow interpolation failed: " << sfa_last_error(ctx) << std::endl; return 4; }
                if (er[i] > 0) { image_erase(fx[i]); image_erase(fy[i]); }
            }
        }
        // :574 -- variational(), here for up to 128 samples at once.  The reference then runs system(epic_cmd) (:575) on a buffer it never
        // initialised; nothing of the kind is done here.
        for (size_t b = 0; b < todo.size(); b += 128) {
            const int n = (int)std::min<size_t>(128, todo.size() - b);
            std::vector<float *> wx(n), wy(n);
            std::vector<const float *> i1(n), i2(n);
            const int w = todo[b]->wx->width, h = todo[b]->wx->height, stride = todo[b]->wx->stride;
            for (int i = 0; i < n; i++) {
                Sample *smp = todo[b + i];
                if (smp->wx->width != w || smp->wx->height != h) { std::cerr << "samples of different sizes in " << S->path << std::endl; return 3; }
                wx[i] = smp->wx->data; wy[i] = smp->wy->data; i1[i] = smp->im[0]->c1; i2[i] = smp->im[1]->c1;
            }
            if (sfa_variational_2frame_batch(ctx, n, wx.data(), wy.data(), w, h, stride, i1.data(), i2.data(), &fp) != SFA_OK) {
                std::cerr << "refinement failed: " << sfa_last_error(ctx) << std::endl;
                return 4;
            }
        }
        for (Sample *smp : todo) {
            writeFlowFile(smp->flo.c_str(), smp->wx, smp->wy);                                  // :585
            std::cout << "Forward flow from frame " << smp->first << " to " << smp->first + skip << " finished!" << std::endl;
        }
        std::vector<const float *> us, vs;
        for (Sample *smp : S->samples) {
            png_write((S->output + "tmp/frame_" + std::to_string(smp->first) + ".png").c_str(), flowColorImg(smp->wx, smp->wy, 0));   // :598-609
            us.push_back(smp->wx->data); vs.push_back(smp->wy->data);
        }
        const int used = (int)us.size();
        if (used == 0) { std::cerr << S->path << ": no sample could be read, no quantile" << std::endl; rc_all = 3; continue; }
        const image_t *f0 = S->samples[0]->wx;
        for (Sample *smp : S->samples)
            if (smp->wx->width != f0->width || smp->wx->height != f0->height || smp->wx->stride != f0->stride) {
                std::cerr << S->path << ": flow fields of different sizes (a .flo from another run?)" << std::endl;
                return 3;
            }
        double quantil = 0, maxq = 0;                                                           // :644-668
        if (sfa_flow_magnitude_quantile(ctx, used, us.data(), vs.data(), f0->width, f0->height, f0->stride, flow_scale, q, &quantil, &maxq) != SFA_OK) {
            std::cerr << "quantile failed: " << sfa_last_error(ctx) << std::endl;
            return 4;
        }
        std::cout << "Quantil: " << quantil << std::endl;
        std::ofstream info((S->output + "results.info").c_str());                               // :673-682
        info << "Adaptive Frame rate\n\nsamples\t" << used << "\nsample_step\t" << sample_step << "\nskip\t" << skip << "\n" << q << " quantil\t" << quantil
             << "\nmax\t" << maxq << "\n";
        info.close();
        overview << S->name << "\t" << q << " quantil\t" << quantil << "\n";                   // :686
        std::ofstream qf;                                                                       // :689-696
        if (!append.empty()) qf.open(append.c_str(), std::ofstream::out | std::ofstream::app);
        else qf.open((S->path + "quantil.dat").c_str());
        qf << quantil << "\n" << maxq << "\n";
    }
    // :706-714: the overview next to the sequences (the reference appends "results.info" to -path as given: pass it with a trailing '/')
    std::ofstream info((path + (path.empty() || path.back() == '/' ? "" : "/") + "results.info").c_str());
    info << "Adaptive Frame rate\n\nsamples\t" << samples << "\nsample_step\t" << sample_step << "\nskip\t" << skip << "\n\n" << overview.str();
    info.close();
    for (auto *S : seqs) delete S;
    sfa_ctx_destroy(ctx);
    std::cout << (rc_all ? "Failed!" : "Done!") << std::endl;
    return rc_all;
}
