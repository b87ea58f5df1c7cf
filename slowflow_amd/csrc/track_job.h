// track_job.h -- what the two halves of the resident track job share: track.hip (the kernels, the job, its uploads, run and downloads) and track_fill.hip (a fill
// job's checks, planes, fill-in stage and entry points).  The plane table, the job and a fill job's state, the entry points' preamble (stream calls: stage_io.hip).
#pragma once
#include <memory>

#include "sfa_internal.h"

// the orchestration's helpers are compiled for size like the files that include them (see track.hip)
#pragma clang attribute push(__attribute__((minsize)), apply_to = function)
// and nothing here is part of the library's interface
#pragma GCC visibility push(hidden)

namespace sfa {

constexpr int kTrackMaxRates = 16, kTrackThreads = 256;                         // track.hip's kTrMaxK and kTrThreads (asserted there)

// a plane of the job's one allocation: its byte offset, and the element type its size is counted in and its pointer comes back as
template <class T> struct Plane { size_t off; };
// a plane whose element type is a run-time choice: counted in bytes, and the use says what it holds
using BytePlane = Plane<char>;

// a host array that goes with its owner.  (std::unique_ptr<T[]> would do; its destructors, out of line in code compiled for size, would join the library's exports)
template <class T> struct HostArray {
    T *p = nullptr;
    HostArray() = default;
    HostArray(const HostArray &) = delete;
    HostArray &operator=(const HostArray &) = delete;
    ~HostArray() { delete[] p; }
    void alloc(size_t n) { delete[] p; p = new T[n](); }                        // n zeros
    T *get() const { return p; }
    T &operator[](size_t i) const { return p[i]; }
};

// hands out the planes one after the other, each rounded up to 256 bytes
struct PlaneCursor {
    size_t top = 0;
    template <class T> void take(Plane<T> &plane, size_t count) { plane.off = top; top += (count * sizeof(T) + 255) / 256 * 256; }
};

// Every plane of the job inside one allocation; this struct is the only statement of the list (sfa_track_job_bytes walks it without a device), and
// track_layout takes the planes in the order they stand here
struct TrackPlanes {
    // fw, bw: float2 planes of an identity source, double2 planes of a resampled one
    struct Rate { BytePlane fw, bw; Plane<unsigned char> mask; Plane<double> acc_u, acc_v; Plane<int> tracked; } rate[kTrackMaxRates];
    Plane<unsigned char> occluded;
    Plane<float> stage;                         // one segment's u and v planes of one direction, of the rate that needs most
    Plane<unsigned char> occ_stage;             // one segment's occlusion images, likewise
    Plane<float> frames, der;
    BytePlane rec;                              // the energies' records of 48 bytes
    Plane<double> wU, wV; Plane<unsigned long long> wocc; Plane<float> jc, oc; Plane<double> ep, E; Plane<unsigned long long> O; Plane<unsigned char> best;
    Plane<double> aU, aV; Plane<float> weight; Plane<unsigned char> nl, lab; Plane<double> theta, P, M; Plane<unsigned char> xcur, xbest;
    Plane<int> slot; Plane<double> fu, fv; Plane<unsigned char> out_occ; Plane<double> seg_energy, seg_bound; Plane<int> seg_iters;
    // a fill job only: the saliency's workspace of one start_jet (15 planes at the device pitch), sal [n][plp], edges (as uploaded) and run_cost (the map
    // as the calls so far left it) [n][cpl], cost [n][rJmax][cpl], full [K][n], the regions' T, P, S [n][gpl] and mask, kept and count [n], the sample
    // positions, block_count, matches [n][rJmax][nx ny][4], fx, fy [n][rJmax][gpl], inf [gpl] doubles of +Inf; per rate the fill-in's trajectories [n][rJ][gpl] and tracked [n][gpl]
    Plane<float> lab_stage, sal, edges, run_cost, cost; Plane<int> full, cT, cP, cS; Plane<unsigned char> mask; Plane<int> kept, count, xs, ys, block_count;
    Plane<float> matches, fx, fy; Plane<double> inf;
    struct Fill { Plane<double> u, v; Plane<int> tracked; } fill[kTrackMaxRates];
    // a job that alternates only (track_alt.hip): two sets of hypothesis lists of 16 positions ([n][16][J][gpl], [n][16][gpl]) that the rounds' stages
    // read and write in turn; flags, srcpos, consistent, chosen [n][gpl]; total [n][2]; map, trk [n][16][gpl]; seq [n]; E1, O1 [gpl]; P16 [n][2][gpl][256];
    // per round and start_jet [rounds][n]: energy, bound, iterations, nodes, accepted proposals
    struct Alt {
        Plane<double> U[2], V[2], energy[2]; Plane<unsigned long long> occ[2]; Plane<unsigned char> origin[2];
        Plane<unsigned char> flags, srcpos, consistent, chosen; Plane<int> total, map, trk; Plane<unsigned> seq; Plane<double> E1; Plane<unsigned long long> O1;
        Plane<double> P16, r_energy, r_bound; Plane<int> r_iters, r_nodes, r_accepted;
    } alt;
    size_t total;
};

// what a fill job derives from its parameters besides the planes: the sample positions, the longest rate, the planes' strides
struct FillGeo { HostArray<int> xs, ys; int nx = 0, ny = 0, rJmax = 0, pitch = 0; size_t cpl = 0, plp = 0; };

// the marks of a rate's fill-in, in stream order
enum FillEvent { kFevBegin, kFevMatched, kFevCosts, kFevChain, kFevTrajectories, kFillEvents };

// What a fill job (sfa_track_job_create_fill) holds besides the planes.  Made by track_fill_create, gone with the job
struct TrackFill {
    sfa_track_fill_params fp{};
    FillGeo g;
    HostArray<int> full, stats;                 // [K][n] r_Jets[r]; [K][n][3] kept_pixels, matches, filled of the last run
    HostArray<double> inf;                      // [gpl] +Inf, the source of the plane inf
    // the interpolation's images of one rate, up to n * rJmax: EpicChainDev's arrays, then each image's start_jet and step, and what the chain says of it
    HostArray<const float *> cost, matches, sal;
    HostArray<float *> fx, fy;
    HostArray<int> nm, seg_of, step_of, rc, status;
    HostArray<int> kept, count;                 // [n]: the host's copy of the planes kept and count
    DevMem ref_stage;                           // sfa_track_job_upload_fill_reference: frame 0 as read, 3 w h floats beside the job's allocation, made by its first call
    int chain_runs[2] = {};                     // the last run's interpolation sub-batches over all rates: completed, cut short and run again
    hipEvent_t ev[kTrackMaxRates][kFillEvents] = {};
    hipEvent_t ev_energy = nullptr;             // after the last rate's fill-in, where the energies begin
    ~TrackFill();
};

// What a job that alternates (sfa_track_job_create_alternate) holds besides the planes: its parameters with slots and the similarity keys filled in from
// the job's, the plan that scores a proposal (r_Jets = Jets, weight 0), and which of the two list sets the last run left its result in
struct TrackAlt {
    sfa_track_alt_params ap{};
    EnergyPlan plan{};
    int cur = 0;
};

// the marks of a run, in stream order (the fusion records its five itself: fuse_device)
enum TrackEvent { kEvStart, kEvRecords, kEvAccumulated, kEvBest, kEvFuse, kEvFuseEnd = kEvFuse + 4, kEvWeight /* before the fusion's clears */, kTrackEvents };

}  // namespace sfa

struct sfa_track_job {
    sfa_ctx *ctx = nullptr;
    sfa_track_params p;
    int gw = 0, gh = 0;
    bool identity[sfa::kTrackMaxRates] = {};
    sfa::EnergyPlan plan[sfa::kTrackMaxRates];
    sfa::TrackPlanes at;
    sfa::DevMem mem;
    hipEvent_t ev[sfa::kTrackEvents] = {};
    bool timed = false, timed_fuse = false;
    std::unique_ptr<sfa::TrackFill> fill;       // null for a plain job
    std::unique_ptr<sfa::TrackAlt> alt;         // null for a job that fuses once
    int slots() const { return fill ? 2 * p.K : p.K; }
    int step() const { return fill ? 2 : 1; }
    // the one place a plane's offset becomes a pointer
    template <class T> T *ptr(sfa::Plane<T> plane) const { return reinterpret_cast<T *>(static_cast<char *>(mem.p) + plane.off); }
};

namespace sfa {

// the preamble of an entry point that takes a job
#define TRACK_JOB(job) \
    if (!(job)) return sfa::set_error(nullptr, SFA_ERR_ARG, "%s: job is null", __func__); \
    sfa_ctx *ctx = (job)->ctx; \
    const sfa_track_params &p = (job)->p; \
    const size_t pl = (size_t)p.w * p.h, gpl = (size_t)(job)->gw * (job)->gh; \
    (void)pl; (void)gpl

int track_range(sfa_ctx *ctx, const char *fn, const sfa_track_params &p, int s0, int ns, int r);

// k_track_pack_frames (track.hip) with one frame: nc <= 3 channel planes of w x h in device memory, element (channel, row, column) at src + the element strides
// -> out: [nc][h][w] packed.  How a fill job packs its Lab images and edge maps
int pack_strided_planes(sfa_ctx *ctx, const float *src, long long s_c, long long s_row, long long s_col, int w, int h, int nc, float *out);

// ---- create and bytes for every kind of job, and the scratch the stages share (track.hip)
int track_bytes(const char *fn, const sfa_track_params *p, const sfa_track_fill_params *fill, bool with_fill, const sfa_track_alt_params *alt, bool with_alt,
                size_t *bytes);
int track_create(sfa_ctx *ctx, const char *fn, const sfa_track_params *p, const sfa_track_fill_params *fill, bool with_fill, const sfa_track_alt_params *alt,
                 bool with_alt, sfa_track_job **out);
EnergyWork energy_work(const sfa_track_job *job);
FuseWork fuse_work(const sfa_track_job *job);

// ---- the alternating job's half (track_alt.hip)
// the checks beyond the plain job's, by the key's name; out (or null): the parameters as the job uses them and the rescoring plan
int alt_check(sfa_ctx *ctx, const char *fn, const sfa_track_params *p, const sfa_track_alt_params *alt, bool with_fill, int gw, int gh, TrackAlt *out);
// the alternation's planes, behind every other plane
void alt_layout(PlaneCursor &c, const sfa_track_params &p, int gw, int gh, const sfa_track_alt_params &alt, TrackPlanes *a);
// The rounds of segments 0 .. ns-1 in place of the one fusion: lists from the slots, then per round prune (p > 0), propose, rescore, fuse -- all enqueued,
// no host wait.  The last round's result lies where the fusion's does (slot = the chosen POSITION), its origin in alt.chosen
int track_run_alternation(sfa_track_job *job, int ns);

// ---- the fill job's half (track_fill.hip), as create, bytes and run call it
// the checks of a fill job beyond the plain job's, by the name of the argument, and what the layout needs of it
int fill_check(sfa_ctx *ctx, const char *fn, const sfa_track_params *p, const sfa_track_fill_params *f, int gw, int gh, FillGeo *g);
// the fill planes, behind every other plane
void fill_layout(PlaneCursor &c, const sfa_track_params &p, int gw, int gh, const sfa_track_fill_params &fill, const FillGeo &g, TrackPlanes *a);
// job->fill (parameters and geometry as fill_check left them) -> its events and host arrays; the constant planes uploaded, and waited for
int track_fill_create(sfa_track_job *job);
// The fill-in of every rate of segments 0 .. ns-1, between the accumulation and the energies (the header's description).  It leaves the trajectories in the
// rates' fill planes and {kept_pixels, matches, filled} in fill->stats
int track_run_fill(sfa_track_job *job, int ns);

}  // namespace sfa

#pragma GCC visibility pop
#pragma clang attribute pop
