// CPU stand-ins for the HIP runtime and for every kernel launcher: they log the call with its arguments; device memory is a bump-allocated host region
#include "sfa_internal.h"
#include <cstdlib>
#include <sys/mman.h>
#include <cstring>
#include <string>

static char *g_region = nullptr;      // "device memory": pointers into it are logged as offsets
static size_t g_used = 0;
static const size_t kRegion = 1ull << 36;
std::string g_log;                    // what driver.cpp prints per case
bool g_mock_bool = true;              // what the bool launchers (the fused fast paths) answer
double g_mock_thres = 0;              // the scale of the norms the update stand-ins write
static unsigned long g_counter = 0;

static void *bump(size_t n) {
    if (!g_region) g_region = (char *)mmap(nullptr, kRegion, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    n = (n + 255) & ~size_t(255);
    if (g_used + n > kRegion) abort();
    void *p = g_region + g_used;
    g_used += n;
    return p;
}
static void begin(const char *n) { g_log += n; g_log += "("; }
static void end() { g_log += ")\n"; }
static void put(const char *k, const std::string &v) { g_log += k; g_log += "="; g_log += v; g_log += " "; }
static std::string ptr(const void *p) {
    if (!p) return "null";
    const char *c = (const char *)p;
    if (g_region && c >= g_region && c < g_region + kRegion) return "R+" + std::to_string(c - g_region);
    return "host";
}
static std::string bytes(const void *p, size_t n) {      // floats and structs are logged as a hash of their bytes
    unsigned long h = 1469598103934665603ul;
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ul;
    return "#" + std::to_string(h);
}
static std::string str(long v) { return std::to_string(v); }
static std::string mask(const sfa::WMask &m) { return std::to_string(m.w[0]) + ":" + std::to_string(m.w[1]); }
template <class T> static void arg(const char *k, T *p) { put(k, ptr((const void *)p)); }
static void arg(const char *k, int v) { put(k, std::to_string(v)); }
static void arg(const char *k, long v) { put(k, std::to_string(v)); }
static void arg(const char *k, size_t v) { put(k, std::to_string(v)); }
static void arg(const char *k, bool v) { put(k, std::to_string(v)); }
static void arg(const char *k, float v) { put(k, bytes(&v, 4)); }
static void arg(const char *k, double v) { put(k, bytes(&v, 8)); }
static void arg(const char *k, const float *v) { put(k, ptr(v) == "host" ? "host" : ptr(v)); }
static void arg(const char *k, const sfa::WMask &m) { put(k, mask(m)); }
static void arg(const char *k, const sfa::Geo &g) {
    put(k, str(g.w) + "x" + str(g.h) + " pitch " + str(g.pitch) + " pl " + str(g.pl) + " es " + str(g.es) + " nb " + str(g.nb) + " active " + mask(g.active) +
               " amask " + ptr(g.amask));
}
static void arg(const char *k, const sfa::PenaltyDev &p) { put(k, std::to_string(p.id) + "," + bytes(&p.eps, 4) + "," + bytes(&p.trunc, 4)); }
static void arg(const char *k, const sfa::SorOperandOut &o) {
    put(k, ptr(o.sa) + "," + ptr(o.sb) + "," + ptr(o.x) + "," + ptr(o.flags) + "," + str(o.ent) + "," + str(o.RP) + "," + str(o.G) + "," + str(o.ntasks) + "," + str(o.nb));
}
static void arg(const char *k, const sfa::WarpJobs &J) {
    std::string s = str(J.n);
    for (int i = 0; i < J.n; i++) s += " [" + str(J.job[i].src_off) + "," + str(J.job[i].dst_off) + "," + str(J.job[i].mask_off) + "," + str(J.job[i].factor) + "]";
    put(k, s);
}
static void arg(const char *k, const sfa::AssembleArgs &a) {
    std::string s = str(a.n);
    for (int i = 0; i < a.n; i++) {
        const sfa::Term &t = a.t[i];
        s += " [" + str(t.stack_off) + "," + str(t.mask_off) + "," + bytes(&t.hd, 4) + "," + bytes(&t.hg, 4) + "," + bytes(&t.s, 4) + "," + str(t.is_ref) + "," +
             str(t.i1_off) + "," + str(t.i2_off) + "," + str(t.backward) + "]";
    }
    s += " dt_norm " + str(a.dt_norm) + " chw " + ptr(a.chw) + "," + str(a.chw_pl) + "," + str(a.chw_es) + "," + str(a.chw_pitch) + "," + str(a.chw_stride0) + "," +
         str(a.lstride) + " acc " + str(a.accumulate) + " lap " + str(a.do_laplacian) + " data_norm " + bytes(&a.data_norm, 4) + " one_dir " + str(a.one_direction) +
         " zero_duv " + str(a.zero_duv) + " chain_ok " + str(a.chain_ok);
    put(k, s);
    arg("color", a.color);
    arg("grad", a.grad);
    arg("op", a.op);
}
static void arg(const char *k, const sfa::OccArgs &a) { put(k, bytes(&a, sizeof a)); }
static void arg(const char *k, const sfa::PackSrc &a) {
    put(k, ptr(a.p) + "," + str(a.dtype) + "," + str(a.sw) + "," + str(a.sf) + "," + str(a.sc) + "," + str(a.sr) + "," + str(a.sx));
}
static void arg(const char *k, const sfa::MosaicSrc &a) { put(k, ptr(a.p)); }
static void arg(const char *k, const sfa::MosaicDst &a) { put(k, ptr(a.p)); }
static void arg(const char *k, sfa::SorWorkspace &w) { put(k, "ws" + std::to_string(w.w) + "x" + std::to_string(w.h)); }
static void arg(const char *k, const long long *v) { put(k, v ? "strides" : "null"); }
static void arg(const char *k, const double *v) { put(k, ptr(v)); }

// ---- launchers that have to act for the host logic to be exercised ----
static void special_launch_set_mask(sfa_ctx *c, const sfa::WMask &v) { memcpy(c->d_amask, &v, sizeof v); }
static void special_launch_outer_threshold(sfa_ctx *c, const sfa::Geo &g, const double *, float thres, const float *, const float *) {
    sfa::WMask m;
    memcpy(&m, c->d_amask, sizeof m);
    for (int b = 0; b < g.nb; b++)
        if (g.active.test(b) && m.test(b))
            for (int k = 0; k < 2; k++) c->d_last->last[2 * b + k] = 0.001 * (double)(++g_counter);
    if (thres > 0 && ++g_counter % 3 == 0) {      // every third call a window meets the outer threshold
        m.clear((int)(g_counter / 3 % g.nb));
        memcpy(c->d_amask, &m, sizeof m);
    }
}
static void norms(const sfa::Geo &g, double *red) {
    static const double f[5] = {2.0, 1.0, 0.5, 1.0003, 3.0};
    for (int b = 0; b < g.nb; b++)
        if (g.active.test(b)) {      // above, at, below, within the band of and above the inner threshold in turn
            const double v = (double)g.w * g.h * g_mock_thres * f[(g_counter++) % 5];
            red[2 * b] = v;
            red[2 * b + 1] = 0.9 * v;
        }
}
typedef const float *CF;
static void special_launch_update_inner(sfa_ctx *, const sfa::Geo &g, float *, float *, CF, CF, CF, CF, CF, CF, double *red, float *, float *) { norms(g, red); }
static void special_launch_update_inner_x(sfa_ctx *, const sfa::Geo &g, float *, float *, CF, CF, const sfa::SorOperandOut &, CF, CF, float *, float *, double *red, float *,
                                          float *) {
    norms(g, red);
}
static void special_launch_update_outer_x(sfa_ctx *, const sfa::Geo &g, float *, float *, float *, float *, const sfa::SorOperandOut &, double *red, float *, float *) {
    norms(g, red);
}
static void special_launch_update_outer(sfa_ctx *, const sfa::Geo &g, float *, float *, CF, CF, double *red, float *, float *) { norms(g, red); }
static void special_launch_exact_norms(sfa_ctx *, const sfa::Geo &g, const float *, const float *, const sfa::WMask &which, float *out) {
    for (int b = 0; b < g.nb; b++)
        if (which.test(b)) out[2 * b] = out[2 * b + 1] = (float)(g_mock_thres * ((g_counter++) % 2 ? 0.5 : 2.0));
}
static void special_sor_operand_target(sfa_ctx *, sfa::SorWorkspace &ws, const sfa::Geo &g, int K, sfa::SorOperandOut *out) {
    if (!ws.sa.p) {
        ws.sa.p = bump(4096);
        ws.sb.p = bump(4096);
        ws.x.p = bump(4096);
        ws.flags.p = bump(4096);
    }
    out->sa = (float4 *)ws.sa.p;
    out->sb = (float4 *)ws.sb.p;
    out->x = (unsigned long long *)ws.x.p;
    out->flags = (unsigned *)ws.flags.p;
    out->ent = (long)g.w * g.h;
    out->RP = g.w;
    out->G = K;
    out->ntasks = 3;
    out->nb = g.nb;
}
namespace sfa {
#include "launchers.inc"
int SorWorkspace::configure(sfa_ctx *, int, int, int, int) { return SFA_OK; }
}
// ---- the HIP runtime ----
static unsigned long g_ev = 0;
static std::string evs(hipEvent_t e) { return "ev" + std::to_string((unsigned long)(uintptr_t)e); }
extern "C" {
hipError_t hipMalloc(void **p, size_t n) { *p = bump(n); begin("hipMalloc"); arg("n", n); arg("p", *p); end(); return hipSuccess; }
hipError_t hipFree(void *p) { begin("hipFree"); arg("p", p); end(); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { *p = bump(n); begin("hipHostMalloc"); arg("n", n); end(); return hipSuccess; }
hipError_t hipHostFree(void *) { return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t) {
    memcpy(d, s, n);
    begin("hipMemcpyAsync"); arg("dst", d); arg("src", s); arg("n", n); arg("kind", (int)k); end();
    return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind k, hipStream_t) {
    for (size_t y = 0; y < h; y++) memcpy((char *)d + y * dp, (const char *)s + y * sp, w);
    begin("hipMemcpy2DAsync"); arg("dst", d); arg("dp", dp); arg("src", s); arg("sp", sp); arg("w", w); arg("h", h); arg("kind", (int)k); end();
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { memset(d, v, n); begin("hipMemsetAsync"); arg("dst", d); arg("v", v); arg("n", n); end(); return hipSuccess; }
hipError_t hipMemset(void *d, int v, size_t n) { memset(d, v, n); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { begin("hipStreamSynchronize"); end(); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { begin("hipEventSynchronize"); put("e", evs(e)); end(); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { begin("hipEventRecord"); put("e", evs(e)); end(); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)(uintptr_t)(++g_ev); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)(uintptr_t)(++g_ev); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)(uintptr_t)1; return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t *p, int) { memset(p, 0, sizeof *p); p->multiProcessorCount = 256; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "mock"; }
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *, const void *) { return hipErrorInvalidValue; }
hipError_t hipMemGetAddressRange(hipDeviceptr_t *, size_t *, hipDeviceptr_t) { return hipErrorInvalidValue; }
}
