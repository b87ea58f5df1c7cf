// the same jobs through the C-ABI for whichever library code is linked in; prints the log of every launch, copy, memset, event and synchronisation
#include "slowflow_amd.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
extern std::string g_log;       // mock.cpp
extern bool g_mock_bool;
extern double g_mock_thres;
extern "C" int sfa_debug_set(const char *, const char *);
struct Case {
    const char *sw;      // a debug switch set for the case, or null
    int S, one_dir, alter, outer, inner, order, occ, layers;
    float tho, thi, sigma;
    int nb, w, h, verbose, occlog, chw, mockbool;
    float omega0;
};
int main() {
    sfa_ctx *c = nullptr;
    if (sfa_ctx_create(0, &c) != SFA_OK) { printf("ctx: %s\n", sfa_last_error(nullptr)); return 1; }
    std::vector<Case> cases;
    const char *sws[] = {nullptr, "SFA_UNFUSED", "SFA_NO_DIRECT_OPERANDS", "SFA_NO_UV_ALIAS", "SFA_NO_EXACT_BREAK", "SFA_PYRAMID_UNFUSED", "SFA_SHARE_SOR", "SFA_DEBUG_ACTIVE"};
    for (const char *sw : sws)
        for (int S = 2; S <= 3; S++)
            for (int inner = 1; inner <= 3; inner += 1)
                for (int th = 0; th < 4; th++)
                    for (int v = 0; v < 2; v++)
                        for (int order = 0; order < 2; order++) {
                            Case k;      // th: bit 0 an outer, bit 1 an inner threshold; v: verbose + presmoothing; the rest varies with them
                            k.sw = sw; k.S = S; k.inner = inner; k.order = order; k.verbose = v;
                            k.one_dir = (S + inner + th) % 3 == 0;
                            k.alter = 1 + (th + v) % 3;
                            k.outer = th & 1 ? 7 : 3;
                            k.occ = (inner + v) & 1;
                            k.layers = 1 + (th & 1);
                            k.tho = th & 1 ? 2e-3f : 0.f;
                            k.thi = th & 2 ? 1e-3f : 0.f;
                            k.sigma = v ? 0.8f : 0.f;
                            k.nb = S == 2 ? 3 : 2; k.w = S == 2 ? 67 : 130; k.h = S == 2 ? 45 : 70;
                            k.occlog = (th >> 1) & 1;
                            k.chw = inner == 2;
                            k.mockbool = !(v && order);
                            k.omega0 = S == 3 ? 0.5f : 0.f;
                            cases.push_back(k);
                        }
    int idx = 0;
    for (const Case &k : cases) {
        g_log.clear();
        if (k.sw) sfa_debug_set(k.sw, "1");
        g_mock_bool = k.mockbool;
        g_mock_thres = k.thi > 0 ? k.thi : 1.0;
        sfa_params p;
        sfa_params_default(&p);
        p.S = k.S; p.one_direction = k.one_dir; p.niter_alter = k.alter; p.niter_outer = k.outer; p.niter_inner = k.inner; p.sor_order = k.order;
        p.occlusion_reasoning = k.occ; p.layers = k.layers; p.p_scale = 0.7f; p.thres_outer = k.tho; p.thres_inner = k.thi; p.presmooth_sigma = k.sigma;
        p.omega[0] = k.omega0;
        sfa_ctx_set_verbose(c, k.verbose);
        sfa_job *j = nullptr;
        int rc = sfa_job_create(c, &p, k.w, k.h, k.nb, &j);
        const int F = 2 * (k.S - 1) + 1, stride = (k.w + 3) / 4 * 4;
        std::vector<float> img((size_t)3 * stride * k.h, 0.5f), fl((size_t)stride * k.h, 0.25f);
        std::vector<const float *> fr(F, img.data());
        const float *chw[3] = {fl.data(), fl.data(), fl.data()};
        if (rc == SFA_OK && k.occlog) rc = sfa_job_keep_alternation_occlusions(j, 1);
        for (int b = 0; rc == SFA_OK && b < k.nb; b++)      // initial flow planes and channel weights present or not, window by window
            rc = sfa_job_upload(j, b, fr.data(), F, b ? fl.data() : nullptr, b == 1 ? nullptr : fl.data(), stride, (k.chw && b != 1) ? chw : nullptr);
        if (rc == SFA_OK && k.chw) rc = sfa_job_set_raw_weights(j, 0, k.nb, 1, 0, 0.5f);
        if (rc == SFA_OK) rc = sfa_job_run(j);
        if (rc == SFA_OK) rc = sfa_job_run(j);
        float ch[2] = {0, 0};
        std::vector<float> ox(fl.size()), oy(fl.size());
        for (int b = 0; rc == SFA_OK && b < k.nb; b++) rc = sfa_job_download(j, b, ox.data(), oy.data(), stride, ch);
        if (rc == SFA_OK) rc = sfa_job_download_occlusions(j, 0, ox.data(), stride);
        if (rc == SFA_OK) rc = sfa_variational(c, &p, ox.data(), oy.data(), k.w, k.h, stride, fr.data(), F, k.chw ? chw : nullptr, oy.data(), ch);
        if (rc == SFA_OK) rc = sfa_compute_one_level(c, &p, ox.data(), oy.data(), k.w, k.h, stride, fr.data(), F, nullptr, nullptr, ch);
        printf("==== case %d sw %s S %d inner %d outer %d alter %d order %d tho %g thi %g verbose %d rc %d %s change %g %g\n", idx++, k.sw ? k.sw : "-", k.S, k.inner,
               k.outer, k.alter, k.order, k.tho, k.thi, k.verbose, rc, rc ? sfa_last_error(c) : "", ch[0], ch[1]);
        fputs(g_log.c_str(), stdout);
        if (j) sfa_job_destroy(j);
        if (k.sw) sfa_debug_set(k.sw, nullptr);
    }
    sfa_ctx_destroy(c);
    return 0;
}
