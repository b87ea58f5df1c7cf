// hyp_device.h -- what the kernels over hypothesis lists share (fuse.hip, neigh.hip): which energy marks a slot as absent, and hypothesis::distance.
#pragma once
#include "sfa_device.h"

#pragma clang fp contract(off)

namespace sfa {

// +Inf marks "no hypothesis"; a NaN energy is absent too, as it is for k_track_best's `e < be` (track.hip): the reference's std::sort on a NaN score is
// undefined, so no parity is lost
__device__ __forceinline__ bool present(double e) { return e < __longlong_as_double(0x7ff0000000000000ll); }

// hypothesis::distance (utils/hypothesis.cpp:223-285) of two hypotheses after adaptFPS (startF 0, endF Jets: first 0, length Jets, prev_flow (0, 0)).
// a, b: the first of Jets doubles `step` apart.  ACC: sum sqrt(dx^2 + dy^2) / l; ADJ: the adjacent-step form, / length.  x - 0.0 is x, so the
// subtraction of prev_flow is left out.
static __device__ double traj_distance(const double *__restrict__ ua, const double *__restrict__ va, const double *__restrict__ ub, const double *__restrict__ vb,
                                       size_t step, int J, int method) {
    double sum = 0;
    double pua = 0, pva = 0, pub = 0, pvb = 0;
    for (int f = 0; f < J; f++) {
        const double a_u = ua[f * step], a_v = va[f * step], b_u = ub[f * step], b_v = vb[f * step];
        double xsq, ysq;
        if (method == 1) {                                                      // ACC
            ysq = a_v - b_v;
            xsq = a_u - b_u;
            sum += sqrt(xsq * xsq + ysq * ysq) / (f + 1);
        } else {                                                                // ADJ; flow_fm1 = (0, 0) at f == first
            ysq = ((a_v - pva) - (b_v - pvb));
            xsq = ((a_u - pua) - (b_u - pub));
            sum += sqrt(xsq * xsq + ysq * ysq);
            pua = a_u; pva = a_v; pub = b_u; pvb = b_v;
        }
    }
    if (method != 1) sum = sum / J;
    return sum;
}

}  // namespace sfa
