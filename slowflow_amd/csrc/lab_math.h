// lab_math.h -- the per-pixel arithmetic of EpicFlow's L*a*b* image (host/epic.cpp: rgb8_to_lab's 8-bit step :19-28 and rgb_to_lab :57-73, which restates
// image.c:694-726), one function for host and device code.  Nothing from HIP and no call of a math library: the cube root and the exponential are written
// here from IEEE fp64 additions, multiplications, divisions and integer operations on the bit pattern, so the g++ build that tests/host/test_lab_math.cpp
// walks over all 2^24 8-bit triples and the gfx950 build inside k_rgb8_to_lab (csrc/epic_init.hip, -ffp-contract=off -fno-fast-math) are the same function.
// The host routine calls glibc's pow(., 1./3) and exp in double and rounds to float once; the two functions below come within a few hundredths of an ulp
// of the exact values before that rounding, and the exhaustive test shows that no float of the whole domain falls on the other side.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SFA_LAB_FN __host__ __device__ inline
#else
#define SFA_LAB_FN inline
#endif

namespace sfa {
namespace lab {

SFA_LAB_FN uint64_t bits_of(double x) { uint64_t u; __builtin_memcpy(&u, &x, sizeof u); return u; }
SFA_LAB_FN double double_of(uint64_t u) { double x; __builtin_memcpy(&x, &u, sizeof x); return x; }
SFA_LAB_FN uint32_t bits_of(float x) { uint32_t u; __builtin_memcpy(&u, &x, sizeof u); return u; }
SFA_LAB_FN float float_of(uint32_t u) { float x; __builtin_memcpy(&x, &u, sizeof x); return x; }

// nearbyintf in the default rounding mode: to nearest, ties to even; -0.0 for what rounds to zero from below; +-Inf and NaN as they are
SFA_LAB_FN float round_even(float v) {
    const uint32_t u = bits_of(v), sign = u & 0x80000000u;
    const float a = float_of(u & 0x7fffffffu);
    if (!(a < 8388608.0f)) return v;                                   // an integer already, Inf or NaN
    const float r = (a + 8388608.0f) - 8388608.0f;                     // the addition rounds at the unit place
    return float_of(bits_of(r) | sign);
}

// a * b = p + e exactly (Veltkamp's split, Dekker's product), for operands far from overflow
SFA_LAB_FN void two_prod(double a, double b, double *p, double *e) {
    const double ca = 134217729.0 * a, cb = 134217729.0 * b;
    const double ah = ca - (ca - a), al = a - ah, bh = cb - (cb - b), bl = b - bh;
    *p = a * b;
    *e = ((ah * bh - *p) + ah * bl + al * bh) + al * bl;
}

// pow(x, 1./3) for a normal x > 0 of moderate exponent (the conversion's X, Y and Z above T lie in (0.008856, 1.0001)).  The exponent 1./3 is the double below
// one third, 1/3 - 2^-54 / 3, so the value is cbrt(x) (1 - ln(x) 2^-54 / 3): up to 0.8 ulp above the cube root at the low end of that range.
SFA_LAB_FN double pow_third(double x) {
    double y = double_of(bits_of(x) / 3 + (715094163ull << 32));       // exponent / 3: within 5 %
    for (int i = 0; i < 5; i++) y = y - (y * y * y - x) / (3.0 * (y * y));   // Newton: 5e-2, 3e-3, 6e-6, 4e-11, then the last place
    double p1, e1, p2, e2;
    two_prod(y, y, &p1, &e1);                                          // y^3 = (p1 + e1) y = p2 + e2 + e1 y
    two_prod(p1, y, &p2, &e2);
    const double res = ((x - p2) - e2) - e1 * y;                       // x - y^3: the first difference is exact
    // ln(x) to 0.07: log2 of the mantissa m in [1, 2) taken as m - 1; a hundredth of an ulp of the result
    const uint64_t u = bits_of(x);
    const double m = double_of((u & 0x000fffffffffffffull) | 0x3ff0000000000000ull);
    const double ln = 0x1.62e42fefa39efp-1 * ((double)((int)(u >> 52) - 1023) + (m - 1.0));
    return y + (res / (3.0 * p1) - y * (0x1.5555555555555p-56 * ln));
}

// exp(z) for z in [-0.625, 0] (the conversion's argument is -1.5 q^2 with q in [-0.6, 0.4]: at least -0.54) and for NaN; NaN elsewhere.
// z = -n / 16 + r with |r| <= 1 / 32: exp(-n / 16) from a table of double-double values, exp(r) - 1 from its series to r^12.
SFA_LAB_FN double exp_neg(double z) {
    if (!(z >= -0.625 && z <= 0.0)) return (z - z) / (z - z);          // NaN
    const double tab[11][2] = {
        {0x1.0000000000000p+0, 0x0.0p+0},
        {0x1.e0fabfbc702a4p-1, -0x1.8d0e700fcfb65p-56},
        {0x1.c3d6a24ed8222p-1, -0x1.e1e0a76cb0685p-55},
        {0x1.a876812c0877cp-1, -0x1.fd36226fadd44p-56},
        {0x1.8ebef9eac820bp-1, -0x1.797d4686c5393p-57},
        {0x1.769652df22f7ep-1, 0x1.3445f7544e0efp-57},
        {0x1.5fe4615e98e8fp-1, -0x1.5613923fd9eeep-55},
        {0x1.4a9271936fd09p-1, -0x1.4edd8a92eb584p-56},
        {0x1.368b2fc6f960ap-1, -0x1.85314b9559e64p-61},
        {0x1.23ba930c1568bp-1, -0x1.b61343fc21a3bp-64},
        {0x1.120dc934993e8p-1, -0x1.5353ad174351dp-55},
    };
    const int n = (int)(0.5 - z * 16.0);                               // 0 .. 10
    const double r = z + (double)n * 0.0625;                           // exact for a z that came from a float
    double s = 0x1.1eed8eff8d898p-29;                                  // 1/12!, then Horner down to 1/2!
    s = s * r + 0x1.ae64567f544e4p-26;
    s = s * r + 0x1.27e4fb7789f5cp-22;
    s = s * r + 0x1.71de3a556c734p-19;
    s = s * r + 0x1.a01a01a01a01ap-16;
    s = s * r + 0x1.a01a01a01a01ap-13;
    s = s * r + 0x1.6c16c16c16c17p-10;
    s = s * r + 0x1.1111111111111p-7;
    s = s * r + 0x1.5555555555555p-5;
    s = s * r + 0x1.5555555555555p-3;
    s = s * r + 0.5;
    const double p = r + (r * r) * s;                                  // exp(r) - 1
    return tab[n][0] + (tab[n][1] + tab[n][0] * p);
}

// a sample as the 8-bit copy holds it (epic.cpp:22-23): times norm, cvRound (to nearest, ties to even), saturate_cast<uchar>; NaN stays NaN
SFA_LAB_FN float sample_8bit(float s, float norm) {
    const float v = round_even(s * norm);
    return v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
}

// One pixel of rgb8_to_lab(rgb, norm): (r, g, b) as the frame holds them -> L, a c, b c with c the colour attenuation of dark and light areas.
SFA_LAB_FN void rgb8_to_lab_pixel(float r_in, float g_in, float b_in, float norm, float *out_L, float *out_a, float *out_b) {
    const float c8[3] = {sample_8bit(r_in, norm), sample_8bit(g_in, norm), sample_8bit(b_in, norm)};
    const float T = 0.008856;                                          // :55-73, the statements in their order
    const float color_attenuation = 1.5f;
    const float r = c8[0] / 255.f, g = c8[1] / 255.f, b = c8[2] / 255.f;
    float X = 0.412453 * r + 0.357580 * g + 0.180423 * b;
    float Y = 0.212671 * r + 0.715160 * g + 0.072169 * b;
    float Z = 0.019334 * r + 0.119193 * g + 0.950227 * b;
    X /= 0.950456;
    Z /= 1.088754;
    const float Y3 = Y > T ? pow_third(Y) : 0.0f;                      // (the host forms it for every Y and reads it where Y > T)
    const float fX = X > T ? pow_third(X) : 7.787 * X + 16 / 116.;
    const float fY = Y > T ? Y3 : 7.787 * Y + 16 / 116.;
    const float fZ = Z > T ? pow_third(Z) : 7.787 * Z + 16 / 116.;
    const float L = Y > T ? 116 * Y3 - 16.0 : 903.3 * Y;
    const float A = 500 * (fX - fY), B = 200 * (fY - fZ);
    const float l2 = (L / 100) * (L / 100);
    const float q = l2 - 0.6;
    const float correct_lab = exp_neg(-color_attenuation * (q * q));
    *out_L = L; *out_a = A * correct_lab; *out_b = B * correct_lab;
}

}  // namespace lab
}  // namespace sfa
