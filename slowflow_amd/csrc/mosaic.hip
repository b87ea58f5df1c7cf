// mosaic.hip -- raw Bayer ingest on the GPU (include/slowflow_amd.h: sfa_demosaic_device, sfa_sequence_upload_mosaic*, sfa_job_set_raw_weights): the two
// demosaicers the driver knows (raw_demosaicing 0: bayer2rgbGR, utils/utils.cpp:1242-1334; 2: cv::cvtColor(CV_Bayer*2RGB) on 8-bit data, slow_flow.cpp:502-520)
// and rawWeighting (utils.cpp:1336-1374), statement for statement as slowflow_amd/host/ingest.cpp restates them, so that a frame demosaiced here holds the bits
// of the same frame demosaiced on the host and uploaded.
//   - one launch covers n frames: a block owns a MOS_TX x MOS_TY tile of the DESTINATION (the crop), reads the mosaic once into LDS with a 2-pixel halo and
//     writes the three fp32 planes; the grid is k_pack_frames' (64 lanes x 4 waves, four rows per thread, frames in z) and so is the 64-bit stride arithmetic,
//   - every LDS tile is indexed by REAL mosaic coordinates.  The reference mirrors an index that leaves the image (x-1 -> x+1 at x = 0, x+1 -> x-1 at x = W-1)
//     and then uses the green of that real pixel, which was formed from that pixel's own (mirrored) neighbours in the order up, down, left, right.  A
//     reflected halo around the border pixel would add the same four numbers in another order -- other bits in fp32.  With real coordinates the green of a
//     pixel is one value whoever asks for it; mirrored indices stay within 1 of the pixel that asks, so green lies within 1 and the mosaic within 2 of the tile,
//   - the colour of a site follows from its coordinates in the FULL mosaic (x0 + x, y0 + y): a crop at an odd origin keeps the pattern,
//   - rounding: the host evaluates 0.25 * (float sum) and g * 0.5 * (float sum) as double products rounded once to float; the kernel does literally that
//     (fp64 multiply, one conversion).  The quotients S / G are IEEE fp32 divisions (correctly rounded, the library's flags); a zero green gives the host's Inf / NaN.
#include "sfa_internal.h"

namespace sfa {

constexpr int MOS_TX = 64, MOS_TY = 16;            // the tile (slowflow_amd.MOSAIC_TILE names it for the tests)
constexpr int MOS_WAVES = 4, MOS_ROWS = MOS_TY / MOS_WAVES;
constexpr int MOS_RW = MOS_TX + 4, MOS_RH = MOS_TY + 4;     // mosaic tile: 2-pixel halo
constexpr int MOS_GW = MOS_TX + 2, MOS_GH = MOS_TY + 2;     // green tile: 1-pixel halo

// (x > 0) ? x - 1 : x + 1 and (x < n - 1) ? x + 1 : x - 1 (utils.cpp:1244-1247)
__device__ __forceinline__ int mirror_m1(int v) { return v > 0 ? v - 1 : v + 1; }
__device__ __forceinline__ int mirror_p1(int v, int n) { return v < n - 1 ? v + 1 : v - 1; }

// the mosaic of the block's tile + halo, as floats at real coordinates [X0 - 2, X0 + MOS_TX + 2) x [Y0 - 2, Y0 + MOS_TY + 2); outside the mosaic: 0, never used
template <typename T>
__device__ __forceinline__ void load_mosaic_tile(float (*raw)[MOS_RW], const MosaicSrc &s, int X0, int Y0) {
    const T *src = static_cast<const T *>(s.p) + (long long)blockIdx.z * s.sf;
    for (int i = threadIdx.y * MOS_TX + threadIdx.x; i < MOS_RW * MOS_RH; i += MOS_TX * MOS_WAVES) {
        const int ly = i / MOS_RW, lx = i - ly * MOS_RW;
        const int X = X0 - 2 + lx, Y = Y0 - 2 + ly;
        raw[ly][lx] = (X >= 0 && X < s.W && Y >= 0 && Y < s.H) ? (float)src[(long long)Y * s.sr + (long long)X * s.sx] : 0.f;
    }
}

// the tiles by real mosaic coordinates (X, Y); (X0, Y0) is the real coordinate of the block's first output pixel
__device__ __forceinline__ float raw_at(const float (*raw)[MOS_RW], int X0, int Y0, int Y, int X) { return raw[Y - (Y0 - 2)][X - (X0 - 2)]; }
__device__ __forceinline__ float grn_at(const float (*grn)[MOS_GW], int X0, int Y0, int Y, int X) { return grn[Y - (Y0 - 1)][X - (X0 - 1)]; }

template <typename T>
__global__ void __launch_bounds__(MOS_TX *MOS_WAVES) k_demosaic_gr(MosaicSrc s, MosaicDst d, int red_x, int red_y) {
    __shared__ float raw[MOS_RH][MOS_RW];
    __shared__ float grn[MOS_GH][MOS_GW];
    const int X0 = s.x0 + blockIdx.x * MOS_TX, Y0 = s.y0 + blockIdx.y * MOS_TY;
    load_mosaic_tile<T>(raw, s, X0, Y0);
    __syncthreads();
#define RAW_(Y, X) raw_at(raw, X0, Y0, Y, X)
#define GRN_(Y, X) grn_at(grn, X0, Y0, Y, X)
    // green first (utils.cpp:1242-1276): at every real pixel of the tile + 1, from that pixel's own neighbours
    for (int i = threadIdx.y * MOS_TX + threadIdx.x; i < MOS_GW * MOS_GH; i += MOS_TX * MOS_WAVES) {
        const int gy = i / MOS_GW, gx = i - gy * MOS_GW;
        const int X = X0 - 1 + gx, Y = Y0 - 1 + gy;
        float g = 0.f;
        if (X >= 0 && X < s.W && Y >= 0 && Y < s.H) {
            const bool blue_row = ((Y + (1 - red_y)) & 1) == 0;
            const bool green = blue_row ? ((X + red_x) & 1) == 0 : ((X + (1 - red_x)) & 1) == 0;
            if (green) g = RAW_(Y, X);
            else {
                const int xm1 = mirror_m1(X), xp1 = mirror_p1(X, s.W), ym1 = mirror_m1(Y), yp1 = mirror_p1(Y, s.H);
                const float sum = RAW_(ym1, X) + RAW_(yp1, X) + RAW_(Y, xm1) + RAW_(Y, xp1);
                g = (float)(0.25 * sum);
            }
        }
        grn[gy][gx] = g;
    }
    __syncthreads();
    // red and blue through the green ratio (:1279-1333)
    const int x = blockIdx.x * MOS_TX + threadIdx.x;
    if (x >= d.w) return;
    const int X = s.x0 + x, xm1 = mirror_m1(X), xp1 = mirror_p1(X, s.W);
    float *dst = d.p + (long long)blockIdx.z * d.sf + (long long)x * d.sx;
#pragma unroll
    for (int k = 0; k < MOS_ROWS; k++) {
        const int y = blockIdx.y * MOS_TY + threadIdx.y + k * MOS_WAVES;
        if (y >= d.h) continue;
        const int Y = s.y0 + y, ym1 = mirror_m1(Y), yp1 = mirror_p1(Y, s.H);
        const float g = GRN_(Y, X), c = RAW_(Y, X);
        const bool blue_row = ((Y + (1 - red_y)) & 1) == 0;
        const bool green = blue_row ? ((X + red_x) & 1) == 0 : ((X + (1 - red_x)) & 1) == 0;
        float r, b;
        if (green) {
            const float vs = RAW_(ym1, X) / GRN_(ym1, X) + RAW_(yp1, X) / GRN_(yp1, X);
            const float hs = RAW_(Y, xm1) / GRN_(Y, xm1) + RAW_(Y, xp1) / GRN_(Y, xp1);
            const float vert = (float)(g * 0.5 * vs), horz = (float)(g * 0.5 * hs);
            r = blue_row ? vert : horz;
            b = blue_row ? horz : vert;
        } else {
            const float ds = RAW_(ym1, xm1) / GRN_(ym1, xm1) + RAW_(ym1, xp1) / GRN_(ym1, xp1) + RAW_(yp1, xm1) / GRN_(yp1, xm1) + RAW_(yp1, xp1) / GRN_(yp1, xp1);
            const float diag = (float)(g * 0.25 * ds);
            r = blue_row ? diag : c;
            b = blue_row ? c : diag;
        }
        float *o = dst + (long long)y * d.sr;
        __builtin_nontemporal_store(r, o);
        __builtin_nontemporal_store(g, o + d.sc);
        __builtin_nontemporal_store(b, o + 2 * d.sc);
    }
#undef GRN_
#undef RAW_
}

// cvRound (lrintf under the default rounding mode: half to even) and saturate_cast<uchar>, as ingest.cpp:66-67 evaluates them: a NaN or a value beyond the
// range of a 64-bit integer converts to the most negative integer there, hence to 0
__device__ __forceinline__ int round_u8(float v) {
    const float r = rintf(v);
    if (!(r >= 0.f && r < 9.2233720368547758e18f)) return 0;
    return r > 255.f ? 255 : (int)r;
}

template <typename T>
__global__ void __launch_bounds__(MOS_TX *MOS_WAVES) k_demosaic_cv8u(MosaicSrc s, MosaicDst d, int red_x, int red_y) {
    __shared__ float raw[MOS_RH][MOS_RW];
    const int X0 = s.x0 + blockIdx.x * MOS_TX, Y0 = s.y0 + blockIdx.y * MOS_TY;
    const bool empty = s.W < 3 || s.H < 3;                  // no interior: nothing to interpolate from (all zeros)
    if (!empty) {
        load_mosaic_tile<T>(raw, s, X0, Y0);
        __syncthreads();
    }
    const int x = blockIdx.x * MOS_TX + threadIdx.x;
    if (x >= d.w) return;
    // the outer ring repeats its inner neighbours, rows first, then columns: pixel (x, y) holds the interior pixel nearest to it
    const int X = min(max(s.x0 + x, 1), s.W - 2);
    const bool red_col = ((X - red_x) & 1) == 0;
    float *dst = d.p + (long long)blockIdx.z * d.sf + (long long)x * d.sx;
#define M_(Y, X) round_u8(raw_at(raw, X0, Y0, Y, X))
#pragma unroll
    for (int k = 0; k < MOS_ROWS; k++) {
        const int y = blockIdx.y * MOS_TY + threadIdx.y + k * MOS_WAVES;
        if (y >= d.h) continue;
        int r = 0, g = 0, b = 0;
        if (!empty) {
            const int Y = min(max(s.y0 + y, 1), s.H - 2);
            const bool red_row = ((Y - red_y) & 1) == 0;
            const int c = M_(Y, X);
            if (red_row == red_col) {                       // a red or a blue site
                const int cross = (M_(Y - 1, X) + M_(Y + 1, X) + M_(Y, X - 1) + M_(Y, X + 1) + 2) >> 2;
                const int diag = (M_(Y - 1, X - 1) + M_(Y - 1, X + 1) + M_(Y + 1, X - 1) + M_(Y + 1, X + 1) + 2) >> 2;
                g = cross; r = red_row ? c : diag; b = red_row ? diag : c;
            } else {                                        // a green site: its row's colour left and right, the other one above and below
                const int horiz = (M_(Y, X - 1) + M_(Y, X + 1) + 1) >> 1, vert = (M_(Y - 1, X) + M_(Y + 1, X) + 1) >> 1;
                g = c; r = red_row ? horiz : vert; b = red_row ? vert : horiz;
            }
        }
        float *o = dst + (long long)y * d.sr;
        __builtin_nontemporal_store((float)r, o);
        __builtin_nontemporal_store((float)g, o + d.sc);
        __builtin_nontemporal_store((float)b, o + 2 * d.sc);
    }
#undef M_
}

// rawWeighting (utils.cpp:1336-1374) into the channel-weight planes of a job's windows: rows of `stride` floats (the level-0 host geometry the data term
// indexes linearly) at pitch cp; the padding columns [w, stride) hold 1, what the driver's planes hold there (slow_flow.cpp:597-598)
__global__ void __launch_bounds__(MOS_TX *MOS_WAVES) k_raw_weights(float *__restrict__ chw, long es, long pl, int cp, int stride, int w, int h, int red_x, int red_y,
                                                                  float weight, float other) {
    const int x = blockIdx.x * MOS_TX + threadIdx.x;
    if (x >= stride) return;
    float *dst = chw + (long)blockIdx.z * es + x;
#pragma unroll
    for (int k = 0; k < MOS_ROWS; k++) {
        const int y = blockIdx.y * MOS_TY + threadIdx.y + k * MOS_WAVES;
        if (y >= h) continue;
        float r = 1.f, g = 1.f, b = 1.f;
        if (x < w) {
            r = g = b = other;
            if (((y + (1 - red_y)) & 1) == 0) {             // blue row (:1342)
                const bool green = (red_y == 1 && ((x + (1 - red_x)) & 1) == 0) || (red_y == 0 && ((x + red_x) & 1) == 0);
                if (green) g = weight; else b = weight;
            } else {                                        // red row (:1357)
                const bool green = (red_y == 0 && ((x + (1 - red_x)) & 1) == 0) || (red_y == 1 && ((x + red_x) & 1) == 0);
                if (green) g = weight; else r = weight;
            }
        }
        float *o = dst + (long)y * cp;
        o[0] = r; o[pl] = g; o[2 * pl] = b;
    }
}

template <typename T>
static void launch_demosaic_t(sfa_ctx *c, const MosaicSrc &s, const MosaicDst &d, int n, int method, int red_x, int red_y) {
    const dim3 grid((d.w + MOS_TX - 1) / MOS_TX, (d.h + MOS_TY - 1) / MOS_TY, n), blk(MOS_TX, MOS_WAVES);
    if (method == 2) hipLaunchKernelGGL(k_demosaic_cv8u<T>, grid, blk, 0, c->stream, s, d, red_x, red_y);
    else hipLaunchKernelGGL(k_demosaic_gr<T>, grid, blk, 0, c->stream, s, d, red_x, red_y);
}

void launch_demosaic(sfa_ctx *c, const MosaicSrc &src, const MosaicDst &dst, int n, int method, int red_x, int red_y) {
    const size_t elem = src.dtype == SFA_DEV_F32 ? 4 : src.dtype == SFA_DEV_U16 ? 2 : 1;
    const int chunk = 32768;                                // frames in the grid's z: below 65536
    for (int i = 0; i < n; i += chunk) {
        MosaicSrc s = src;
        MosaicDst d = dst;
        s.p = static_cast<const char *>(src.p) + (size_t)i * src.sf * elem;
        d.p = dst.p + (long long)i * dst.sf;
        const int m = n - i < chunk ? n - i : chunk;
        if (src.dtype == SFA_DEV_U8) launch_demosaic_t<unsigned char>(c, s, d, m, method, red_x, red_y);
        else if (src.dtype == SFA_DEV_U16) launch_demosaic_t<unsigned short>(c, s, d, m, method, red_x, red_y);
        else launch_demosaic_t<float>(c, s, d, m, method, red_x, red_y);
    }
}

void launch_raw_weights(sfa_ctx *c, float *chw, long es, long pl, int cp, int stride, int w, int h, int nwin, int red_x, int red_y, float weight) {
    weight = fminf(fmaxf(weight, 0.0f), 3.0f);              // utils.cpp:1337
    const float other = 0.5f * (3 - weight);
    const dim3 grid((stride + MOS_TX - 1) / MOS_TX, (h + MOS_TY - 1) / MOS_TY, nwin);
    hipLaunchKernelGGL(k_raw_weights, grid, dim3(MOS_TX, MOS_WAVES), 0, c->stream, chw, es, pl, cp, stride, w, h, red_x, red_y, weight, other);
}

}  // namespace sfa
