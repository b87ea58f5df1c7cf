// device_io.hip -- the device seam: frames, initial flow and results that already live in GPU memory (include/slowflow_amd.h: sfa_job_upload_device,
// sfa_job_set_flow_device, sfa_job_download_device, sfa_sequence_upload_device).  Three kernels that convert ((float) of the element) and move, nothing
// else: a job filled by them holds the bits of the same job filled by the host copies.  One launch per call instead of a copy per plane.
//   - the caller's side is addressed with 64-bit element strides (a view into a large tensor can lie beyond 2^31 elements); the job's side with the
//     offsets the job itself uses (pitch, pl, element stride es: job.hip Level::layout),
//   - columns >= width of the job's planes are never written (the project's rule for padding lanes: they keep what the job put there),
//   - the job reads the packed planes only later (the pyramid of the next sfa_job_run, after every window of the call has been packed: 2 GB at
//     128 windows), so they leave as non-temporal stores -- what k_warp_smooth's warped images taught (the kernel waited for its write
//     path, and its neighbours gained more than it did),
//   - a thread issues the loads of its four rows before the first store, so that no load queues behind a store in the wave's in-order memory counter.
// The checks of the arguments (strides, overlap: dev_view.h; device pointers of this GPU: api.hip's check_view) come first: nothing here is launched on a
// refused argument.
#include "sfa_internal.h"

namespace sfa {

typedef float v4f_ __attribute__((ext_vector_type(4)));

constexpr int IO_X = 64, IO_Y = 4, IO_ROWS = 4;      // a block: 64 lanes x 4 waves, every thread IO_ROWS rows IO_Y apart: 64 columns (or quads) x 16 rows

struct PackDst { float *p; long es, pl; int pitch, w, h, F; };

// plane z of the launch -> the source and destination offsets of its first pixel
__device__ __forceinline__ void plane_of(int z, int F, const PackSrc &s, const PackDst &d, long long *so, long *dof) {
    const int c = z % 3, wf = z / 3, f = wf % F, wi = wf / F;
    *so = (long long)wi * s.sw + (long long)f * s.sf + (long long)c * s.sc;
    *dof = (long)wi * d.es + ((long)f * 3 + c) * d.pl;
}

// any layout: one element per thread and row; coalesced where the column stride is 1
template <typename T>
__global__ void __launch_bounds__(IO_X *IO_Y) k_pack_frames(PackSrc s, PackDst d) {
    const int x = blockIdx.x * IO_X + threadIdx.x, y0 = blockIdx.y * (IO_Y * IO_ROWS) + threadIdx.y;
    if (x >= d.w) return;
    long long so; long dof;
    plane_of(blockIdx.z, d.F, s, d, &so, &dof);
    const T *src = static_cast<const T *>(s.p) + so + (long long)x * s.sx;
    float v[IO_ROWS];
#pragma unroll
    for (int i = 0; i < IO_ROWS; i++) { const int y = y0 + i * IO_Y; v[i] = y < d.h ? (float)src[(long long)y * s.sr] : 0.f; }
#pragma unroll
    for (int i = 0; i < IO_ROWS; i++) { const int y = y0 + i * IO_Y; if (y < d.h) __builtin_nontemporal_store(v[i], d.p + dof + (long)y * d.pitch + x); }
}

// interleaved colour (channel stride 1, column stride 3: [B,F,H,W,3]): a thread reads the three consecutive elements of its pixel -- a wave reads 192
// consecutive elements, every fetched line is used whole -- and writes one element of each of the three planes, 64 consecutive floats per wave and plane
template <typename T>
__global__ void __launch_bounds__(IO_X *IO_Y) k_pack_frames_interleaved(PackSrc s, PackDst d) {
    const int x = blockIdx.x * IO_X + threadIdx.x, y0 = blockIdx.y * (IO_Y * IO_ROWS) + threadIdx.y;
    if (x >= d.w) return;
    const int f = blockIdx.z % d.F, wi = blockIdx.z / d.F;
    const T *src = static_cast<const T *>(s.p) + (long long)wi * s.sw + (long long)f * s.sf + (long long)x * 3;
    float *dst = d.p + (long)wi * d.es + (long)f * 3 * d.pl + x;
    float v[IO_ROWS][3];
#pragma unroll
    for (int i = 0; i < IO_ROWS; i++) {
        const int y = y0 + i * IO_Y;
#pragma unroll
        for (int c = 0; c < 3; c++) v[i][c] = y < d.h ? (float)src[(long long)y * s.sr + c] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < IO_ROWS; i++) {
        const int y = y0 + i * IO_Y;
#pragma unroll
        for (int c = 0; c < 3; c++)
            if (y < d.h) __builtin_nontemporal_store(v[i][c], dst + c * d.pl + (long)y * d.pitch);
    }
}

// planar fp32, column stride 1, every other stride and the base a multiple of four elements: 128-bit loads and stores, a quad of columns per thread; the
// quad that straddles the width goes element by element (columns >= width are not written, and not read either: they may lie outside the caller's view)
__global__ void __launch_bounds__(IO_X *IO_Y) k_pack_frames_f32x4(PackSrc s, PackDst d) {
    const int x = (blockIdx.x * IO_X + threadIdx.x) * 4, y0 = blockIdx.y * (IO_Y * IO_ROWS) + threadIdx.y;
    if (x >= d.w) return;
    long long so; long dof;
    plane_of(blockIdx.z, d.F, s, d, &so, &dof);
    const float *src = static_cast<const float *>(s.p) + so + x;
    float *dst = d.p + dof + x;
    if (x + 4 <= d.w) {
        v4f_ v[IO_ROWS];
#pragma unroll
        for (int i = 0; i < IO_ROWS; i++) {
            const int y = y0 + i * IO_Y;
            v[i] = y < d.h ? *reinterpret_cast<const v4f_ *>(src + (long long)y * s.sr) : (v4f_){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < IO_ROWS; i++) { const int y = y0 + i * IO_Y; if (y < d.h) __builtin_nontemporal_store(v[i], reinterpret_cast<v4f_ *>(dst + (long)y * d.pitch)); }
    } else {
        for (int i = 0; i < IO_ROWS; i++) {
            const int y = y0 + i * IO_Y;
            if (y >= d.h) break;
            for (int k = 0; x + k < d.w; k++) __builtin_nontemporal_store(src[(long long)y * s.sr + k], dst + (long)y * d.pitch + k);
        }
    }
}

// the initial flow [B,2,H,W] (strided fp32) into init_flow; src null: zeros
__global__ void __launch_bounds__(IO_X *IO_Y) k_pack_flow(const float *__restrict__ src, long long sw, long long sp, long long sr, long long sx, float *__restrict__ dst,
                                                         long dst_es, long pl, int pitch, int w, int h) {
    const int x = blockIdx.x * IO_X + threadIdx.x, y0 = blockIdx.y * (IO_Y * IO_ROWS) + threadIdx.y;
    if (x >= w) return;
    const int p = blockIdx.z & 1, wi = blockIdx.z >> 1;
    const float *s = src ? src + (long long)wi * sw + (long long)p * sp + (long long)x * sx : nullptr;
    float *d = dst + (long)wi * dst_es + (long)p * pl + x;
    float v[IO_ROWS];
#pragma unroll
    for (int i = 0; i < IO_ROWS; i++) { const int y = y0 + i * IO_Y; v[i] = (s && y < h) ? s[(long long)y * sr] : 0.f; }
#pragma unroll
    for (int i = 0; i < IO_ROWS; i++) { const int y = y0 + i * IO_Y; if (y < h) __builtin_nontemporal_store(v[i], d + (long)y * pitch); }
}

// P_WX, P_WY (and P_OCC) of the windows of the launch into the caller's strided fp32 destinations; plane z % np of window z / np
struct UnpackArgs {
    const float *src[3]; long src_es; int pitch, w, h, np;
    float *flow; long long fw, fp, fr, fx;
    float *occ; long long ow, orow, ox;
};
__global__ void __launch_bounds__(IO_X *IO_Y) k_unpack_planes(UnpackArgs a) {
    const int x = blockIdx.x * IO_X + threadIdx.x, y0 = blockIdx.y * (IO_Y * IO_ROWS) + threadIdx.y;
    if (x >= a.w) return;
    const int p = blockIdx.z % a.np, wi = blockIdx.z / a.np;
    const float *s = a.src[p] + (long)wi * a.src_es + x;
    float *d;
    long long dr;
    if (p < 2) { d = a.flow + (long long)wi * a.fw + (long long)p * a.fp + (long long)x * a.fx; dr = a.fr; }
    else { d = a.occ + (long long)wi * a.ow + (long long)x * a.ox; dr = a.orow; }
    float v[IO_ROWS];
#pragma unroll
    for (int i = 0; i < IO_ROWS; i++) { const int y = y0 + i * IO_Y; v[i] = y < a.h ? s[(long)y * a.pitch] : 0.f; }
#pragma unroll
    for (int i = 0; i < IO_ROWS; i++) { const int y = y0 + i * IO_Y; if (y < a.h) d[(long long)y * dr] = v[i]; }
}
// the same with 128-bit accesses: column stride 1, every other stride of both destinations and their bases a multiple of four floats
__global__ void __launch_bounds__(IO_X *IO_Y) k_unpack_planes_x4(UnpackArgs a) {
    const int x = (blockIdx.x * IO_X + threadIdx.x) * 4, y0 = blockIdx.y * (IO_Y * IO_ROWS) + threadIdx.y;
    if (x >= a.w) return;
    const int p = blockIdx.z % a.np, wi = blockIdx.z / a.np;
    const float *s = a.src[p] + (long)wi * a.src_es + x;
    float *d;
    long long dr;
    if (p < 2) { d = a.flow + (long long)wi * a.fw + (long long)p * a.fp + x; dr = a.fr; }
    else { d = a.occ + (long long)wi * a.ow + x; dr = a.orow; }
    v4f_ v[IO_ROWS];                                  // the job's rows are 256-byte aligned and pitch >= width rounded up to 64: the quad is inside the row
#pragma unroll
    for (int i = 0; i < IO_ROWS; i++) { const int y = y0 + i * IO_Y; v[i] = y < a.h ? *reinterpret_cast<const v4f_ *>(s + (long)y * a.pitch) : (v4f_){0.f, 0.f, 0.f, 0.f}; }
    if (x + 4 <= a.w) {
#pragma unroll
        for (int i = 0; i < IO_ROWS; i++) { const int y = y0 + i * IO_Y; if (y < a.h) *reinterpret_cast<v4f_ *>(d + (long long)y * dr) = v[i]; }
    } else {
        for (int i = 0; i < IO_ROWS; i++) {
            const int y = y0 + i * IO_Y;
            if (y >= a.h) break;
            for (int k = 0; x + k < a.w; k++) d[(long long)y * dr + k] = v[i][k];
        }
    }
}

static dim3 io_grid(int columns, int h, int planes) { return dim3((columns + IO_X - 1) / IO_X, (h + IO_Y * IO_ROWS - 1) / (IO_Y * IO_ROWS), planes); }
static bool quad_aligned(const void *p, std::initializer_list<long long> strides) {
    if (reinterpret_cast<uintptr_t>(p) & 15) return false;
    for (long long s : strides) if (s & 3) return false;
    return true;
}

void launch_pack_frames(sfa_ctx *c, float *dst, long dst_es, long pl, int pitch, int w, int h, int nwin, int F, const PackSrc &s) {
    const PackDst d{dst, dst_es, pl, pitch, w, h, F};
    const dim3 blk(IO_X, IO_Y);
    if (s.sc == 1 && s.sx == 3) {
        const dim3 g = io_grid(w, h, nwin * F);
        if (s.dtype == SFA_DEV_U8) hipLaunchKernelGGL(k_pack_frames_interleaved<unsigned char>, g, blk, 0, c->stream, s, d);
        else if (s.dtype == SFA_DEV_U16) hipLaunchKernelGGL(k_pack_frames_interleaved<unsigned short>, g, blk, 0, c->stream, s, d);
        else hipLaunchKernelGGL(k_pack_frames_interleaved<float>, g, blk, 0, c->stream, s, d);
    } else if (s.dtype == SFA_DEV_F32 && s.sx == 1 && quad_aligned(s.p, {s.sw, s.sf, s.sc, s.sr})) {
        hipLaunchKernelGGL(k_pack_frames_f32x4, io_grid((w + 3) / 4, h, nwin * F * 3), blk, 0, c->stream, s, d);
    } else {
        const dim3 g = io_grid(w, h, nwin * F * 3);
        if (s.dtype == SFA_DEV_U8) hipLaunchKernelGGL(k_pack_frames<unsigned char>, g, blk, 0, c->stream, s, d);
        else if (s.dtype == SFA_DEV_U16) hipLaunchKernelGGL(k_pack_frames<unsigned short>, g, blk, 0, c->stream, s, d);
        else hipLaunchKernelGGL(k_pack_frames<float>, g, blk, 0, c->stream, s, d);
    }
}

void launch_pack_flow(sfa_ctx *c, float *dst, long dst_es, long pl, int pitch, int w, int h, int nwin, const float *src, const long long st[4]) {
    hipLaunchKernelGGL(k_pack_flow, io_grid(w, h, nwin * 2), dim3(IO_X, IO_Y), 0, c->stream, src, src ? st[0] : 0, src ? st[1] : 0, src ? st[2] : 0, src ? st[3] : 0,
                       dst, dst_es, pl, pitch, w, h);
}

void launch_unpack_planes(sfa_ctx *c, const float *wx, const float *wy, const float *occ, long src_es, int pitch, int w, int h, int nwin, float *flow,
                          const long long st[4], float *occ_dst, const long long ost[3]) {
    UnpackArgs a{};
    a.src[0] = wx; a.src[1] = wy; a.src[2] = occ; a.src_es = src_es; a.pitch = pitch; a.w = w; a.h = h; a.np = occ_dst ? 3 : 2;
    a.flow = flow; a.fw = st[0]; a.fp = st[1]; a.fr = st[2]; a.fx = st[3];
    a.occ = occ_dst;
    if (occ_dst) { a.ow = ost[0]; a.orow = ost[1]; a.ox = ost[2]; }
    const bool x4 = st[3] == 1 && quad_aligned(flow, {st[0], st[1], st[2]}) && (!occ_dst || (ost[2] == 1 && quad_aligned(occ_dst, {ost[0], ost[1]})));
    if (x4) hipLaunchKernelGGL(k_unpack_planes_x4, io_grid((w + 3) / 4, h, nwin * a.np), dim3(IO_X, IO_Y), 0, c->stream, a);
    else hipLaunchKernelGGL(k_unpack_planes, io_grid(w, h, nwin * a.np), dim3(IO_X, IO_Y), 0, c->stream, a);
}

}  // namespace sfa
