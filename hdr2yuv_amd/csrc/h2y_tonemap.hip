/*
 * h2y_tonemap.hip -- the tone curve of include/hdr2yuv_hip.h ("tone mapping"), on the device.
 *
 *   k_tonemap<IN>  planes G, B, R of float (F32) or half (F16) samples in linear light -> the same planes, every pixel scaled by one
 *                  gain read from the curve's table at m = max(G, B, R)
 *                  (h2y_tonemap_batch, and in place on a forward ring's decoded planes: h2y_stream_tonemap)
 *
 * The curve and every check stay on the host (h2y_tonemap_curve in h2y_measure.hip): the kernel sees H2Y_LIGHTDIST_BINS binary32
 * gains on the nodes of bin_of's geometry and interpolates between two of them.  A streaming pass as k_gamut is, with one gather
 * per pixel in between.  The block copies the table (34 KiB) into LDS once, before its first unit, so the gather of two
 * neighbouring entries per pixel does not share the vector memory path with the six plane streams (the choice was made by
 * reasoning, not by measuring it against a gather through L2).  Four blocks of 256 threads fit a CU's 160 KiB; the launch asks
 * for no more (h2y_tonemap_grid).  Every product, difference and sum is rounded on its own
 * (__fmul_rn / __fsub_rn / __fadd_rn: never contracted, whatever the build's flags).  Default cache policy on both sides, as k_gamut.
 */
#include <hip/hip_runtime.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_planes.h"

namespace {

constexpr uint32_t kNodes = H2Y_LIGHTDIST_BINS, kLast = kNodes - 1u;

/* c > 0 ? min(c, 1) : +0: a NaN, -0.0 and every negative become +0.0, +inf becomes 1 */
__device__ __forceinline__ float tm_clamp(float c) { return c > 0.0f ? fminf(c, 1.0f) : 0.0f; }

/* one pixel, in place in g, b, r; T: the block's copy of the gains */
__device__ __forceinline__ void tonemap_pixel(const float *T, float cap, float &g, float &b, float &r)
{
    g = tm_clamp(g), b = tm_clamp(b), r = tm_clamp(r);
    const float m = fmaxf(fmaxf(g, b), r);
    const uint32_t e = __builtin_bit_cast(uint32_t, m);
    /* h2y_light1.h's bin_of: m <= 1, so k <= kLast whatever the planes hold */
    uint32_t k = e < H2Y_LIGHTDIST_FIRST_BITS ? 0u : ((e - H2Y_LIGHTDIST_FIRST_BITS) >> 14) + 1u;
    k = k < kLast ? k : kLast;
    const float lo = T[k], hi = T[k < kLast ? k + 1u : kLast];
    const float t = (float)(e & 0x3FFFu) * 0x1p-14f; /* exact */
    const float gain = (k == 0u || k == kLast) ? lo : __fadd_rn(lo, __fmul_rn(__fsub_rn(hi, lo), t));
    g = fminf(__fmul_rn(g, gain), cap), b = fminf(__fmul_rn(b, gain), cap), r = fminf(__fmul_rn(r, gain), cap);
}

} // namespace

/* k_gamut's walk: grid-stride over (frame, chunk of 256 groups) units; a group is the 4 float or 8 half pixels of one 16-byte
 * access, and a frame's last chunk also takes its npix % 4 (8) single pixels.  One 16-byte load and one 16-byte store per plane and
 * group where the frame's six planes are 16-byte aligned, single samples elsewhere.  A destination plane may be its source plane:
 * every thread has read the three samples of a pixel before it writes any of them, and no pixel belongs to two threads. */
template <int IN>
__global__ __launch_bounds__(256) void k_tonemap(tonemap_args a, const gamut_frame *frames, int n_frames)
{
    typedef plane_sample<IN> S;
    typedef typename S::bits bits;
    constexpr uint32_t G = S::per_group;
    __shared__ float s_gain[kNodes];
    for (uint32_t w = threadIdx.x; w < kNodes; w += 256u) s_gain[w] = a.gain[w];
    __syncthreads();
    const uint32_t groups = a.npix / G, tail = a.npix - groups * G;
    const uint32_t chunks = (groups + tail + 255u) / 256u, units = (uint32_t)n_frames * chunks;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t f = unit / chunks, i = (unit - f * chunks) * 256u + threadIdx.x;
        const gamut_frame fr = frames[f];
        const H2Y_GLOBAL bits *sg = (const H2Y_GLOBAL bits *)fr.src[0], *sb = (const H2Y_GLOBAL bits *)fr.src[1],
                              *sr = (const H2Y_GLOBAL bits *)fr.src[2];
        H2Y_GLOBAL bits *dg = (H2Y_GLOBAL bits *)fr.dst[0], *db = (H2Y_GLOBAL bits *)fr.dst[1], *dr = (H2Y_GLOBAL bits *)fr.dst[2];
        const bool vec16 = (((uintptr_t)sg | (uintptr_t)sb | (uintptr_t)sr | (uintptr_t)dg | (uintptr_t)db | (uintptr_t)dr) & 15u) == 0;
        if (i < groups) {
            const size_t o = (size_t)i * G;
            float g[G], b[G], r[G];
            if (vec16) {
                S::unpack(*reinterpret_cast<const H2Y_GLOBAL u32x4 *>(sg + o), g);
                S::unpack(*reinterpret_cast<const H2Y_GLOBAL u32x4 *>(sb + o), b);
                S::unpack(*reinterpret_cast<const H2Y_GLOBAL u32x4 *>(sr + o), r);
            } else
                for (uint32_t k = 0; k < G; k++) g[k] = S::widen(sg[o + k]), b[k] = S::widen(sb[o + k]), r[k] = S::widen(sr[o + k]);
            for (uint32_t k = 0; k < G; k++) tonemap_pixel(s_gain, a.cap, g[k], b[k], r[k]);
            if (vec16) {
                *reinterpret_cast<H2Y_GLOBAL u32x4 *>(dg + o) = S::pack(g);
                *reinterpret_cast<H2Y_GLOBAL u32x4 *>(db + o) = S::pack(b);
                *reinterpret_cast<H2Y_GLOBAL u32x4 *>(dr + o) = S::pack(r);
            } else
                for (uint32_t k = 0; k < G; k++) dg[o + k] = (bits)S::narrow(g[k]), db[o + k] = (bits)S::narrow(b[k]), dr[o + k] = (bits)S::narrow(r[k]);
        } else if (i < groups + tail) {
            const size_t j = (size_t)groups * G + (i - groups);
            float g = S::widen(sg[j]), b = S::widen(sb[j]), r = S::widen(sr[j]);
            tonemap_pixel(s_gain, a.cap, g, b, r);
            dg[j] = (bits)S::narrow(g), db[j] = (bits)S::narrow(b), dr[j] = (bits)S::narrow(r);
        }
    }
}

int h2y_tonemap_grid(int n_cu, uint64_t units)
{
    const uint64_t max_grid = (uint64_t)n_cu * 4u; /* what the LDS table leaves room for */
    return (int)(units < max_grid ? (units ? units : 1) : max_grid);
}

hipError_t h2y_launch_tonemap(int in_kind, int grid, hipStream_t st, const tonemap_args &a, const gamut_frame *frames, int n_frames)
{
    if (in_kind == H2Y_IN_F32) hipLaunchKernelGGL((k_tonemap<H2Y_IN_F32>), dim3(grid), dim3(256), 0, st, a, frames, n_frames);
    else if (in_kind == H2Y_IN_F16) hipLaunchKernelGGL((k_tonemap<H2Y_IN_F16>), dim3(grid), dim3(256), 0, st, a, frames, n_frames);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
