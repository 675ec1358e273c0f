/*
 * h2y_gamut.hip -- the conversion between colour primaries of include/hdr2yuv_hip.h, on the device.
 *
 *   k_gamut<IN>  planes G, B, R of float (F32) or half (F16) samples -> the same planes in the destination's primaries
 *                (h2y_gamut_batch, and in place on a forward ring's decoded planes: h2y_stream_gamut)
 *
 * The matrix and every check stay on the host (h2y_gamut_matrix in h2y_measure.hip).  A pure streaming pass: three planes in, three
 * planes out, nine multiplies and six adds per pixel in between, each rounded on its own (__fmul_rn / __fadd_rn: never contracted
 * into a fused multiply-add, whatever the build's flags).  Default cache policy on both sides, as k_dpx_decode and k_tiff_decode:
 * in place the store goes to the line the load just brought in, and what the pass leaves in the caches is what pic_stats and the
 * conversion read next.
 */
#include <hip/hip_runtime.h>

#include "h2y_kernels.h"
#include "h2y_planes.h"

namespace {

/* (r, g, b) -> o = M (r, g, b), clipped at 0 where asked: o[0] = R', o[1] = G', o[2] = B' */
__device__ __forceinline__ void gamut_pixel(const gamut_args &a, float r, float g, float b, float o[3])
{
    for (int i = 0; i < 3; i++) {
        const float s = __fadd_rn(__fadd_rn(__fmul_rn(a.m[3 * i], r), __fmul_rn(a.m[3 * i + 1], g)), __fmul_rn(a.m[3 * i + 2], b));
        o[i] = a.clip ? (s > 0.0f ? s : 0.0f) : s; /* a NaN, -0.0 and every negative: +0.0 */
    }
}

} // namespace

/* Grid-stride over (frame, chunk of 256 groups) units; a group is the 4 float or 8 half pixels of one 16-byte access, and a frame's
 * last chunk also takes its npix % 4 (8) single pixels.  The frame is block-uniform: its pointers are scalar loads from the table.
 * One 16-byte load and one 16-byte store per plane and group where the frame's six planes are 16-byte aligned, single samples
 * elsewhere.  A destination plane may be its source plane: every thread has read the three samples of a pixel before it writes
 * any of them, and no pixel belongs to two threads. */
template <int IN>
__global__ __launch_bounds__(256) void k_gamut(gamut_args a, const gamut_frame *frames, int n_frames)
{
    typedef plane_sample<IN> S;
    typedef typename S::bits bits;
    constexpr uint32_t G = S::per_group;
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
            for (uint32_t k = 0; k < G; k++) {
                float out[3];
                gamut_pixel(a, r[k], g[k], b[k], out);
                r[k] = out[0], g[k] = out[1], b[k] = out[2];
            }
            if (vec16) {
                *reinterpret_cast<H2Y_GLOBAL u32x4 *>(dg + o) = S::pack(g);
                *reinterpret_cast<H2Y_GLOBAL u32x4 *>(db + o) = S::pack(b);
                *reinterpret_cast<H2Y_GLOBAL u32x4 *>(dr + o) = S::pack(r);
            } else
                for (uint32_t k = 0; k < G; k++) dg[o + k] = (bits)S::narrow(g[k]), db[o + k] = (bits)S::narrow(b[k]), dr[o + k] = (bits)S::narrow(r[k]);
        } else if (i < groups + tail) {
            const size_t j = (size_t)groups * G + (i - groups);
            const float g = S::widen(sg[j]), b = S::widen(sb[j]), r = S::widen(sr[j]);
            float out[3];
            gamut_pixel(a, r, g, b, out);
            dg[j] = (bits)S::narrow(out[1]), db[j] = (bits)S::narrow(out[2]), dr[j] = (bits)S::narrow(out[0]);
        }
    }
}

uint32_t h2y_gamut_chunks(int in_kind, uint32_t npix)
{
    const uint32_t per_group = in_kind == H2Y_IN_F16 ? 8u : 4u;
    return (npix / per_group + npix % per_group + 255u) / 256u;
}

hipError_t h2y_launch_gamut(int in_kind, int grid, hipStream_t st, const gamut_args &a, const gamut_frame *frames, int n_frames)
{
    if (in_kind == H2Y_IN_F32) hipLaunchKernelGGL((k_gamut<H2Y_IN_F32>), dim3(grid), dim3(256), 0, st, a, frames, n_frames);
    else if (in_kind == H2Y_IN_F16) hipLaunchKernelGGL((k_gamut<H2Y_IN_F16>), dim3(grid), dim3(256), 0, st, a, frames, n_frames);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
