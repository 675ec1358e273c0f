/*
 * h2y_gamut_compress.hip -- the gamut compression pass of include/hdr2yuv_hip.h ("gamut compression"), on the device.
 *
 *   k_gamut_compress<IN>  planes G, B, R of float (F32) or half (F16) samples in linear light -> the same planes in the
 *                         destination's primaries, out-of-gamut colours rolled off toward the pixel's largest channel
 *                         (h2y_gamut_compress_batch, and in place on a forward ring's decoded planes: h2y_stream_gamut_compress)
 *
 * The matrix, the limits, the curves' tables and every check stay on the host (h2y_gamut_compress_curve in h2y_measure.hip): no pow
 * runs here.  One pixel is gamut_compress_pixel of h2y_gamut1.h, which the host twin compiles too.  k_gamut's matrix and the
 * compression in one trip of the planes through memory: a streaming pass as k_gamut is, with at most one gather of two neighbouring
 * table entries per channel in between.
 * The three tables (3 x 1025 floats, 12.3 KB) are copied into LDS once per block, before its first unit, as k_tonemap keeps its
 * table: the gather is data-dependent and divergent (only the lanes whose channel lies between the threshold and the limit read),
 * and from LDS it does not share the vector memory path with the six plane streams.  12.3 KB leaves room for the eight blocks of 256
 * threads a CU holds anyway, so the launch's shape is k_gamut's.  (The choice was made by reasoning, not by measuring it against a
 * gather through L2.)
 * Most pixels of a picture lie inside the threshold on all three channels: they leave gamut_compress_pixel after the matrix, one
 * maximum, one minimum, one product and a compare, without a quotient.  The branch behind it diverges per lane; a wave of in-gamut
 * pixels skips it whole.  Default cache policy on both sides, as k_gamut.
 */
#include <hip/hip_runtime.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_planes.h"
#include "h2y_gamut1.h"

namespace {

constexpr uint32_t kTable = 3u * H2Y_GAMUT_COMPRESS_NODES;

} // namespace

/* k_gamut's walk: grid-stride over (frame, chunk of 256 groups) units; a group is the 4 float or 8 half pixels of one 16-byte
 * access, and a frame's last chunk also takes its npix % 4 (8) single pixels.  One 16-byte load and one 16-byte store per plane and
 * group where the frame's six planes are 16-byte aligned, single samples elsewhere.  A destination plane may be its source plane:
 * every thread has read the three samples of a pixel before it writes any of them, and no pixel belongs to two threads. */
template <int IN>
__global__ __launch_bounds__(256) void k_gamut_compress(gamut_compress_args a, const gamut_frame *frames, int n_frames)
{
    typedef plane_sample<IN> S;
    typedef typename S::bits bits;
    constexpr uint32_t G = S::per_group;
    __shared__ float s_tab[kTable];
    for (uint32_t w = threadIdx.x; w < kTable; w += 256u) s_tab[w] = a.tables[w];
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
            for (uint32_t k = 0; k < G; k++) {
                float out[3];
                gamut_compress_pixel(a.c, s_tab, r[k], g[k], b[k], out);
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
            gamut_compress_pixel(a.c, s_tab, r, g, b, out);
            dg[j] = (bits)S::narrow(out[1]), db[j] = (bits)S::narrow(out[2]), dr[j] = (bits)S::narrow(out[0]);
        }
    }
}

hipError_t h2y_launch_gamut_compress(int in_kind, int grid, hipStream_t st, const gamut_compress_args &a, const gamut_frame *frames,
                                     int n_frames)
{
    if (in_kind == H2Y_IN_F32) hipLaunchKernelGGL((k_gamut_compress<H2Y_IN_F32>), dim3(grid), dim3(256), 0, st, a, frames, n_frames);
    else if (in_kind == H2Y_IN_F16) hipLaunchKernelGGL((k_gamut_compress<H2Y_IN_F16>), dim3(grid), dim3(256), 0, st, a, frames, n_frames);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
