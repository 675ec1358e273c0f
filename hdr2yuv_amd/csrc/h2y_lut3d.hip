/*
 * h2y_lut3d.hip -- the 3D LUT pass of include/hdr2yuv_hip.h ("3D LUT"), on the device.
 *
 *   k_lut3d<IN, INTERP, SIGNAL>      planes G, B, R of float (F32) or half (F16) samples -> the table's value at (R, G, B),
 *                                    interpolated between the nodes of one cell: tetrahedral (four nodes) or trilinear (eight); in
 *                                    planes mode stored in the source's type, in signal mode clamped, scaled to code values and
 *                                    stored as floats (h2y_lut3d1.h has the pixel)
 *   k_lut3d_lds<IN, INTERP, SIGNAL>  the same for a table of up to 17 nodes per axis, read from the block's copy in LDS
 *                                    (h2y_lut3d_batch, and in place on a forward ring's decoded planes: h2y_stream_lut3d)
 *
 * The parser and every check stay on the host (h2y_measure.hip).  A streaming pass with k_gamut's walk and a data-dependent gather
 * in between.  A table of 33^3 nodes (575 KB at 16 bytes a node) is too big for LDS, so k_lut3d reads it from device memory through
 * L2: a node is 16 bytes (r, g, b and a pad), so a corner is one 16-byte load, four a pixel tetrahedral and eight trilinear.  A
 * thread owns the 4 float or 8 half pixels of one 16-byte access; the pixels are independent, so their gathers are in flight
 * together.  Measured on an MI355X over 64 4K frames (tools/streambench.py lut3d): on pictures whose neighbouring
 * pixels share a cell the pass runs near k_tonemap's time; on uniformly random samples every lane of a gather touches another
 * cache line and the vector cache's rate of lines, not L2's bytes, is the limit -- N = 17, whose table would fit two L1s, is barely
 * faster than N = 33.  k_lut3d_lds answers that for N <= 17: 17^3 nodes x 12 bytes = 59 KB, two blocks of 1024 threads a CU.
 * Default cache policy on both sides, as k_gamut.
 */
#include <hip/hip_runtime.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_planes.h"
#include "h2y_lut3d1.h"

namespace {

constexpr uint32_t kLdsNodes = H2Y_LUT3D_LDS_MAX_N * H2Y_LUT3D_LDS_MAX_N * H2Y_LUT3D_LDS_MAX_N;

/* k_gamut's walk with blocks of TH threads: grid-stride over (frame, chunk of TH groups) units; a group is the 4 float or 8 half
 * pixels of one 16-byte read, and a frame's last chunk also takes its npix % 4 (8) single pixels.  One 16-byte load per source plane
 * and group and one 16-byte store per destination plane and 4 floats or 8 halves where the frame's six planes are 16-byte aligned,
 * single samples elsewhere.  A destination plane of the source's type may be its source plane: every thread has read the three
 * samples of a pixel before it writes any of them, and no pixel belongs to two threads. */
template <int IN, int INTERP, int SIGNAL, uint32_t TH, typename TAB>
__device__ __forceinline__ void lut3d_walk(const TAB &T, const lut3d_args &a, const gamut_frame *frames, int n_frames)
{
    typedef plane_sample<IN> S;
    typedef plane_sample<SIGNAL ? H2Y_IN_F32 : IN> D;
    typedef typename S::bits sbits;
    typedef typename D::bits dbits;
    constexpr uint32_t G = S::per_group, DG = D::per_group;
    const uint32_t groups = a.npix / G, tail = a.npix - groups * G;
    const uint32_t chunks = (groups + tail + TH - 1u) / TH, units = (uint32_t)n_frames * chunks;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t f = unit / chunks, i = (unit - f * chunks) * TH + threadIdx.x;
        const gamut_frame fr = frames[f];
        const H2Y_GLOBAL sbits *sg = (const H2Y_GLOBAL sbits *)fr.src[0], *sb = (const H2Y_GLOBAL sbits *)fr.src[1],
                               *sr = (const H2Y_GLOBAL sbits *)fr.src[2];
        H2Y_GLOBAL dbits *dg = (H2Y_GLOBAL dbits *)fr.dst[0], *db = (H2Y_GLOBAL dbits *)fr.dst[1], *dr = (H2Y_GLOBAL dbits *)fr.dst[2];
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
            for (uint32_t k = 0; k < G; k++) lut3d_pixel<INTERP, SIGNAL>(T, a.c, g[k], b[k], r[k]);
            if (vec16) {
                for (uint32_t q = 0; q < G; q += DG) { /* F16 in signal mode: the 8 pixels of a read are two stores of floats a plane */
                    *reinterpret_cast<H2Y_GLOBAL u32x4 *>(dg + o + q) = D::pack(g + q);
                    *reinterpret_cast<H2Y_GLOBAL u32x4 *>(db + o + q) = D::pack(b + q);
                    *reinterpret_cast<H2Y_GLOBAL u32x4 *>(dr + o + q) = D::pack(r + q);
                }
            } else
                for (uint32_t k = 0; k < G; k++) dg[o + k] = (dbits)D::narrow(g[k]), db[o + k] = (dbits)D::narrow(b[k]), dr[o + k] = (dbits)D::narrow(r[k]);
        } else if (i < groups + tail) {
            const size_t j = (size_t)groups * G + (i - groups);
            float g = S::widen(sg[j]), b = S::widen(sb[j]), r = S::widen(sr[j]);
            lut3d_pixel<INTERP, SIGNAL>(T, a.c, g, b, r);
            dg[j] = (dbits)D::narrow(g), db[j] = (dbits)D::narrow(b), dr[j] = (dbits)D::narrow(r);
        }
    }
}

} // namespace

template <int IN, int INTERP, int SIGNAL>
__global__ __launch_bounds__(256) void k_lut3d(lut3d_args a, const gamut_frame *frames, int n_frames)
{
    lut3d_walk<IN, INTERP, SIGNAL, 256u>(lut3d_nodes16{a.nodes}, a, frames, n_frames);
}

/* a.c.n <= H2Y_LUT3D_LDS_MAX_N (the launcher checks): the block copies the n^3 nodes, 12 bytes each, into LDS before its first unit */
template <int IN, int INTERP, int SIGNAL>
__global__ __launch_bounds__(H2Y_LUT3D_LDS_THREADS, IN == H2Y_IN_F32 ? 8 : 4) void k_lut3d_lds(lut3d_args a, const gamut_frame *frames, int n_frames)
{
    __shared__ float s_nodes[3u * kLdsNodes];
    const uint32_t count = a.c.n * a.c.n * a.c.n;
    for (uint32_t w = threadIdx.x; w < count; w += (uint32_t)H2Y_LUT3D_LDS_THREADS) {
        const lut3d_node v = a.nodes[w];
        s_nodes[3u * w] = v.r, s_nodes[3u * w + 1u] = v.g, s_nodes[3u * w + 2u] = v.b;
    }
    __syncthreads();
    lut3d_walk<IN, INTERP, SIGNAL, (uint32_t)H2Y_LUT3D_LDS_THREADS>(lut3d_nodes12{s_nodes}, a, frames, n_frames);
}

uint32_t h2y_lut3d_chunks(int lds, int in_kind, uint32_t npix)
{
    const uint32_t G = in_kind == H2Y_IN_F16 ? 8u : 4u, groups = npix / G, tail = npix - groups * G;
    const uint32_t th = lds ? (uint32_t)H2Y_LUT3D_LDS_THREADS : 256u;
    return (groups + tail + th - 1u) / th;
}

int h2y_lut3d_grid(int n_cu, int lds, uint64_t units)
{
    const uint64_t max_grid = (uint64_t)n_cu * (lds ? 2u : 8u); /* what the LDS table leaves room for; eight blocks of 256 otherwise */
    return (int)(units < max_grid ? (units ? units : 1) : max_grid);
}

template <int IN>
static void launch_in(int interp, int signal, int lds, int grid, hipStream_t st, const lut3d_args &a, const gamut_frame *frames, int n_frames)
{
    const dim3 g(grid), b(256), bl(H2Y_LUT3D_LDS_THREADS);
    if (lds) {
        if (interp && signal) hipLaunchKernelGGL((k_lut3d_lds<IN, 1, 1>), g, bl, 0, st, a, frames, n_frames);
        else if (interp) hipLaunchKernelGGL((k_lut3d_lds<IN, 1, 0>), g, bl, 0, st, a, frames, n_frames);
        else if (signal) hipLaunchKernelGGL((k_lut3d_lds<IN, 0, 1>), g, bl, 0, st, a, frames, n_frames);
        else hipLaunchKernelGGL((k_lut3d_lds<IN, 0, 0>), g, bl, 0, st, a, frames, n_frames);
    } else if (interp && signal) hipLaunchKernelGGL((k_lut3d<IN, 1, 1>), g, b, 0, st, a, frames, n_frames);
    else if (interp) hipLaunchKernelGGL((k_lut3d<IN, 1, 0>), g, b, 0, st, a, frames, n_frames);
    else if (signal) hipLaunchKernelGGL((k_lut3d<IN, 0, 1>), g, b, 0, st, a, frames, n_frames);
    else hipLaunchKernelGGL((k_lut3d<IN, 0, 0>), g, b, 0, st, a, frames, n_frames);
}

hipError_t h2y_launch_lut3d(int in_kind, int interp, int signal, int lds, int grid, hipStream_t st, const lut3d_args &a,
                            const gamut_frame *frames, int n_frames)
{
    if ((interp != 0 && interp != 1) || (signal != 0 && signal != 1) || !a.nodes || a.c.n < 2u || a.c.n > 128u) return hipErrorInvalidValue;
    if (lds && a.c.n > (uint32_t)H2Y_LUT3D_LDS_MAX_N) return hipErrorInvalidValue;
    if (in_kind == H2Y_IN_F32) launch_in<H2Y_IN_F32>(interp, signal, lds, grid, st, a, frames, n_frames);
    else if (in_kind == H2Y_IN_F16) launch_in<H2Y_IN_F16>(interp, signal, lds, grid, st, a, frames, n_frames);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
