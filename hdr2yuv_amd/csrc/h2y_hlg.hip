/*
 * h2y_hlg.hip -- the HLG pass of include/hdr2yuv_hip.h ("HLG"), on the device.
 *
 *   k_hlg<IN>  planes G, B, R of float (F32) or half (F16) samples of display light -> float planes of code-valued HLG samples:
 *              BT.2100's inverse OOTF and OETF read from two tables, then the conversion's scale step (h2y_hlg1.h has the pixel)
 *              (h2y_hlg_batch, and in place on a forward ring's decoded F32 planes: h2y_stream_hlg)
 *
 * The tables and every check stay on the host (h2y_hlg_tables in h2y_measure.hip).  A streaming pass with k_tonemap's walk, and
 * up to four gathers of two neighbouring entries per pixel in between: one in the gain table at the pixel's luminance (at 256
 * times it below the table's first node), one per
 * channel in the OETF's table.  The block copies both into LDS once, before its first unit: the H2Y_LIGHTDIST_BINS gains (34 KiB)
 * and the 2049 entries of the OETF's table from the node of 2^-4 up (8 KiB) -- the logarithmic branch starts above 1/12, so
 * nothing below is ever read.  Together 42 KiB: three blocks fit a CU's 160 KiB, one fewer than k_tonemap has, and the launch asks
 * for no more (h2y_hlg_grid).  The blocks have 512 threads, so a SIMD holds six waves (35 VGPRs: the LDS is what limits it).
 * Measured on an MI355X over 64 4K F32 frames (tools/streambench.py hlg): with blocks of 256, three waves a SIMD, 48.1 us a frame,
 * 1.22 times k_tonemap's time in the same job; with 512, 41.0 us, 1.10 times.  Keeping the tables in LDS rather than gathering
 * through L2, and the table's size, were chosen by reasoning and not measured against the alternatives.  Default cache policy on
 * both sides, as k_gamut.
 */
#include <hip/hip_runtime.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_planes.h"
#include "h2y_hlg1.h"

/* k_gamut's walk with wider blocks: grid-stride over (frame, chunk of H2Y_HLG_THREADS groups) units; a group is the 4 float or 8 half pixels of one 16-byte
 * read, and a frame's last chunk also takes its npix % 4 (8) single pixels.  One 16-byte load per source plane and group and one
 * 16-byte store per 4 pixels and destination plane where the frame's six planes are 16-byte aligned, single samples elsewhere.
 * With F32 a destination plane may be its source plane: every thread has read the three samples of a pixel before it writes any
 * of them, and no pixel belongs to two threads. */
template <int IN>
__global__ __launch_bounds__(H2Y_HLG_THREADS) void k_hlg(hlg_args a, const gamut_frame *frames, int n_frames)
{
    typedef plane_sample<IN> S;
    typedef plane_sample<H2Y_IN_F32> D;
    typedef typename S::bits bits;
    constexpr uint32_t G = S::per_group, T = H2Y_HLG_THREADS;
    __shared__ float s_gain[H2Y_HLG_NODES];
    __shared__ float s_oetf[H2Y_HLG_OETF_NODES];
    for (uint32_t w = threadIdx.x; w < (uint32_t)H2Y_HLG_NODES; w += (uint32_t)H2Y_HLG_THREADS) s_gain[w] = a.gain[w];
    for (uint32_t w = threadIdx.x; w < (uint32_t)H2Y_HLG_OETF_NODES; w += (uint32_t)H2Y_HLG_THREADS) s_oetf[w] = a.oetf[H2Y_HLG_OETF_FIRST + w];
    __syncthreads();
    const uint32_t groups = a.npix / G, tail = a.npix - groups * G;
    const uint32_t chunks = (groups + tail + T - 1u) / T, units = (uint32_t)n_frames * chunks;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t f = unit / chunks, i = (unit - f * chunks) * T + threadIdx.x;
        const gamut_frame fr = frames[f];
        const H2Y_GLOBAL bits *sg = (const H2Y_GLOBAL bits *)fr.src[0], *sb = (const H2Y_GLOBAL bits *)fr.src[1],
                              *sr = (const H2Y_GLOBAL bits *)fr.src[2];
        H2Y_GLOBAL uint32_t *dg = (H2Y_GLOBAL uint32_t *)fr.dst[0], *db = (H2Y_GLOBAL uint32_t *)fr.dst[1],
                            *dr = (H2Y_GLOBAL uint32_t *)fr.dst[2];
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
            for (uint32_t k = 0; k < G; k++) hlg_pixel(s_gain, s_oetf, a.c, g[k], b[k], r[k]);
            if (vec16) {
                for (uint32_t q = 0; q < G; q += 4u) { /* F16: the 8 pixels of a read are two 16-byte stores of floats a plane */
                    *reinterpret_cast<H2Y_GLOBAL u32x4 *>(dg + o + q) = D::pack(g + q);
                    *reinterpret_cast<H2Y_GLOBAL u32x4 *>(db + o + q) = D::pack(b + q);
                    *reinterpret_cast<H2Y_GLOBAL u32x4 *>(dr + o + q) = D::pack(r + q);
                }
            } else
                for (uint32_t k = 0; k < G; k++) dg[o + k] = D::narrow(g[k]), db[o + k] = D::narrow(b[k]), dr[o + k] = D::narrow(r[k]);
        } else if (i < groups + tail) {
            const size_t j = (size_t)groups * G + (i - groups);
            float g = S::widen(sg[j]), b = S::widen(sb[j]), r = S::widen(sr[j]);
            hlg_pixel(s_gain, s_oetf, a.c, g, b, r);
            dg[j] = D::narrow(g), db[j] = D::narrow(b), dr[j] = D::narrow(r);
        }
    }
}

uint32_t h2y_hlg_chunks(int in_kind, uint32_t npix)
{
    const uint32_t G = in_kind == H2Y_IN_F16 ? 8u : 4u, groups = npix / G, tail = npix - groups * G;
    return (groups + tail + (uint32_t)H2Y_HLG_THREADS - 1u) / (uint32_t)H2Y_HLG_THREADS;
}

int h2y_hlg_grid(int n_cu, uint64_t units)
{
    const uint64_t max_grid = (uint64_t)n_cu * 3u; /* what the two LDS tables leave room for */
    return (int)(units < max_grid ? (units ? units : 1) : max_grid);
}

hipError_t h2y_launch_hlg(int in_kind, int grid, hipStream_t st, const hlg_args &a, const gamut_frame *frames, int n_frames)
{
    if (in_kind == H2Y_IN_F32) hipLaunchKernelGGL((k_hlg<H2Y_IN_F32>), dim3(grid), dim3(H2Y_HLG_THREADS), 0, st, a, frames, n_frames);
    else if (in_kind == H2Y_IN_F16) hipLaunchKernelGGL((k_hlg<H2Y_IN_F16>), dim3(grid), dim3(H2Y_HLG_THREADS), 0, st, a, frames, n_frames);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
