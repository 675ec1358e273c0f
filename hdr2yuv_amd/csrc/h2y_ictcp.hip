/*
 * h2y_ictcp.hip -- the ICtCp pass of include/hdr2yuv_hip.h ("ICtCp"), on the device.
 *
 *   k_ictcp<IN>  planes G, B, R of float (F32) or half (F16) samples of display light -> float planes of code-valued I, Ct, Cp
 *                samples: BT.2100's LMS (k / 4096), PQ10000_r through the forward conversion's own destination-stage tiers (code1,
 *                h2y_light1.h), the ICtCp matrix and H.273's scale step with the rounding half and the clamp
 *                (h2y_ictcp_batch, and in place on a forward ring's decoded F32 planes: h2y_stream_ictcp)
 *
 * k_hlg's walk.  A pixel is three tiered PQ evaluations, as a pixel of k_linearize is, and 24 algorithmic bytes: the pass is bound
 * by that arithmetic, not by its bytes.  PQ10000_r's table is staged in LDS as k_deltae stages it (51 KB), so three blocks fit a
 * CU's 160 KB and the launch asks for no more (h2y_ictcp_grid); with blocks of 512 threads that is six waves a SIMD, which leaves a
 * wave 80 VGPRs.  Chosen by that reasoning and by k_deltae's measurement that the LDS copy beats reading the table through the cache
 * (DESIGN.md 7.22), not measured against other block sizes.  This file is built -ffp-contract=off: every product, sum and
 * difference is rounded by itself.  Default cache policy on both sides, as k_gamut.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_math.h"
#include "h2y_device.h"
#include "h2y_light1.h"
#include "h2y_planes.h"

namespace {

__device__ __forceinline__ float clean01(float v) { return v > 0.0f ? fminf(v, 1.0f) : 0.0f; }

/* one code-valued sample: the product, the offset, the rounding half, the clamp to [0, 2^n - 1] */
__device__ __forceinline__ float to_code(float v, float mul, float add, float top)
{
    return fminf(fmaxf(((v * mul) + add) + 0.5f, 0.0f), top);
}

/* one pixel, in place in g, b, r: display light in, code-valued I, Ct, Cp out */
__device__ __forceinline__ void ictcp_pixel(const ictcp_args &a, const pq_recA *tab_r, float &g, float &b, float &r)
{
    const float G = clean01(g), B = clean01(b), R = clean01(r);
    /* BT.2100 LMS, k / 4096: Delta E ITP's step 2 */
    const float l = clean01(((1688.0f / 4096.0f) * R + (2146.0f / 4096.0f) * G) + (262.0f / 4096.0f) * B);
    const float m = clean01(((683.0f / 4096.0f) * R + (2951.0f / 4096.0f) * G) + (462.0f / 4096.0f) * B);
    const float s = clean01(((99.0f / 4096.0f) * R + (309.0f / 4096.0f) * G) + (3688.0f / 4096.0f) * B);
    const float lp = code1(a.pp, tab_r, l), mp = code1(a.pp, tab_r, m), sp = code1(a.pp, tab_r, s);
    const float I = 0.5f * lp + 0.5f * mp;
    const float Ct = ((6610.0f / 4096.0f) * lp - (13613.0f / 4096.0f) * mp) + (7003.0f / 4096.0f) * sp;
    const float Cp = ((17933.0f / 4096.0f) * lp - (17390.0f / 4096.0f) * mp) - (543.0f / 4096.0f) * sp;
    g = to_code(I, a.oY, a.aY, a.top);
    b = to_code(Ct, a.oC, a.aC, a.top);
    r = to_code(Cp, a.oC, a.aC, a.top);
}

/* k_hlg's walk: grid-stride over (frame, chunk of H2Y_ICTCP_THREADS groups) units; a group is the 4 float or 8 half pixels of one
 * 16-byte read, and a frame's last chunk also takes its npix % 4 (8) single pixels.  With F32 a destination plane may be its source
 * plane: every thread has read the three samples of a pixel before it writes any of them, and no pixel belongs to two threads.
 * code1's tiers vote over the lanes that are at work. */
template <int IN>
__global__ __launch_bounds__(H2Y_ICTCP_THREADS) void k_ictcp(ictcp_args a, const gamut_frame *frames, int n_frames)
{
    typedef plane_sample<IN> S;
    typedef plane_sample<H2Y_IN_F32> D;
    typedef typename S::bits bits;
    constexpr uint32_t G = S::per_group, T = H2Y_ICTCP_THREADS;
    __shared__ pq_recA s_tab[2 * H2Y_PQ_NREC]; /* PQ10000_r's table: A records, then B records */
    stage_table<H2Y_ICTCP_THREADS>(a.table_r, s_tab);
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
#pragma unroll
            for (uint32_t k = 0; k < G; k++) ictcp_pixel(a, s_tab, g[k], b[k], r[k]);
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
            ictcp_pixel(a, s_tab, g, b, r);
            dg[j] = D::narrow(g), db[j] = D::narrow(b), dr[j] = D::narrow(r);
        }
    }
}

} // namespace

uint32_t h2y_ictcp_chunks(int in_kind, uint32_t npix)
{
    const uint32_t G = in_kind == H2Y_IN_F16 ? 8u : 4u, groups = npix / G, tail = npix - groups * G;
    return (groups + tail + (uint32_t)H2Y_ICTCP_THREADS - 1u) / (uint32_t)H2Y_ICTCP_THREADS;
}

int h2y_ictcp_grid(int n_cu, uint64_t units)
{
    const uint64_t max_grid = (uint64_t)n_cu * 3u; /* what the table in LDS leaves room for */
    return (int)(units < max_grid ? (units ? units : 1) : max_grid);
}

hipError_t h2y_launch_ictcp(int in_kind, int grid, hipStream_t st, const ictcp_args &a, const gamut_frame *frames, int n_frames)
{
    if (in_kind == H2Y_IN_F32) hipLaunchKernelGGL((k_ictcp<H2Y_IN_F32>), dim3(grid), dim3(H2Y_ICTCP_THREADS), 0, st, a, frames, n_frames);
    else if (in_kind == H2Y_IN_F16) hipLaunchKernelGGL((k_ictcp<H2Y_IN_F16>), dim3(grid), dim3(H2Y_ICTCP_THREADS), 0, st, a, frames, n_frames);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
