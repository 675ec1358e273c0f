/*
 * h2y_sdrsrc.hip -- a finished SDR master (BT.1886) placed in absolute light: frames of three u16 code planes, 4:4:4 (4:2:0 chroma
 * arrives upsampled by k_up444, h2y_resample.hip), into three binary32 planes G, B, R that hold L_G, L_B, L_R of
 * include/hdr2yuv_hip.h, "light of SDR code planes": Rep. ITU-R BT.2408's display-referred direct mapping, reference white at W
 * cd/m2.  Steps 2-3 are k_linearize's (code_primes of h2y_codepixel.h; this file is built -ffp-contract=off), step 5s is the forward
 * conversion's own BT.1886 source stage (light1<true> with H2Y_TFN_G24's table, its full-range table and the careful tier), step 6s
 * one product.
 *
 *   k_sdr_linearize<MATRIX>  k_linearize's walk and launch shape: (block column, frame) blocks; a block takes a contiguous share
 *                            of its frame's 8-pixel groups; a thread reads a group with one 16-byte load per plane whose start is
 *                            16-byte aligned (u16 loads for a plane that is not, and for the npix % 8 pixels behind the last
 *                            group, which the frame's last block takes) and writes it with two 16-byte stores per output plane;
 *                            the next step's codes are asked for first.  MATRIX 0: G, B, R planes; 1: BT.709; 9: BT.2020nc.
 *                            No reduction, no LDS, no atomics.
 *
 * Three table-tier evaluations per pixel, as in k_linearize, and one product more each: they bind the kernel, not its 18 bytes per
 * pixel.  Measured on an MI355X over 64 4K frames (tools/streambench.py sdrsrc): 73.8 us a 10-bit 4:4:4 frame, a
 * quarter of the HBM peak and 0.82 of k_linearize's time in the same job (H2Y_TFN_G24's table has one cut, PQ10000_f's two).  69 to
 * 70 VGPRs, no scratch.  Plain stores, as k_linearize: the next kernel reads the planes at once.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_math.h"
#include "h2y_device.h"
#include "h2y_light1.h"
#include "h2y_codepixel.h"

namespace {

constexpr uint32_t kThreads = 256u;
constexpr uint32_t kGroupsPerThread = 2u; /* 8-pixel groups per thread a one-frame launch aims at */
constexpr uint32_t kMaxBlocks = 2048u;    /* blocks of a launch: eight of 256 threads per CU */

/* eight codes of a plane as four words, two codes each: group q of a plane that starts 16-byte aligned, else put together from u16 loads */
__device__ __forceinline__ u32x4 load8_raw(const uint16_t *p, bool vec, uint32_t q)
{
    if (vec) return gload_nt<u32x4>(p, q);
    u32x4 v;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) v[j] = (uint32_t)gload<uint16_t>(p, 8u * q + 2u * j) | (uint32_t)gload<uint16_t>(p, 8u * q + 2u * j + 1u) << 16;
    return v;
}

template <int MATRIX>
__global__ __launch_bounds__(kThreads) void k_sdr_linearize(sdrsrc_args a, const linearize_frame *frames)
{
    const linearize_frame &fr = frames[blockIdx.y];
    const uint16_t *const p0 = uniform_ptr(fr.p[0]), *const p1 = uniform_ptr(fr.p[1]), *const p2 = uniform_ptr(fr.p[2]);
    float *const o0 = uniform_ptr(fr.out[0]), *const o1 = uniform_ptr(fr.out[1]), *const o2 = uniform_ptr(fr.out[2]);
    const pq_recA *tab = static_cast<const pq_recA *>(a.c.table);
    const uint32_t tid = threadIdx.x;
    /* groups [begin, end) of the frame's n8 (light1's tiers vote over the lanes that are at work, as in k_linearize) */
    const uint32_t n8 = a.c.n8;
    const uint32_t begin = (uint32_t)((uint64_t)blockIdx.x * n8 / gridDim.x), end = (uint32_t)((uint64_t)(blockIdx.x + 1u) * n8 / gridDim.x);
    /* the next step's codes are asked for before this step's pixels are worked out */
    u32x4 n0 = {0u, 0u, 0u, 0u}, n1 = n0, n2 = n0;
    if (begin + tid < end) {
        n0 = load8_raw(p0, a.c.vec & 1u, begin + tid);
        n1 = load8_raw(p1, a.c.vec & 2u, begin + tid);
        n2 = load8_raw(p2, a.c.vec & 4u, begin + tid);
    }
    for (uint32_t base = begin; base < end; base += kThreads) {
        const uint32_t q = base + tid;
        if (q >= end) continue;
        const u32x4 r0 = n0, r1 = n1, r2 = n2;
        if (q + kThreads < end) {
            n0 = load8_raw(p0, a.c.vec & 1u, q + kThreads);
            n1 = load8_raw(p1, a.c.vec & 2u, q + kThreads);
            n2 = load8_raw(p2, a.c.vec & 4u, q + kThreads);
        }
#pragma unroll
        for (uint32_t h = 0; h < 2u; h++) { /* the output planes start 16-byte aligned, and a group is 32 bytes of each */
            float lg[4], lb[4], lr[4];
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t w = 2u * h + (j >> 1), sh = 16u * (j & 1u);
                code_sdr_lights<MATRIX>(a.c, tab, a.kappa, (r0[w] >> sh) & 0xFFFFu, (r1[w] >> sh) & 0xFFFFu, (r2[w] >> sh) & 0xFFFFu, lg[j], lb[j], lr[j]);
            }
            gstore<f32x4>(o0, 2u * q + h, f32x4{lg[0], lg[1], lg[2], lg[3]});
            gstore<f32x4>(o1, 2u * q + h, f32x4{lb[0], lb[1], lb[2], lb[3]});
            gstore<f32x4>(o2, 2u * q + h, f32x4{lr[0], lr[1], lr[2], lr[3]});
        }
    }
    /* the npix % 8 pixels behind the last group: the frame's last block */
    if (blockIdx.x == gridDim.x - 1u) {
        const uint32_t i = 8u * n8 + tid;
        if (i < a.c.npix) {
            float lg, lb, lr;
            code_sdr_lights<MATRIX>(a.c, tab, a.kappa, gload<uint16_t>(p0, i), gload<uint16_t>(p1, i), gload<uint16_t>(p2, i), lg, lb, lr);
            gstore<float>(o0, i, lg);
            gstore<float>(o1, i, lb);
            gstore<float>(o2, i, lr);
        }
    }
}

template <int MATRIX> hipError_t launch_m(int grid, hipStream_t st, const sdrsrc_args &a, const linearize_frame *frames, int n_frames)
{
    hipLaunchKernelGGL((k_sdr_linearize<MATRIX>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames);
    return hipGetLastError();
}

} // namespace

int h2y_sdr_linearize_grid(uint32_t npix, int n_frames)
{
    const uint32_t n8 = npix / 8u > 0u ? npix / 8u : 1u, want = (n8 + kThreads * kGroupsPerThread - 1u) / (kThreads * kGroupsPerThread);
    const uint32_t cap = kMaxBlocks / (uint32_t)(n_frames > 0 ? n_frames : 1);
    return (int)(want < cap ? want : cap > 0u ? cap : 1u);
}

hipError_t h2y_launch_sdr_linearize(int matrix, int grid, hipStream_t st, const sdrsrc_args &a, const linearize_frame *frames, int n_frames)
{
    if (matrix == H2Y_MATRIX_BT2020NC) return launch_m<H2Y_MATRIX_BT2020NC>(grid, st, a, frames, n_frames);
    if (matrix == H2Y_MATRIX_BT709) return launch_m<H2Y_MATRIX_BT709>(grid, st, a, frames, n_frames);
    if (matrix == H2Y_MATRIX_GBR) return launch_m<H2Y_MATRIX_GBR>(grid, st, a, frames, n_frames);
    return hipErrorInvalidValue;
}
