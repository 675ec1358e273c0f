/*
 * h2y_sigsrc.hip -- a finished master's codes as the non-linear signal they are: frames of three u16 code planes, 4:4:4 (4:2:0 chroma
 * arrives upsampled by k_up444, h2y_resample.hip), into three binary32 planes G', B', R' in [+0, 1] of include/hdr2yuv_hip.h, "signal
 * of code planes".  No transfer is applied: a signal-domain 3D LUT (k_lut3d in signal mode) reads the planes and decides what the
 * codes mean, so one decode serves PQ, HLG and SDR masters.  Steps 2-3 are k_linearize's (code_primes of h2y_codepixel.h; this file is
 * built -ffp-contract=off), the last step its clamp01.
 *
 *   k_code_signal<MATRIX>    k_sdr_linearize's walk and launch shape: (block column, frame) blocks; a block takes a contiguous share
 *                            of its frame's 8-pixel groups; a thread reads a group with one 16-byte nontemporal load per plane whose
 *                            start is 16-byte aligned (u16 loads for a plane that is not, and for the npix % 8 pixels behind the last
 *                            group, which the frame's last block takes) and writes it with two 16-byte plain stores per output plane;
 *                            the next step's codes are asked for first.  MATRIX 0: G, B, R planes; 1: BT.709; 9: BT.2020nc.
 *                            No tables, no LDS, no atomics.
 *
 * 6 bytes in and 12 bytes out per pixel; three IEEE divisions per pixel are part of the definition.  Plain stores, as k_linearize:
 * the next kernel (k_lut3d) reads the planes at once.  Measured on an MI355X over 64 4K frames, medians of five (2026-10-21, one run,
 * tools/streambench.py sigsrc): 37.90 us a 10-bit 4:4:4 frame (3.94 TB/s, 0.49 of the HBM peak), 37.94 us a 16-bit
 * G,B,R frame, 61.48 us a 10-bit 4:2:0 frame with k_up444; k_tiff_decode, which moves 12 bytes a pixel where this kernel moves 18,
 * took 19.67 us in the same job: 1.93 times its time, 1.5 of it the bytes.  The signal code ring ran at 888.8 frames/s from host
 * memory, the PQ code ring with the same LUT at 975.1, spreads overlapping.  40 VGPRs, 42 to 46 SGPRs, no scratch, no LDS.
 *
 * h2y_code_signal_host is the host twin's loop: the same code_primes and clamp01, compiled for the host without contraction.
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

/* one pixel's codes -> its signal G', B', R' in [+0, 1] ("signal of code planes": normalise, matrix, clamp) */
template <int MATRIX>
__host__ __device__ __forceinline__ void code_signal(const codelight_args &a, uint32_t c0, uint32_t c1, uint32_t c2, float &g, float &b, float &r)
{
    code_primes<MATRIX>(a, c0, c1, c2, g, b, r);
    g = clamp01(g), b = clamp01(b), r = clamp01(r);
}

template <int MATRIX>
__global__ __launch_bounds__(kThreads) void k_code_signal(codelight_args a, const linearize_frame *frames)
{
    const linearize_frame &fr = frames[blockIdx.y];
    const uint16_t *const p0 = uniform_ptr(fr.p[0]), *const p1 = uniform_ptr(fr.p[1]), *const p2 = uniform_ptr(fr.p[2]);
    float *const o0 = uniform_ptr(fr.out[0]), *const o1 = uniform_ptr(fr.out[1]), *const o2 = uniform_ptr(fr.out[2]);
    const uint32_t tid = threadIdx.x;
    /* groups [begin, end) of the frame's n8 */
    const uint32_t n8 = a.n8;
    const uint32_t begin = (uint32_t)((uint64_t)blockIdx.x * n8 / gridDim.x), end = (uint32_t)((uint64_t)(blockIdx.x + 1u) * n8 / gridDim.x);
    /* the next step's codes are asked for before this step's pixels are worked out */
    u32x4 n0 = {0u, 0u, 0u, 0u}, n1 = n0, n2 = n0;
    if (begin + tid < end) {
        n0 = load8_raw(p0, a.vec & 1u, begin + tid);
        n1 = load8_raw(p1, a.vec & 2u, begin + tid);
        n2 = load8_raw(p2, a.vec & 4u, begin + tid);
    }
    for (uint32_t base = begin; base < end; base += kThreads) {
        const uint32_t q = base + tid;
        if (q >= end) continue;
        const u32x4 r0 = n0, r1 = n1, r2 = n2;
        if (q + kThreads < end) {
            n0 = load8_raw(p0, a.vec & 1u, q + kThreads);
            n1 = load8_raw(p1, a.vec & 2u, q + kThreads);
            n2 = load8_raw(p2, a.vec & 4u, q + kThreads);
        }
#pragma unroll
        for (uint32_t h = 0; h < 2u; h++) { /* the output planes start 16-byte aligned, and a group is 32 bytes of each */
            float sg[4], sb[4], sr[4];
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t w = 2u * h + (j >> 1), sh = 16u * (j & 1u);
                code_signal<MATRIX>(a, (r0[w] >> sh) & 0xFFFFu, (r1[w] >> sh) & 0xFFFFu, (r2[w] >> sh) & 0xFFFFu, sg[j], sb[j], sr[j]);
            }
            gstore<f32x4>(o0, 2u * q + h, f32x4{sg[0], sg[1], sg[2], sg[3]});
            gstore<f32x4>(o1, 2u * q + h, f32x4{sb[0], sb[1], sb[2], sb[3]});
            gstore<f32x4>(o2, 2u * q + h, f32x4{sr[0], sr[1], sr[2], sr[3]});
        }
    }
    /* the npix % 8 pixels behind the last group: the frame's last block */
    if (blockIdx.x == gridDim.x - 1u) {
        const uint32_t i = 8u * n8 + tid;
        if (i < a.npix) {
            float g, b, r;
            code_signal<MATRIX>(a, gload<uint16_t>(p0, i), gload<uint16_t>(p1, i), gload<uint16_t>(p2, i), g, b, r);
            gstore<float>(o0, i, g);
            gstore<float>(o1, i, b);
            gstore<float>(o2, i, r);
        }
    }
}

template <int MATRIX> hipError_t launch_m(int grid, hipStream_t st, const codelight_args &a, const linearize_frame *frames, int n_frames)
{
    hipLaunchKernelGGL((k_code_signal<MATRIX>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames);
    return hipGetLastError();
}

template <int MATRIX> void host_m(const codelight_args &a, size_t npix, const uint16_t *const src[3], float *const dst[3])
{
    for (size_t i = 0; i < npix; i++) code_signal<MATRIX>(a, src[0][i], src[1][i], src[2][i], dst[0][i], dst[1][i], dst[2][i]);
}

} // namespace

int h2y_code_signal_grid(uint32_t npix, int n_frames)
{
    const uint32_t n8 = npix / 8u > 0u ? npix / 8u : 1u, want = (n8 + kThreads * kGroupsPerThread - 1u) / (kThreads * kGroupsPerThread);
    const uint32_t cap = kMaxBlocks / (uint32_t)(n_frames > 0 ? n_frames : 1);
    return (int)(want < cap ? want : cap > 0u ? cap : 1u);
}

hipError_t h2y_launch_code_signal(int matrix, int grid, hipStream_t st, const codelight_args &a, const linearize_frame *frames, int n_frames)
{
    if (matrix == H2Y_MATRIX_BT2020NC) return launch_m<H2Y_MATRIX_BT2020NC>(grid, st, a, frames, n_frames);
    if (matrix == H2Y_MATRIX_BT709) return launch_m<H2Y_MATRIX_BT709>(grid, st, a, frames, n_frames);
    if (matrix == H2Y_MATRIX_GBR) return launch_m<H2Y_MATRIX_GBR>(grid, st, a, frames, n_frames);
    return hipErrorInvalidValue;
}

bool h2y_code_signal_host(int matrix, const codelight_args &a, size_t npix, const uint16_t *const src[3], float *const dst[3])
{
    if (matrix == H2Y_MATRIX_BT2020NC) host_m<H2Y_MATRIX_BT2020NC>(a, npix, src, dst);
    else if (matrix == H2Y_MATRIX_BT709) host_m<H2Y_MATRIX_BT709>(a, npix, src, dst);
    else if (matrix == H2Y_MATRIX_GBR) host_m<H2Y_MATRIX_GBR>(a, npix, src, dst);
    else return false;
    return true;
}
