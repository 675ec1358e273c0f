/*
 * h2y_hlgsrc.hip -- a finished HLG master back in display light: frames of three u16 code planes, 4:4:4 (4:2:0 chroma arrives
 * upsampled by k_up444, h2y_resample.hip), into three binary32 planes G, B, R that hold L_G, L_B, L_R of include/hdr2yuv_hip.h,
 * "light of HLG code planes".  Steps 2-3 are k_linearize's (code_primes of h2y_codepixel.h; this file is built -ffp-contract=off),
 * steps 4h-7h the one function of h2y_hlg1.h, which the host twin h2y_hlg_inverse_planes compiles too.
 *
 *   k_hlg_linearize<MATRIX>  k_linearize's walk and launch shape: (block column, frame) blocks; a block takes a contiguous share
 *                            of its frame's 8-pixel groups; a thread reads a group with one 16-byte load per plane whose start is
 *                            16-byte aligned (u16 loads for a plane that is not, and for the npix % 8 pixels behind the last
 *                            group, which the frame's last block takes) and writes it with two 16-byte stores per output plane;
 *                            the next step's codes are asked for first.  MATRIX 0: G, B, R planes; 1: BT.709; 9: BT.2020nc.
 *
 * The block copies both tables into LDS before its first group, as k_hlg does: the H2Y_LIGHTDIST_BINS gains of the OOTF (34 KiB)
 * and the 513 entries of the OETF's inverse from the node of 2^-1 up (2 KiB) -- the exponential branch starts above 0.5, nothing
 * below is read.  Per pixel one pair of neighbouring gains and up to three pairs of neighbouring inv entries.  36 KiB a block: four
 * blocks of 256 threads fit a CU's 160 KiB, four waves a SIMD.
 * The table copy is 36 loads a thread.  Where k_linearize gives a block two groups a thread (16 pixels, three PQ evaluations each),
 * this kernel gives it at least eight, so that the copy stays under a tenth of the block's loads and stores, and a launch asks for
 * no more blocks than the card holds at once (h2y_hlg_linearize_grid): a block that waits for a CU would copy the tables again.
 * All of that is reasoned from the sizes; keeping the tables in LDS rather than gathering through L2 and the groups a thread were
 * not measured against their alternatives.  Measured on an MI355X over 64 4K frames (tools/streambench.py hlgsrc):
 * 49.0 us a 10-bit 4:4:4 frame, 0.53 of k_linearize's time in the same job and 1.23 times k_hlg's; with blocks of 512 threads and
 * four groups a thread (48 VGPRs, eight waves a SIMD instead of four) 49.2 and 49.0 us against 50.3 and 50.9 in alternating
 * processes of one job, which is of the size of the spread between jobs, so the blocks stay k_linearize's.  More waves do not help
 * because the kernel is bound by its arithmetic: about 180 vector instructions a pixel in the compiled loop (counted in the ISA,
 * not with counters) -- six IEEE divisions (three of the normalisation, three by 3.0f) and four table reads with their clamps --
 * come to 38 us a 4K frame at one instruction per four cycles and SIMD, of the 49 measured.  Plain stores, as k_linearize: the next
 * kernel reads the planes at once.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_math.h"
#include "h2y_device.h"
#include "h2y_light1.h"
#include "h2y_codepixel.h"
#include "h2y_hlg1.h"

namespace {

constexpr uint32_t kThreads = 256u;
constexpr uint32_t kGroupsPerThread = 8u; /* 8-pixel groups per thread a launch aims at, at the least */
constexpr uint32_t kBlocksPerCu = 4u;     /* what the two LDS tables leave room for */

/* eight codes of a plane as four words, two codes each: group q of a plane that starts 16-byte aligned, else put together from u16 loads */
__device__ __forceinline__ u32x4 load8_raw(const uint16_t *p, bool vec, uint32_t q)
{
    if (vec) return gload_nt<u32x4>(p, q);
    u32x4 v;
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) v[j] = (uint32_t)gload<uint16_t>(p, 8u * q + 2u * j) | (uint32_t)gload<uint16_t>(p, 8u * q + 2u * j + 1u) << 16;
    return v;
}

/* one pixel's codes -> its three lights: normalise, matrix, then h2y_hlg1.h's way back */
template <int MATRIX>
__device__ __forceinline__ void code_hlg_lights(const hlgsrc_args &a, const float *ootf, const float *inv_hi, uint32_t c0, uint32_t c1, uint32_t c2,
                                                float &lg, float &lb, float &lr)
{
    code_primes<MATRIX>(a.c, c0, c1, c2, lg, lb, lr);
    hlg_inverse_pixel(ootf, inv_hi, a.kappa, lg, lb, lr);
}

template <int MATRIX>
__global__ __launch_bounds__(kThreads) void k_hlg_linearize(hlgsrc_args a, const linearize_frame *frames)
{
    __shared__ float s_ootf[H2Y_HLG_NODES];
    __shared__ float s_inv[H2Y_HLG_INV_NODES];
    const uint32_t tid = threadIdx.x;
    for (uint32_t w = tid; w < (uint32_t)H2Y_HLG_NODES; w += kThreads) s_ootf[w] = a.ootf[w];
    for (uint32_t w = tid; w < (uint32_t)H2Y_HLG_INV_NODES; w += kThreads) s_inv[w] = a.inv[H2Y_HLG_INV_FIRST + w];
    const linearize_frame &fr = frames[blockIdx.y];
    const uint16_t *const p0 = uniform_ptr(fr.p[0]), *const p1 = uniform_ptr(fr.p[1]), *const p2 = uniform_ptr(fr.p[2]);
    float *const o0 = uniform_ptr(fr.out[0]), *const o1 = uniform_ptr(fr.out[1]), *const o2 = uniform_ptr(fr.out[2]);
    /* groups [begin, end) of the frame's n8 */
    const uint32_t n8 = a.c.n8;
    const uint32_t begin = (uint32_t)((uint64_t)blockIdx.x * n8 / gridDim.x), end = (uint32_t)((uint64_t)(blockIdx.x + 1u) * n8 / gridDim.x);
    /* the first step's codes are on their way while the tables settle */
    u32x4 n0 = {0u, 0u, 0u, 0u}, n1 = n0, n2 = n0;
    if (begin + tid < end) {
        n0 = load8_raw(p0, a.c.vec & 1u, begin + tid);
        n1 = load8_raw(p1, a.c.vec & 2u, begin + tid);
        n2 = load8_raw(p2, a.c.vec & 4u, begin + tid);
    }
    __syncthreads();
    for (uint32_t base = begin; base < end; base += kThreads) {
        const uint32_t q = base + tid;
        if (q >= end) continue;
        const u32x4 r0 = n0, r1 = n1, r2 = n2;
        if (q + kThreads < end) { /* the next step's codes, before this step's pixels are worked out */
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
                code_hlg_lights<MATRIX>(a, s_ootf, s_inv, (r0[w] >> sh) & 0xFFFFu, (r1[w] >> sh) & 0xFFFFu, (r2[w] >> sh) & 0xFFFFu, lg[j], lb[j], lr[j]);
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
            code_hlg_lights<MATRIX>(a, s_ootf, s_inv, gload<uint16_t>(p0, i), gload<uint16_t>(p1, i), gload<uint16_t>(p2, i), lg, lb, lr);
            gstore<float>(o0, i, lg);
            gstore<float>(o1, i, lb);
            gstore<float>(o2, i, lr);
        }
    }
}

template <int MATRIX> hipError_t launch_m(int grid, hipStream_t st, const hlgsrc_args &a, const linearize_frame *frames, int n_frames)
{
    hipLaunchKernelGGL((k_hlg_linearize<MATRIX>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames);
    return hipGetLastError();
}

} // namespace

int h2y_hlg_linearize_grid(int n_cu, uint32_t npix, int n_frames)
{
    const uint32_t n8 = npix / 8u > 0u ? npix / 8u : 1u, want = (n8 + kThreads * kGroupsPerThread - 1u) / (kThreads * kGroupsPerThread);
    const uint32_t cap = (uint32_t)(n_cu > 0 ? n_cu : 1) * kBlocksPerCu / (uint32_t)(n_frames > 0 ? n_frames : 1);
    return (int)(want < cap ? want : cap > 0u ? cap : 1u);
}

hipError_t h2y_launch_hlg_linearize(int matrix, int grid, hipStream_t st, const hlgsrc_args &a, const linearize_frame *frames, int n_frames)
{
    if (matrix == H2Y_MATRIX_BT2020NC) return launch_m<H2Y_MATRIX_BT2020NC>(grid, st, a, frames, n_frames);
    if (matrix == H2Y_MATRIX_BT709) return launch_m<H2Y_MATRIX_BT709>(grid, st, a, frames, n_frames);
    if (matrix == H2Y_MATRIX_GBR) return launch_m<H2Y_MATRIX_GBR>(grid, st, a, frames, n_frames);
    return hipErrorInvalidValue;
}
