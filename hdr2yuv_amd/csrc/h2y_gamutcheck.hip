/*
 * h2y_gamutcheck.hip -- the gamut containment check of a finished PQ master, from its codes: how much of every frame lies outside a
 * primaries set narrower than the file's own (BT.2020 files against P3-D65 and BT.709).  include/hdr2yuv_hip.h, "gamut containment of
 * PQ code planes", states every step: the three lights of "light of PQ code planes" (code_lights, h2y_codepixel.h, word for word
 * what k_codelight computes), then per check set the matrix in k_gamut's row form, the excursion below 0 and the two classes
 * (h2y_gamutcheck1.h, shared with the host twin).  This file is built -ffp-contract=off as k_codelight's is.
 *
 *   k_gamutcheck<MATRIX, NSETS>  k_codelight's shape: (block column, frame) blocks, a block takes a contiguous share of its frame's
 *                                8-pixel groups; a thread reads a group with one 16-byte load per plane whose start is 16-byte aligned
 *                                (u16 loads for a plane that is not, and for the npix % 8 pixels behind the last group, which go to
 *                                the frame's last block).  Per thread and set a 64-bit key, a 64-bit sum and two 32-bit counts,
 *                                reduced over the wave by shuffles, over the block through LDS, then one set of atomics per block.
 *                                The matrices, t and a are kernel arguments: they stay in scalar registers.  No LDS bins.
 *
 * Every figure is an integer sum or maximum: exact whatever the order of the atomics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_math.h"
#include "h2y_device.h"
#include "h2y_light1.h"
#include "h2y_codepixel.h"
#include "h2y_gamut1.h"
#include "h2y_gamutcheck1.h"

namespace {

constexpr uint32_t kThreads = 512u, kWaves = kThreads / WAVE;
/* the launch's grid is h2y_codelight_grid's: the entries call that one function for both kernels, so the two stay on the same grid */

/* one pixel (index i of its frame) into the thread's registers */
template <int MATRIX, int NSETS>
__device__ __forceinline__ void check_pixel(const gamutcheck_args &a, const pq_recA *tab, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t i,
                                            gamutcheck_regs (&k)[NSETS])
{
    float lg, lb, lr;
    code_lights<MATRIX>(a.c, tab, c0, c1, c2, lg, lb, lr);
    const float mx = fmaxf(fmaxf(lg, lb), lr);
#pragma unroll
    for (int s = 0; s < NSETS; s++) gamutcheck_keep(a.m[s], a.t, a.a, lg, lb, lr, mx, i, k[s]);
}

template <int MATRIX, int NSETS>
__global__ __launch_bounds__(kThreads) void k_gamutcheck(gamutcheck_args a, const codelight_frame *frames, gamutcheck_frame_acc *acc)
{
    __shared__ gamutcheck_regs s_part[kWaves][NSETS];
    const codelight_frame &fr = frames[blockIdx.y];
    const uint16_t *const p0 = uniform_ptr(fr.p[0]), *const p1 = uniform_ptr(fr.p[1]), *const p2 = uniform_ptr(fr.p[2]);
    const pq_recA *tab = static_cast<const pq_recA *>(a.c.table);
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1u);
    gamutcheck_regs k[NSETS];
#pragma unroll
    for (int s = 0; s < NSETS; s++) k[s] = gamutcheck_regs{0ull, 0ull, 0u, 0u};
    /* groups [begin, end) of the frame's n8; every thread of the block takes every step (the last one with lanes past `end` idle) */
    const uint32_t begin = (uint32_t)((uint64_t)blockIdx.x * a.c.n8 / gridDim.x), end = (uint32_t)((uint64_t)(blockIdx.x + 1u) * a.c.n8 / gridDim.x);
    for (uint32_t base = begin; base < end; base += kThreads) {
        const uint32_t q = base + tid;
        if (q < end) {
            uint32_t c0[8], c1[8], c2[8];
            load8(p0, a.c.vec & 1u, q, c0);
            load8(p1, a.c.vec & 2u, q, c1);
            load8(p2, a.c.vec & 4u, q, c2);
#pragma unroll
            for (uint32_t j = 0; j < 8u; j++) check_pixel<MATRIX, NSETS>(a, tab, c0[j], c1[j], c2[j], 8u * q + j, k);
        }
    }
    /* the npix % 8 pixels behind the last group: the frame's last block */
    if (blockIdx.x == gridDim.x - 1u) {
        const uint32_t i = 8u * a.c.n8 + tid;
        if (i < a.c.npix) check_pixel<MATRIX, NSETS>(a, tab, gload<uint16_t>(p0, i), gload<uint16_t>(p1, i), gload<uint16_t>(p2, i), i, k);
    }
#pragma unroll
    for (int s = 0; s < NSETS; s++) {
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            const unsigned long long other = shfl_xor_u64(k[s].key, o);
            k[s].key = other > k[s].key ? other : k[s].key;
            k[s].sum += shfl_xor_u64(k[s].sum, o);
            k[s].outside += (uint32_t)__shfl_xor((int)k[s].outside, o, WAVE);
            k[s].beyond += (uint32_t)__shfl_xor((int)k[s].beyond, o, WAVE);
        }
        if (lane == 0u) s_part[tid / WAVE][s] = k[s];
    }
    __syncthreads();
    if (tid == 0u) {
        gamutcheck_frame_acc *o = acc + blockIdx.y;
#pragma unroll
        for (int s = 0; s < NSETS; s++) {
            for (uint32_t v = 1; v < kWaves; v++) {
                k[s].key = s_part[v][s].key > k[s].key ? s_part[v][s].key : k[s].key;
                k[s].sum += s_part[v][s].sum;
                k[s].outside += s_part[v][s].outside;
                k[s].beyond += s_part[v][s].beyond;
            }
            atomicMax(&o->set[s].key, k[s].key);
            if (k[s].sum) atomicAdd(&o->set[s].sum, k[s].sum);
            if (k[s].outside) atomicAdd(&o->set[s].outside, k[s].outside);
            if (k[s].beyond) atomicAdd(&o->set[s].beyond, k[s].beyond);
        }
    }
}

template <int MATRIX>
hipError_t launch_m(int grid, hipStream_t st, const gamutcheck_args &a, const codelight_frame *frames, int n_frames, gamutcheck_frame_acc *acc)
{
    if (a.n_sets == 2u) hipLaunchKernelGGL((k_gamutcheck<MATRIX, 2>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc);
    else if (a.n_sets == 1u) hipLaunchKernelGGL((k_gamutcheck<MATRIX, 1>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace

hipError_t h2y_launch_gamutcheck(int matrix, int grid, hipStream_t st, const gamutcheck_args &a, const codelight_frame *frames, int n_frames,
                                 gamutcheck_frame_acc *acc)
{
    if (matrix == H2Y_MATRIX_BT2020NC) return launch_m<H2Y_MATRIX_BT2020NC>(grid, st, a, frames, n_frames, acc);
    if (matrix == H2Y_MATRIX_BT709) return launch_m<H2Y_MATRIX_BT709>(grid, st, a, frames, n_frames, acc);
    if (matrix == H2Y_MATRIX_GBR) return launch_m<H2Y_MATRIX_GBR>(grid, st, a, frames, n_frames, acc);
    if (matrix == H2Y_MATRIX_ICTCP) return launch_m<H2Y_MATRIX_ICTCP>(grid, st, a, frames, n_frames, acc);
    return hipErrorInvalidValue;
}
