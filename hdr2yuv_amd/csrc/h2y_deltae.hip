/*
 * h2y_deltae.hip -- Delta E ITP (Rec. ITU-R BT.2124) of a PQ picture against a reference of the same geometry: pairs of frames of
 * three u16 code planes, 4:4:4 (4:2:0 chroma of both sides arrives upsampled by k_up444, h2y_resample.hip).
 * include/hdr2yuv_hip.h, "Delta E ITP of PQ code planes", states every step: each side's three lights by code_lights<MATRIX>
 * (h2y_codepixel.h, shared with k_codelight and k_linearize), L, M, S with every product and sum rounded by itself (this file is
 * built -ffp-contract=off), PQ10000_r through the forward conversion's own destination-stage tiers (code1, h2y_light1.h), I, T, P,
 * and d = 720 x sqrt((dI dI + dT dT) + dP dP) with the correctly rounded square root.
 *
 *   k_deltae<MATRIX>  (block column, frame pair) blocks: a block takes a contiguous share of its pair's 8-pixel groups; a thread
 *                     reads a group with one 16-byte load per plane and side whose start is 16-byte aligned (u16 loads for a plane
 *                     that is not, and for the npix % 8 pixels behind the last group), and works through it two pixels a step: a
 *                     pixel is twelve table transfers, and a step's 24 are as much code as k_codelight's whole group.
 *                     PQ10000_f's table is read from global memory through the cache, as k_codelight reads it; PQ10000_r's is
 *                     staged in LDS as k_fused2<...,TFN> stages it (51 KB: three blocks a CU), which measured a third faster than
 *                     reading it through the cache too.  It accumulates the pair's deltae_acc.
 *
 * Every figure is an integer sum, count or maximum: exact whatever the order of the atomics.
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

constexpr uint32_t kThreads = 512u, kWaves = kThreads / WAVE;
constexpr uint32_t kGroupsPerThread = 4u; /* 8-pixel groups per thread a one-pair launch aims at */
constexpr uint32_t kMaxBlocks = 1024u;    /* blocks of a launch, k_codelight's: each stages the table once */

/* what a thread keeps of its pixels */
struct de_regs {
    unsigned long long key, sum;
    uint32_t over;
};

/* one side's pixel: its codes -> I, T, P */
template <int MATRIX>
__device__ __forceinline__ void code_itp(const deltae_args &a, const pq_recA *tab_f, const pq_recA *tab_r, uint32_t c0, uint32_t c1, uint32_t c2, float &I,
                                         float &T, float &P)
{
    float G, B, R;
    code_lights<MATRIX>(a.c, tab_f, c0, c1, c2, G, B, R);
    /* BT.2100 LMS, k / 4096 */
    const float l = clamp01(((1688.0f / 4096.0f) * R + (2146.0f / 4096.0f) * G) + (262.0f / 4096.0f) * B);
    const float m = clamp01(((683.0f / 4096.0f) * R + (2951.0f / 4096.0f) * G) + (462.0f / 4096.0f) * B);
    const float s = clamp01(((99.0f / 4096.0f) * R + (309.0f / 4096.0f) * G) + (3688.0f / 4096.0f) * B);
    const float lp = code1(a.c.pp, tab_r, l), mp = code1(a.c.pp, tab_r, m), sp = code1(a.c.pp, tab_r, s);
    I = 0.5f * lp + 0.5f * mp;
    T = ((6610.0f / 8192.0f) * lp - (13613.0f / 8192.0f) * mp) + (7003.0f / 8192.0f) * sp;
    P = ((17933.0f / 4096.0f) * lp - (17390.0f / 4096.0f) * mp) - (543.0f / 4096.0f) * sp;
}

/* one pixel pair (index i of its frame) into the thread's registers */
template <int MATRIX>
__device__ __forceinline__ void de_pixel(const deltae_args &a, const pq_recA *tab_f, const pq_recA *tab_r, const uint32_t ca[3], const uint32_t cb[3],
                                         uint32_t i, de_regs &k)
{
    float Ia, Ta, Pa, Ib, Tb, Pb;
    code_itp<MATRIX>(a, tab_f, tab_r, ca[0], ca[1], ca[2], Ia, Ta, Pa);
    code_itp<MATRIX>(a, tab_f, tab_r, cb[0], cb[1], cb[2], Ib, Tb, Pb);
    const float dI = Ia - Ib, dT = Ta - Tb, dP = Pa - Pb;
    const float d = 720.0f * __builtin_sqrtf((dI * dI + dT * dT) + dP * dP);
    const unsigned long long key = ((unsigned long long)f2bits(d) << 32) | (unsigned long long)~i;
    k.key = key > k.key ? key : k.key;
    k.sum += (unsigned long long)__builtin_rintf(d * 0x1p20f); /* d x 2^20 is exact; below 2^33 */
    k.over += d > a.threshold;
}

/* codes 2 w and 2 w + 1 of a group, packed: w varies at run time, the group stays in registers */
__device__ __forceinline__ uint32_t pair_of(const uint32_t c[8], uint32_t w)
{
    const uint32_t w0 = c[0] | (c[1] << 16), w1 = c[2] | (c[3] << 16), w2 = c[4] | (c[5] << 16), w3 = c[6] | (c[7] << 16);
    return w == 0u ? w0 : w == 1u ? w1 : w == 2u ? w2 : w3;
}

template <int MATRIX>
__global__ __launch_bounds__(kThreads) void k_deltae(deltae_args a, const deltae_frame *frames, deltae_acc *acc)
{
    __shared__ de_regs s_part[kWaves];
    const deltae_frame &fr = frames[blockIdx.y];
    const uint16_t *const a0 = uniform_ptr(fr.a[0]), *const a1 = uniform_ptr(fr.a[1]), *const a2 = uniform_ptr(fr.a[2]);
    const uint16_t *const b0 = uniform_ptr(fr.b[0]), *const b1 = uniform_ptr(fr.b[1]), *const b2 = uniform_ptr(fr.b[2]);
    __shared__ pq_recA s_tab[2 * H2Y_PQ_NREC]; /* PQ10000_r's table: A records, then B records */
    stage_table<kThreads>(a.table_r, s_tab);
    __syncthreads();
    const pq_recA *tab_f = static_cast<const pq_recA *>(a.c.table), *tab_r = s_tab;
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1u);
    de_regs k{0ull, 0ull, 0u};
    /* groups [begin, end) of the frame's n8 */
    const uint32_t begin = (uint32_t)((uint64_t)blockIdx.x * a.c.n8 / gridDim.x), end = (uint32_t)((uint64_t)(blockIdx.x + 1u) * a.c.n8 / gridDim.x);
    for (uint32_t q = begin + tid; q < end; q += kThreads) {
        uint32_t ga[3][8], gb[3][8];
        load8(a0, a.c.vec & 1u, q, ga[0]);
        load8(a1, a.c.vec & 2u, q, ga[1]);
        load8(a2, a.c.vec & 4u, q, ga[2]);
        load8(b0, a.c.vec & 1u, q, gb[0]);
        load8(b1, a.c.vec & 2u, q, gb[1]);
        load8(b2, a.c.vec & 4u, q, gb[2]);
#pragma unroll 1
        for (uint32_t w = 0; w < 4u; w++) {
            uint32_t pa[3], pb[3];
#pragma unroll
            for (int c = 0; c < 3; c++) pa[c] = pair_of(ga[c], w), pb[c] = pair_of(gb[c], w);
#pragma unroll
            for (uint32_t j = 0; j < 2u; j++) {
                const uint32_t ca[3] = {j ? pa[0] >> 16 : pa[0] & 0xFFFFu, j ? pa[1] >> 16 : pa[1] & 0xFFFFu, j ? pa[2] >> 16 : pa[2] & 0xFFFFu};
                const uint32_t cb[3] = {j ? pb[0] >> 16 : pb[0] & 0xFFFFu, j ? pb[1] >> 16 : pb[1] & 0xFFFFu, j ? pb[2] >> 16 : pb[2] & 0xFFFFu};
                de_pixel<MATRIX>(a, tab_f, tab_r, ca, cb, 8u * q + 2u * w + j, k);
            }
        }
    }
    /* the npix % 8 pixels behind the last group: the frame's last block */
    if (blockIdx.x == gridDim.x - 1u) {
        const uint32_t i = 8u * a.c.n8 + tid;
        if (i < a.c.npix) {
            const uint32_t ca[3] = {gload<uint16_t>(a0, i), gload<uint16_t>(a1, i), gload<uint16_t>(a2, i)};
            const uint32_t cb[3] = {gload<uint16_t>(b0, i), gload<uint16_t>(b1, i), gload<uint16_t>(b2, i)};
            de_pixel<MATRIX>(a, tab_f, tab_r, ca, cb, i, k);
        }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const unsigned long long other = shfl_xor_u64(k.key, o);
        k.key = other > k.key ? other : k.key;
        k.sum += shfl_xor_u64(k.sum, o);
        k.over += (uint32_t)__shfl_xor((int)k.over, o, WAVE);
    }
    if (lane == 0u) s_part[tid / WAVE] = k;
    __syncthreads();
    if (tid == 0u) {
        unsigned long long over = k.over;
        for (uint32_t v = 1; v < kWaves; v++) {
            k.key = s_part[v].key > k.key ? s_part[v].key : k.key;
            k.sum += s_part[v].sum;
            over += s_part[v].over;
        }
        deltae_acc *o = acc + blockIdx.y;
        atomicMax(&o->key, k.key);
        atomicAdd(&o->sum, k.sum);
        if (over) atomicAdd(&o->over, over);
    }
}

} // namespace

int h2y_deltae_grid(uint32_t npix, int n_frames)
{
    const uint32_t n8 = npix / 8u > 0u ? npix / 8u : 1u, want = (n8 + kThreads * kGroupsPerThread - 1u) / (kThreads * kGroupsPerThread);
    const uint32_t cap = kMaxBlocks / (uint32_t)(n_frames > 0 ? n_frames : 1);
    return (int)(want < cap ? want : cap > 0u ? cap : 1u);
}

hipError_t h2y_launch_deltae(int matrix, int grid, hipStream_t st, const deltae_args &a, const deltae_frame *frames, int n_frames, deltae_acc *acc)
{
    if (matrix == H2Y_MATRIX_BT2020NC) hipLaunchKernelGGL((k_deltae<H2Y_MATRIX_BT2020NC>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc);
    else if (matrix == H2Y_MATRIX_BT709) hipLaunchKernelGGL((k_deltae<H2Y_MATRIX_BT709>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc);
    else if (matrix == H2Y_MATRIX_GBR) hipLaunchKernelGGL((k_deltae<H2Y_MATRIX_GBR>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc);
    else if (matrix == H2Y_MATRIX_ICTCP) hipLaunchKernelGGL((k_deltae<H2Y_MATRIX_ICTCP>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
