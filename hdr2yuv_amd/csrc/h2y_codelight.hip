/*
 * h2y_codelight.hip -- the light of a finished PQ master, from its codes: content light (MaxCLL / MaxFALL) and the light
 * distribution (ST 2094-40) of frames of three u16 code planes, 4:4:4 (4:2:0 chroma arrives upsampled by k_up444, h2y_resample.hip).
 * include/hdr2yuv_hip.h, "light of PQ code planes", states every step: the codes normalised by one subtraction and one IEEE
 * division, Y'CbCr -> R'G'B' with every product and sum rounded by itself (this file is built -ffp-contract=off), the clamp to
 * [+0, 1], PQ10000_f through light1<true>'s tiers (these steps in h2y_codepixel.h, shared with k_linearize), and from there k_light's
 * and k_lightdist's own statement (h2y_light1.h).
 *
 *   k_codelight<MATRIX, DIST>  (block column, frame) blocks: a block takes a contiguous share of its frame's 8-pixel groups; a
 *                              thread reads a group with one 16-byte load per plane whose start is 16-byte aligned (u16 loads
 *                              for a plane that is not, and for the npix % 8 pixels behind the last group).  MATRIX 0: G, B, R
 *                              planes; 1: BT.709; 9: BT.2020nc.  It accumulates the frame's light_acc; with DIST the frame's
 *                              lightdist_acc and bins too, the bins in LDS as k_lightdist has them (34 KiB: four blocks a CU).
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

namespace {

constexpr uint32_t kThreads = 512u, kWaves = kThreads / WAVE;
constexpr uint32_t kGroupsPerThread = 4u; /* 8-pixel groups per thread a one-frame launch aims at: the flush of the bins is paid per block */
constexpr uint32_t kMaxBlocks = 1024u;    /* blocks of a launch: four per CU, what the LDS bins leave room for */
constexpr uint32_t kBins = H2Y_LIGHTDIST_BINS;
constexpr uint32_t kNone = 0xFFFFFFFFu;

/* what a thread keeps of its pixels */
struct code_regs {
    unsigned long long key;
    dist_regs t; /* t.sum serves both structs; mx and below with DIST only */
};

/* one pixel (index i of its frame) into the thread's registers; returns its bin */
template <int MATRIX, bool DIST>
__device__ __forceinline__ uint32_t code_pixel(const codelight_args &a, const pq_recA *tab, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t i,
                                               code_regs &k)
{
    float lg, lb, lr;
    code_lights<MATRIX>(a, tab, c0, c1, c2, lg, lb, lr);
    if (DIST) {
        const float m = dist_keep(lg, lb, lr, k.t);
        const unsigned long long key = ((unsigned long long)f2bits(m) << 32) | (unsigned long long)~i;
        k.key = key > k.key ? key : k.key;
        return bin_of(f2bits(m));
    }
    light_keep(fmaxf(fmaxf(lg, lb), lr), i, k.key, k.t.sum);
    return 0u;
}

template <int MATRIX, bool DIST>
__global__ __launch_bounds__(kThreads) void k_codelight(codelight_args a, const codelight_frame *frames, light_acc *acc, lightdist_acc *dacc,
                                                        uint32_t *bins)
{
    __shared__ uint32_t s_bins[DIST ? kBins : 1u];
    __shared__ code_regs s_part[kWaves];
    const codelight_frame &fr = frames[blockIdx.y];
    const uint16_t *const p0 = uniform_ptr(fr.p[0]), *const p1 = uniform_ptr(fr.p[1]), *const p2 = uniform_ptr(fr.p[2]);
    const pq_recA *tab = static_cast<const pq_recA *>(a.table);
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1u);
    if (DIST) {
        for (uint32_t w = tid; w < kBins; w += kThreads) s_bins[w] = 0u;
        __syncthreads();
    }
    code_regs k{0ull, {{0u, 0u, 0u}, 0u, 0ull}};
    /* groups [begin, end) of the frame's n8; every thread of the block takes every step (the last one with lanes past `end` idle) */
    const uint32_t begin = (uint32_t)((uint64_t)blockIdx.x * a.n8 / gridDim.x), end = (uint32_t)((uint64_t)(blockIdx.x + 1u) * a.n8 / gridDim.x);
    for (uint32_t base = begin; base < end; base += kThreads) {
        const uint32_t q = base + tid;
        const bool busy = q < end;
        uint32_t bn[8] = {kNone, kNone, kNone, kNone, kNone, kNone, kNone, kNone};
        if (busy) {
            uint32_t c0[8], c1[8], c2[8];
            load8(p0, a.vec & 1u, q, c0);
            load8(p1, a.vec & 2u, q, c1);
            load8(p2, a.vec & 4u, q, c2);
#pragma unroll
            for (uint32_t j = 0; j < 8u; j++) bn[j] = code_pixel<MATRIX, DIST>(a, tab, c0[j], c1[j], c2[j], 8u * q + j, k);
        }
        if (DIST) { /* k_lightdist's adds: the wave's pixels in one bin, a lane's pixels in one bin, or one by one */
            bool same = true;
#pragma unroll
            for (uint32_t j = 1; j < 8u; j++) same = same && bn[j] == bn[0];
            const uint32_t b0 = __builtin_amdgcn_readfirstlane(bn[0]); /* lane 0's: busy whenever a lane of the wave is */
            const unsigned long long busy_lanes = __builtin_amdgcn_ballot_w64(busy);
            if (__builtin_amdgcn_ballot_w64(busy && !(same && bn[0] == b0)) == 0ull) {
                if (lane == 0u && busy_lanes) atomicAdd(&s_bins[b0], 8u * (uint32_t)__builtin_popcountll(busy_lanes));
            } else if (busy) {
                if (same) atomicAdd(&s_bins[bn[0]], 8u);
                else {
#pragma unroll
                    for (uint32_t j = 0; j < 8u; j++) atomicAdd(&s_bins[bn[j]], 1u);
                }
            }
        }
    }
    /* the npix % 8 pixels behind the last group: the frame's last block */
    if (blockIdx.x == gridDim.x - 1u) {
        const uint32_t i = 8u * a.n8 + tid;
        if (i < a.npix) {
            const uint32_t b = code_pixel<MATRIX, DIST>(a, tab, gload<uint16_t>(p0, i), gload<uint16_t>(p1, i), gload<uint16_t>(p2, i), i, k);
            if (DIST) atomicAdd(&s_bins[b], 1u);
        }
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const unsigned long long other = shfl_xor_u64(k.key, o);
        k.key = other > k.key ? other : k.key;
        k.t.sum += shfl_xor_u64(k.t.sum, o);
        if (DIST) {
#pragma unroll
            for (int c = 0; c < 3; c++) k.t.mx[c] = max(k.t.mx[c], (uint32_t)__shfl_xor((int)k.t.mx[c], o, WAVE));
            k.t.below += (uint32_t)__shfl_xor((int)k.t.below, o, WAVE);
        }
    }
    if (lane == 0u) s_part[tid / WAVE] = k;
    __syncthreads(); /* also: every LDS add of the block is done */
    if (tid == 0u) {
        for (uint32_t v = 1; v < kWaves; v++) {
            k.key = s_part[v].key > k.key ? s_part[v].key : k.key;
            k.t.sum += s_part[v].t.sum;
            if (DIST) {
                for (int c = 0; c < 3; c++) k.t.mx[c] = max(k.t.mx[c], s_part[v].t.mx[c]);
                k.t.below += s_part[v].t.below;
            }
        }
        light_acc *o = acc + blockIdx.y;
        atomicMax(&o->key, k.key);
        atomicAdd(&o->sum, k.t.sum);
        if (DIST) {
            lightdist_acc *d = dacc + blockIdx.y;
            atomicAdd(&d->sum, k.t.sum);
            for (int c = 0; c < 3; c++) atomicMax(&d->maxscl[c], k.t.mx[c]);
            if (k.t.below) atomicAdd(&d->below, k.t.below);
        }
    }
    if (DIST) {
        uint32_t *gb = bins + (size_t)blockIdx.y * kBins;
        for (uint32_t w = tid; w < kBins; w += kThreads) {
            const uint32_t x = s_bins[w];
            if (x) atomicAdd(&gb[w], x);
        }
    }
}

template <int MATRIX>
hipError_t launch_m(int grid, hipStream_t st, const codelight_args &a, const codelight_frame *frames, int n_frames, light_acc *acc,
                    lightdist_acc *dacc, uint32_t *bins)
{
    if (dacc) hipLaunchKernelGGL((k_codelight<MATRIX, true>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc, dacc, bins);
    else hipLaunchKernelGGL((k_codelight<MATRIX, false>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc, dacc, bins);
    return hipGetLastError();
}

} // namespace

int h2y_codelight_grid(uint32_t npix, int n_frames)
{
    const uint32_t n8 = npix / 8u > 0u ? npix / 8u : 1u, want = (n8 + kThreads * kGroupsPerThread - 1u) / (kThreads * kGroupsPerThread);
    const uint32_t cap = kMaxBlocks / (uint32_t)(n_frames > 0 ? n_frames : 1);
    return (int)(want < cap ? want : cap > 0u ? cap : 1u);
}

hipError_t h2y_launch_codelight(int matrix, int grid, hipStream_t st, const codelight_args &a, const codelight_frame *frames, int n_frames,
                                light_acc *acc, lightdist_acc *dacc, uint32_t *bins)
{
    if (matrix == H2Y_MATRIX_BT2020NC) return launch_m<H2Y_MATRIX_BT2020NC>(grid, st, a, frames, n_frames, acc, dacc, bins);
    if (matrix == H2Y_MATRIX_BT709) return launch_m<H2Y_MATRIX_BT709>(grid, st, a, frames, n_frames, acc, dacc, bins);
    if (matrix == H2Y_MATRIX_GBR) return launch_m<H2Y_MATRIX_GBR>(grid, st, a, frames, n_frames, acc, dacc, bins);
    if (matrix == H2Y_MATRIX_ICTCP) return launch_m<H2Y_MATRIX_ICTCP>(grid, st, a, frames, n_frames, acc, dacc, bins);
    return hipErrorInvalidValue;
}
