/*
 * h2y_lightdist.hip -- the light distribution (SMPTE ST 2094-40, "HDR10+") of the forward conversion's input, on the device: per
 * pixel m = max(L_G, L_B, L_R) of the three linear-light samples k_light measures (light1, h2y_light1.h), per frame the largest L
 * of each plane, the exact sum of the m in units of 2^-32, the pixels at or below 100 cd/m2, and an exact histogram of m on a
 * logarithmic scale: H2Y_LIGHTDIST_BINS bins of m's binary32 bit pattern, 512 per binade from 2^-17 up (include/hdr2yuv_hip.h
 * states every step).  The host turns the bins into percentiles (h2y_measure.hip).
 *
 *   k_lightdist<IN, TFN>  (block column, frame) blocks: a block takes a contiguous share of its frame's 4-pixel groups, reading the
 *                         three planes with one vector load each (the conversion's loaders, in_traits), and counts into an LDS
 *                         histogram (34 KiB: four blocks a CU); the maxima, the sum and the count stay in registers.  At the end
 *                         it adds its non-zero bins to the frame's global bins and merges the rest with one set of atomics.
 *
 * Every figure is an integer sum or maximum (L >= +0 orders as its bit pattern): exact whatever the order of the atomics.
 *
 * Contention: a wave whose 256 pixels of one step all fall in one bin (a constant picture, black bars, a dark scene) adds them
 * with one lane; otherwise a lane whose four pixels share a bin adds 4 once, and any other lane its four pixels one by one.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_math.h"
#include "h2y_device.h"
#include "h2y_light1.h"

namespace {

constexpr uint32_t kThreads = 512u, kWaves = kThreads / WAVE;
constexpr uint32_t kGroupsPerThread = 8u;  /* 4-pixel groups per thread a one-frame launch aims at: the flush of 8706 bins is paid per block */
constexpr uint32_t kMaxBlocks = 1024u;     /* blocks of a launch: four per CU, what the LDS bins leave room for */
constexpr uint32_t kBins = H2Y_LIGHTDIST_BINS;
constexpr uint32_t kNone = 0xFFFFFFFFu;

/* one pixel into the thread's registers; returns its bin */
template <bool TFN>
__device__ __forceinline__ uint32_t dist_pixel(const pix_params &pp, const pq_recA *tab, float g, float b, float r, dist_regs &t)
{
    const float lg = light1<TFN>(pp, tab, 0, g), lb = light1<TFN>(pp, tab, 1, b), lr = light1<TFN>(pp, tab, 2, r);
    const float m = dist_keep(lg, lb, lr, t);
    return bin_of(f2bits(m));
}

template <int IN_KIND, bool TFN>
__global__ __launch_bounds__(kThreads) void k_lightdist(light_args a, const light_frame *frames, lightdist_acc *acc, uint32_t *bins)
{
    typedef in_traits<IN_KIND> IN;
    __shared__ uint32_t s_bins[kBins];
    __shared__ dist_regs s_part[kWaves];
    const light_frame &fr = frames[blockIdx.y];
    const void *const p0 = uniform_ptr(fr.in[0]), *const p1 = uniform_ptr(fr.in[1]), *const p2 = uniform_ptr(fr.in[2]);
    const pix_params pp = with_assumed(a.pp, fr.assumed);
    const pq_recA *tab = static_cast<const pq_recA *>(a.table);
    const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1u);
    for (uint32_t w = tid; w < kBins; w += kThreads) s_bins[w] = 0u;
    __syncthreads();
    dist_regs t{{0u, 0u, 0u}, 0u, 0ull};
    /* groups [begin, end) of the frame's n4; every thread of the block takes every step (the last one with lanes past `end` idle:
     * a block's busy threads, and so a wave's busy lanes, are its first ones) */
    const uint32_t begin = (uint32_t)((uint64_t)blockIdx.x * a.n4 / gridDim.x), end = (uint32_t)((uint64_t)(blockIdx.x + 1u) * a.n4 / gridDim.x);
    for (uint32_t base = begin; base < end; base += kThreads) {
        const uint32_t q = base + tid;
        const bool busy = q < end;
        uint32_t bn[4] = {kNone, kNone, kNone, kNone};
        if (busy) {
            float g[4], b[4], r[4];
            IN::load4q(p0, q, g);
            IN::load4q(p1, q, b);
            IN::load4q(p2, q, r);
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) bn[j] = dist_pixel<TFN>(pp, tab, g[j], b[j], r[j], t);
        }
        const bool same = bn[1] == bn[0] && bn[2] == bn[0] && bn[3] == bn[0];
        const uint32_t b0 = __builtin_amdgcn_readfirstlane(bn[0]); /* lane 0's: busy whenever a lane of the wave is */
        const unsigned long long busy_lanes = __builtin_amdgcn_ballot_w64(busy);
        if (__builtin_amdgcn_ballot_w64(busy && !(same && bn[0] == b0)) == 0ull) { /* the wave's pixels in one bin: one add */
            if (lane == 0u && busy_lanes) atomicAdd(&s_bins[b0], 4u * (uint32_t)__builtin_popcountll(busy_lanes));
        } else if (busy) {
            if (same) atomicAdd(&s_bins[bn[0]], 4u);
            else {
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++) atomicAdd(&s_bins[bn[j]], 1u);
            }
        }
    }
    /* the npix % 4 pixels behind the last group: the frame's last block */
    if (blockIdx.x == gridDim.x - 1u) {
        const uint32_t i = 4u * a.n4 + tid;
        if (i < a.npix) atomicAdd(&s_bins[dist_pixel<TFN>(pp, tab, IN::load1(p0, i), IN::load1(p1, i), IN::load1(p2, i), t)], 1u);
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; c++) t.mx[c] = max(t.mx[c], (uint32_t)__shfl_xor((int)t.mx[c], o, WAVE));
        t.below += (uint32_t)__shfl_xor((int)t.below, o, WAVE);
        t.sum += shfl_xor_u64(t.sum, o);
    }
    if (lane == 0u) s_part[tid / WAVE] = t;
    __syncthreads(); /* also: every LDS add of the block is done */
    if (tid == 0u) {
        for (uint32_t v = 1; v < kWaves; v++) {
            for (int c = 0; c < 3; c++) t.mx[c] = max(t.mx[c], s_part[v].mx[c]);
            t.below += s_part[v].below;
            t.sum += s_part[v].sum;
        }
        lightdist_acc *o = acc + blockIdx.y;
        atomicAdd(&o->sum, t.sum);
        for (int c = 0; c < 3; c++) atomicMax(&o->maxscl[c], t.mx[c]);
        if (t.below) atomicAdd(&o->below, t.below);
    }
    uint32_t *gb = bins + (size_t)blockIdx.y * kBins;
    for (uint32_t w = tid; w < kBins; w += kThreads) {
        const uint32_t x = s_bins[w];
        if (x) atomicAdd(&gb[w], x);
    }
}

template <int IN_KIND>
hipError_t launch_in(int grid, hipStream_t st, const light_args &a, const light_frame *frames, int n_frames, lightdist_acc *acc, uint32_t *bins)
{
    if (a.table) hipLaunchKernelGGL((k_lightdist<IN_KIND, true>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc, bins);
    else hipLaunchKernelGGL((k_lightdist<IN_KIND, false>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc, bins);
    return hipGetLastError();
}

} // namespace

int h2y_lightdist_grid(uint32_t npix, int n_frames)
{
    const uint32_t n4 = npix / 4u > 0u ? npix / 4u : 1u, want = (n4 + kThreads * kGroupsPerThread - 1u) / (kThreads * kGroupsPerThread);
    const uint32_t cap = kMaxBlocks / (uint32_t)(n_frames > 0 ? n_frames : 1);
    return (int)(want < cap ? want : cap > 0u ? cap : 1u);
}

hipError_t h2y_launch_lightdist(int in_kind, int grid, hipStream_t st, const light_args &a, const light_frame *frames, int n_frames,
                                lightdist_acc *acc, uint32_t *bins)
{
    if (in_kind == H2Y_IN_F32) return launch_in<H2Y_IN_F32>(grid, st, a, frames, n_frames, acc, bins);
    if (in_kind == H2Y_IN_F16) return launch_in<H2Y_IN_F16>(grid, st, a, frames, n_frames, acc, bins);
    return launch_in<H2Y_IN_U16>(grid, st, a, frames, n_frames, acc, bins);
}
