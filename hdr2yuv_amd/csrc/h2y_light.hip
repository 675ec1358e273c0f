/*
 * h2y_light.hip -- the content light level (MaxCLL / MaxFALL, CTA-861.3) of the forward conversion's input, on the device:
 * per pixel the largest of the three linear-light samples matrix_convert() hands to PQ10000_r (convert.cpp:930-1040), per frame
 * its maximum, the first pixel holding it and the exact sum of the maxima in units of 2^-32 (include/hdr2yuv_hip.h states every
 * step).
 *
 *   k_light<IN, TFN>  (block column, frame) blocks: each thread walks 4-pixel groups of its frame at a grid stride, reading the
 *                     three planes with one vector load each (the conversion's loaders, in_traits); one pair of 64-bit atomics
 *                     per block into the frame's light_acc.
 *
 * A sample is normalised with the frame's floor and ceiling exactly as the conversion does (with_assumed, norm1).  A LINEAR source
 * stops there; any other source goes through the conversion's own tiers of its transfer function (tfn_fast on the function's
 * table, then the full-range table, then the careful tier), the path pixel_fast() takes, so no arithmetic is new here.  A NaN
 * counts as 0 and the value is clamped to [0, 1].  The cross-block merge is a 64-bit unsigned max of (m bits << 32 | ~index) --
 * m >= +0 orders as its bit pattern, and the complemented index makes the first pixel win a tie -- and an integer sum of
 * rint(m x 2^32): both are independent of the order in which blocks arrive.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_math.h"
#include "h2y_device.h"
#include "h2y_light1.h"

namespace {

constexpr uint32_t kThreads = 256u;
constexpr uint32_t kGroupsPerThread = 4u; /* 4-pixel groups per thread a one-frame launch aims at */
constexpr uint32_t kMaxBlocks = 2048u;    /* blocks of a launch: eight per CU */

template <bool TFN>
__device__ __forceinline__ void light_pixel(const pix_params &pp, const pq_recA *tab, float g, float b, float r, uint32_t i,
                                            unsigned long long &key, unsigned long long &sum)
{
    const float m = fmaxf(fmaxf(light1<TFN>(pp, tab, 0, g), light1<TFN>(pp, tab, 1, b)), light1<TFN>(pp, tab, 2, r));
    light_keep(m, i, key, sum);
}

template <int IN_KIND, bool TFN>
__global__ __launch_bounds__(kThreads) void k_light(light_args a, const light_frame *frames, light_acc *acc)
{
    typedef in_traits<IN_KIND> IN;
    __shared__ unsigned long long s_key[kThreads / WAVE], s_sum[kThreads / WAVE];
    const light_frame &fr = frames[blockIdx.y];
    const void *const p0 = uniform_ptr(fr.in[0]), *const p1 = uniform_ptr(fr.in[1]), *const p2 = uniform_ptr(fr.in[2]);
    const pix_params pp = with_assumed(a.pp, fr.assumed);
    const pq_recA *tab = static_cast<const pq_recA *>(a.table);
    unsigned long long key = 0ull, sum = 0ull;
    const uint32_t stride = gridDim.x * kThreads;
    for (uint32_t q = blockIdx.x * kThreads + threadIdx.x; q < a.n4; q += stride) {
        float g[4], b[4], r[4];
        IN::load4q(p0, q, g);
        IN::load4q(p1, q, b);
        IN::load4q(p2, q, r);
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) light_pixel<TFN>(pp, tab, g[j], b[j], r[j], 4u * q + j, key, sum);
    }
    for (uint32_t i = 4u * a.n4 + blockIdx.x * kThreads + threadIdx.x; i < a.npix; i += stride)
        light_pixel<TFN>(pp, tab, IN::load1(p0, i), IN::load1(p1, i), IN::load1(p2, i), i, key, sum);
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        const unsigned long long k = shfl_xor_u64(key, o);
        key = k > key ? k : key;
        sum += shfl_xor_u64(sum, o);
    }
    const uint32_t w = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        s_key[w] = key;
        s_sum[w] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t v = 1; v < kThreads / WAVE; v++) {
            key = s_key[v] > key ? s_key[v] : key;
            sum += s_sum[v];
        }
        light_acc *o = acc + blockIdx.y;
        atomicMax(&o->key, key);
        atomicAdd(&o->sum, sum);
    }
}

template <int IN_KIND>
hipError_t launch_in(int grid, hipStream_t st, const light_args &a, const light_frame *frames, int n_frames, light_acc *acc)
{
    if (a.table) hipLaunchKernelGGL((k_light<IN_KIND, true>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc);
    else hipLaunchKernelGGL((k_light<IN_KIND, false>), dim3(grid, n_frames), dim3(kThreads), 0, st, a, frames, acc);
    return hipGetLastError();
}

} // namespace

int h2y_light_grid(uint32_t npix, int n_frames)
{
    const uint32_t n4 = npix / 4u > 0u ? npix / 4u : 1u, want = (n4 + kThreads * kGroupsPerThread - 1u) / (kThreads * kGroupsPerThread);
    const uint32_t cap = kMaxBlocks / (uint32_t)(n_frames > 0 ? n_frames : 1);
    return (int)(want < cap ? want : cap > 0u ? cap : 1u);
}

hipError_t h2y_launch_light(int in_kind, int grid, hipStream_t st, const light_args &a, const light_frame *frames, int n_frames, light_acc *acc)
{
    if (in_kind == H2Y_IN_F32) return launch_in<H2Y_IN_F32>(grid, st, a, frames, n_frames, acc);
    if (in_kind == H2Y_IN_F16) return launch_in<H2Y_IN_F16>(grid, st, a, frames, n_frames, acc);
    return launch_in<H2Y_IN_U16>(grid, st, a, frames, n_frames, acc);
}
