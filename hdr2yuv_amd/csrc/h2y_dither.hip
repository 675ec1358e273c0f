/*
 * h2y_dither.hip -- the reduction to the output bit depth of include/hdr2yuv_hip.h ("dither"), on the device.
 *
 *   k_dither<MODE>  (frame, plane, chunk) units of frames of three u16 planes at depth W -> the same planes at depth D
 *                   (h2y_dither_batch, the last stage of an armed forward ring, the dither-only ring)
 *
 * A pure streaming pass: out = clamp((v + t) >> s), t from h2y_dither1.h, the sum in 32 bits (65535 + 255 does not fit a u16).
 * A plane is walked in groups of 8 samples, k_compare's way: group g holds plane indices 8g - shift .. 8g - shift + 7, shift
 * being the plane's start modulo 8 samples (a 4:2:0 chroma plane of an odd width starts mid-vector), so that every whole group
 * is one 16-byte load and one 16-byte store where the frame's two bases are 16-byte aligned; groups cut by a plane's ends, and
 * frames on other bases, take u16 accesses of their own samples only.  A thread reads all of a group before it writes any of
 * it, and no sample belongs to two threads: a frame's destination may be its source.  Default cache policy on both sides, as
 * k_gamut.  No atomics, no LDS.
 */
#include <hip/hip_runtime.h>

#include "h2y_kernels.h"
#include "h2y_dither1.h"

namespace {

#define H2Y_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kThreads = 256u, kGroupsPerThread = 4u, kGroupsPerUnit = kThreads * kGroupsPerThread; /* 8192 samples */

/* The eight samples e[] of the group whose first plane index is i0 (negative in a plane's first group: those samples are not
 * the plane's and stay as they are), reduced.  The row of the first sample comes from one multiply by the plane's reciprocal
 * (h2y_dither_plane), and the row's part of t is computed where the walk enters a row, not per sample: a whole group inside
 * one row takes it once, a group that straddles a row end (any width that is no multiple of 8 has them) walks sample by
 * sample. */
template <int MODE, bool WHOLE>
__device__ __forceinline__ void reduce_group(uint32_t (&e)[8], int32_t i0, const dither_plane &P, uint32_t kp, uint32_t s)
{
    uint32_t x = 0, row = 0, y = 0;
    if (MODE != H2Y_DITHER_CUT) {
        const uint32_t i = WHOLE || i0 > 0 ? (uint32_t)i0 : 0u;
        y = (uint32_t)(((uint64_t)i * P.div_m) >> P.div_k); /* i / w, exact for i < 2^28 */
        x = i - y * P.w;
        row = dither_row<MODE>(kp, y);
    }
    if (MODE == H2Y_DITHER_CUT || (WHOLE && x + 8u <= P.w)) {
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) {
            const uint32_t q = (e[j] + dither_t<MODE>(kp, row, x + j, s)) >> s;
            e[j] = q < P.lo ? P.lo : q > P.hi ? P.hi : q;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (!WHOLE && i0 + j < 0) continue;
        const uint32_t q = (e[j] + dither_t<MODE>(kp, row, x, s)) >> s;
        e[j] = q < P.lo ? P.lo : q > P.hi ? P.hi : q;
        if (++x == P.w) {
            x = 0;
            row = dither_row<MODE>(kp, ++y);
        }
    }
}

__device__ __forceinline__ void unpack8(uint32_t (&e)[8], const u32x4 v)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++) e[2 * k] = w[k] & 0xFFFFu, e[2 * k + 1] = w[k] >> 16;
}

__device__ __forceinline__ u32x4 pack8(const uint32_t (&e)[8])
{
    return u32x4{e[0] | e[1] << 16, e[2] | e[3] << 16, e[4] | e[5] << 16, e[6] | e[7] << 16};
}

} // namespace

/* Grid-stride over (frame, plane, chunk of kGroupsPerUnit groups) units; the frame and the plane are block-uniform, and so are
 * the keys.  A unit whose groups are all whole and aligned issues its four loads before it reduces any of them; the others go
 * group by group. */
template <int MODE>
__global__ __launch_bounds__(256) void k_dither(dither_args a, const dither_frame *__restrict__ frames, int n_frames)
{
    const uint32_t per_frame = a.p[0].chunks + a.p[1].chunks + a.p[2].chunks, units = (uint32_t)n_frames * per_frame;
    const uint32_t tid = threadIdx.x, s = a.shift;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t f = unit / per_frame, r = unit - f * per_frame;
        const uint32_t p = r < a.p[0].chunks ? 0u : r < a.p[0].chunks + a.p[1].chunks ? 1u : 2u;
        const uint32_t chunk = r - (p > 0u ? a.p[0].chunks : 0u) - (p > 1u ? a.p[1].chunks : 0u);
        dither_plane P = a.p[0];
        if (p == 1u) P = a.p[1];
        if (p == 2u) P = a.p[2];
        const dither_frame fr = frames[f];
        const H2Y_GLOBAL uint16_t *src = (const H2Y_GLOBAL uint16_t *)fr.src + P.off;
        H2Y_GLOBAL uint16_t *dst = (H2Y_GLOBAL uint16_t *)fr.dst + P.off;
        const bool vec = (((uintptr_t)fr.src | (uintptr_t)fr.dst) & 15u) == 0;
        const uint32_t n = P.n, sh = P.off & 7u, groups = (n + sh + 7u) / 8u, g0 = chunk * kGroupsPerUnit;
        const uint32_t kp = dither_plane_key(a.key, a.temporal, a.first + f, p);
        if (vec && g0 * 8u >= sh && (g0 + kGroupsPerUnit) * 8u - sh <= n) { /* every group of the unit whole */
            u32x4 v[kGroupsPerThread];
#pragma unroll
            for (uint32_t k = 0; k < kGroupsPerThread; k++)
                v[k] = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(src + ((g0 + k * kThreads + tid) * 8u - sh));
#pragma unroll
            for (uint32_t k = 0; k < kGroupsPerThread; k++) {
                const uint32_t i0 = (g0 + k * kThreads + tid) * 8u - sh;
                uint32_t e[8];
                unpack8(e, v[k]);
                reduce_group<MODE, true>(e, (int32_t)i0, P, kp, s);
                *reinterpret_cast<H2Y_GLOBAL u32x4 *>(dst + i0) = pack8(e);
            }
        } else {
            for (uint32_t k = 0; k < kGroupsPerThread; k++) {
                const uint32_t gi = g0 + k * kThreads + tid;
                if (gi >= groups) break;
                const int32_t i0 = (int32_t)(gi * 8u) - (int32_t)sh;
                const bool whole = i0 >= 0 && (uint32_t)i0 + 8u <= n;
                uint32_t e[8];
                if (vec && whole) {
                    unpack8(e, *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(src + i0));
                    reduce_group<MODE, true>(e, i0, P, kp, s);
                    *reinterpret_cast<H2Y_GLOBAL u32x4 *>(dst + i0) = pack8(e);
                } else { /* its own samples only, all read before any is written */
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int32_t i = i0 + j;
                        e[j] = (i >= 0 && (uint32_t)i < n) ? src[i] : 0u;
                    }
                    reduce_group<MODE, false>(e, i0, P, kp, s);
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int32_t i = i0 + j;
                        if (i >= 0 && (uint32_t)i < n) dst[i] = (uint16_t)e[j];
                    }
                }
            }
        }
    }
}

dither_plane h2y_dither_plane(uint32_t w, uint32_t rows, uint32_t off, uint32_t lo, uint32_t hi)
{
    dither_plane P{};
    P.w = w, P.n = w * rows, P.off = off, P.lo = lo, P.hi = hi;
    const uint32_t groups = (P.n + (off & 7u) + 7u) / 8u;
    P.chunks = (groups + kGroupsPerUnit - 1u) / kGroupsPerUnit;
    /* floor(i m / 2^k) = floor(i / w) for every i < 2^28 with k = 28 + ceil(log2 w), m = ceil(2^k / w) < 2^30 */
    uint32_t l = 0;
    while ((1ull << l) < w) l++;
    P.div_k = 28u + l;
    P.div_m = (uint32_t)(((1ull << P.div_k) + w - 1u) / w);
    return P;
}

hipError_t h2y_launch_dither(int mode, int grid, hipStream_t st, const dither_args &a, const dither_frame *frames, int n_frames)
{
    if (mode == H2Y_DITHER_CUT) hipLaunchKernelGGL((k_dither<H2Y_DITHER_CUT>), dim3(grid), dim3(256), 0, st, a, frames, n_frames);
    else if (mode == H2Y_DITHER_ORDERED) hipLaunchKernelGGL((k_dither<H2Y_DITHER_ORDERED>), dim3(grid), dim3(256), 0, st, a, frames, n_frames);
    else if (mode == H2Y_DITHER_NOISE) hipLaunchKernelGGL((k_dither<H2Y_DITHER_NOISE>), dim3(grid), dim3(256), 0, st, a, frames, n_frames);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}
