/*
 * h2y_compare.hip -- the comparison of an output with a reference (the reference parses --ref_filename and --sigma_compare,
 * hdr2yuv.cpp:91-100, and leaves the work a TODO at :827-833), on the device.
 *
 *   k_compare      (frame, plane, chunk) units of two u16 frames A and B -> one cmp_partial per unit
 *   k_compare_sum  one block per (frame, plane): its units' partials -> h2y_compare_stats
 *
 * Every figure is an integer sum, maximum or minimum, so the result is exact and does not depend on how the work is dealt.
 * A plane is read in groups of 8 samples: group g holds plane indices 8g - shift .. 8g - shift + 7, where shift is the plane's
 * start modulo 8 samples when it is the same on both sides (a 4:2:0 chroma plane of an odd-sized frame starts mid-vector), so
 * that every whole group is one 16-byte load per side; groups cut by the plane's ends, and planes whose two sides start at
 * different offsets modulo 8, take u16 loads of their own samples only.  A square of two u16 fits 32 bits (65535^2 < 2^32), a sum
 * of two does not: the squares are summed in 64 bits per thread.
 */
#include <hip/hip_runtime.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"

namespace {

#define H2Y_GLOBAL __attribute__((address_space(1)))
typedef const H2Y_GLOBAL uint16_t gu16_c;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kThreads = 256u, kGroupsPerThread = 8u, kGroupsPerUnit = kThreads * kGroupsPerThread; /* 16384 samples */
constexpr uint32_t kNone = 0xFFFFFFFFu;

struct acc_t {
    uint64_t sse;
    uint32_t sad, mx, over, first;
};

__device__ __forceinline__ uint32_t absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

/* the 8 differences of one group (d[j] = 0 for a sample outside the plane), plane index of d[0] = i0 */
__device__ __forceinline__ void add_group(acc_t &s, const uint32_t (&d)[8], int32_t i0, uint32_t sigma)
{
    uint32_t gmax = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        s.sad += d[j];
        s.sse += (uint64_t)(d[j] * d[j]);
        gmax = gmax > d[j] ? gmax : d[j];
    }
    s.mx = s.mx > gmax ? s.mx : gmax;
    if (gmax > sigma) { /* rare where the frames agree: the count and the position only here */
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (d[j] > sigma) {
                s.over++;
                s.first = s.first < (uint32_t)(i0 + j) ? s.first : (uint32_t)(i0 + j);
            }
    }
}

__device__ __forceinline__ void diff_vec(uint32_t (&d)[8], const u32x4 a, const u32x4 b)
{
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        d[2 * k] = absdiff(aw[k] & 0xFFFFu, bw[k] & 0xFFFFu);
        d[2 * k + 1] = absdiff(aw[k] >> 16, bw[k] >> 16);
    }
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m)
{
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
    return (uint64_t)hi << 32 | lo;
}

} // namespace

/* Grid-stride over (frame, plane, chunk of kGroupsPerUnit groups) units; the frame and plane are block-uniform.  A unit whose
 * groups are all whole and 16-byte aligned issues its 16 loads before it reduces any of them; the others go group by group.
 * Wave reduction by shuffles, the block's four waves through LDS, one plain store of the unit's partial. */
__global__ __launch_bounds__(256) void k_compare(cmp_geom g, const cmp_frame *__restrict__ frames, int n_frames,
                                                 cmp_partial *__restrict__ partials)
{
    __shared__ acc_t wsum[kThreads / 64u];
    const uint32_t per_frame = g.chunks[0] + g.chunks[1] + g.chunks[2], units = (uint32_t)n_frames * per_frame;
    const uint32_t tid = threadIdx.x;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t f = unit / per_frame, r = unit - f * per_frame;
        const uint32_t p = r < g.chunks[0] ? 0u : r < g.chunks[0] + g.chunks[1] ? 1u : 2u;
        const uint32_t chunk = r - (p > 0u ? g.chunks[0] : 0u) - (p > 1u ? g.chunks[1] : 0u);
        const cmp_frame fr = frames[f];
        gu16_c *pa = (gu16_c *)fr.a + g.a_off[p], *pb = (gu16_c *)fr.b + g.b_off[p];
        const uint32_t n = g.n[p], s = g.shift[p], groups = (n + s + 7u) / 8u, g0 = chunk * kGroupsPerUnit;
        const bool vec = (g.vec >> p) & 1u;
        acc_t acc{0, 0, 0, 0, kNone};
        if (vec && g0 * 8u >= s && (g0 + kGroupsPerUnit) * 8u - s <= n) { /* every group of the unit whole */
            u32x4 va[kGroupsPerThread], vb[kGroupsPerThread];
#pragma unroll
            for (uint32_t k = 0; k < kGroupsPerThread; k++) {
                const uint32_t i0 = (g0 + k * kThreads + tid) * 8u - s;
                va[k] = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(pa + i0);
                vb[k] = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(pb + i0);
            }
#pragma unroll
            for (uint32_t k = 0; k < kGroupsPerThread; k++) {
                uint32_t d[8];
                diff_vec(d, va[k], vb[k]);
                add_group(acc, d, (int32_t)((g0 + k * kThreads + tid) * 8u - s), g.sigma);
            }
        } else {
            for (uint32_t k = 0; k < kGroupsPerThread; k++) {
                const uint32_t gi = g0 + k * kThreads + tid;
                if (gi >= groups) break;
                const int32_t i0 = (int32_t)(gi * 8u) - (int32_t)s;
                uint32_t d[8];
                if (vec && i0 >= 0 && (uint32_t)i0 + 8u <= n)
                    diff_vec(d, *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(pa + i0), *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(pb + i0));
                else
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        const int32_t i = i0 + j;
                        d[j] = (i >= 0 && (uint32_t)i < n) ? absdiff(pa[i], pb[i]) : 0u;
                    }
                add_group(acc, d, i0, g.sigma);
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            acc.sse += shfl_xor_u64(acc.sse, m);
            acc.sad += __shfl_xor(acc.sad, m);
            const uint32_t mx = __shfl_xor(acc.mx, m), fi = __shfl_xor(acc.first, m);
            acc.mx = acc.mx > mx ? acc.mx : mx;
            acc.first = acc.first < fi ? acc.first : fi;
            acc.over += __shfl_xor(acc.over, m);
        }
        if ((tid & 63u) == 0u) wsum[tid >> 6] = acc;
        __syncthreads();
        if (tid == 0u) {
            cmp_partial out{0, 0, 0, 0, kNone};
            for (uint32_t w = 0; w < kThreads / 64u; w++) {
                out.sse += wsum[w].sse;
                out.sad += wsum[w].sad;
                out.max_abs = out.max_abs > wsum[w].mx ? out.max_abs : wsum[w].mx;
                out.over += wsum[w].over;
                out.first = out.first < wsum[w].first ? out.first : wsum[w].first;
            }
            partials[unit] = out;
        }
        __syncthreads(); /* wsum is reused by the next unit */
    }
}

/* One block per (frame, plane): the plane's partials summed in 64 bits, the stats written with plain stores (the three planes'
 * blocks write disjoint fields), a and b at first_over read back from the frames. */
__global__ __launch_bounds__(256) void k_compare_sum(cmp_geom g, const cmp_frame *__restrict__ frames,
                                                     const cmp_partial *__restrict__ partials, h2y_compare_stats *__restrict__ stats)
{
    __shared__ uint64_t s_sse[kThreads], s_sad[kThreads], s_over[kThreads];
    __shared__ uint32_t s_max[kThreads], s_first[kThreads];
    const uint32_t f = blockIdx.x / 3u, p = blockIdx.x - 3u * f, tid = threadIdx.x;
    const uint32_t per_frame = g.chunks[0] + g.chunks[1] + g.chunks[2];
    const cmp_partial *part = partials + (size_t)f * per_frame + (p > 0u ? g.chunks[0] : 0u) + (p > 1u ? g.chunks[1] : 0u);
    uint64_t sse = 0, sad = 0, over = 0;
    uint32_t mx = 0, first = kNone;
    for (uint32_t c = tid; c < g.chunks[p]; c += kThreads) {
        const cmp_partial q = part[c];
        sse += q.sse;
        sad += q.sad;
        over += q.over;
        mx = mx > q.max_abs ? mx : q.max_abs;
        first = first < q.first ? first : q.first;
    }
    s_sse[tid] = sse, s_sad[tid] = sad, s_over[tid] = over, s_max[tid] = mx, s_first[tid] = first;
    __syncthreads();
    for (uint32_t h = kThreads / 2u; h > 0u; h >>= 1) {
        if (tid < h) {
            s_sse[tid] += s_sse[tid + h];
            s_sad[tid] += s_sad[tid + h];
            s_over[tid] += s_over[tid + h];
            s_max[tid] = s_max[tid] > s_max[tid + h] ? s_max[tid] : s_max[tid + h];
            s_first[tid] = s_first[tid] < s_first[tid + h] ? s_first[tid] : s_first[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0u) {
        h2y_compare_stats &o = stats[f];
        o.samples[p] = g.n[p];
        o.sse[p] = s_sse[0];
        o.sad[p] = s_sad[0];
        o.over[p] = s_over[0];
        o.max_abs[p] = s_max[0];
        const uint32_t i = s_first[0];
        o.first_over[p] = i == kNone ? -1 : (int64_t)i;
        o.first_a[p] = i == kNone ? 0u : frames[f].a[g.a_off[p] + i];
        o.first_b[p] = i == kNone ? 0u : frames[f].b[g.b_off[p] + i];
        if (p == 0u) o.reserved = 0u;
    }
}

uint32_t h2y_compare_chunks(uint32_t n, uint32_t shift)
{
    return n ? ((n + shift + 7u) / 8u + kGroupsPerUnit - 1u) / kGroupsPerUnit : 0u;
}

hipError_t h2y_launch_compare(int grid, hipStream_t st, const cmp_geom &g, const cmp_frame *frames, int n_frames, cmp_partial *partials,
                              h2y_compare_stats *stats)
{
    if (g.chunks[0] + g.chunks[1] + g.chunks[2]) hipLaunchKernelGGL(k_compare, dim3(grid), dim3(256), 0, st, g, frames, n_frames, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_compare_sum, dim3(3 * n_frames), dim3(256), 0, st, g, frames, partials, stats);
    return hipGetLastError();
}
