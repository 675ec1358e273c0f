/*
 * h2y_histogram.hip -- code-value histograms and the legal-range check of u16 frames (the reference's "hist" and "check video
 * range", left a TODO at hdr2yuv.cpp:658 and :797), on the device.
 *
 *   k_histogram         (frame, plane, chunk) units -> per (frame, plane) bins and range counts, by device-scope atomic adds
 *   k_histogram_finish  one thread per (frame, plane): the counts -> h2y_histogram_stats
 *
 * A block takes a contiguous run of units, so it meets one or two (frame, plane) segments; it counts a segment's bins in LDS and
 * adds the non-zero ones to the segment's global bins when the segment ends.  bin = min(code >> shift, nbins - 1): a code above
 * 2^bit_depth - 1 lands in the last bin.  min, max and the range counts come from the samples, so they are exact at any bits.
 * Every figure is an integer sum, maximum or minimum: exact whatever the order of the atomics.
 *
 * LDS counters: up to 14 bits one u32 per bin (64 KiB at most).  At 15 and 16 bits two u16 counters share a u32 word (128 KiB at
 * 16 bits): the adder whose add carries a counter from below 32768 to 32768 or more takes 32768 off it again and adds 32768 to
 * the global bin.  A counter holds at most 32767 at a block barrier, one is taken after every step, and a step adds at most
 * kThreads x kGroups x 8 = 32768 to any counter: a counter never passes 65535 and never carries into its neighbour.
 *
 * Contention: a wave whose 512 samples of one step all fall in one bin (a constant picture, a row of one code) adds them with one
 * lane; otherwise every lane adds its 8 samples one by one, with no branch per sample (branches per sample cost more in saved
 * exec masks than merging equal neighbours saved).  The range counts take packed 16-bit arithmetic, two samples an instruction.
 */
#include <hip/hip_runtime.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"

namespace {

#define H2Y_GLOBAL __attribute__((address_space(1)))
typedef const H2Y_GLOBAL uint16_t gu16_c;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kThreads = 512u, kGroups = 8u, kGroupsPerUnit = kThreads * kGroups; /* 32768 samples a step */
constexpr uint32_t kWaves = kThreads / 64u;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxBlocksPerCu = 2u; /* 512 threads of about 96 VGPRs: 16 waves per CU */

struct counts_t {
    uint32_t mn, mx, below, above, at_low, at_high;
};

/* the range counts of one step, two samples per lane of a u16x2: v < lo, v <= lo, v > hi, v >= hi */
struct pcounts_t {
    u16x2 mn, mx, lt_lo, le_lo, gt_hi, ge_hi;
};

__device__ __forceinline__ u16x2 as_u16x2(uint32_t w) { return __builtin_bit_cast(u16x2, w); }
__device__ __forceinline__ u16x2 ones_if(u16x2 x) { return __builtin_elementwise_min(x, (u16x2){1, 1}); } /* x != 0 -> 1 */

/* one dword: two valid samples (a sample outside the plane is given as lo + 1, which no count but min / max sees, and those are
 * not fed with it) */
struct range_t {
    u16x2 lo, lo1, hi, hi1; /* lo, lo + 1, hi, hi - 1 in both halves */
};

__device__ __forceinline__ void pcount(pcounts_t &c, u16x2 v, const range_t &r)
{
    c.mn = __builtin_elementwise_min(c.mn, v);
    c.mx = __builtin_elementwise_max(c.mx, v);
    c.lt_lo += ones_if(__builtin_elementwise_sub_sat(r.lo, v));
    c.le_lo += ones_if(__builtin_elementwise_sub_sat(r.lo1, v));
    c.gt_hi += ones_if(__builtin_elementwise_sub_sat(v, r.hi));
    c.ge_hi += ones_if(__builtin_elementwise_sub_sat(v, r.hi1));
}

/* a step's packed counts into the segment's (at most 32 per half: no u16 overflows) */
__device__ __forceinline__ void fold(counts_t &c, pcounts_t &p)
{
    const uint32_t mn = min((uint32_t)p.mn.x, (uint32_t)p.mn.y), mx = max((uint32_t)p.mx.x, (uint32_t)p.mx.y);
    c.mn = c.mn < mn ? c.mn : mn;
    c.mx = c.mx > mx ? c.mx : mx;
    const uint32_t lt = (uint32_t)p.lt_lo.x + p.lt_lo.y, le = (uint32_t)p.le_lo.x + p.le_lo.y;
    const uint32_t gt = (uint32_t)p.gt_hi.x + p.gt_hi.y, ge = (uint32_t)p.ge_hi.x + p.ge_hi.y;
    c.below += lt;
    c.at_low += le - lt;
    c.above += gt;
    c.at_high += ge - gt;
    p = pcounts_t{{0xFFFF, 0xFFFF}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}};
}

/* one sample into the LDS bins; packed counters: 1 when this add carried its counter to 32768 (the caller spills it) */
template <bool kPacked> __device__ __forceinline__ uint32_t lds_add1(uint32_t *lds, uint32_t bin)
{
    if (!kPacked) {
        atomicAdd(&lds[bin], 1u);
        return 0u;
    }
    const uint32_t sh = (bin & 1u) << 4;
    return ((atomicAdd(&lds[bin >> 1], 1u << sh) >> sh) & 0xFFFFu) == 32767u;
}

/* 32768 of a packed counter go to the global bin */
__device__ __forceinline__ void spill(uint32_t *lds, uint32_t bin, uint32_t *gb)
{
    atomicSub(&lds[bin >> 1], 32768u << ((bin & 1u) << 4));
    atomicAdd(&gb[bin], 32768u);
}

/* the range counts of one sample (the groups cut by a plane's ends) */
__device__ __forceinline__ void count(counts_t &c, uint32_t v, uint32_t lo, uint32_t hi)
{
    c.mn = c.mn < v ? c.mn : v;
    c.mx = c.mx > v ? c.mx : v;
    c.below += v < lo;
    c.above += v > hi;
    c.at_low += v == lo;
    c.at_high += v == hi;
}

/* k samples of one bin at once (one lane of a wave whose samples share it) */
template <bool kPacked> __device__ __forceinline__ void lds_add(uint32_t *lds, uint32_t bin, uint32_t k, uint32_t *gb)
{
    if (!kPacked) {
        atomicAdd(&lds[bin], k);
        return;
    }
    const uint32_t sh = (bin & 1u) << 4;
    const uint32_t old = (atomicAdd(&lds[bin >> 1], k << sh) >> sh) & 0xFFFFu;
    if (old < 32768u && old + k >= 32768u) spill(lds, bin, gb);
}

/* the 8 bins of one lane into LDS (kWhole: all 8 are samples; else kNone marks a bin without one) */
template <bool kPacked, bool kWhole> __device__ __forceinline__ void add8(uint32_t *lds, const uint32_t (&b)[8], uint32_t *gb)
{
    uint32_t carried = 0;
#pragma unroll
    for (int j = 0; j < 8; j++)
        if (kWhole || b[j] != kNone) carried |= lds_add1<kPacked>(lds, b[j]) << j;
    if (kPacked && carried)
#pragma unroll
        for (int j = 0; j < 8; j++)
            if ((carried >> j) & 1u) spill(lds, b[j], gb);
}

} // namespace

/* Block b takes units [b U / G, (b + 1) U / G) of the U = n_frames x (units of the three planes); a unit is kGroupsPerUnit groups of
 * 8 samples, group g holding plane indices 8g - shift .. 8g - shift + 7 (shift: the plane's start modulo 8 samples), so that a
 * whole group is one 16-byte load.  A unit whose groups are all whole issues its kGroups loads per thread before it counts any of
 * them; the others (a plane's first and last unit) go group by group with u16 loads. */
template <bool kPacked>
__global__ __launch_bounds__(512) void k_histogram(hist_geom g, const hist_frame *__restrict__ frames, int n_frames,
                                                   hist_acc *__restrict__ acc, uint32_t *__restrict__ bins)
{
    extern __shared__ uint32_t lds[]; /* kPacked ? nbins / 2 : nbins words */
    __shared__ counts_t wsum[kWaves];
    const uint32_t words = kPacked ? g.nbins >> 1 : g.nbins;
    const uint32_t per_frame = g.units[0] + g.units[1] + g.units[2], units = (uint32_t)n_frames * per_frame;
    const uint32_t u_begin = (uint32_t)((uint64_t)blockIdx.x * units / gridDim.x);
    const uint32_t u_end = (uint32_t)((uint64_t)(blockIdx.x + 1u) * units / gridDim.x);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t w = tid; w < words; w += kThreads) lds[w] = 0u;
    __syncthreads();
    counts_t c{kNone, 0, 0, 0, 0, 0};
    for (uint32_t unit = u_begin; unit < u_end; unit++) {
        const uint32_t f = unit / per_frame, r = unit - f * per_frame;
        const uint32_t p = r < g.units[0] ? 0u : r < g.units[0] + g.units[1] ? 1u : 2u;
        const uint32_t chunk = r - (p > 0u ? g.units[0] : 0u) - (p > 1u ? g.units[1] : 0u);
        gu16_c *pa = (gu16_c *)frames[f].base + g.off[p];
        uint32_t *gb = bins + ((size_t)f * 3u + p) * g.nbins;
        const uint32_t n = g.n[p], s = g.shift[p], groups = (n + s + 7u) / 8u, g0 = chunk * kGroupsPerUnit;
        const uint32_t lo = g.lo[p], hi = g.hi[p], down = g.down, last = g.nbins - 1u;
        const bool vec = (g.vec >> p) & 1u;
        if (vec && g0 * 8u >= s && (g0 + kGroupsPerUnit) * 8u - s <= n) { /* every group of the unit whole */
            u32x4 q[kGroups];
#pragma unroll
            for (uint32_t k = 0; k < kGroups; k++)
                q[k] = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(pa + (g0 + k * kThreads + tid) * 8u - s);
            const range_t rg{{(uint16_t)lo, (uint16_t)lo}, {(uint16_t)(lo + 1u), (uint16_t)(lo + 1u)}, {(uint16_t)hi, (uint16_t)hi},
                             {(uint16_t)(hi - 1u), (uint16_t)(hi - 1u)}};
            const u16x2 down2 = {(uint16_t)down, (uint16_t)down}, last2 = {(uint16_t)last, (uint16_t)last};
            pcounts_t pc{{0xFFFF, 0xFFFF}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}};
#pragma unroll
            for (uint32_t k = 0; k < kGroups; k++) {
                const uint32_t w[4] = {q[k].x, q[k].y, q[k].z, q[k].w};
                uint32_t b[8];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const u16x2 v = as_u16x2(w[i]);
                    pcount(pc, v, rg);
                    const u16x2 bb = __builtin_elementwise_min(v >> down2, last2);
                    b[2 * i] = bb.x;
                    b[2 * i + 1] = bb.y;
                }
                bool same = true;
#pragma unroll
                for (int j = 1; j < 8; j++) same = same && b[j] == b[0];
                const uint32_t b0 = __builtin_amdgcn_readfirstlane(b[0]);
                if (__all(same && b[0] == b0)) { /* the wave's 512 samples in one bin: one add */
                    if (lane == 0u) lds_add<kPacked>(lds, b0, 512u, gb);
                } else add8<kPacked, true>(lds, b, gb);
            }
            fold(c, pc);
        } else {
            for (uint32_t k = 0; k < kGroups; k++) {
                const uint32_t gi = g0 + k * kThreads + tid;
                if (gi >= groups) break;
                const int32_t i0 = (int32_t)(gi * 8u) - (int32_t)s;
                uint32_t b[8];
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int32_t i = i0 + j;
                    b[j] = kNone;
                    if (i >= 0 && (uint32_t)i < n) {
                        const uint32_t x = pa[i];
                        count(c, x, lo, hi);
                        b[j] = min(x >> down, last);
                    }
                }
                add8<kPacked, false>(lds, b, gb);
            }
        }
        if (kPacked) __syncthreads(); /* every counter back below 32768 before the next step adds to it */
        if (chunk + 1u < g.units[p] && unit + 1u < u_end) continue;
        /* the segment (f, p) ends here: its counts and its bins go out, the LDS bins are cleared */
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t mn = __shfl_xor(c.mn, m), mx = __shfl_xor(c.mx, m);
            c.mn = c.mn < mn ? c.mn : mn;
            c.mx = c.mx > mx ? c.mx : mx;
            c.below += __shfl_xor(c.below, m);
            c.above += __shfl_xor(c.above, m);
            c.at_low += __shfl_xor(c.at_low, m);
            c.at_high += __shfl_xor(c.at_high, m);
        }
        if (lane == 0u) wsum[tid >> 6] = c;
        __syncthreads(); /* also: every LDS add of the segment is done */
        if (tid == 0u) {
            counts_t t = wsum[0];
            for (uint32_t w = 1; w < kWaves; w++) {
                t.mn = t.mn < wsum[w].mn ? t.mn : wsum[w].mn;
                t.mx = t.mx > wsum[w].mx ? t.mx : wsum[w].mx;
                t.below += wsum[w].below, t.above += wsum[w].above, t.at_low += wsum[w].at_low, t.at_high += wsum[w].at_high;
            }
            if (t.mn != kNone) { /* the segment had samples */
                hist_acc &a = acc[(size_t)f * 3u + p];
                atomicMax(&a.nmin, 0xFFFFu - t.mn);
                atomicMax(&a.max, t.mx);
                if (t.below) atomicAdd(&a.below, t.below);
                if (t.above) atomicAdd(&a.above, t.above);
                if (t.at_low) atomicAdd(&a.at_low, t.at_low);
                if (t.at_high) atomicAdd(&a.at_high, t.at_high);
            }
        }
        for (uint32_t w = tid; w < words; w += kThreads) {
            const uint32_t x = lds[w];
            if (!x) continue;
            lds[w] = 0u;
            if (!kPacked) atomicAdd(&gb[w], x);
            else {
                if (x & 0xFFFFu) atomicAdd(&gb[2u * w], x & 0xFFFFu);
                if (x >> 16) atomicAdd(&gb[2u * w + 1u], x >> 16);
            }
        }
        c = counts_t{kNone, 0, 0, 0, 0, 0};
        __syncthreads(); /* wsum and the cleared bins are reused by the next segment */
    }
}

/* one thread per (frame, plane): the segment counts into the frame's stats */
__global__ __launch_bounds__(256) void k_histogram_finish(hist_geom g, int n_frames, const hist_acc *__restrict__ acc,
                                                          h2y_histogram_stats *__restrict__ stats)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint32_t)n_frames * 3u) return;
    const uint32_t f = i / 3u, p = i - 3u * f;
    const hist_acc a = acc[i];
    h2y_histogram_stats &o = stats[f];
    const bool any = g.n[p] != 0u;
    o.samples[p] = g.n[p];
    o.below[p] = a.below;
    o.above[p] = a.above;
    o.at_low[p] = a.at_low;
    o.at_high[p] = a.at_high;
    o.min[p] = any ? 0xFFFFu - a.nmin : 0u;
    o.max[p] = any ? a.max : 0u;
    o.lo[p] = g.lo[p];
    o.hi[p] = g.hi[p];
    if (p == 0u) {
        o.nbins = g.nbins;
        o.shift = g.down;
    }
}

uint32_t h2y_histogram_units(uint32_t n, uint32_t shift)
{
    return n ? ((n + shift + 7u) / 8u + kGroupsPerUnit - 1u) / kGroupsPerUnit : 0u;
}

bool h2y_histogram_packed(uint32_t nbins) { return nbins > 16384u; }

size_t h2y_histogram_lds(uint32_t nbins) { return (size_t)(h2y_histogram_packed(nbins) ? nbins / 2u : nbins) * sizeof(uint32_t); }

int h2y_histogram_grid(int n_cu, const hist_geom &g, int n_frames)
{
    const uint64_t units = (uint64_t)n_frames * (g.units[0] + g.units[1] + g.units[2]);
    const size_t lds = h2y_histogram_lds(g.nbins) + 1024u; /* with wsum and headroom */
    uint32_t per_cu = (uint32_t)((160u * 1024u) / lds);
    per_cu = per_cu < 1u ? 1u : per_cu > kMaxBlocksPerCu ? kMaxBlocksPerCu : per_cu;
    const uint64_t max_grid = (uint64_t)n_cu * per_cu;
    return (int)(units < max_grid ? (units ? units : 1) : max_grid);
}

hipError_t h2y_launch_histogram(int grid, hipStream_t st, const hist_geom &g, const hist_frame *frames, int n_frames, hist_acc *acc,
                                uint32_t *bins, h2y_histogram_stats *stats)
{
    const size_t lds = h2y_histogram_lds(g.nbins);
    if (g.units[0] + g.units[1] + g.units[2]) {
        if (h2y_histogram_packed(g.nbins)) {
            hipError_t e = hipFuncSetAttribute((const void *)k_histogram<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(k_histogram<true>, dim3(grid), dim3(kThreads), lds, st, g, frames, n_frames, acc, bins);
        } else {
            hipError_t e = hipFuncSetAttribute((const void *)k_histogram<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(k_histogram<false>, dim3(grid), dim3(kThreads), lds, st, g, frames, n_frames, acc, bins);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_histogram_finish, dim3((3u * (uint32_t)n_frames + 255u) / 256u), dim3(256), 0, st, g, n_frames, acc, stats);
    return hipGetLastError();
}
