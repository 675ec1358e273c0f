/*
 * h2y_ssim.hip -- SSIM of an output against a reference, on code values (x264's and FFmpeg's 8x8 windows at a stride of 4), on
 * the device: the "SNR, etc. computation on orig vs. decoded" the reference leaves a TODO at hdr2yuv.cpp:826.
 *
 *   k_ssim      (frame, plane, strip, segment) units, one wave each -> one int64 partial per unit
 *   k_ssim_sum  one block per frame: each plane's partials -> h2y_ssim_stats
 *
 * A plane is cut into 4x4 blocks; a window is a 2x2 group of neighbouring blocks.  A unit's wave owns a strip of 128 block
 * columns (lane l: columns 2l and 2l + 1, one 16-byte load per row and side where the row allows) and walks down a segment of
 * kRows window rows, reading kRows + 1 block rows.  Lane l + 1's first block reaches lane l by a shuffle; lane 63 only lends its
 * blocks, so strips advance by 126 block columns and the column halo is the one extra lane.  The previous block row's column-pair
 * sums stay in registers, so every sample is read once, apart from the halos (one block row per segment, two block columns per
 * strip).  Block and window sums are exact integers: u32 up to 12 bits (a window's SS < 2^31), ss and s12 in u64 above.
 *
 * Each window's SSIM is evaluated in binary64 with separate roundings (-ffp-contract=off, IEEE division) in the order
 * h2y_ssim_stats states, and added as q = rint(s x 2^32) in int64: every sum is an integer sum, so the result is exact and does
 * not depend on how the work is dealt.
 */
#include <hip/hip_runtime.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"

namespace {

#define H2Y_GLOBAL __attribute__((address_space(1)))
typedef const H2Y_GLOBAL uint16_t gu16_c;
typedef const H2Y_GLOBAL uint32_t gu32_c;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kThreads = 256u, kWaves = kThreads / 64u;
constexpr uint32_t kStripBlocks = 126u; /* window columns per strip: lanes 0..62, two each */
constexpr uint32_t kRows = 16u;         /* window rows per segment */

/* the sums of one 4x4 block, or of several */
template <typename W> struct bsum {
    uint32_t s1, s2;
    W ss, s12;
};

template <typename W> __device__ __forceinline__ bsum<W> operator+(const bsum<W> &x, const bsum<W> &y)
{
    return bsum<W>{x.s1 + y.s1, x.s2 + y.s2, x.ss + y.ss, x.s12 + y.s12};
}

/* two samples of each side, packed low-high in a dword */
template <typename W> __device__ __forceinline__ void add_words(bsum<W> &b, uint32_t wa, uint32_t wb)
{
    const uint32_t a0 = wa & 0xFFFFu, a1 = wa >> 16, b0 = wb & 0xFFFFu, b1 = wb >> 16;
    b.s1 += a0 + a1;
    b.s2 += b0 + b1;
    b.ss += (W)(a0 * a0) + (W)(a1 * a1) + (W)(b0 * b0) + (W)(b1 * b1);
    b.s12 += (W)(a0 * b0) + (W)(a1 * b1);
}

/* a lane's row of nb (0..2) blocks at plane index i, the row's start being `al` samples past a 16-byte boundary: one 16-byte load
 * when both blocks are there and the row is aligned, dwords when its start is even, u16 otherwise; absent blocks read as 0 */
__device__ __forceinline__ void load_row(uint32_t (&w)[4], gu16_c *p, uint32_t i, uint32_t al, uint32_t nb)
{
    if (nb == 2u && al == 0u) {
        const u32x4 v = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(p + i);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        w[k] = 0u;
        if (k < 2u * nb) w[k] = (al & 1u) == 0u ? reinterpret_cast<gu32_c *>(p + i)[k] : (uint32_t)p[i + 2u * k] | (uint32_t)p[i + 2u * k + 1u] << 16;
    }
}

/* one window's rint(SSIM x 2^32) */
template <typename W> __device__ __forceinline__ int64_t window_q(const bsum<W> &s, double c1, double c2)
{
    const double fs1 = (double)s.s1, fs2 = (double)s.s2, fss = (double)s.ss, fs12 = (double)s.s12;
    const double vars = ((fss * 64.0) - (fs1 * fs1)) - (fs2 * fs2);
    const double covar = (fs12 * 64.0) - (fs1 * fs2);
    const double num = (((2.0 * fs1) * fs2) + c1) * ((2.0 * covar) + c2);
    const double den = (((fs1 * fs1) + (fs2 * fs2)) + c1) * (vars + c2);
    return (int64_t)__builtin_rint((num / den) * 4294967296.0);
}

__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v)
{
    const uint32_t lo = __shfl_down((uint32_t)v, 1), hi = __shfl_down((uint32_t)(v >> 32), 1);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint32_t shfl_down_w(uint32_t v) { return __shfl_down(v, 1); }
__device__ __forceinline__ uint64_t shfl_down_w(uint64_t v) { return shfl_down_u64(v); }

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int m)
{
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)((uint64_t)v >> 32), m);
    return (int64_t)((uint64_t)hi << 32 | lo);
}

/* Grid-stride over units, one per wave; the frame, plane, strip and segment are wave-uniform, so the waves of a block need no
 * barrier.  Every lane runs every row (the shuffles need the whole wave); a lane past the plane's blocks adds zeros. */
template <typename W>
__global__ __launch_bounds__(256) void k_ssim(ssim_geom g, const cmp_frame *__restrict__ frames, int n_frames, int64_t *__restrict__ partials)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t per_frame = g.units[0] + g.units[1] + g.units[2], units = (uint32_t)n_frames * per_frame;
    for (uint32_t unit = blockIdx.x * kWaves + (threadIdx.x >> 6); unit < units; unit += gridDim.x * kWaves) {
        const uint32_t f = unit / per_frame, r = unit - f * per_frame;
        const uint32_t p = r < g.units[0] ? 0u : r < g.units[0] + g.units[1] ? 1u : 2u;
        const uint32_t u = r - (p > 0u ? g.units[0] : 0u) - (p > 1u ? g.units[1] : 0u);
        const uint32_t seg = u / g.strips[p], strip = u - seg * g.strips[p];
        const uint32_t pw = g.pw[p], bw = pw >> 2, bh = g.ph[p] >> 2;
        const cmp_frame fr = frames[f];
        gu16_c *pa = (gu16_c *)fr.a + g.a_off[p], *pb = (gu16_c *)fr.b + g.b_off[p];
        const uint32_t c = strip * kStripBlocks + 2u * lane; /* the lane's first block column */
        const uint32_t nb = c < bw ? (bw - c < 2u ? bw - c : 2u) : 0u;
        const bool w0 = lane < 63u && c + 1u < bw, w1 = lane < 63u && c + 2u < bw; /* windows c and c + 1 */
        const uint32_t jb0 = seg * kRows, jb1 = jb0 + kRows < bh - 1u ? jb0 + kRows : bh - 1u;
        const bool fast = ((pw | g.a_off[p] | g.b_off[p]) & 7u) == 0u && nb == 2u; /* every row of both sides 16-byte aligned */
        bsum<W> h0{0, 0, 0, 0}, h1{0, 0, 0, 0}; /* the previous block row's column pairs (c, c+1), (c+1, c+2) */
        int64_t acc = 0;
        for (uint32_t jb = jb0; jb <= jb1; jb++) {
            uint32_t wa[4][4], wb[4][4];
            const uint32_t y0 = 4u * jb, i0 = y0 * pw + 4u * c;
            if (fast) {
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    const u32x4 va = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(pa + i0 + k * pw);
                    const u32x4 vb = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(pb + i0 + k * pw);
                    wa[k][0] = va.x, wa[k][1] = va.y, wa[k][2] = va.z, wa[k][3] = va.w;
                    wb[k][0] = vb.x, wb[k][1] = vb.y, wb[k][2] = vb.z, wb[k][3] = vb.w;
                }
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    const uint32_t rs = (y0 + k) * pw;
                    load_row(wa[k], pa, i0 + k * pw, (g.a_off[p] + rs) & 7u, nb);
                    load_row(wb[k], pb, i0 + k * pw, (g.b_off[p] + rs) & 7u, nb);
                }
            }
            bsum<W> b0{0, 0, 0, 0}, b1{0, 0, 0, 0};
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                add_words(b0, wa[k][0], wb[k][0]);
                add_words(b0, wa[k][1], wb[k][1]);
                add_words(b1, wa[k][2], wb[k][2]);
                add_words(b1, wa[k][3], wb[k][3]);
            }
            const bsum<W> n{shfl_down_w(b0.s1), shfl_down_w(b0.s2), shfl_down_w(b0.ss), shfl_down_w(b0.s12)}; /* block c + 2 */
            const bsum<W> c0 = b0 + b1, c1 = b1 + n;
            if (jb > jb0) {
                if (w0) acc += window_q(h0 + c0, g.c1, g.c2);
                if (w1) acc += window_q(h1 + c1, g.c1, g.c2);
            }
            h0 = c0, h1 = c1;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc += shfl_xor_i64(acc, m);
        if (lane == 0u) partials[unit] = acc;
    }
}

/* One block per frame: each plane's partials summed in int64 (an integer sum: any order gives the same), then the figures */
__global__ __launch_bounds__(256) void k_ssim_sum(ssim_geom g, const int64_t *__restrict__ partials, h2y_ssim_stats *__restrict__ stats)
{
    __shared__ int64_t s_sum[kThreads];
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    const uint32_t per_frame = g.units[0] + g.units[1] + g.units[2];
    h2y_ssim_stats &o = stats[f];
    for (uint32_t p = 0; p < 3u; p++) {
        const int64_t *part = partials + (size_t)f * per_frame + (p > 0u ? g.units[0] : 0u) + (p > 1u ? g.units[1] : 0u);
        int64_t s = 0;
        for (uint32_t c = tid; c < g.units[p]; c += kThreads) s += part[c];
        s_sum[tid] = s;
        __syncthreads();
        for (uint32_t h = kThreads / 2u; h > 0u; h >>= 1) {
            if (tid < h) s_sum[tid] += s_sum[tid + h];
            __syncthreads();
        }
        if (tid == 0u) {
            const uint64_t windows = (uint64_t)((g.pw[p] >> 2) - 1u) * (uint64_t)((g.ph[p] >> 2) - 1u);
            o.windows[p] = windows;
            o.sum_q[p] = s_sum[0];
            o.ssim[p] = ((double)s_sum[0] * 0x1p-32) / (double)windows;
        }
        __syncthreads(); /* s_sum is reused by the next plane */
    }
    if (tid == 0u) {
        const double n0 = (double)g.pw[0] * (double)g.ph[0], n1 = (double)g.pw[1] * (double)g.ph[1], n2 = (double)g.pw[2] * (double)g.ph[2];
        o.all = ((o.ssim[0] * n0 + o.ssim[1] * n1) + o.ssim[2] * n2) / ((n0 + n1) + n2);
    }
}

} // namespace

uint32_t h2y_ssim_strips(uint32_t plane_width) { return ((plane_width >> 2) - 2u) / kStripBlocks + 1u; }
uint32_t h2y_ssim_segments(uint32_t plane_height) { return ((plane_height >> 2) - 2u) / kRows + 1u; }

int h2y_ssim_grid(int n_cu, const ssim_geom &g, int n_frames)
{
    const uint64_t waves = (uint64_t)n_frames * (g.units[0] + g.units[1] + g.units[2]), blocks = (waves + kWaves - 1u) / kWaves;
    const uint64_t max_grid = (uint64_t)n_cu * 8u;
    return (int)(blocks < max_grid ? (blocks ? blocks : 1) : max_grid);
}

hipError_t h2y_launch_ssim(int grid, hipStream_t st, const ssim_geom &g, const cmp_frame *frames, int n_frames, int64_t *partials,
                           h2y_ssim_stats *stats)
{
    if (g.wide) hipLaunchKernelGGL(k_ssim<uint64_t>, dim3(grid), dim3(kThreads), 0, st, g, frames, n_frames, partials);
    else hipLaunchKernelGGL(k_ssim<uint32_t>, dim3(grid), dim3(kThreads), 0, st, g, frames, n_frames, partials);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ssim_sum, dim3(n_frames), dim3(kThreads), 0, st, g, partials, stats);
    return hipGetLastError();
}
