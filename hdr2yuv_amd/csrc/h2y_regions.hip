/*
 * h2y_regions.hip -- PSNR of flat and of busy areas, and over- and undershoot, of an output against a reference, on the device:
 * entries 2 and 3 of the reference's wish list ("measure undershoot and overshoot", "measure PSNR on flat areas separate from busy
 * areas").  include/hdr2yuv_hip.h states the figures (h2y_regions_stats).
 *
 *   k_regions      (frame, plane, strip, segment) units, one wave each -> one regions_partial per unit
 *   k_regions_sum  one block per frame: each plane's partials -> h2y_regions_stats
 *
 * A plane is cut into 8x8 tiles.  A unit's wave owns a strip of kStripTiles = 62 tile columns (lane l: column 62 x strip + l - 1,
 * 8 samples, one 16-byte load per row and side where the row allows) and walks down a segment of kSegRows = 32 sample rows (four
 * tile rows).  Lanes 0 and 63 only lend their samples of B: the r <= 4 samples left and right of a lane's eight reach it by
 * shuffles from lanes l - 1 and l + 1, two u16 to a dword.  A row of B becomes its horizontal min and max over [x - r, x + r]
 * (packed u16 min / max on the even pairs and on the pairs shifted by one sample); the last 2r + 1 rows' min, max and samples stay
 * in registers (the row loop is unrolled 2r + 1 times, so every index into them is a constant), and the row of A that lies r rows
 * back is read when the window below it is complete; both rows of a step are asked for one step ahead.  Rows above and below the plane are the nearest row read again and samples
 * past its sides read as 65535 for the min and 0 for the max, which is the window cut to the plane.  So every sample of A is
 * read once, and every sample of B once apart from the halos (2r rows per segment, two tile columns per strip).
 *
 * A tile's S, SS, sse and sad are added up over its rows and go to its class when the tile closes.  Every figure is an integer
 * sum or maximum (no atomics, no floating point), so nothing depends on how the work is dealt.
 */
#include <hip/hip_runtime.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"

namespace {

#define H2Y_GLOBAL __attribute__((address_space(1)))
typedef const H2Y_GLOBAL uint16_t gu16_c;
typedef const H2Y_GLOBAL uint32_t gu32_c;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kThreads = 256u, kWaves = kThreads / 64u;
constexpr uint32_t kStripTiles = 62u; /* tile columns per strip: lanes 1..62 */
constexpr uint32_t kSegRows = 32u;    /* sample rows per segment: a multiple of 8 */

/* two u16 to a dword: min, max and the difference clamped at 0 */
__device__ __forceinline__ u16x2 pk(uint32_t x) { return __builtin_bit_cast(u16x2, x); }
__device__ __forceinline__ uint32_t pk_min(uint32_t x, uint32_t y) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(pk(x), pk(y))); }
__device__ __forceinline__ uint32_t pk_max(uint32_t x, uint32_t y) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(pk(x), pk(y))); }
__device__ __forceinline__ uint32_t pk_sub_sat(uint32_t x, uint32_t y) { return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(pk(x), pk(y))); }
__device__ __forceinline__ uint32_t pk_add(uint32_t x, uint32_t y) { return __builtin_bit_cast(uint32_t, pk(x) + pk(y)); }
/* acc + |x.lo - y.lo| + |x.hi - y.hi| in one instruction; with y = 0, acc + the two halves of x */
__device__ __forceinline__ uint32_t add_abs_diff(uint32_t x, uint32_t y, uint32_t acc) { return __builtin_amdgcn_sad_u16(x, y, acc); }
/* the value of the lane below (lane 0: 0) and of the lane above (lane 63: 0), without the LDS crossbar */
__device__ __forceinline__ uint32_t from_lane_below(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, true); }
__device__ __forceinline__ uint32_t from_lane_above(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xF, 0xF, true); }

/* the samples of tile column cc that lie in a plane pw wide: 0..8 */
__device__ __forceinline__ uint32_t tile_width(int cc, uint32_t pw)
{
    if (cc < 0) return 0u;
    const uint32_t x = 8u * (uint32_t)cc;
    return x >= pw ? 0u : pw - x < 8u ? pw - x : 8u;
}

/* 0xFFFF in every half of dword j of a tile row whose sample lies at or past n */
__device__ __forceinline__ uint32_t absent_mask(uint32_t n, uint32_t j) { return (2u * j < n ? 0u : 0xFFFFu) | (2u * j + 1u < n ? 0u : 0xFFFF0000u); }

/* a lane's row of n (0..8) samples at plane index i, the row's start being `al` samples past a 16-byte boundary: one 16-byte load
 * when all eight are there and the row is aligned, dwords when its start is even, u16 otherwise; absent samples read as 0 */
__device__ __forceinline__ void load_row(uint32_t (&w)[4], gu16_c *p, uint32_t i, uint32_t al, uint32_t n)
{
    if (n == 8u && al == 0u) {
        const u32x4 v = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(p + i);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        w[k] = 0u;
        if (2u * k + 1u < n && (al & 1u) == 0u) w[k] = *reinterpret_cast<gu32_c *>(p + i + 2u * k);
        else {
            if (2u * k < n) w[k] = (uint32_t)p[i + 2u * k];
            if (2u * k + 1u < n) w[k] |= (uint32_t)p[i + 2u * k + 1u] << 16;
        }
    }
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m)
{
    const uint32_t lo = __shfl_xor((uint32_t)v, m), hi = __shfl_xor((uint32_t)(v >> 32), m);
    return (uint64_t)hi << 32 | lo;
}

/* Grid-stride over units, one per wave; the frame, plane, strip and segment are wave-uniform, so the waves of a block need no
 * barrier.  Every lane runs every row (the shuffles need the whole wave); a lane that owns no tile column adds nothing. */
template <int R> __global__ __launch_bounds__(256) void k_regions(regions_geom g, const cmp_frame *__restrict__ frames, int n_frames, regions_partial *__restrict__ partials)
{
    constexpr int N = 2 * R + 1;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t per_frame = g.units[0] + g.units[1] + g.units[2], units = (uint32_t)n_frames * per_frame;
    for (uint32_t unit = blockIdx.x * kWaves + (threadIdx.x >> 6); unit < units; unit += gridDim.x * kWaves) {
        const uint32_t f = unit / per_frame, ru = unit - f * per_frame;
        const uint32_t p = ru < g.units[0] ? 0u : ru < g.units[0] + g.units[1] ? 1u : 2u;
        const uint32_t u = ru - (p > 0u ? g.units[0] : 0u) - (p > 1u ? g.units[1] : 0u);
        const uint32_t seg = u / g.strips[p], strip = u - seg * g.strips[p];
        const uint32_t pw = g.pw[p], ph = g.ph[p];
        const cmp_frame fr = frames[f];
        gu16_c *pa = (gu16_c *)fr.a + g.a_off[p], *pb = (gu16_c *)fr.b + g.b_off[p];
        const int c = (int)(strip * kStripTiles + lane) - 1; /* the lane's tile column */
        const uint32_t nv = tile_width(c, pw), x0 = c < 0 ? 0u : 8u * (uint32_t)c;
        const bool own = lane >= 1u && lane <= kStripTiles && nv > 0u;
        const uint32_t na = own ? nv : 0u; /* a lender reads no A */
        /* the sixteen samples a row's windows reach, two to a dword: the left lane's last four, the lane's eight, the right lane's
         * first four; mk marks the halves that lie outside the plane */
        uint32_t mk[8];
        {
            const uint32_t nl = tile_width(c - 1, pw), nr = tile_width(c + 1, pw);
            mk[0] = absent_mask(nl, 2u), mk[1] = absent_mask(nl, 3u);
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) mk[2u + j] = absent_mask(nv, j);
            mk[6] = absent_mask(nr, 0u), mk[7] = absent_mask(nr, 1u);
        }
        const uint32_t y0 = seg * kSegRows, y1 = y0 + kSegRows < ph ? y0 + kSegRows : ph;

        uint32_t raw[N][4], hmn[N][4], hmx[N][4]; /* the last 2R + 1 rows of B: the lane's samples, their horizontal min and max */
        auto load_b = [&](uint32_t (&w)[4], uint32_t yb) {
            const uint32_t rs = yb * pw;
            load_row(w, pb, rs + x0, (g.b_off[p] + rs) & 7u, nv);
        };
        auto load_a = [&](uint32_t (&w)[4], uint32_t y) {
            const uint32_t rs = y * pw;
            load_row(w, pa, rs + x0, (g.a_off[p] + rs) & 7u, na);
        };
        /* a row w of B into slot s (a constant wherever this is called) */
        auto b_row = [&](const uint32_t (&w)[4], int s) {
            uint32_t e[8];
            e[0] = R > 2 ? from_lane_below(w[2]) : 0u;
            e[1] = from_lane_below(w[3]);
            e[6] = from_lane_above(w[0]);
            e[7] = R > 2 ? from_lane_above(w[1]) : 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) e[2 + j] = raw[s][j] = w[j];
            uint32_t lo[8], ql[7], qh[7]; /* the even pairs' min form; the pairs one sample on, min and max form */
#pragma unroll
            for (int i = 0; i < 8; i++) lo[i] = e[i] | mk[i];
#pragma unroll
            for (int i = 0; i < 7; i++) {
                qh[i] = e[i] >> 16 | e[i + 1] << 16;
                ql[i] = lo[i] >> 16 | lo[i + 1] << 16;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t mn = lo[2 + j], mx = e[2 + j];
#pragma unroll
                for (int d = 1; d <= R; d++) {
                    if (d & 1) {
                        mn = pk_min(mn, pk_min(ql[2 + j + (-d - 1) / 2], ql[2 + j + (d - 1) / 2]));
                        mx = pk_max(mx, pk_max(qh[2 + j + (-d - 1) / 2], qh[2 + j + (d - 1) / 2]));
                    } else {
                        mn = pk_min(mn, pk_min(lo[2 + j - d / 2], lo[2 + j + d / 2]));
                        mx = pk_max(mx, pk_max(e[2 + j - d / 2], e[2 + j + d / 2]));
                    }
                }
                hmn[s][j] = mn, hmx[s][j] = mx;
            }
        };

        /* the open tile's sums, and the unit's: every tile's, and the flat tiles' */
        uint32_t t_s = 0u, t_sad = 0u;
        uint64_t t_ss = 0u, t_sse = 0u;
        uint32_t all_tiles = 0u, all_samples = 0u, all_sad = 0u, flat_tiles = 0u, flat_samples = 0u, flat_sad = 0u;
        uint64_t all_sse = 0u, flat_sse = 0u;
        /* over, under: two counts to a dword (a lane sees 4 x kSegRows samples in each half); *_mx: two running maxima */
        uint32_t over = 0u, over_sum = 0u, over_mx = 0u, under = 0u, under_sum = 0u, under_mx = 0u;
        /* row y of A against the window that the 2R + 1 slots hold; B's row y lies in slot s */
        auto a_row = [&](const uint32_t (&a)[4], uint32_t y, int s) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t mn = hmn[0][j], mx = hmx[0][j];
#pragma unroll
                for (int k = 1; k < N; k++) mn = pk_min(mn, hmn[k][j]), mx = pk_max(mx, hmx[k][j]);
                const uint32_t o = pk_sub_sat(a[j], mx), un = pk_sub_sat(mn, a[j] | mk[2 + j]);
                over = pk_add(over, pk_min(o, 0x00010001u));
                over_sum = add_abs_diff(o, 0u, over_sum);
                over_mx = pk_max(over_mx, o);
                under = pk_add(under, pk_min(un, 0x00010001u));
                under_sum = add_abs_diff(un, 0u, under_sum);
                under_mx = pk_max(under_mx, un);
                const uint32_t b = raw[s][j];
                const uint32_t d = pk_sub_sat(a[j], b) | pk_sub_sat(b, a[j]); /* |a - b|, two to a dword */
                const uint32_t b0 = b & 0xFFFFu, b1 = b >> 16, d0 = d & 0xFFFFu, d1 = d >> 16;
                t_s = add_abs_diff(b, 0u, t_s);
                t_ss += (uint64_t)(b0 * b0) + (uint64_t)(b1 * b1);
                t_sad = add_abs_diff(a[j], b, t_sad);
                t_sse += (uint64_t)(d0 * d0) + (uint64_t)(d1 * d1);
            }
            if ((y & 7u) == 7u || y + 1u == y1) { /* the tile closes: a segment ends with a tile row, or with the plane */
                const uint32_t n = nv * ((y & 7u) + 1u);
                const uint64_t act = (uint64_t)n * t_ss - (uint64_t)t_s * t_s;
                const bool flat = act <= (uint64_t)g.flat_var * (uint64_t)(n * n);
                all_tiles += 1u, all_samples += n, all_sad += t_sad, all_sse += t_sse;
                flat_tiles += flat ? 1u : 0u, flat_samples += flat ? n : 0u, flat_sad += flat ? t_sad : 0u, flat_sse += flat ? t_sse : 0u;
                t_s = t_sad = 0u;
                t_ss = t_sse = 0u;
            }
        };

        /* rows y0 - R .. y0 + R - 1 of B, then a row of B and a row of A per step; the next step's two rows are asked for before
         * this step's are worked on */
#pragma unroll
        for (int i = 0; i < 2 * R; i++) {
            const int yb = (int)y0 - R + i;
            uint32_t w[4];
            load_b(w, yb < 0 ? 0u : (uint32_t)yb < ph ? (uint32_t)yb : ph - 1u);
            b_row(w, i);
        }
        uint32_t nb[4], na4[4];
        load_b(nb, y0 + R < ph ? y0 + R : ph - 1u);
        load_a(na4, y0);
        for (uint32_t y = y0; y < y1; y += (uint32_t)N) {
#pragma unroll
            for (int s = 0; s < N; s++) {
                const uint32_t yy = y + (uint32_t)s;
                if (yy < y1) {
                    const uint32_t cb[4] = {nb[0], nb[1], nb[2], nb[3]}, ca[4] = {na4[0], na4[1], na4[2], na4[3]};
                    if (yy + 1u < y1) {
                        load_b(nb, yy + 1u + R < ph ? yy + 1u + R : ph - 1u);
                        load_a(na4, yy + 1u);
                    }
                    b_row(cb, (2 * R + s) % N);
                    a_row(ca, yy, (R + s) % N);
                }
            }
        }

        regions_partial r;
        r.sse_all = own ? all_sse : 0u, r.sse_flat = own ? flat_sse : 0u;
        r.sad_all = own ? all_sad : 0u, r.sad_flat = own ? flat_sad : 0u;
        r.over_sum = own ? over_sum : 0u, r.under_sum = own ? under_sum : 0u;
        r.tiles_all = own ? all_tiles : 0u, r.tiles_flat = own ? flat_tiles : 0u;
        r.samples_all = own ? all_samples : 0u, r.samples_flat = own ? flat_samples : 0u;
        r.over = own ? (over & 0xFFFFu) + (over >> 16) : 0u, r.under = own ? (under & 0xFFFFu) + (under >> 16) : 0u;
        r.over_max = own ? ((over_mx & 0xFFFFu) > over_mx >> 16 ? over_mx & 0xFFFFu : over_mx >> 16) : 0u;
        r.under_max = own ? ((under_mx & 0xFFFFu) > under_mx >> 16 ? under_mx & 0xFFFFu : under_mx >> 16) : 0u;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            r.sse_all += shfl_xor_u64(r.sse_all, m), r.sse_flat += shfl_xor_u64(r.sse_flat, m);
            r.sad_all += shfl_xor_u64(r.sad_all, m), r.sad_flat += shfl_xor_u64(r.sad_flat, m);
            r.over_sum += shfl_xor_u64(r.over_sum, m), r.under_sum += shfl_xor_u64(r.under_sum, m);
            r.tiles_all += __shfl_xor(r.tiles_all, m), r.tiles_flat += __shfl_xor(r.tiles_flat, m);
            r.samples_all += __shfl_xor(r.samples_all, m), r.samples_flat += __shfl_xor(r.samples_flat, m);
            r.over += __shfl_xor(r.over, m), r.under += __shfl_xor(r.under, m);
            const uint32_t om = __shfl_xor(r.over_max, m), um = __shfl_xor(r.under_max, m);
            r.over_max = om > r.over_max ? om : r.over_max;
            r.under_max = um > r.under_max ? um : r.under_max;
        }
        if (lane == 0u) partials[unit] = r;
    }
}

/* One block per frame: each plane's partials summed (integer sums and maxima: any order gives the same), then the figures */
__global__ __launch_bounds__(256) void k_regions_sum(regions_geom g, const regions_partial *__restrict__ partials, h2y_regions_stats *__restrict__ stats)
{
    __shared__ uint64_t s_sum[12][kThreads];
    __shared__ uint32_t s_max[2][kThreads];
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    const uint32_t per_frame = g.units[0] + g.units[1] + g.units[2];
    h2y_regions_stats &o = stats[f];
    for (uint32_t p = 0; p < 3u; p++) {
        const regions_partial *part = partials + (size_t)f * per_frame + (p > 0u ? g.units[0] : 0u) + (p > 1u ? g.units[1] : 0u);
        uint64_t s[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        uint32_t mo = 0u, mu = 0u;
        for (uint32_t c = tid; c < g.units[p]; c += kThreads) {
            const regions_partial r = part[c];
            s[0] += r.tiles_all, s[1] += r.tiles_flat, s[2] += r.samples_all, s[3] += r.samples_flat;
            s[4] += r.sse_all, s[5] += r.sse_flat, s[6] += r.sad_all, s[7] += r.sad_flat;
            s[8] += r.over, s[9] += r.over_sum, s[10] += r.under, s[11] += r.under_sum;
            mo = r.over_max > mo ? r.over_max : mo;
            mu = r.under_max > mu ? r.under_max : mu;
        }
        for (uint32_t k = 0; k < 12u; k++) s_sum[k][tid] = s[k];
        s_max[0][tid] = mo, s_max[1][tid] = mu;
        __syncthreads();
        for (uint32_t h = kThreads / 2u; h > 0u; h >>= 1) {
            if (tid < h) {
                for (uint32_t k = 0; k < 12u; k++) s_sum[k][tid] += s_sum[k][tid + h];
                for (uint32_t k = 0; k < 2u; k++) s_max[k][tid] = s_max[k][tid + h] > s_max[k][tid] ? s_max[k][tid + h] : s_max[k][tid];
            }
            __syncthreads();
        }
        if (tid == 0u) { /* busy = all - flat */
            o.tiles[p][0] = s_sum[1][0], o.tiles[p][1] = s_sum[0][0] - s_sum[1][0];
            o.samples[p][0] = s_sum[3][0], o.samples[p][1] = s_sum[2][0] - s_sum[3][0];
            o.sse[p][0] = s_sum[5][0], o.sse[p][1] = s_sum[4][0] - s_sum[5][0];
            o.sad[p][0] = s_sum[7][0], o.sad[p][1] = s_sum[6][0] - s_sum[7][0];
            o.over[p] = s_sum[8][0], o.over_sum[p] = s_sum[9][0];
            o.under[p] = s_sum[10][0], o.under_sum[p] = s_sum[11][0];
            o.over_max[p] = s_max[0][0], o.under_max[p] = s_max[1][0];
        }
        __syncthreads(); /* s_sum is reused by the next plane */
    }
    if (tid == 0u) o.flat_var = g.flat_var, o.radius = g.radius;
}

} // namespace

uint32_t h2y_regions_strips(uint32_t plane_width) { return ((plane_width + 7u) / 8u + kStripTiles - 1u) / kStripTiles; }
uint32_t h2y_regions_segments(uint32_t plane_height) { return (plane_height + kSegRows - 1u) / kSegRows; }

int h2y_regions_grid(int n_cu, const regions_geom &g, int n_frames)
{
    const uint64_t waves = (uint64_t)n_frames * (g.units[0] + g.units[1] + g.units[2]), blocks = (waves + kWaves - 1u) / kWaves;
    const uint64_t max_grid = (uint64_t)n_cu * 8u;
    return (int)(blocks < max_grid ? (blocks ? blocks : 1) : max_grid);
}

hipError_t h2y_launch_regions(int grid, hipStream_t st, const regions_geom &g, const cmp_frame *frames, int n_frames, regions_partial *partials,
                              h2y_regions_stats *stats)
{
    switch (g.radius) {
    case 1: hipLaunchKernelGGL(k_regions<1>, dim3(grid), dim3(kThreads), 0, st, g, frames, n_frames, partials); break;
    case 2: hipLaunchKernelGGL(k_regions<2>, dim3(grid), dim3(kThreads), 0, st, g, frames, n_frames, partials); break;
    case 3: hipLaunchKernelGGL(k_regions<3>, dim3(grid), dim3(kThreads), 0, st, g, frames, n_frames, partials); break;
    case 4: hipLaunchKernelGGL(k_regions<4>, dim3(grid), dim3(kThreads), 0, st, g, frames, n_frames, partials); break;
    default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_regions_sum, dim3(n_frames), dim3(kThreads), 0, st, g, partials, stats);
    return hipGetLastError();
}
