/*
 * h2y_scale.hip -- the Lanczos resampler of include/hdr2yuv_hip.h ("scaling"), on the device.
 *
 *   k_scale  (frame, plane, tile) units: a tile of 64 x 32 outputs of one plane of one frame
 *
 * The tap tables come from the host (h2y_scale_taps' rows, one table per axis and plane kind); the device only multiplies and adds
 * integers.  A block loads its tile's two table slices into LDS, then walks the source rows the tile needs sixteen at a time: the
 * rows' segments are staged into LDS as u16 (16-byte loads where the whole group lies inside the plane -- the staged segment
 * starts at the 16-byte boundary below its first sample, so every group is aligned --, u16 loads at the plane's two ends; the
 * next chunk's loads are in flight while this one is summed), and the horizontal sums H of those rows go into an int32 LDS
 * tile (four rows per thread, one coefficient read for the four).  The
 * vertical sums are 64-bit multiply-adds over that tile (two columns per thread, one 8-byte LDS read for both); the result is
 * rounded once, clamped and stored as one dword per thread where the address is even.  No atomics, no float arithmetic.
 */
#include <hip/hip_runtime.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"

namespace {

#define H2Y_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kTW = H2Y_SCALE_TILE_W, kTH = H2Y_SCALE_TILE_H, kTaps = H2Y_SCALE_MAX_TAPS, kStage = H2Y_SCALE_STAGE_ROWS;
static_assert(kTW == 64 && kTH == 32 && kStage == 16 && kTaps == 32, "k_scale's thread mapping is written for these");

__device__ __forceinline__ uint32_t clamp_round(long long v, int32_t lo, int32_t hi)
{
    const long long q = (v + (1ll << 27)) >> 28;
    return (uint32_t)(q < lo ? lo : q > hi ? hi : q);
}

} // namespace

extern __shared__ __attribute__((aligned(16))) unsigned char k_scale_lds[];

__global__ __launch_bounds__(256) void k_scale(scale_geom g, const scale_frame *__restrict__ frames, int n_frames)
{
    int32_t *s_H = reinterpret_cast<int32_t *>(k_scale_lds);                /* [h_rows][64] */
    uint16_t *s_src = reinterpret_cast<uint16_t *>(s_H + g.h_rows * kTW);   /* [16][src_cols] */
    int16_t *s_ch = reinterpret_cast<int16_t *>(s_src + kStage * g.src_cols); /* [tap][64]: lanes of one tap side by side */
    int16_t *s_cv = s_ch + kTaps * kTW;                                     /* [32][tap] */
    int32_t *s_fh = reinterpret_cast<int32_t *>(s_cv + kTH * kTaps), *s_nh = s_fh + kTW, *s_fv = s_nh + kTW, *s_nv = s_fv + kTH;
    const uint32_t per_frame = g.p[0].tiles + g.p[1].tiles + g.p[2].tiles, units = (uint32_t)n_frames * per_frame;
    const uint32_t tid = threadIdx.x;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t f = unit / per_frame, r = unit - f * per_frame;
        const uint32_t p = r < g.p[0].tiles ? 0u : r < g.p[0].tiles + g.p[1].tiles ? 1u : 2u;
        const uint32_t tile = r - (p > 0u ? g.p[0].tiles : 0u) - (p > 1u ? g.p[1].tiles : 0u);
        scale_plane P = g.p[0];
        if (p == 1u) P = g.p[1];
        if (p == 2u) P = g.p[2];
        const scale_frame fr = frames[f];
        const H2Y_GLOBAL uint16_t *src = (const H2Y_GLOBAL uint16_t *)fr.src + P.src_off;
        const uint32_t x0 = (tile % P.tiles_x) * kTW, y0 = (tile / P.tiles_x) * kTH;
        const uint32_t nx = P.dw - x0 < kTW ? P.dw - x0 : kTW, ny = P.dh - y0 < kTH ? P.dh - y0 : kTH;
        /* the tile's slices of the two tables */
        if (tid < kTW) {
            s_fh[tid] = tid < nx ? P.h.first[x0 + tid] : 0;
            s_nh[tid] = tid < nx ? P.h.count[x0 + tid] : 0;
        } else if (tid < kTW + kTH) {
            const uint32_t j = tid - kTW;
            s_fv[j] = j < ny ? P.v.first[y0 + j] : 0;
            s_nv[j] = j < ny ? P.v.count[y0 + j] : 0;
        }
        {
            const uint32_t *ch = reinterpret_cast<const uint32_t *>(P.h.coef), *cv = reinterpret_cast<const uint32_t *>(P.v.coef);
#pragma unroll
            for (uint32_t k = 0; k < kTW * kTaps / 2u / 256u; k++) {
                const uint32_t d = tid + 256u * k, col = d / (kTaps / 2u), pair = d % (kTaps / 2u);
                const uint32_t w = col < nx ? ch[(size_t)(x0 + col) * (kTaps / 2u) + pair] : 0u;
                s_ch[(2u * pair) * kTW + col] = (int16_t)(w & 0xFFFFu);
                s_ch[(2u * pair + 1u) * kTW + col] = (int16_t)(w >> 16);
            }
#pragma unroll
            for (uint32_t k = 0; k < kTH * kTaps / 2u / 256u; k++) {
                const uint32_t d = tid + 256u * k, row = d / (kTaps / 2u);
                reinterpret_cast<uint32_t *>(s_cv)[d] = row < ny ? cv[(size_t)y0 * (kTaps / 2u) + d] : 0u;
            }
        }
        __syncthreads();
        const uint32_t x_lo = (uint32_t)s_fh[0], seg = (uint32_t)(s_fh[nx - 1u] + s_nh[nx - 1u]) - x_lo;
        const uint32_t row0 = (uint32_t)s_fv[0], rows = (uint32_t)(s_fv[ny - 1u] + s_nv[ny - 1u]) - row0;
        const uint32_t n_src = P.sw * P.sh;
        /* the host sized the LDS from the same tables: a tile that does not fit is a fault of the tables, and is left unwritten */
        const bool fits = rows <= g.h_rows && seg + 7u <= g.src_cols && g.src_cols <= 512u && x_lo + seg <= P.sw && row0 + rows <= P.sh;
        /* A thread's share of a chunk of kStage source rows: rows (tid >> 5) + 8 j, groups (tid & 31) + 32 q of each.  The next
         * chunk's loads are issued before the horizontal sums of the one in LDS and written to LDS after them. */
        constexpr uint32_t kStageRows = kStage / 8u;
        u32x4 held[kStageRows][2];
        const uint32_t srow = tid >> 5, slane = tid & 31u;
        auto stage_load = [&](uint32_t c0) {
#pragma unroll
            for (uint32_t j = 0; j < kStageRows; j++) {
                const uint32_t k = srow + 8u * j;
                const uint32_t i0 = (row0 + c0 + k) * P.sw + x_lo, shift = (P.src_off + i0) & 7u;
                const int32_t start = (int32_t)i0 - (int32_t)shift;
                const uint32_t groups = (seg + shift + 7u) / 8u;
#pragma unroll
                for (uint32_t q2 = 0; q2 < 2u; q2++) {
                    const uint32_t q = slane + 32u * q2;
                    u32x4 v = {0u, 0u, 0u, 0u};
                    if (c0 + k < rows && q < groups) {
                        const int32_t idx = start + (int32_t)(8u * q);
                        if (idx >= 0 && (uint32_t)idx + 8u <= n_src)
                            v = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(src + idx);
                        else { /* a group cut by one of the plane's ends: its own samples only */
                            uint32_t e[8];
#pragma unroll
                            for (int t = 0; t < 8; t++) {
                                const int32_t i = idx + t;
                                e[t] = (i >= 0 && (uint32_t)i < n_src) ? src[i] : 0u;
                            }
                            v.x = e[0] | e[1] << 16, v.y = e[2] | e[3] << 16, v.z = e[4] | e[5] << 16, v.w = e[6] | e[7] << 16;
                        }
                    }
                    held[j][q2] = v;
                }
            }
        };
        auto stage_store = [&](uint32_t c0) {
#pragma unroll
            for (uint32_t j = 0; j < kStageRows; j++) {
                const uint32_t k = srow + 8u * j;
                const uint32_t shift = (P.src_off + (row0 + c0 + k) * P.sw + x_lo) & 7u, groups = (seg + shift + 7u) / 8u;
#pragma unroll
                for (uint32_t q2 = 0; q2 < 2u; q2++) {
                    const uint32_t q = slane + 32u * q2;
                    if (c0 + k < rows && q < groups) *reinterpret_cast<u32x4 *>(s_src + k * g.src_cols + 8u * q) = held[j][q2];
                }
            }
        };
        if (fits) stage_load(0u);
        for (uint32_t c0 = 0; fits && c0 < rows; c0 += kStage) {
            stage_store(c0);
            __syncthreads();
            if (c0 + kStage < rows) stage_load(c0 + kStage);
            { /* H of four staged rows per thread: one coefficient read serves the four */
                const uint32_t x = tid & 63u, k0 = (tid >> 6) * (kStage / 4u);
#pragma unroll
                for (uint32_t pass = 0; pass < kStage / 16u; pass++) {
                    const uint32_t kb = k0 + 4u * pass;
                    if (x >= nx || c0 + kb >= rows) continue;
                    const uint32_t n = (uint32_t)s_nh[x], fx = (uint32_t)s_fh[x] - x_lo;
                    const uint16_t *p[4];
                    int32_t acc[4] = {0, 0, 0, 0};
#pragma unroll
                    for (uint32_t r = 0; r < 4u; r++) {
                        const uint32_t k = c0 + kb + r < rows ? kb + r : kb; /* a row past the tile's last repeats the first: not stored */
                        p[r] = s_src + k * g.src_cols + ((P.src_off + (row0 + c0 + k) * P.sw + x_lo) & 7u) + fx;
                    }
                    for (uint32_t i = 0; i < n; i++) {
                        const int32_t c = s_ch[i * kTW + x];
#pragma unroll
                        for (uint32_t r = 0; r < 4u; r++) acc[r] += c * (int32_t)p[r][i];
                    }
#pragma unroll
                    for (uint32_t r = 0; r < 4u; r++)
                        if (c0 + kb + r < rows) s_H[(c0 + kb + r) * kTW + x] = acc[r];
                }
            }
            __syncthreads();
        }
        if (fits) { /* V of two columns per thread, four rows each */
            const uint32_t xp = (tid & 31u) * 2u, yr = tid >> 5;
            uint16_t *dst = fr.dst;
#pragma unroll
            for (uint32_t k = 0; k < kTH / 8u; k++) {
                const uint32_t y = yr + 8u * k;
                if (y >= ny || xp >= nx) continue;
                const uint32_t n = (uint32_t)s_nv[y], hr = (uint32_t)s_fv[y] - row0;
                long long a0 = 0, a1 = 0;
                for (uint32_t j = 0; j < n; j++) {
                    const long long c = s_cv[y * kTaps + j];
                    const int2 h = *reinterpret_cast<const int2 *>(s_H + (hr + j) * kTW + xp);
                    a0 += c * h.x;
                    a1 += c * h.y;
                }
                const uint32_t o0 = clamp_round(a0, P.lo, P.hi), o1 = clamp_round(a1, P.lo, P.hi);
                const size_t di = (size_t)P.dst_off + (size_t)(y0 + y) * P.dw + x0 + xp;
                if (xp + 1u >= nx) dst[di] = (uint16_t)o0;
                else if ((di & 1u) == 0u) *reinterpret_cast<uint32_t *>(dst + di) = o0 | o1 << 16;
                else dst[di] = (uint16_t)o0, dst[di + 1u] = (uint16_t)o1;
            }
        }
        __syncthreads(); /* the LDS is reused by the next unit */
    }
}

size_t h2y_scale_lds(const scale_geom &g)
{
    return (size_t)g.h_rows * kTW * sizeof(int32_t) + (size_t)kStage * g.src_cols * sizeof(uint16_t) + (size_t)kTaps * kTW * sizeof(int16_t) +
           (size_t)kTH * kTaps * sizeof(int16_t) + (size_t)(2u * kTW + 2u * kTH) * sizeof(int32_t);
}

hipError_t h2y_launch_scale(int grid, hipStream_t st, const scale_geom &g, const scale_frame *frames, int n_frames)
{
    hipLaunchKernelGGL(k_scale, dim3(grid), dim3(256), h2y_scale_lds(g), st, g, frames, n_frames);
    return hipGetLastError();
}
