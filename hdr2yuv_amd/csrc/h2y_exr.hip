/*
 * h2y_exr.hip -- the per-pixel work of read_exr() (the reference's exr.cpp:138-255) on the device.
 *
 *   k_exr_decode  unpacked scanline chunks -> half planes G, B, R (h2y_exr_decode_batch, the EXR ring)
 *
 * The header, the offset table, zlib and RLE stay on the host (h2y_exr_parse, h2y_exr_unpack in h2y_api.hip).  A payload is
 * one flag byte per chunk (padded to flags_bytes), then every chunk's lines in row order.  A raw chunk holds its lines as an
 * uncompressed file would: per line, `width` samples of each channel in channel-list order.  An encoded chunk (RLE or ZIP,
 * expanded) holds the same n bytes after OpenEXR's reorder and predictor, which this kernel undoes:
 *   predictor  t[i] = t[i-1] + t[i] - 128 (mod 256) for i >= 1, over the whole chunk
 *   reorder    output byte 2k = t[k], output byte 2k+1 = t[n/2 + k] (n is even: every sample is 2 or 4 bytes)
 * So 16-bit word k of the chunk is t[k] | t[n/2 + k] << 8, where t[i] = 128 + sum_{j<=i} (raw[j] - 128) mod 256.
 * What each sample becomes is RgbaInputFile's: HALF bit for bit, FLOAT through floatToHalf, UINT through uintToHalf;
 * a missing R, G or B channel reads +0.0.
 */
#include <hip/hip_runtime.h>

#include "h2y_kernels.h"

namespace {

#define H2Y_GLOBAL __attribute__((address_space(1)))
typedef const H2Y_GLOBAL unsigned char gbyte_c;
typedef H2Y_GLOBAL uint16_t gu16;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4))); /* one 16-byte access */

constexpr uint32_t kThreads = 256, kWave = 64, kWaves = kThreads / kWave;
constexpr uint32_t kTile = kThreads * 16u; /* bytes of each half an encoded chunk advances per step */

/* OpenEXR 2.x floatToHalf (ImfRgbaFile.cpp): a finite |f| > HALF_MAX becomes +-inf before any rounding; otherwise half(f):
 * round to nearest even, float subnormals to +-0, half subnormals rounded likewise; a NaN keeps the top 10 mantissa bits and
 * gets a 1 when they are all 0 (half::convert). */
__device__ __forceinline__ uint32_t float_to_half(uint32_t i)
{
    const uint32_t s = (i >> 16) & 0x8000u, e = (i >> 23) & 0xFFu;
    uint32_t m = i & 0x7FFFFFu;
    if (e == 0xFFu) {
        if (!m) return s | 0x7C00u;
        m >>= 13;
        return s | 0x7C00u | m | (m == 0u);
    }
    if ((i & 0x7FFFFFFFu) > 0x477FE000u) return s | 0x7C00u; /* |f| > 65504 */
    const int E = (int)e - 112;
    if (E <= 0) {
        if (E < -10) return s;
        m |= 0x800000u;
        const int t = 14 - E;
        const uint32_t a = (1u << (t - 1)) - 1u, b = (m >> t) & 1u;
        return s | ((m + a + b) >> t);
    }
    m = m + 0xFFFu + ((m >> 13) & 1u);
    return s | (((uint32_t)E << 10) + (m >> 13)); /* a carry out of the mantissa moves into the exponent */
}

/* uintToHalf: u > HALF_MAX is +inf, otherwise half((float)u) (exact up to 2^24, then float's round to nearest even) */
__device__ __forceinline__ uint32_t uint_to_half(uint32_t u)
{
    return u > 65504u ? 0x7C00u : float_to_half(__float_as_uint((float)u));
}

/* Where word w (bytes 2w, 2w+1) of a chunk goes: plane c, element idx, and whether it completes a 4-byte sample (hi: the
 * sample is word w-1 | word w << 16).  -1: a word of a skipped channel, or the low half of a 4-byte sample. */
__device__ __forceinline__ int locate(const exr_geom &g, uint32_t row0, uint32_t w, uint32_t &idx, bool &hi)
{
    const uint32_t b = 2u * w, line = b / g.line_bytes, lb = b - line * g.line_bytes;
    for (int c = 0; c < 3; c++) {
        if (g.type[c] < 0) continue;
        const uint32_t size = g.type[c] == 1 ? 2u : 4u;
        const uint32_t rel = lb - (uint32_t)g.offset[c]; /* wraps when lb lies before the channel */
        if (rel >= g.width * size) continue;
        if (size == 4u && (rel & 3u) != 2u) return -1;
        idx = (row0 + line) * g.width + rel / size;
        hi = size == 4u;
        return c;
    }
    return -1;
}

__device__ __forceinline__ void emit(const exr_geom &g, const payload_frame &fr, int c, uint32_t idx, bool hi, uint32_t cur, uint32_t prev)
{
    uint32_t v = cur;
    if (hi) v = g.type[c] == 2 ? float_to_half(prev | cur << 16) : uint_to_half(prev | cur << 16);
    ((gu16 *)fr.plane[c])[idx] = (uint16_t)v;
}

/* the 16 bytes at p as four words, byte loads past `end` reading `fill` */
__device__ __forceinline__ void load16(gbyte_c *p, uint32_t avail, bool vec, uint32_t fill, uint32_t w[4])
{
    if (vec && avail >= 16u) {
        const u32x4 v = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(p);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
        return;
    }
    for (int k = 0; k < 4; k++) {
        uint32_t x = 0;
        for (int j = 0; j < 4; j++) x |= (uint32_t)(4u * k + j < avail ? p[4 * k + j] : fill) << (8 * j);
        w[k] = x;
    }
}

__device__ __forceinline__ uint32_t byte_sum(uint32_t x) { return (x & 0x00FF00FFu) + ((x >> 8) & 0x00FF00FFu); } /* 2 lanes of 16 bits */

/* block-wide sum of v (every thread gets it); part: 4 words of LDS, not touched by any other thread until a later barrier */
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *part)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
    if ((threadIdx.x & (kWave - 1u)) == 0u) part[threadIdx.x / kWave] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

/* block-wide exclusive prefix sum of v; *total gets the sum over the block */
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *part, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & (kWave - 1u), wid = threadIdx.x / kWave;
    uint32_t x = v;
    for (int o = 1; o < (int)kWave; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, kWave);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == kWave - 1u) part[wid] = x;
    __syncthreads();
    const uint32_t p0 = part[0], p1 = part[1], p2 = part[2], p3 = part[3];
    *total = p0 + p1 + p2 + p3;
    return (wid > 0u ? p0 : 0u) + (wid > 1u ? p1 : 0u) + (wid > 2u ? p2 : 0u) + x - v;
}

/* 8 half words from word g of an all-half chunk into their plane with one 16-byte store, if their channel is read (the 8
 * lie in one channel's run of a line: g and width are multiples of 8) */
__device__ __forceinline__ void store8(const exr_geom &g, const payload_frame &fr, uint32_t row0, uint32_t gw, const uint32_t v[4])
{
    const uint32_t seg = gw / g.width, line = seg / g.n_channels, k = seg - line * g.n_channels, x = gw - seg * g.width;
    for (int c = 0; c < 3; c++)
        if (g.type[c] >= 0 && (uint32_t)g.offset[c] == k * 2u * g.width) {
            gu16 *dst = (gu16 *)fr.plane[c] + (size_t)(row0 + line) * g.width + x;
            *reinterpret_cast<H2Y_GLOBAL u32x4 *>(dst) = u32x4{v[0], v[1], v[2], v[3]};
        }
}

} // namespace

/* Grid-stride over (frame, chunk) units, both uniform per block; the chunk's flag byte picks the path.
 *   raw      every word read once from the payload; all-half files whose width is a multiple of 8 move 8 samples per
 *            16-byte load and store, and read only the channels that become planes
 *   encoded  first the sum of (t[j] - 128) over the first half (the predictor's value where the second half begins), then
 *            both halves in step, 16 bytes of each per thread: a byte prefix sum in registers, one block scan of the two
 *            thread totals (packed in one word: each total is < 256, 256 of them < 2^16), two running carries; each 16-bit
 *            word is assembled once and goes to its plane (directly on the all-half fast path, else through an LDS tile so
 *            that a 4-byte sample split between two threads is whole)
 * Missing channels: the unit zeroes its lines of that plane. */
__global__ __launch_bounds__(256) void k_exr_decode(exr_geom g, const payload_frame *__restrict__ frames, int n_frames)
{
    __shared__ uint32_t s_part[2][kWaves];
    __shared__ uint16_t s_words[1 + kTile];
    const uint32_t units = (uint32_t)n_frames * g.n_chunks;
    const uint32_t tid = threadIdx.x;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t f = __builtin_amdgcn_readfirstlane(unit / g.n_chunks), c = unit - f * g.n_chunks;
        const payload_frame fr = frames[f];
        gbyte_c *pay = (gbyte_c *)fr.payload;
        const uint32_t row0 = c * g.lines_per_chunk;
        const uint32_t lines = g.height - row0 < g.lines_per_chunk ? g.height - row0 : g.lines_per_chunk;
        const uint32_t n = lines * g.line_bytes, nw = n / 2u;
        gbyte_c *base = pay + g.flags_bytes + (size_t)row0 * g.line_bytes;
        const bool encoded = __builtin_amdgcn_readfirstlane(pay[c]) != 0u;
        const bool planes16 = (((uintptr_t)fr.plane[0] | (uintptr_t)fr.plane[1] | (uintptr_t)fr.plane[2]) & 15u) == 0;
        const bool fast = g.all_half && (g.width & 7u) == 0u && planes16;
        for (int p = 0; p < 3; p++)
            if (g.type[p] < 0)
                for (uint32_t i = tid; i < lines * g.width; i += kThreads) ((gu16 *)fr.plane[p])[(size_t)row0 * g.width + i] = 0;
        if (!encoded) {
            if (fast && ((uintptr_t)base & 15u) == 0) {
                for (uint32_t i = tid; i < nw / 8u; i += kThreads) {
                    const uint32_t gw = 8u * i, seg = gw / g.width, k = seg - seg / g.n_channels * g.n_channels;
                    bool read = false;
                    for (int p = 0; p < 3; p++) read |= g.type[p] >= 0 && (uint32_t)g.offset[p] == k * 2u * g.width;
                    if (!read) continue; /* a skipped channel's run: not even loaded */
                    const u32x4 v = reinterpret_cast<const H2Y_GLOBAL u32x4 *>(base)[i];
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                    store8(g, fr, row0, gw, w);
                }
            } else {
                const gu16 *src = (const gu16 *)base;
                for (uint32_t w = tid; w < nw; w += kThreads) {
                    uint32_t idx;
                    bool hi;
                    const int p = locate(g, row0, w, idx, hi);
                    if (p >= 0) emit(g, fr, p, idx, hi, src[w], hi ? src[w - 1u] : 0u);
                }
            }
        } else {
            const uint32_t h = nw; /* bytes in each half */
            const bool vec = (((uintptr_t)base | h) & 15u) == 0;
            uint32_t sum = 0; /* sum of the first half's bytes (mod 2^32: only its low 8 bits matter) */
            for (uint32_t i = tid * 16u; i < h; i += kTile) {
                uint32_t w[4];
                load16(base + i, h - i, vec, 0u, w);
                const uint32_t s = byte_sum(w[0]) + byte_sum(w[1]) + byte_sum(w[2]) + byte_sum(w[3]);
                sum += (s & 0xFFFFu) + (s >> 16);
            }
            sum = block_sum(sum, s_part[1]);
            uint32_t carry_a = 128u, carry_b = 128u + sum - 128u * h; /* t[-1] := 128; t[h-1] */
            uint32_t last = 0; /* thread 255: the previous step's last word */
            for (uint32_t t0 = 0, step = 0; t0 < h; t0 += kTile, step++) {
                const uint32_t p = t0 + tid * 16u, avail = p < h ? h - p : 0u;
                uint32_t a[4], b[4];
                load16(base + p, avail, vec, 128u, a); /* past the end: 128, a zero step of the predictor */
                load16(base + h + p, avail, vec, 128u, b);
                uint32_t sa[16], sb[16], ra = 0, rb = 0;
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    ra += ((a[k >> 2] >> (8 * (k & 3))) & 0xFFu) - 128u;
                    rb += ((b[k >> 2] >> (8 * (k & 3))) & 0xFFu) - 128u;
                    sa[k] = ra, sb[k] = rb;
                }
                uint32_t total;
                const uint32_t excl = block_excl_scan((ra & 0xFFu) | (rb & 0xFFu) << 16, s_part[step & 1u], &total);
                const uint32_t ca = carry_a + (excl & 0xFFFFu), cb = carry_b + (excl >> 16);
                carry_a += total & 0xFFFFu;
                carry_b += total >> 16;
                uint32_t wv[8]; /* words p .. p+15, two per entry */
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const uint32_t w0 = ((ca + sa[2 * k]) & 0xFFu) | ((cb + sb[2 * k]) & 0xFFu) << 8;
                    const uint32_t w1 = ((ca + sa[2 * k + 1]) & 0xFFu) | ((cb + sb[2 * k + 1]) & 0xFFu) << 8;
                    wv[k] = w0 | w1 << 16;
                }
                if (fast && vec) { /* h % 16 == 0: a thread has 16 words or none */
                    if (avail) {
                        store8(g, fr, row0, p, wv);
                        store8(g, fr, row0, p + 8u, wv + 4);
                    }
                } else {
                    if (tid == kThreads - 1u) s_words[0] = (uint16_t)last;
#pragma unroll
                    for (int k = 0; k < 16; k++) s_words[1u + tid * 16u + k] = (uint16_t)(wv[k >> 1] >> (16 * (k & 1)));
                    last = wv[7] >> 16;
                    __syncthreads();
                    for (uint32_t j = tid; j < kTile && t0 + j < h; j += kThreads) {
                        uint32_t idx;
                        bool hi;
                        const int pl = locate(g, row0, t0 + j, idx, hi);
                        if (pl >= 0) emit(g, fr, pl, idx, hi, s_words[1u + j], s_words[j]);
                    }
                }
            }
        }
        __syncthreads(); /* the next unit reuses s_part and s_words */
    }
}

hipError_t h2y_launch_exr_decode(int grid, hipStream_t st, const exr_geom &g, const payload_frame *frames, int n_frames)
{
    hipLaunchKernelGGL(k_exr_decode, dim3(grid), dim3(256), 0, st, g, frames, n_frames);
    return hipGetLastError();
}
