/*
 * h2y_dpx.hip -- the per-pixel loop of dpx_read() (/root/reference/dpx.cpp:412-520) followed by
 * muxed_dpx_to_planar_float_buf() (common.cpp:14-27), on the device.
 *
 *   k_dpx_decode<FMT, SWAP>  interleaved R,G,B DPX payloads -> planar float G, B, R (h2y_dpx_decode_batch, the DPX stream)
 *
 * The header, the file read and every check stay on the host (h2y_dpx_parse in h2y_api.hip).  The payload is one contiguous
 * run of width x height pixels (dpx_read honours no row padding) and the planes have none either, so a frame is a flat run of
 * pixels: no tiles.  What each pixel becomes is the reference's, bit for bit:
 *   10-bit  one 32-bit word per pixel, R = w >> 22, G = (w >> 12) & 1023, B = (w >> 2) & 1023, each (float)(c / 1023.0)
 *   16-bit  R, G, B u16 in a row, (float)(u / 65535.0)
 *   float   R, G, B binary32 bit patterns, copied as they are (NaN payloads survive)
 * with every 32-bit word (10-bit, float) or 16-bit word (16-bit) byte-swapped for a big-endian file.  The divides are the
 * reference's binary64 ones (correctly rounded, then rounded to float), not a reciprocal multiply: -ffp-contract=off and no
 * fast-math keep them exact.
 */
#include <hip/hip_runtime.h>

#include "h2y_kernels.h"

namespace {

/* pixels of one group: one 16-byte load per 4 pixels (10-bit), three per 8 (16-bit) or per 4 (float) */
template <int FMT> constexpr uint32_t dpx_group() { return FMT == H2Y_DPX_16 ? 8u : 4u; }
/* payload bytes of one pixel */
template <int FMT> constexpr uint32_t dpx_bpp() { return FMT == H2Y_DPX_10 ? 4u : FMT == H2Y_DPX_16 ? 6u : 12u; }

/* The table holds generic pointers; the accesses through them are declared global (address space 1) so that they are
 * global_load / global_store rather than flat ones */
#define H2Y_GLOBAL __attribute__((address_space(1)))
typedef const H2Y_GLOBAL char gchar_c;
typedef H2Y_GLOBAL uint32_t gu32;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4))); /* one 16-byte access */

__device__ __forceinline__ uint32_t swap32(uint32_t w) { return __builtin_bswap32(w); }
/* SHORT_SW on both halves of a word: the bytes of each u16 exchanged, the two u16 left in place */
__device__ __forceinline__ uint32_t swap16x2(uint32_t w) { return __builtin_amdgcn_perm(w, w, 0x02030001u); }

__device__ __forceinline__ float c10(uint32_t c) { return (float)((double)c / 1023.0); }
__device__ __forceinline__ float c16(uint32_t c) { return (float)((double)c / 65535.0); }

/* one group of pixels from `n` payload words `w` (already in file order) into g[], b[], r[] */
template <int FMT, bool SWAP> __device__ __forceinline__ void decode_words(const uint32_t *w, uint32_t *g, uint32_t *b, uint32_t *r)
{
    if constexpr (FMT == H2Y_DPX_10) {
        for (int k = 0; k < 4; k++) {
            const uint32_t x = SWAP ? swap32(w[k]) : w[k];
            r[k] = __float_as_uint(c10(x >> 22));
            g[k] = __float_as_uint(c10((x >> 12) & 1023u));
            b[k] = __float_as_uint(c10((x >> 2) & 1023u));
        }
    } else if constexpr (FMT == H2Y_DPX_16) {
        uint32_t u[24]; /* R0 G0 B0 R1 ... B7 */
        for (int k = 0; k < 12; k++) {
            const uint32_t x = SWAP ? swap16x2(w[k]) : w[k];
            u[2 * k] = x & 0xFFFFu;
            u[2 * k + 1] = x >> 16;
        }
        for (int k = 0; k < 8; k++) {
            r[k] = __float_as_uint(c16(u[3 * k]));
            g[k] = __float_as_uint(c16(u[3 * k + 1]));
            b[k] = __float_as_uint(c16(u[3 * k + 2]));
        }
    } else {
        for (int k = 0; k < 4; k++) {
            r[k] = SWAP ? swap32(w[3 * k]) : w[3 * k];
            g[k] = SWAP ? swap32(w[3 * k + 1]) : w[3 * k + 1];
            b[k] = SWAP ? swap32(w[3 * k + 2]) : w[3 * k + 2];
        }
    }
}

/* pixel group i of one frame.  vec16: the payload and all three planes start on a 16-byte boundary (every group then does) */
template <int FMT, bool SWAP>
__device__ __forceinline__ void decode_group(gchar_c *__restrict__ pay, gu32 *__restrict__ pg, gu32 *__restrict__ pb, gu32 *__restrict__ pr,
                                             uint32_t i, bool vec16)
{
    constexpr uint32_t P = dpx_group<FMT>(), NW = P * dpx_bpp<FMT>() / 4;
    const H2Y_GLOBAL uint32_t *src = reinterpret_cast<const H2Y_GLOBAL uint32_t *>(pay + (size_t)i * P * dpx_bpp<FMT>());
    uint32_t w[NW], g[P], b[P], r[P];
    if (vec16) {
        for (uint32_t k = 0; k < NW / 4; k++) {
            const u32x4 v = reinterpret_cast<const H2Y_GLOBAL u32x4 *>(src)[k];
            w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
        }
    } else
        for (uint32_t k = 0; k < NW; k++) w[k] = src[k];
    decode_words<FMT, SWAP>(w, g, b, r);
    const size_t o = (size_t)i * P;
    if (vec16) {
        for (uint32_t k = 0; k < P / 4; k++) {
            reinterpret_cast<H2Y_GLOBAL u32x4 *>(pg + o)[k] = u32x4{g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]};
            reinterpret_cast<H2Y_GLOBAL u32x4 *>(pb + o)[k] = u32x4{b[4 * k], b[4 * k + 1], b[4 * k + 2], b[4 * k + 3]};
            reinterpret_cast<H2Y_GLOBAL u32x4 *>(pr + o)[k] = u32x4{r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]};
        }
    } else
        for (uint32_t k = 0; k < P; k++) pg[o + k] = g[k], pb[o + k] = b[k], pr[o + k] = r[k];
}

/* one pixel j (the npix % group tail): 4-byte loads, 2-byte ones for a 16-bit payload (its pixels are 6 bytes apart) */
template <int FMT, bool SWAP>
__device__ __forceinline__ void decode_one(gchar_c *__restrict__ pay, gu32 *__restrict__ pg, gu32 *__restrict__ pb, gu32 *__restrict__ pr,
                                           uint32_t j)
{
    uint32_t g, b, r;
    if constexpr (FMT == H2Y_DPX_10) {
        uint32_t x = reinterpret_cast<const H2Y_GLOBAL uint32_t *>(pay)[j];
        if (SWAP) x = swap32(x);
        r = __float_as_uint(c10(x >> 22));
        g = __float_as_uint(c10((x >> 12) & 1023u));
        b = __float_as_uint(c10((x >> 2) & 1023u));
    } else if constexpr (FMT == H2Y_DPX_16) {
        const H2Y_GLOBAL uint16_t *s = reinterpret_cast<const H2Y_GLOBAL uint16_t *>(pay) + (size_t)3 * j;
        uint32_t u[3];
        for (int c = 0; c < 3; c++) u[c] = SWAP ? (uint32_t)__builtin_bswap16(s[c]) : (uint32_t)s[c];
        r = __float_as_uint(c16(u[0]));
        g = __float_as_uint(c16(u[1]));
        b = __float_as_uint(c16(u[2]));
    } else {
        const H2Y_GLOBAL uint32_t *s = reinterpret_cast<const H2Y_GLOBAL uint32_t *>(pay) + (size_t)3 * j;
        r = SWAP ? swap32(s[0]) : s[0];
        g = SWAP ? swap32(s[1]) : s[1];
        b = SWAP ? swap32(s[2]) : s[2];
    }
    pg[j] = g, pb[j] = b, pr[j] = r;
}

} // namespace

/* Grid-stride over (frame, chunk of 256 groups) units; a frame's last chunk also takes its npix % group single pixels.  The
 * frame is block-uniform: its payload and plane pointers are scalar loads from the table (__restrict__ const: nothing the
 * kernel stores can alias it).  Payload and planes need only be 4-byte aligned; the 16-byte accesses are taken per frame. */
template <int FMT, bool SWAP>
__global__ __launch_bounds__(256) void k_dpx_decode(uint32_t npix, const payload_frame *__restrict__ frames, int n_frames)
{
    constexpr uint32_t P = dpx_group<FMT>();
    const uint32_t groups = npix / P, tail = npix - groups * P;
    const uint32_t chunks = (groups + tail + 255) / 256, units = (uint32_t)n_frames * chunks;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t f = unit / chunks, i = (unit - f * chunks) * 256 + threadIdx.x;
        const payload_frame fr = frames[f];
        gchar_c *pay = (gchar_c *)fr.payload;
        gu32 *pg = (gu32 *)fr.plane[0], *pb = (gu32 *)fr.plane[1], *pr = (gu32 *)fr.plane[2];
        const bool vec16 = (((uintptr_t)pay | (uintptr_t)pg | (uintptr_t)pb | (uintptr_t)pr) & 15u) == 0;
        if (i < groups) decode_group<FMT, SWAP>(pay, pg, pb, pr, i, vec16);
        else if (i < groups + tail) decode_one<FMT, SWAP>(pay, pg, pb, pr, groups * P + (i - groups));
    }
}

namespace {

template <int FMT> void launch_fmt(bool swap, int grid, hipStream_t st, uint32_t npix, const payload_frame *frames, int n_frames)
{
    if (swap) hipLaunchKernelGGL((k_dpx_decode<FMT, true>), dim3(grid), dim3(256), 0, st, npix, frames, n_frames);
    else hipLaunchKernelGGL((k_dpx_decode<FMT, false>), dim3(grid), dim3(256), 0, st, npix, frames, n_frames);
}

} // namespace

uint32_t h2y_dpx_chunks(int fmt, uint32_t npix)
{
    const uint32_t p = fmt == H2Y_DPX_16 ? 8u : 4u, groups = npix / p;
    return (groups + (npix - groups * p) + 255) / 256;
}

hipError_t h2y_launch_dpx_decode(int fmt, bool swap, int grid, hipStream_t st, uint32_t npix, const payload_frame *frames, int n_frames)
{
    switch (fmt) {
    case H2Y_DPX_10: launch_fmt<H2Y_DPX_10>(swap, grid, st, npix, frames, n_frames); break;
    case H2Y_DPX_16: launch_fmt<H2Y_DPX_16>(swap, grid, st, npix, frames, n_frames); break;
    default: launch_fmt<H2Y_DPX_F32>(swap, grid, st, npix, frames, n_frames); break;
    }
    return hipGetLastError();
}
