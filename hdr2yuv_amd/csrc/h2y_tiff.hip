/*
 * h2y_tiff.hip -- the per-pixel work of read_tiff() (the reference's tiff.cpp:54-362) and write_tiff() (tiff.cpp:559-652), on
 * the device.
 *
 *   k_tiff_decode<SWAP, CLAMP>  rows of interleaved R,G,B u16 -> planes G, B, R (h2y_tiff_decode_batch, the TIFF ring)
 *   k_rgb_interleave            planes G, B, R -> interleaved R,G,B u16 (h2y_rgb_interleave_batch, the TIFF inverse ring)
 *
 * The IFD, the file read and every check stay on the host (h2y_tiff_parse in h2y_api.hip).  A decode payload is `height` whole
 * file rows of row_bytes = 6 x file width, packed one after the other; the decoded picture is pixels x0 .. x0 + width - 1 of
 * each row (read_tiff's centre crop).  What each pixel becomes is the reference's: u16 samples R, G, B taken as they are (with
 * the bytes of each u16 exchanged for an "MM" file -- an extension: the reference reads those unswapped), clamped to
 * [4096, 60160] when the input picture is video range (set_pic_clip of a 16-bit picture, common.cpp:300-327), and stored as
 * G -> plane 0, B -> plane 1, R -> plane 2.  The interleave is write_tiff's Line[]: R, G, B per pixel, from planes 2, 0, 1.
 */
#include <hip/hip_runtime.h>

#include "h2y_kernels.h"

namespace {

#define H2Y_GLOBAL __attribute__((address_space(1)))
typedef const H2Y_GLOBAL char gchar_c;
typedef H2Y_GLOBAL uint16_t gu16;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4))); /* one 16-byte access */

constexpr uint32_t kVideoMin = 4096u, kVideoMax = 60160u; /* minVR, maxVR of a 16-bit picture */

template <bool SWAP, bool CLAMP> __device__ __forceinline__ uint32_t sample(uint32_t u)
{
    if (SWAP) u = ((u & 0xFFu) << 8) | (u >> 8);
    if (CLAMP) u = u < kVideoMin ? kVideoMin : u > kVideoMax ? kVideoMax : u;
    return u;
}

} // namespace

/* Grid-stride over (frame, chunk of 256 groups) units; a group is 8 pixels of one row (the last group of a row fewer when
 * width % 8).  The frame is block-uniform: its pointers are scalar loads from the table.  Full groups take three 16-byte loads
 * where the frame's payload, row_bytes and 6 x0 are multiples of 16 (every group's 48 bytes then start on a 16-byte boundary),
 * and one 16-byte store per plane where the planes and the plane row (2 x width) are; u16 accesses elsewhere. */
template <bool SWAP, bool CLAMP>
__global__ __launch_bounds__(256) void k_tiff_decode(tiff_geom g, const payload_frame *__restrict__ frames, int n_frames)
{
    const uint32_t gpr = (g.width + 7u) / 8u, groups = gpr * g.height;
    const uint32_t chunks = (groups + 255u) / 256u, units = (uint32_t)n_frames * chunks;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t f = unit / chunks, i = (unit - f * chunks) * 256u + threadIdx.x;
        const payload_frame fr = frames[f];
        if (i >= groups) continue;
        const uint32_t row = i / gpr, px = (i - row * gpr) * 8u;
        const uint32_t cnt = g.width - px < 8u ? g.width - px : 8u;
        gchar_c *src = (gchar_c *)fr.payload + (size_t)row * g.row_bytes + (size_t)(g.x0 + px) * 6u;
        gu16 *pg = (gu16 *)fr.plane[0], *pb = (gu16 *)fr.plane[1], *pr = (gu16 *)fr.plane[2];
        const bool vload = (((uintptr_t)fr.payload | g.row_bytes | g.x0 * 6u) & 15u) == 0;
        const bool vstore = (((uintptr_t)pg | (uintptr_t)pb | (uintptr_t)pr | g.width * 2u) & 15u) == 0;
        const size_t o = (size_t)row * g.width + px;
        if (cnt == 8u && vload) {
            uint32_t w[12];
            for (int k = 0; k < 3; k++) {
                const u32x4 v = reinterpret_cast<const H2Y_GLOBAL u32x4 *>(src)[k];
                w[4 * k] = v.x, w[4 * k + 1] = v.y, w[4 * k + 2] = v.z, w[4 * k + 3] = v.w;
            }
            uint32_t u[24]; /* R0 G0 B0 R1 ... B7 */
            for (int k = 0; k < 12; k++) {
                u[2 * k] = sample<SWAP, CLAMP>(w[k] & 0xFFFFu);
                u[2 * k + 1] = sample<SWAP, CLAMP>(w[k] >> 16);
            }
            if (vstore) {
                uint32_t pgw[4], pbw[4], prw[4];
                for (int k = 0; k < 4; k++) {
                    prw[k] = u[6 * k] | u[6 * k + 3] << 16;
                    pgw[k] = u[6 * k + 1] | u[6 * k + 4] << 16;
                    pbw[k] = u[6 * k + 2] | u[6 * k + 5] << 16;
                }
                *reinterpret_cast<H2Y_GLOBAL u32x4 *>(pg + o) = u32x4{pgw[0], pgw[1], pgw[2], pgw[3]};
                *reinterpret_cast<H2Y_GLOBAL u32x4 *>(pb + o) = u32x4{pbw[0], pbw[1], pbw[2], pbw[3]};
                *reinterpret_cast<H2Y_GLOBAL u32x4 *>(pr + o) = u32x4{prw[0], prw[1], prw[2], prw[3]};
            } else
                for (int k = 0; k < 8; k++) pg[o + k] = (uint16_t)u[3 * k + 1], pb[o + k] = (uint16_t)u[3 * k + 2], pr[o + k] = (uint16_t)u[3 * k];
        } else {
            const H2Y_GLOBAL uint16_t *s = reinterpret_cast<const H2Y_GLOBAL uint16_t *>(src);
            for (uint32_t k = 0; k < cnt; k++) {
                pr[o + k] = (uint16_t)sample<SWAP, CLAMP>(s[3 * k]);
                pg[o + k] = (uint16_t)sample<SWAP, CLAMP>(s[3 * k + 1]);
                pb[o + k] = (uint16_t)sample<SWAP, CLAMP>(s[3 * k + 2]);
            }
        }
    }
}

/* Grid-stride over (frame, chunk of 256 groups of 8 pixels) units; a frame's last chunk also takes its npix % 8 single pixels.
 * 16-byte accesses (one load per plane, three stores) where the three planes and the output of that frame are 16-byte aligned. */
__global__ __launch_bounds__(256) void k_rgb_interleave(uint32_t npix, const rgb_frame *__restrict__ frames, int n_frames)
{
    const uint32_t groups = npix / 8u, tail = npix - groups * 8u;
    const uint32_t chunks = (groups + tail + 255u) / 256u, units = (uint32_t)n_frames * chunks;
    for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x) {
        const uint32_t f = unit / chunks, i = (unit - f * chunks) * 256u + threadIdx.x;
        const rgb_frame fr = frames[f];
        const gu16 *pg = (const gu16 *)fr.plane[0], *pb = (const gu16 *)fr.plane[1], *pr = (const gu16 *)fr.plane[2];
        gu16 *out = (gu16 *)fr.rgb;
        const bool vec16 = (((uintptr_t)pg | (uintptr_t)pb | (uintptr_t)pr | (uintptr_t)out) & 15u) == 0;
        if (i < groups) {
            const size_t o = (size_t)i * 8u;
            if (vec16) {
                const u32x4 g = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(pg + o);
                const u32x4 b = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(pb + o);
                const u32x4 r = *reinterpret_cast<const H2Y_GLOBAL u32x4 *>(pr + o);
                const uint32_t gw[4] = {g.x, g.y, g.z, g.w}, bw[4] = {b.x, b.y, b.z, b.w}, rw[4] = {r.x, r.y, r.z, r.w};
                uint32_t w[12]; /* pixels 2k, 2k+1: R G | B R | G B */
                for (int k = 0; k < 4; k++) {
                    w[3 * k] = (rw[k] & 0xFFFFu) | gw[k] << 16;
                    w[3 * k + 1] = (bw[k] & 0xFFFFu) | (rw[k] & 0xFFFF0000u);
                    w[3 * k + 2] = gw[k] >> 16 | (bw[k] & 0xFFFF0000u);
                }
                H2Y_GLOBAL u32x4 *dst = reinterpret_cast<H2Y_GLOBAL u32x4 *>(out + 3 * o);
                for (int k = 0; k < 3; k++) dst[k] = u32x4{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
            } else
                for (uint32_t k = 0; k < 8u; k++) {
                    out[3 * (o + k)] = pr[o + k];
                    out[3 * (o + k) + 1] = pg[o + k];
                    out[3 * (o + k) + 2] = pb[o + k];
                }
        } else if (i < groups + tail) {
            const size_t j = (size_t)groups * 8u + (i - groups);
            out[3 * j] = pr[j];
            out[3 * j + 1] = pg[j];
            out[3 * j + 2] = pb[j];
        }
    }
}

uint32_t h2y_tiff_chunks(uint32_t width, uint32_t height) { return ((width + 7u) / 8u * height + 255u) / 256u; }

uint32_t h2y_rgb_chunks(uint32_t npix) { return (npix / 8u + npix % 8u + 255u) / 256u; }

hipError_t h2y_launch_tiff_decode(bool swap, bool clamp, int grid, hipStream_t st, const tiff_geom &g, const payload_frame *frames, int n_frames)
{
    if (swap) {
        if (clamp) hipLaunchKernelGGL((k_tiff_decode<true, true>), dim3(grid), dim3(256), 0, st, g, frames, n_frames);
        else hipLaunchKernelGGL((k_tiff_decode<true, false>), dim3(grid), dim3(256), 0, st, g, frames, n_frames);
    } else {
        if (clamp) hipLaunchKernelGGL((k_tiff_decode<false, true>), dim3(grid), dim3(256), 0, st, g, frames, n_frames);
        else hipLaunchKernelGGL((k_tiff_decode<false, false>), dim3(grid), dim3(256), 0, st, g, frames, n_frames);
    }
    return hipGetLastError();
}

hipError_t h2y_launch_rgb_interleave(int grid, hipStream_t st, uint32_t npix, const rgb_frame *frames, int n_frames)
{
    hipLaunchKernelGGL(k_rgb_interleave, dim3(grid), dim3(256), 0, st, npix, frames, n_frames);
    return hipGetLastError();
}
