/*
 * h2y_pack.hip -- the sample packings of include/hdr2yuv_hip.h ("sample packings"), on the device.
 *
 *   k_pack<PACKING>    (frame, job, chunk) units of frames of three u16 planes -> the frames packed as PLANAR8, NV12 or P010
 *   k_unpack<PACKING>  the reverse
 *                      (h2y_pack_batch / h2y_unpack_batch, the pack stage of an armed ring)
 *
 * Pure streaming passes: every sample is read once and written once, 3 bytes a sample for the byte packings and 4 for P010; only
 * the frame table is read twice.  A frame is a few jobs (pack_job, h2y_kernels.h): a plane that becomes bytes or words, or the two
 * chroma planes that become one block of (P1, P2) pairs.  A job is walked in groups, k_dither's way: group g holds the job's indices
 * G g - sh .. G g - sh + G - 1, with G = 16 samples for a plane that becomes bytes and 8 samples or pairs otherwise, and sh chosen by
 * the host (h2y_pack_args) so that a whole group starts on a 16-byte boundary on one side.  Where that also puts the group on
 * a 16-byte boundary of the other side (and of the second chroma plane), the job is a vector job: every whole group is 16-byte
 * nontemporal loads and 16-byte stores, and the interleaved chroma is put together in registers from one vector of P1 and one of P2.
 * No access is wider than the alignment of its address: the groups cut by a job's ends, and every group of a job that does not
 * qualify (a chroma block behind a luma plane of w h samples with w h not a multiple of 16, say), take accesses of one element of
 * their own samples only; such a job's indices are dealt across the block's lanes, so that a wave's one-element accesses lie side
 * by side.  Frame bases are 16-byte aligned (the entries refuse others).  A thread never touches a byte outside its frame.  No
 * atomics, no LDS.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_math.h"
#include "h2y_device.h"
#include "h2y_pack1.h"

namespace {

constexpr uint32_t kThreads = 256u, kGroupsPerThread = 4u, kGroupsPerUnit = kThreads * kGroupsPerThread;

enum { PLANE8, PLANE16, PAIR8, PAIR16 }; /* what a job is: a plane to bytes, a plane to words, chroma pairs to bytes, to words */

template <int KIND> constexpr uint32_t group_of() { return KIND == PLANE8 ? 16u : 8u; }

__device__ __forceinline__ uint32_t lo16(uint32_t x) { return x & 0xFFFFu; }
__device__ __forceinline__ uint32_t hi16(uint32_t x) { return x >> 16; }

/* ---- whole groups of a vector job: the raw vectors of group i0 (i0 + the job's planar offset is a multiple of the group) ---- */

template <int KIND, bool UNPACK>
__device__ __forceinline__ void load_group(const void *planar, const void *packed, const pack_job &J, uint32_t i0, u32x4 (&r)[2])
{
    if (!UNPACK) {
        const uint32_t q = (J.pl + i0) >> 3;
        r[0] = gload_nt<u32x4>(planar, q);
        if (KIND == PLANE8) r[1] = gload_nt<u32x4>(planar, q + 1u);
        else if (KIND == PAIR8 || KIND == PAIR16) r[1] = gload_nt<u32x4>(planar, (J.pl2 + i0) >> 3);
    } else if (KIND == PLANE8) r[0] = gload_nt<u32x4>(packed, (J.pk + i0) >> 4);
    else if (KIND == PLANE16) r[0] = gload_nt<u32x4>(packed, (J.pk + i0) >> 3);
    else if (KIND == PAIR8) r[0] = gload_nt<u32x4>(packed, (J.pk + 2u * i0) >> 4);
    else {
        const uint32_t q = (J.pk + 2u * i0) >> 3;
        r[0] = gload_nt<u32x4>(packed, q);
        r[1] = gload_nt<u32x4>(packed, q + 1u);
    }
}

template <int KIND, bool UNPACK>
__device__ __forceinline__ void store_group(void *planar, void *packed, const pack_job &J, uint32_t i0, const u32x4 (&r)[2], uint32_t M,
                                            uint32_t s)
{
    if (!UNPACK) {
        if (KIND == PLANE8) { /* sixteen codes in eight words -> sixteen bytes */
            u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t a = r[k >> 1][2 * (k & 1)], b = r[k >> 1][2 * (k & 1) + 1];
                o[k] = pack_code(lo16(a), M, 0u) | pack_code(hi16(a), M, 0u) << 8 | pack_code(lo16(b), M, 0u) << 16 | pack_code(hi16(b), M, 0u) << 24;
            }
            gstore<u32x4>(packed, (J.pk + i0) >> 4, o);
        } else if (KIND == PLANE16) {
            u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = pack_code(lo16(r[0][k]), M, s) | pack_code(hi16(r[0][k]), M, s) << 16;
            gstore<u32x4>(packed, (J.pk + i0) >> 3, o);
        } else if (KIND == PAIR8) { /* eight P1 codes and eight P2 codes -> eight (P1, P2) byte pairs */
            u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t a = r[0][k], b = r[1][k];
                o[k] = pack_code(lo16(a), M, 0u) | pack_code(lo16(b), M, 0u) << 8 | pack_code(hi16(a), M, 0u) << 16 | pack_code(hi16(b), M, 0u) << 24;
            }
            gstore<u32x4>(packed, (J.pk + 2u * i0) >> 4, o);
        } else { /* -> eight (P1, P2) word pairs */
            u32x4 o[2];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t a = r[0][k], b = r[1][k];
                o[k >> 1][2 * (k & 1)] = pack_code(lo16(a), M, s) | pack_code(lo16(b), M, s) << 16;
                o[k >> 1][2 * (k & 1) + 1] = pack_code(hi16(a), M, s) | pack_code(hi16(b), M, s) << 16;
            }
            const uint32_t q = (J.pk + 2u * i0) >> 3;
            gstore<u32x4>(packed, q, o[0]);
            gstore<u32x4>(packed, q + 1u, o[1]);
        }
    } else {
        if (KIND == PLANE8) { /* sixteen bytes -> sixteen codes in eight words */
            u32x4 o[2];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t x = r[0][k];
                o[k >> 1][2 * (k & 1)] = (x & 0xFFu) | (x & 0xFF00u) << 8;
                o[k >> 1][2 * (k & 1) + 1] = ((x >> 16) & 0xFFu) | (x >> 24) << 16;
            }
            const uint32_t q = (J.pl + i0) >> 3;
            gstore<u32x4>(planar, q, o[0]);
            gstore<u32x4>(planar, q + 1u, o[1]);
        } else if (KIND == PLANE16) {
            u32x4 o;
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = unpack_code(lo16(r[0][k]), s) | unpack_code(hi16(r[0][k]), s) << 16;
            gstore<u32x4>(planar, (J.pl + i0) >> 3, o);
        } else if (KIND == PAIR8) {
            u32x4 a, b;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t x = r[0][k];
                a[k] = (x & 0xFFu) | (x & 0xFF0000u);
                b[k] = ((x >> 8) & 0xFFu) | (x >> 24) << 16;
            }
            gstore<u32x4>(planar, (J.pl + i0) >> 3, a);
            gstore<u32x4>(planar, (J.pl2 + i0) >> 3, b);
        } else {
            u32x4 a, b;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t x = r[k >> 1][2 * (k & 1)], y = r[k >> 1][2 * (k & 1) + 1]; /* pairs 2k and 2k + 1 */
                a[k] = unpack_code(lo16(x), s) | unpack_code(lo16(y), s) << 16;
                b[k] = unpack_code(hi16(x), s) | unpack_code(hi16(y), s) << 16;
            }
            gstore<u32x4>(planar, (J.pl + i0) >> 3, a);
            gstore<u32x4>(planar, (J.pl2 + i0) >> 3, b);
        }
    }
}

/* ---- the narrow path: index i (< n) of a job, one element an access ------------------------------------------------------------ */

template <int KIND, bool UNPACK>
__device__ __forceinline__ void narrow_one(void *planar, void *packed, const pack_job &J, uint32_t i, uint32_t M, uint32_t s)
{
    constexpr bool PAIR = KIND == PAIR8 || KIND == PAIR16, BYTES = KIND == PLANE8 || KIND == PAIR8;
    uint16_t *pl = static_cast<uint16_t *>(planar);
    uint8_t *pk8 = static_cast<uint8_t *>(packed);
    uint16_t *pk16 = static_cast<uint16_t *>(packed);
    const uint32_t e = J.pk + (PAIR ? 2u * i : i);
    if (!UNPACK) {
        const uint32_t a = pack_code(pl[J.pl + i], M, s);
        if (BYTES) pk8[e] = (uint8_t)a;
        else pk16[e] = (uint16_t)a;
        if (PAIR) {
            const uint32_t b = pack_code(pl[J.pl2 + i], M, s);
            if (BYTES) pk8[e + 1u] = (uint8_t)b;
            else pk16[e + 1u] = (uint16_t)b;
        }
    } else {
        pl[J.pl + i] = (uint16_t)unpack_code(BYTES ? (uint32_t)pk8[e] : (uint32_t)pk16[e], s);
        if (PAIR) pl[J.pl2 + i] = (uint16_t)unpack_code(BYTES ? (uint32_t)pk8[e + 1u] : (uint32_t)pk16[e + 1u], s);
    }
}

/* a group cut by a vector job's ends: its own elements i0 .. i0 + G - 1 that lie in [0, n) */
template <int KIND, bool UNPACK>
__device__ __forceinline__ void narrow_group(void *planar, void *packed, const pack_job &J, int32_t i0, uint32_t M, uint32_t s)
{
#pragma unroll
    for (int j = 0; j < (int)group_of<KIND>(); j++) {
        const int32_t i = i0 + j;
        if (i >= 0 && (uint32_t)i < J.n) narrow_one<KIND, UNPACK>(planar, packed, J, (uint32_t)i, M, s);
    }
}

/* one unit of a job: a unit of a vector job whose groups are all whole asks for all its vectors before it writes any */
template <int KIND, bool UNPACK>
__device__ __forceinline__ void unit(void *planar, void *packed, const pack_job &J, uint32_t chunk, uint32_t M, uint32_t s)
{
    constexpr uint32_t G = group_of<KIND>();
    const uint32_t tid = threadIdx.x, n = J.n, sh = J.sh, groups = (n + sh + G - 1u) / G, g0 = chunk * kGroupsPerUnit;
    if (!J.vec) { /* no group of the job qualifies: the unit's indices are dealt across the block, so a wave's accesses lie side by side */
        const uint32_t first = g0 * G > sh ? g0 * G - sh : 0u, end = (g0 + kGroupsPerUnit) * G - sh, last = end < n ? end : n;
        for (uint32_t i = first + tid; i < last; i += kThreads) narrow_one<KIND, UNPACK>(planar, packed, J, i, M, s);
        return;
    }
    if (J.vec && g0 * G >= sh && (g0 + kGroupsPerUnit) * G - sh <= n) {
        u32x4 r[kGroupsPerThread][2];
#pragma unroll
        for (uint32_t k = 0; k < kGroupsPerThread; k++) load_group<KIND, UNPACK>(planar, packed, J, (g0 + k * kThreads + tid) * G - sh, r[k]);
#pragma unroll
        for (uint32_t k = 0; k < kGroupsPerThread; k++) store_group<KIND, UNPACK>(planar, packed, J, (g0 + k * kThreads + tid) * G - sh, r[k], M, s);
        return;
    }
    for (uint32_t k = 0; k < kGroupsPerThread; k++) {
        const uint32_t gi = g0 + k * kThreads + tid;
        if (gi >= groups) break;
        const int32_t i0 = (int32_t)(gi * G) - (int32_t)sh;
        if (J.vec && i0 >= 0 && (uint32_t)i0 + G <= n) {
            u32x4 r[2];
            load_group<KIND, UNPACK>(planar, packed, J, (uint32_t)i0, r);
            store_group<KIND, UNPACK>(planar, packed, J, (uint32_t)i0, r, M, s);
        } else narrow_group<KIND, UNPACK>(planar, packed, J, i0, M, s);
    }
}

/* Grid-stride over (frame, job, chunk of kGroupsPerUnit groups) units; the frame and the job are block-uniform */
template <int PACKING, bool UNPACK>
__device__ __forceinline__ void walk(const pack_args &a, const pack_frame *__restrict__ frames, int n_frames)
{
    const uint32_t per_frame = a.j[0].chunks + a.j[1].chunks + a.j[2].chunks, units = (uint32_t)n_frames * per_frame;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
        const uint32_t f = u / per_frame, r = u - f * per_frame;
        const uint32_t p = r < a.j[0].chunks ? 0u : r < a.j[0].chunks + a.j[1].chunks ? 1u : 2u;
        const uint32_t chunk = r - (p > 0u ? a.j[0].chunks : 0u) - (p > 1u ? a.j[1].chunks : 0u);
        pack_job J = a.j[0];
        if (p == 1u) J = a.j[1];
        if (p == 2u) J = a.j[2];
        const pack_frame fr = frames[f];
        void *planar = uniform_ptr(const_cast<void *>(fr.planar)), *packed = uniform_ptr(const_cast<void *>(fr.packed));
        if (PACKING == H2Y_PACK_PLANAR8 || (PACKING == H2Y_PACK_NV12 && p == 0u)) unit<PLANE8, UNPACK>(planar, packed, J, chunk, a.maxv, a.shift);
        else if (PACKING == H2Y_PACK_NV12) unit<PAIR8, UNPACK>(planar, packed, J, chunk, a.maxv, a.shift);
        else if (p == 0u) unit<PLANE16, UNPACK>(planar, packed, J, chunk, a.maxv, a.shift);
        else unit<PAIR16, UNPACK>(planar, packed, J, chunk, a.maxv, a.shift);
    }
}

} // namespace

template <int PACKING>
__global__ __launch_bounds__(256) void k_pack(pack_args a, const pack_frame *__restrict__ frames, int n_frames)
{
    walk<PACKING, false>(a, frames, n_frames);
}

template <int PACKING>
__global__ __launch_bounds__(256) void k_unpack(pack_args a, const pack_frame *__restrict__ frames, int n_frames)
{
    walk<PACKING, true>(a, frames, n_frames);
}

/* A job's groups, units and whether its whole groups may take 16-byte accesses.  Group g starts at index G g - sh.  A plane's sh is
 * its packed start modulo the elements of a 16-byte vector, so that a whole group is one packed vector; it is a vector job where
 * that puts the group on a 16-byte boundary of the planar side too (always, in a frame whose planes lie one after the other: a
 * plane then starts as many samples into the planar frame as elements into the packed one).  A chroma block's sh is P1's start
 * modulo 8 samples; it is a vector job where P2 starts a multiple of 8 samples behind P1 and the group's first pair lies on a
 * 16-byte boundary of the packed side. */
static pack_job job_of(uint32_t n, uint32_t pl, uint32_t pl2, uint32_t pk, bool pair, bool bytes)
{
    pack_job J{};
    const uint32_t G = !pair && bytes ? 16u : 8u, pk_mask = bytes ? 15u : 7u;
    J.n = n, J.pl = pl, J.pl2 = pl2, J.pk = pk;
    if (!pair) {
        J.sh = pk & (G - 1u);
        J.vec = ((pl + G - J.sh) & 7u) == 0u;
    } else {
        J.sh = pl & 7u;
        J.vec = ((pl2 - pl) & 7u) == 0u && ((pk + 2u * (8u - J.sh)) & pk_mask) == 0u;
    }
    J.chunks = n ? ((n + J.sh + G - 1u) / G + kGroupsPerUnit - 1u) / kGroupsPerUnit : 0u;
    return J;
}

pack_args h2y_pack_args(uint32_t w, uint32_t h, int chroma, int bit_depth, int packing, const uint32_t off[3])
{
    pack_args a{};
    const uint32_t n = w * h, nc = pack_cw(w, chroma) * pack_ch(h, chroma);
    if (packing == H2Y_PACK_PLANAR8) {
        a.j[0] = job_of(n, off[0], 0u, 0u, false, true);
        a.j[1] = job_of(nc, off[1], 0u, n, false, true);
        a.j[2] = job_of(nc, off[2], 0u, n + nc, false, true);
    } else {
        const bool bytes = packing == H2Y_PACK_NV12;
        a.j[0] = job_of(n, off[0], 0u, 0u, false, bytes);
        a.j[1] = job_of(nc, off[1], off[2], n, true, bytes);
    }
    a.maxv = (1u << bit_depth) - 1u;
    a.shift = packing == H2Y_PACK_P010 ? 16u - (uint32_t)bit_depth : 0u;
    return a;
}

hipError_t h2y_launch_pack(int packing, bool unpack, int grid, hipStream_t st, const pack_args &a, const pack_frame *frames, int n_frames)
{
#define H2Y_PACK_LAUNCH(P)                                                                                        \
    if (packing == P) {                                                                                           \
        if (unpack) hipLaunchKernelGGL((k_unpack<P>), dim3(grid), dim3(256), 0, st, a, frames, n_frames);         \
        else hipLaunchKernelGGL((k_pack<P>), dim3(grid), dim3(256), 0, st, a, frames, n_frames);                  \
        return hipGetLastError();                                                                                 \
    }
    H2Y_PACK_LAUNCH(H2Y_PACK_PLANAR8)
    H2Y_PACK_LAUNCH(H2Y_PACK_NV12)
    H2Y_PACK_LAUNCH(H2Y_PACK_P010)
#undef H2Y_PACK_LAUNCH
    return hipErrorInvalidValue;
}
