/*
 * h2y_siting.hip -- 4:4:4 -> 4:2:0 with the chroma co-sited with the top-left luma sample of every 2x2 block
 * (chroma_sample_loc_type 2: HDR10, UHD Blu-ray), then write_yuv()'s shift and range clamp.
 *
 *   k_fir420_tl   one plane of 4:4:4 codes (matrix_convert's output in scratch) -> one 4:2:0 plane of the .yuv frame
 *
 * The reference carries chroma_sample_loc_type through pic_t and never acts on it, so there are no bytes of its to match: the
 * definition is this project's (include/hdr2yuv_hip.h, "Chroma siting"), built from the reference's own filter:
 *   1. horizontal: Subsample444to420_FIR's stage 1 unchanged -- fir_h() at every row and every even column, co-sited already,
 *      clamped to [0, maxCV] and truncated to the u16 4:2:2 intermediate (convert.cpp:305-317), bit for bit the reference's;
 *   2. vertical: the same seven taps down the column at every EVEN row, in exact integers:
 *        S = 21 (M[j-5] + M[j+5]) - 52 (M[j-3] + M[j+3]) + 159 (M[j-1] + M[j+1]) + 256 M[j],  V = med3((S + 256) >> 9, 0, maxCV)
 *      with row indices clamped into the picture.  |S| <= 616 x 65535 < 2^26.  (The reference's stage 2 is an even 12-tap filter
 *      half a row lower: centre sited.)  Up to 14-bit codes this is fir_h() down the column (h2y_math.h, above fir_h_int); in
 *      integers the result depends on no order of summation at 16-bit codes either;
 *   3. write_yuv's shift and per-plane range clamp (pix_yuv_clamp), as k_fir420 applies it.
 * k_fir420's structure (h2y_kernels.hip): a block is a 64 x 32 chroma tile of one plane of one frame, the 4:4:4 tile staged into
 * LDS (16-byte loads where the tile is interior and aligned), stage 1 into a u16 4:2:2 tile in LDS, stage 2 from there.  The
 * vertical halo is rows 2 r0 - 5 .. 2 r0 + 2 TH + 3: one row fewer than the 12-tap stage needs.
 */
#include <hip/hip_runtime.h>

#include "h2y_device.h"
#include "h2y_kernels.h"
#include "h2y_math.h"

using namespace h2y;

namespace {

constexpr int TL_TW = 64, TL_TH = 32;     /* the output tile, chroma samples */
constexpr int TL_ROWS = 2 * TL_TH + 9;    /* staged rows 2*r0-5 .. 2*r0+2*TL_TH+3 */
constexpr int TL_LCOLS = 2 * TL_TW + 16;  /* staged columns: 8 left of the tile (16-byte aligned), 8 right */

} // namespace

__global__ __launch_bounds__(256) void k_fir420_tl(fir_args a)
{
    /* 4:4:4 source rows 2*r0-5 .. 2*r0+67, columns 2*c0-8 .. 2*c0+135 (16-byte aligned start) */
    __shared__ __attribute__((aligned(16))) uint16_t s444[TL_ROWS][TL_LCOLS];
    __shared__ __attribute__((aligned(16))) uint16_t s422[TL_ROWS][TL_TW];
    const int W = a.width, H = a.height, wc = W >> 1, hc = H >> 1;
    const uint16_t *src;
    uint16_t *dst;
    if (a.frames) { /* batch form: blockIdx.z = 2*frame + plane */
        const frame_io io = a.frames[blockIdx.z >> 1];
        uint16_t *cb = io.out + (size_t)W * H;
        src = (blockIdx.z & 1) ? io.tmp_cr : io.tmp_cb;
        dst = (blockIdx.z & 1) ? cb + (size_t)wc * hc : cb;
    } else {
        src = blockIdx.z == 0 ? a.src_cb : a.src_cr;
        dst = blockIdx.z == 0 ? a.dst_cb : a.dst_cr;
    }
    const int c0 = blockIdx.x * TL_TW, r0 = blockIdx.y * TL_TH;
    const int ys = 2 * r0 - 5, xs = 2 * c0 - 8;

    /* 1. stage the source tile; rows and columns outside the picture replicate the edge (the reference's clamped indices,
     *    convert.cpp:295-300; the rows the same way) */
    const bool interior = xs >= 0 && xs + TL_LCOLS <= W && (W & 7) == 0 && ((uintptr_t)src & 15) == 0;
    if (interior) {
        /* all of a thread's loads are issued before the first is stored to LDS */
        constexpr int N16 = TL_ROWS * (TL_LCOLS / 8), ROUNDS = (N16 + 255) / 256;
        typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
        u32x4v q[ROUNDS];
#pragma unroll
        for (int k = 0; k < ROUNDS; k++) {
            const int i = min((int)threadIdx.x + 256 * k, N16 - 1);
            const int r = i / (TL_LCOLS / 8), c8 = i - r * (TL_LCOLS / 8);
            const int y = min(max(ys + r, 0), H - 1);
            q[k] = gload<u32x4v>(src, (size_t)(((size_t)y * W + xs + c8 * 8) >> 3));
        }
#pragma unroll
        for (int k = 0; k < ROUNDS; k++) {
            const int i = (int)threadIdx.x + 256 * k;
            if (i < N16) {
                const int r = i / (TL_LCOLS / 8), c8 = i - r * (TL_LCOLS / 8);
                *reinterpret_cast<u32x4v *>(&s444[r][c8 * 8]) = q[k];
            }
        }
    } else {
        for (int i = threadIdx.x; i < TL_ROWS * TL_LCOLS; i += 256) {
            const int r = i / TL_LCOLS, c = i - r * TL_LCOLS;
            const int y = min(max(ys + r, 0), H - 1), x = min(max(xs + c, 0), W - 1);
            s444[r][c] = src[(size_t)y * W + x];
        }
    }
    __syncthreads();

    /* 2. horizontal 7-tap at the even columns -> u16 4:2:2 tile (clamped and truncated exactly as the reference stores dst422,
     *    convert.cpp:314-317).  One item = one row x 8 outputs: 32 source samples from four 16-byte LDS reads. */
    for (int i = threadIdx.x; i < TL_ROWS * (TL_TW / 8); i += 256) {
        const int r = i / (TL_TW / 8), g = i - r * (TL_TW / 8);
        uint32_t w[16];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 t = *reinterpret_cast<const uint4 *>(&s444[r][16 * g + 8 * q]);
            w[4 * q] = t.x; w[4 * q + 1] = t.y; w[4 * q + 2] = t.z; w[4 * q + 3] = t.w;
        }
        float s[32];
#pragma unroll
        for (int q = 0; q < 16; q++) {
            s[2 * q] = (float)(w[q] & 0xFFFFu);
            s[2 * q + 1] = (float)(w[q] >> 16);
        }
        uint32_t o[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int ctr = 8 + 2 * j; /* local index of the even column 2*(c0 + 8g + j) */
            o[j] = fir_h(s[ctr - 5], s[ctr - 3], s[ctr - 1], s[ctr], s[ctr + 1], s[ctr + 3], s[ctr + 5], a.fir_max);
        }
        *reinterpret_cast<uint4 *>(&s422[r][8 * g]) =
            make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
    }
    __syncthreads();

    /* 3. vertical 7-tap at the even rows in integers (4:2:2 rows 2r-5, -3, -1, 0, +1, +3, +5 of output row r: local rows
     *    2r + 0, 2, 4, 5, 6, 8, 10), then write_yuv's shift + range clamp.  One item = one output row x 4 outputs. */
    const int32_t maxcv = (int32_t)a.fir_max;
    for (int i = threadIdx.x; i < TL_TH * (TL_TW / 4); i += 256) {
        const int r = i / (TL_TW / 4), g = i - r * (TL_TW / 4);
        const int yo = r0 + r, xo = c0 + 4 * g;
        if (yo >= hc || xo >= wc) continue;
        constexpr int kRow[7] = {0, 2, 4, 5, 6, 8, 10};
        int32_t t[7][4];
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const uint2 q = *reinterpret_cast<const uint2 *>(&s422[2 * r + kRow[k]][4 * g]);
            t[k][0] = (int32_t)(q.x & 0xFFFFu); t[k][1] = (int32_t)(q.x >> 16);
            t[k][2] = (int32_t)(q.y & 0xFFFFu); t[k][3] = (int32_t)(q.y >> 16);
        }
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            uint32_t v = fir_h_int(t[0][j], t[1][j], t[2][j], t[3][j], t[4][j], t[5][j], t[6][j], maxcv);
            if (a.apply_yuv_clamp) v = pix_yuv_clamp(a.pp, v, true);
            o[j] = v;
        }
        uint16_t *d = dst + (size_t)yo * wc + xo;
        if (xo + 3 < wc && (((uintptr_t)d) & 7) == 0) *reinterpret_cast<uint2 *>(d) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
        else
            for (int j = 0; j < 4 && xo + j < wc; j++) d[j] = (uint16_t)o[j];
    }
}

hipError_t h2y_launch_fir420_tl(hipStream_t st, const fir_args &a)
{
    const int wc = a.width >> 1, hc = a.height >> 1;
    dim3 grid((wc + TL_TW - 1) / TL_TW, (hc + TL_TH - 1) / TL_TH, a.frames ? 2 * a.n_frames : (a.src_cr ? 2 : 1));
    hipLaunchKernelGGL(k_fir420_tl, grid, dim3(256), 0, st, a);
    return hipGetLastError();
}
