/*
 * h2y_yuvp2.hip -- convert()'s Y'u'v' 4:2:0 branch (the reference's convert.cpp:533-800, matrix_coeffs 15 "YUVPrime2"),
 * then write_yuv()'s shift and range clamp (tiff.cpp:457-550).
 *
 *   k_yuvp2_420<BOX|FIR>  tmp_pic (U16 4:4:4: Y', Z = Cb, X = Cr) -> the .yuv frame (Y, u', v')
 *
 * The fused kernel has written tmp_pic -- matrix_convert()'s output, neither shifted nor range-clamped -- into scratch first
 * (run_frames() in h2y_forward.hip).  What the reference then does, per picture:
 *   - Y: tmp Y' copied (convert.cpp:857-859).
 *   - four planes, each subsampled by Subsample444to420_box or _FIR with tmp_pic's clip (convert.cpp:520: in_pic->clip, the
 *     temporary picture's maxCV, whatever the planes hold): lin(Y'), Z, X and Y'.  lin(c) is
 *     (unsigned short)(RHO_GAMMA_f((float)(c / 65535.0)) * 65535.0) (convert.cpp:587-592), a table of 65 536 entries built
 *     once on the host (h2y_yuvp2_lin_table).  The subsampled Y' only feeds u''v'', which the reference overwrites with
 *     u'v' (its "HACK", convert.cpp:732-734): it has no effect on any output byte and is not computed here.
 *   - per 4:2:0 site, in binary64 and the reference's order: X, Y, Z divided by 65 535 (at every bit depth), sum =
 *     X + 15 Y + 3 Z, u' = 4 X / sum and v' = 9 Y / sum when sum > 0 (else 0), clipped to [0, 1], and
 *     (unsigned short)(u' * 65535.0) as the chroma sample (convert.cpp:674-745).
 * Everything here is integer or IEEE binary32 / binary64 arithmetic in a fixed order (-ffp-contract=off), so the bytes are the
 * reference's.  The FIR is the reference's two stages with their intermediate truncations: fir_h() / fir_v(), the code
 * k_fir420 runs.
 */
#include <hip/hip_runtime.h>

#include "h2y_device.h"
#include "h2y_kernels.h"
#include "h2y_math.h"

using namespace h2y;

namespace {

/* u', v' of one 4:2:0 site from its three subsampled samples, as convert.cpp:674-745 computes and clips them */
__device__ __forceinline__ void yuvp2_uv(uint32_t sx, uint32_t sy, uint32_t sz, uint32_t &u, uint32_t &v)
{
    const double X = (double)sx / 65535.0;
    const double Z = (double)sz / 65535.0;
    const double Y = (double)sy / 65535.0;
    const double sum = (X + 15.0 * Y + 3.0 * Z);
    double up = 0.0, vp = 0.0;
    if (sum > 0.0) {
        up = 4.0 * X / sum;
        vp = 9.0 * Y / sum;
    }
    up = up < 0.0 ? 0.0 : up;
    vp = vp < 0.0 ? 0.0 : vp;
    up = up > 1.0 ? 1.0 : up;
    vp = vp > 1.0 ? 1.0 : vp;
    u = (uint32_t)(up * 65535.0);
    v = (uint32_t)(vp * 65535.0);
}

/* The box (convert.cpp:91-172: the truncating mean of every 2x2 block, no clip).  One thread = two sites: four columns of
 * two picture rows of each plane (8-byte accesses; the box needs width % 4 == 0).  Grid: x over a frame's site pairs,
 * y over the frames. */
__device__ __forceinline__ void yuvp2_box(const yuvp2_args &a)
{
    const uint32_t W = (uint32_t)a.width, H = (uint32_t)a.height, wq = W >> 2, pairs = wq * (H >> 1);
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= pairs) return;
    const frame_io io = uniform_io(a.frames + blockIdx.y);
    const uint32_t npix = W * H, rp = p / wq, cq = p - rp * wq;
    const uint32_t q0 = 2u * rp * wq + cq, q1 = q0 + wq; /* quads of the two rows */
    const uint16_t *Yp = io.out, *Zp = io.out + npix, *Xp = io.out + 2 * (size_t)npix;
    const u32x2 y0 = gload<u32x2>(Yp, q0), y1 = gload<u32x2>(Yp, q1);
    const u32x2 z0 = gload<u32x2>(Zp, q0), z1 = gload<u32x2>(Zp, q1);
    const u32x2 x0 = gload<u32x2>(Xp, q0), x1 = gload<u32x2>(Xp, q1);
    uint32_t u[2], v[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const uint32_t ya = s ? y0.y : y0.x, yb = s ? y1.y : y1.x; /* the site's two columns of either row */
        const uint32_t za = s ? z0.y : z0.x, zb = s ? z1.y : z1.x;
        const uint32_t xa = s ? x0.y : x0.x, xb = s ? x1.y : x1.x;
        const uint32_t ly = (uint32_t)a.lin[ya & 0xFFFFu] + a.lin[ya >> 16] + a.lin[yb & 0xFFFFu] + a.lin[yb >> 16];
        const uint32_t sz = (za & 0xFFFFu) + (za >> 16) + (zb & 0xFFFFu) + (zb >> 16);
        const uint32_t sx = (xa & 0xFFFFu) + (xa >> 16) + (xb & 0xFFFFu) + (xb >> 16);
        uint32_t uu, vv;
        yuvp2_uv(sx >> 2, ly >> 2, sz >> 2, uu, vv);
        u[s] = pix_yuv_clamp(a.pp, uu, true);
        v[s] = pix_yuv_clamp(a.pp, vv, true);
    }
    uint16_t *out = io.yuv;
    auto luma = [&](uint32_t w) { return pix_yuv_clamp(a.pp, w & 0xFFFFu, false) | (pix_yuv_clamp(a.pp, w >> 16, false) << 16); };
    gstore<u32x2>(out, q0, u32x2{luma(y0.x), luma(y0.y)});
    gstore<u32x2>(out, q1, u32x2{luma(y1.x), luma(y1.y)});
    /* the two sites are dword p of either chroma plane (rp * W / 2 + 2 cq = 2 p) */
    const uint32_t ncb = (W >> 1) * (H >> 1);
    gstore<uint32_t>(out + npix, p, u[0] | (u[1] << 16));
    gstore<uint32_t>(out + npix + ncb, p, v[0] | (v[1] << 16));
}

/* The FIR (convert.cpp:261-383).  Block = an output tile of YF_TW x YF_TH sites of one frame (blockIdx.z):
 *   1. stage picture rows 2 r0 - 5 .. 2 r0 + 2 YF_TH + 4 and columns 2 c0 - 5 .. 2 c0 + 2 YF_TW + 4 of lin(Y'), Z and X in
 *      LDS, indices clamped to the picture (the reference's border logic, convert.cpp:295-300 and :337-347); the tile's own
 *      Y' samples go to the output's Y plane on the way
 *   2. horizontal 7-tap at the even columns -> u16 4:2:2 rows (fir_h: clamped and truncated as dst422 stores them)
 *   3. vertical 12-tap -> the site's three samples (fir_v), u', v', write_yuv's shift and clamp */
#define YF_TW 32
#define YF_TH 16
#define YF_ROWS (2 * YF_TH + 10)
#define YF_COLS (2 * YF_TW + 10)
__device__ __forceinline__ void yuvp2_fir(const yuvp2_args &a)
{
    __shared__ uint16_t s444[3][YF_ROWS][YF_COLS]; /* lin(Y'), Z, X */
    __shared__ uint16_t s422[3][YF_ROWS][YF_TW];
    const int W = a.width, H = a.height, wc = W >> 1, hc = H >> 1;
    const frame_io io = uniform_io(a.frames + blockIdx.z);
    const size_t npix = (size_t)W * H;
    const uint16_t *Yp = io.out, *Zp = io.out + npix, *Xp = io.out + 2 * npix;
    uint16_t *out = io.yuv;
    const int c0 = blockIdx.x * YF_TW, r0 = blockIdx.y * YF_TH;
    const int ys = 2 * r0 - 5, xs = 2 * c0 - 5;

    /* 1. */
    for (int i = threadIdx.x; i < YF_ROWS * YF_COLS; i += 256) {
        const int r = i / YF_COLS, c = i - r * YF_COLS;
        const int yy = ys + r, xx = xs + c;
        const size_t at = (size_t)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1);
        const uint32_t yp = Yp[at];
        s444[0][r][c] = a.lin[yp];
        s444[1][r][c] = Zp[at];
        s444[2][r][c] = Xp[at];
        if (r >= 5 && r < 5 + 2 * YF_TH && c >= 5 && c < 5 + 2 * YF_TW && yy < H && xx < W) /* the tile's own samples */
            out[at] = (uint16_t)pix_yuv_clamp(a.pp, yp, false);
    }
    __syncthreads();

    /* 2. site column k sits at local column 2 k + 5 */
    for (int i = threadIdx.x; i < 3 * YF_ROWS * YF_TW; i += 256) {
        const int pl = i / (YF_ROWS * YF_TW), rem = i - pl * (YF_ROWS * YF_TW), r = rem / YF_TW, k = rem - r * YF_TW;
        const uint16_t *s = &s444[pl][r][2 * k + 5];
        s422[pl][r][k] = (uint16_t)fir_h((float)s[-5], (float)s[-3], (float)s[-1], (float)s[0], (float)s[1], (float)s[3], (float)s[5], a.fir_max);
    }
    __syncthreads();

    /* 3. site row rr takes the 4:2:2 rows 2 rr .. 2 rr + 11 (picture rows 2 yo - 5 .. 2 yo + 6) */
    for (int i = threadIdx.x; i < YF_TH * YF_TW; i += 256) {
        const int rr = i / YF_TW, k = i - rr * YF_TW;
        const int yo = r0 + rr, xo = c0 + k;
        if (yo >= hc || xo >= wc) continue;
        uint32_t v3[3];
#pragma unroll
        for (int pl = 0; pl < 3; pl++) {
            float t[12];
#pragma unroll
            for (int j = 0; j < 12; j++) t[j] = (float)s422[pl][2 * rr + j][k];
            v3[pl] = fir_v(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], t[9], t[10], t[11], a.fir_max);
        }
        uint32_t uu, vv;
        yuvp2_uv(v3[2], v3[0], v3[1], uu, vv);
        const size_t at = (size_t)yo * wc + xo;
        out[npix + at] = (uint16_t)pix_yuv_clamp(a.pp, uu, true);
        out[npix + (size_t)wc * hc + at] = (uint16_t)pix_yuv_clamp(a.pp, vv, true);
    }
}

} // namespace

template <bool FIR> __global__ __launch_bounds__(256) void k_yuvp2_420(yuvp2_args a)
{
    if (FIR) yuvp2_fir(a);
    else yuvp2_box(a);
}

hipError_t h2y_launch_yuvp2_420(bool fir, hipStream_t st, const yuvp2_args &a)
{
    const uint32_t wc = (uint32_t)a.width >> 1, hc = (uint32_t)a.height >> 1;
    if (fir) {
        dim3 grid((wc + YF_TW - 1) / YF_TW, (hc + YF_TH - 1) / YF_TH, (uint32_t)a.n_frames);
        hipLaunchKernelGGL(k_yuvp2_420<true>, grid, dim3(256), 0, st, a);
    } else {
        const uint32_t pairs = ((uint32_t)a.width >> 2) * hc;
        hipLaunchKernelGGL(k_yuvp2_420<false>, dim3((pairs + 255) / 256, (uint32_t)a.n_frames), dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

/* convert.cpp:586-592 for every u16 code: (float)(c / 65535.0), RHO_GAMMA_f in binary32 (tf_to_linear: glibc's powf restated,
 * then the outer pow in binary64), times 65535.0 in binary64, truncated.  RHO_GAMMA_f maps [0, 1] into [0, 1]. */
void h2y_yuvp2_lin_table(uint16_t *lin)
{
    for (uint32_t c = 0; c < 65536u; c++) {
        const float V = (float)((double)c / 65535.0);
        const float L = tf_to_linear(H2Y_TF_RHO_GAMMA, V);
        lin[c] = (uint16_t)((double)L * 65535.0);
    }
}
