/*
 * h2y_scenesig.hip -- the scene signature of a frame (include/hdr2yuv_hip.h, "scene signature and scene cuts"): the frame divided
 * into H2Y_SCENESIG_COLS x H2Y_SCENESIG_ROWS cells, per cell the sum over its pixels of b = bin_of(bits(m)), the logarithmic bin of
 * m = max(L_G, L_B, L_R) that k_lightdist and k_codelight count.  The per-pixel light is theirs, word for word: light1 and dist_keep
 * (h2y_light1.h) on the forward flow's decoded planes, code_lights (h2y_codepixel.h) on PQ code planes; this file is built
 * -ffp-contract=off as theirs are.
 *
 *   k_scenesig<IN, TFN>     (band, frame) blocks on three planes of F32 / F16 / U16 samples, groups of 4 pixels (in_traits' loaders)
 *   k_codescenesig<MATRIX>  the same on three u16 code planes, groups of 8 pixels (load8; 4:2:0 chroma arrives upsampled by k_up444)
 *
 * A block takes a band of whole rows of one frame.  The planes are read in the aligned groups of the plane, not of the row: row y
 * starts at pixel y x W, which lies `phase` pixels into a group, so thread t's k-th group of the row holds x = G k - phase .. + G - 1,
 * of which those in [0, W) are the row's (a group that straddles a row end is read once for either row, each time for that row's
 * pixels alone; the frame's last, incomplete group is read sample by sample).  A wave reads 64 consecutive groups of a row: whole
 * cache lines.  A thread keeps its k and walks down the band's rows, so its x moves by less than a group and its cell changes a few
 * times per band at the most: it sums b in a register for the cell it is in and adds the sum to the block's 144 cells in LDS when
 * the cell changes.  At the end the block adds its non-zero cells to the frame's with one 64-bit atomic each.
 *
 * No division per pixel: a thread finds the cell column of the smallest x it can meet once per k, a cell's end is
 * ceil(c W / 16) (x 16 / W >= c exactly when x >= ceil(c W / 16)), and the pixels step over the ends.  Every product stays below
 * 2^32: W x H < 2^28.
 *
 * Every figure is an integer sum: exact whatever the order of the atomics.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hdr2yuv_hip.h"
#include "h2y_kernels.h"
#include "h2y_math.h"
#include "h2y_device.h"
#include "h2y_light1.h"
#include "h2y_codepixel.h"

namespace {

constexpr uint32_t kThreads = 256u;
constexpr uint32_t kCols = H2Y_SCENESIG_COLS, kRows = H2Y_SCENESIG_ROWS, kCells = kCols * kRows;
constexpr uint32_t kGroupsPerThread = 64u; /* groups a thread of a many-frame launch aims at: the flush of the cells is paid per block */
constexpr uint32_t kMinBlocks = 2048u;     /* a launch of few frames takes lower bands to get so many blocks, down to two rows */

/* the first x of cell column c, and the first y of cell row c */
__device__ __forceinline__ uint32_t col_begin(uint32_t c, uint32_t w) { return (c * w + (kCols - 1u)) / kCols; }
__device__ __forceinline__ uint32_t row_begin(uint32_t c, uint32_t h) { return (c * h + (kRows - 1u)) / kRows; }

/* The band of block blockIdx.x into out[kCells].  bins(q, lo, hi, bn): the bins of pixels lo <= j < hi of the plane's group q
 * (bn[j] of the others may hold anything). */
template <uint32_t G, typename BINS>
__device__ __forceinline__ void sig_band(const scenesig_geom &g, unsigned long long *s_cell, unsigned long long *out, BINS bins)
{
    const uint32_t tid = threadIdx.x, W = g.width, H = g.height;
    for (uint32_t w = tid; w < kCells; w += kThreads) s_cell[w] = 0ull;
    __syncthreads();
    const uint32_t r0 = blockIdx.x * g.rows, r1 = r0 + g.rows < H ? r0 + g.rows : H;
    const uint32_t cy0 = r0 * kRows / H;
    uint32_t cur = 0u;
    unsigned long long acc = 0ull;
    for (uint32_t k = tid; G * k < W + (G - 1u); k += kThreads) {
        const uint32_t xmin = G * k >= G - 1u ? G * k - (G - 1u) : 0u; /* the smallest x the thread meets in any row: below W */
        const uint32_t c_lo = xmin * kCols / W, e_lo = col_begin(c_lo + 1u, W);
        uint32_t cy = cy0, ey = row_begin(cy0 + 1u, H);
        for (uint32_t y = r0; y < r1; y++) {
            while (y >= ey) ey = row_begin(++cy + 1u, H); /* y < H = row_begin(kRows): cy stays below kRows */
            const uint32_t start = y * W, phase = start % G;
            if (G * k >= W + phase) continue; /* the group lies behind the row's end */
            const uint32_t lo = G * k < phase ? phase - G * k : 0u;          /* pixels before x = 0 are the row above's */
            const uint32_t x0 = G * k + lo - phase;                          /* x of pixel lo */
            const uint32_t hi = W - x0 < G - lo ? lo + (W - x0) : G;         /* pixels from x = W on are the row below's */
            uint32_t bn[G];
            bins(start / G + k, lo, hi, bn);
            uint32_t c = c_lo, e = e_lo;
#pragma unroll
            for (uint32_t j = 0; j < G; j++) {
                if (j < lo || j >= hi) continue;
                const uint32_t x = x0 + (j - lo);
                while (x >= e) e = col_begin(++c + 1u, W); /* x < W = col_begin(kCols): c stays below kCols */
                const uint32_t cell = cy * kCols + c;
                if (cell != cur) {
                    if (acc) atomicAdd(&s_cell[cur], acc);
                    cur = cell;
                    acc = 0ull;
                }
                acc += bn[j];
            }
        }
    }
    if (acc) atomicAdd(&s_cell[cur], acc);
    __syncthreads();
    for (uint32_t w = tid; w < kCells; w += kThreads) {
        const unsigned long long v = s_cell[w];
        if (v) atomicAdd(&out[w], v);
    }
}

/* one pixel's bin from its three lights: m by dist_keep, whose other figures nobody reads here */
__device__ __forceinline__ uint32_t bin_of_lights(float lg, float lb, float lr)
{
    dist_regs unused{{0u, 0u, 0u}, 0u, 0ull};
    return bin_of(f2bits(dist_keep(lg, lb, lr, unused)));
}

template <int IN_KIND, bool TFN>
__global__ __launch_bounds__(kThreads) void k_scenesig(light_args a, scenesig_geom g, const light_frame *frames, unsigned long long *sig)
{
    typedef in_traits<IN_KIND> IN;
    __shared__ unsigned long long s_cell[kCells];
    const light_frame &fr = frames[blockIdx.y];
    const void *const p0 = uniform_ptr(fr.in[0]), *const p1 = uniform_ptr(fr.in[1]), *const p2 = uniform_ptr(fr.in[2]);
    const pix_params pp = with_assumed(a.pp, fr.assumed);
    const pq_recA *tab = static_cast<const pq_recA *>(a.table);
    auto bin1 = [&](float gv, float bv, float rv) {
        return bin_of_lights(light1<TFN>(pp, tab, 0, gv), light1<TFN>(pp, tab, 1, bv), light1<TFN>(pp, tab, 2, rv));
    };
    sig_band<4u>(g, s_cell, sig + (size_t)blockIdx.y * kCells, [&](uint32_t q, uint32_t lo, uint32_t hi, uint32_t bn[4]) {
        if (q < a.n4) { /* a whole group of the plane: one vector load a plane */
            float gv[4], bv[4], rv[4];
            IN::load4q(p0, q, gv);
            IN::load4q(p1, q, bv);
            IN::load4q(p2, q, rv);
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) bn[j] = bin1(gv[j], bv[j], rv[j]);
        } else { /* the npix % 4 pixels behind the frame's last group */
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++)
                if (j >= lo && j < hi) {
                    const uint32_t i = 4u * q + j;
                    bn[j] = bin1(IN::load1(p0, i), IN::load1(p1, i), IN::load1(p2, i));
                }
        }
    });
}

template <int MATRIX>
__global__ __launch_bounds__(kThreads) void k_codescenesig(codelight_args a, scenesig_geom g, const codelight_frame *frames, unsigned long long *sig)
{
    __shared__ unsigned long long s_cell[kCells];
    const codelight_frame &fr = frames[blockIdx.y];
    const uint16_t *const p0 = uniform_ptr(fr.p[0]), *const p1 = uniform_ptr(fr.p[1]), *const p2 = uniform_ptr(fr.p[2]);
    const pq_recA *tab = static_cast<const pq_recA *>(a.table);
    auto bin1 = [&](uint32_t c0, uint32_t c1, uint32_t c2) {
        float lg, lb, lr;
        code_lights<MATRIX>(a, tab, c0, c1, c2, lg, lb, lr);
        return bin_of_lights(lg, lb, lr);
    };
    sig_band<8u>(g, s_cell, sig + (size_t)blockIdx.y * kCells, [&](uint32_t q, uint32_t lo, uint32_t hi, uint32_t bn[8]) {
        if (q < a.n8) { /* a whole group of the plane: one 16-byte load where the plane starts 16-byte aligned */
            uint32_t c0[8], c1[8], c2[8];
            load8(p0, a.vec & 1u, q, c0);
            load8(p1, a.vec & 2u, q, c1);
            load8(p2, a.vec & 4u, q, c2);
#pragma unroll
            for (uint32_t j = 0; j < 8u; j++) bn[j] = bin1(c0[j], c1[j], c2[j]);
        } else { /* the npix % 8 pixels behind the frame's last group */
#pragma unroll
            for (uint32_t j = 0; j < 8u; j++)
                if (j >= lo && j < hi) {
                    const uint32_t i = 8u * q + j;
                    bn[j] = bin1(gload<uint16_t>(p0, i), gload<uint16_t>(p1, i), gload<uint16_t>(p2, i));
                }
        }
    });
}

template <int IN_KIND>
hipError_t launch_in(hipStream_t st, const light_args &a, const scenesig_geom &g, const light_frame *frames, int n_frames, unsigned long long *sig)
{
    const dim3 grid((g.height + g.rows - 1u) / g.rows, n_frames);
    if (a.table) hipLaunchKernelGGL((k_scenesig<IN_KIND, true>), grid, dim3(kThreads), 0, st, a, g, frames, sig);
    else hipLaunchKernelGGL((k_scenesig<IN_KIND, false>), grid, dim3(kThreads), 0, st, a, g, frames, sig);
    return hipGetLastError();
}

template <int MATRIX>
hipError_t launch_m(hipStream_t st, const codelight_args &a, const scenesig_geom &g, const codelight_frame *frames, int n_frames, unsigned long long *sig)
{
    hipLaunchKernelGGL((k_codescenesig<MATRIX>), dim3((g.height + g.rows - 1u) / g.rows, n_frames), dim3(kThreads), 0, st, a, g, frames, sig);
    return hipGetLastError();
}

} // namespace

scenesig_geom h2y_scenesig_geom(uint32_t width, uint32_t height, uint32_t group, int n_frames)
{
    const uint32_t groups = (width + 2u * (group - 1u)) / group;      /* a row's groups at the most */
    const uint32_t turns = (groups + kThreads - 1u) / kThreads;       /* groups of a row a thread takes */
    uint32_t rows = kGroupsPerThread / turns > 0u ? kGroupsPerThread / turns : 1u;
    const uint64_t n = (uint64_t)(n_frames > 0 ? n_frames : 1);
    while (rows > 2u && (uint64_t)((height + rows - 1u) / rows) * n < kMinBlocks) rows /= 2u;
    return scenesig_geom{width, height, rows};
}

hipError_t h2y_launch_scenesig(int in_kind, hipStream_t st, const light_args &a, const scenesig_geom &g, const light_frame *frames, int n_frames,
                               unsigned long long *sig)
{
    if (in_kind == H2Y_IN_F32) return launch_in<H2Y_IN_F32>(st, a, g, frames, n_frames, sig);
    if (in_kind == H2Y_IN_F16) return launch_in<H2Y_IN_F16>(st, a, g, frames, n_frames, sig);
    return launch_in<H2Y_IN_U16>(st, a, g, frames, n_frames, sig);
}

hipError_t h2y_launch_codescenesig(int matrix, hipStream_t st, const codelight_args &a, const scenesig_geom &g, const codelight_frame *frames,
                                   int n_frames, unsigned long long *sig)
{
    if (matrix == H2Y_MATRIX_BT2020NC) return launch_m<H2Y_MATRIX_BT2020NC>(st, a, g, frames, n_frames, sig);
    if (matrix == H2Y_MATRIX_BT709) return launch_m<H2Y_MATRIX_BT709>(st, a, g, frames, n_frames, sig);
    if (matrix == H2Y_MATRIX_GBR) return launch_m<H2Y_MATRIX_GBR>(st, a, g, frames, n_frames, sig);
    if (matrix == H2Y_MATRIX_ICTCP) return launch_m<H2Y_MATRIX_ICTCP>(st, a, g, frames, n_frames, sig);
    return hipErrorInvalidValue;
}
