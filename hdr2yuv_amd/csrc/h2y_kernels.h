/* h2y_kernels.h -- argument blocks and launch entry points shared by
 * h2y_kernels.hip (device code) and the C-ABI shim (h2y_api.hip, h2y_forward.hip, h2y_ring.hip, h2y_measure.hip). */
#ifndef H2Y_KERNELS_H
#define H2Y_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "h2y_math.h"
#include "h2y_walk.h" /* H2Y_FF_OWN_LANES, h2y_firf_vblock */

#ifndef H2Y_FUSED_THREADS
#define H2Y_FUSED_THREADS 512
#endif
#ifndef H2Y_FUSED_MINWAVES
#define H2Y_FUSED_MINWAVES 4 /* waves per SIMD the fused kernel is register-budgeted for: 2 blocks of 512 per CU */
#endif

/* k_fused2 / k_fused_lut16: one block of 1024 per CU -- all sixteen waves of a CU draw their tiles from one
 * counter (wave_deal); with two blocks of 512 the older block's waves run ahead of the younger's */
#ifndef H2Y_LOOP_THREADS
#define H2Y_LOOP_THREADS 1024
#endif

#define H2Y_LUT16_N 16384 /* halves 0x0000..0x3FFF = [0, 2) */

enum { H2Y_IN_F32 = 0, H2Y_IN_F16 = 1, H2Y_IN_U16 = 2 };
enum { H2Y_OUT_420BOX = 0, H2Y_OUT_444 = 1, H2Y_OUT_444TMP = 2 };

/* one frame's buffers (device pointers) */
struct frame_io {
    const void *in[3]; /* planes G,B,R (convert.cpp:980-982) */
    uint16_t *out;     /* .yuv frame: Y | Cb | Cr (the Y'u'v' 4:2:0 form: the scratch 4:4:4 tmp_pic, Y' | Z | X) */
    union {
        uint16_t *tmp_cb; /* H2Y_OUT_444TMP only: 4:4:4 matrix_convert output */
        uint16_t *yuv;    /* the Y'u'v' 4:2:0 form only: the .yuv frame k_yuvp2_420 writes from tmp_pic */
    };
    uint16_t *tmp_cr;
};

/* what k_stats_final leaves per frame */
struct frame_stats {
    float mm[6];       /* min0,max0,min1,max1,min2,max2 */
    int32_t floor_[3]; /* pic_stats estimated_floor   */
    int32_t ceil_[3];  /* pic_stats estimated_ceiling */
    int32_t mismatch;  /* assumed != measured         */
    uint32_t redone;   /* k_fused_t1: tiles of this frame the first tier could not settle (redone by the exact tiers) */
};

/* estimated_floor/ceiling the pixel kernels normalise with (convert.cpp:939-940).
 * Lives in device memory so that a stats pre-pass can hand it to the next
 * kernel without a host round trip. */
struct assumed_stats {
    int32_t floor_[3];
    int32_t ceil_[3];
};

struct fused_args {
    const frame_io *frames; /* device array, n_frames entries */
    int n_frames;
    uint32_t width, height;
    uint32_t wq;              /* width/4 (k_fused) or width (k_fused_narrow) */
    uint32_t wq_magic;        /* floor(2^32 / wq) */
    uint32_t tiles_per_frame; /* thread-tiles per frame */
    uint32_t chunks_per_frame;
    uint32_t groups;          /* k_fused2 / k_fused_t1 / k_fused_lut16: the grid works as this many groups of gridDim.x / groups
                                 blocks, group g on frames g, g + groups, ... (1: every block on every frame); divides gridDim.x */
    uint32_t xcd_layout;      /* 1: gridDim.x is a multiple of 8 * groups and groups are made of whole rounds of the eight XCDs */
    unsigned long long *block_clock; /* [gridDim.x][2]: start, finish (wall_clock64) of each block, or NULL; finish entries zero at launch */
    const uint32_t *slice_ranges; /* xcd_layout, loop-form kernels: [gridDim.x / groups + 1] first 64-tile slice of every block of a group
                                     (the last entry = slices per frame): block i of a group takes slices [r[i], r[i+1]) of each of the
                                     group's frames; NULL = the round-robin dealing of frame_walk */
    uint32_t *tail_ctr = nullptr; /* not NULL (k_fused_t1, slice ranges in force): the last frame of every group is drawn dynamically (h2y_walk.h,
                                 "The dynamic last frame"): [groups][H2Y_TAIL_WORDS] counters and bits, zero at launch (k_stats_final clears them again) */
    uint32_t tail_slices = 0; /* slices of such a frame */
    uint32_t range_stride = 0; /* 0: one table for every group; else the words from one group's table to the next's (each group cut by
                                 the speeds of its own blocks) */
    const void *table;        /* pq_recA[NREC] then pq_recB[NREC] */
    const void *table_src, *table_dst; /* k_fused, generic transfer pair (pp.convert_transfer == 2): the two stages' tables in the same
                                          format (tfn_build_table), or NULL for a stage that is the identity */
    const float *lut16;       /* k_fused_lut16: PQ of every half in [0,2) */
    const void *table1;       /* k_fused_t1: pq_rec1[H2Y_T1_NREC] */
    h2y::t1_sens sn;          /* k_fused_t1: sensitivity windows */
    uint32_t tiles_magic;     /* floor(2^32 / tiles_per_frame): k_fused_t1's redo list holds frame * tiles + tile */
    float *partial;           /* [n_frames][grid / groups][waves][6] (k_fused: [n_frames][grid][6]) */
    uint32_t *redo_count;     /* k_fused_t1: [n_frames][grid / groups * waves] tiles sent to the redo list, or NULL */
    uint32_t *low_flag;       /* k_fused_t1 with assumed floor 0 / ceiling 1: [n_frames], kept zero between launches, or NULL */
    const assumed_stats *assumed;
    h2y::pix_params pp;       /* offset/range/norm_identity are filled in-kernel from *assumed */
};

/* which instantiation of the fused kernel */
struct fused_variant {
    int in_kind, out_kind, mode;
    int pipe;      /* 0 runtime flags, 1 LINEAR->PQ with floor 0/ceiling 1, 2 LINEAR->PQ general normalisation,
                      3 as 1 for half input through the 16 384-entry table (k_fused_lut16),
                      4 / 5 as 1 / 2 with the binary32 first tier in front (k_fused_t1),
                      6 equal transfers, no PQ at all (k_fused2) */
    bool narrow;   /* width % 4 != 0: scalar-load variant */
    bool even_h;   /* height % 2 == 0: the branch-free loop forms (k_fused2, k_fused_t1) apply */
    bool t1_ok = false; /* the binary32 first tier applies to this descriptor (whatever pipe was chosen in the end): t1_sens is filled in */
    bool cols8 = false; /* k_fused_lut16 only: 8-column thread tiles (width % 8 == 0, all planes 16-byte aligned); wq and tiles count those */
};

struct stats_args {
    const void *in[3];
    size_t npix;
    int vec_ok;     /* planes 16-byte aligned and npix % 4 == 0 handled by tail loop */
    float *partial; /* [grid][6] */
};

struct final_args {
    const float *partial; /* [n_frames][nblk][6] */
    const uint32_t *redo_count; /* [n_frames][nblk] or NULL */
    uint32_t *low_flag;         /* [n_frames] or NULL: see fused_args; read and cleared */
    int nblk;
    frame_stats *out; /* [n_frames] */
    int is_u16, src_bit_depth;
    int check;                     /* compare against *assumed, set frame_stats.mismatch */
    const assumed_stats *assumed;  /* may be NULL when check == 0 */
    assumed_stats *publish;        /* not NULL: frame 0's floor/ceiling are written here */
    unsigned long long *block_clock; /* not NULL: fused_args.block_clock of the launch just finished ... */
    int grid;                        /* ... its grid ... */
    float *xcd_time;                 /* ... and where block 0 leaves the mean run time (us) of the blocks of each XCD [8]; clears the finish entries */
    float *block_time = nullptr;     /* not NULL: [min(grid, 1024)] every block's own run time (us), for the per-block balancing */
    uint32_t *tail_ctr = nullptr;    /* not NULL: fused_args.tail_ctr, cleared for the next launch ... */
    int tail_n = 0;                  /* ... its words */
};

struct fir_args {
    const frame_io *frames;          /* batch form: n_frames entries (tmp_cb/tmp_cr -> out's chroma planes); else NULL */
    int n_frames;
    const uint16_t *src_cb, *src_cr; /* single form: 4:4:4 planes; src_cr may be NULL (one plane) */
    uint16_t *dst_cb, *dst_cr;
    int width, height;
    float fir_max;       /* (float)clip->maxCV of the tmp picture, convert.cpp:314 */
    int apply_yuv_clamp; /* 1: follow with write_yuv's shift + range clamp */
    h2y::pix_params pp;
};

/* k_yuvp2_420 (h2y_yuvp2.hip): convert()'s Y'u'v' 4:2:0 branch, convert.cpp:533-800, then write_yuv */
struct yuvp2_args {
    const frame_io *frames; /* n_frames entries: out = tmp_pic (Y' | Z | X, 4:4:4), yuv = the .yuv frame */
    int n_frames;
    int width, height;
    const uint16_t *lin;    /* [65536]: (unsigned short)(RHO_GAMMA_f(c / 65535.0) * 65535.0), convert.cpp:587-592 */
    float fir_max;          /* (float)maxCV of tmp_pic: the FIR's clip (convert.cpp:520, in_pic->clip) */
    h2y::pix_params pp;     /* write_yuv's shift and range clamp of the output picture */
};

struct inverse_args {
    const void *in[3]; /* Y, Cb/Dz, Cr/Dx: U16 4:4:4 planes, 8-byte aligned */
    void *out[3];      /* G, B, R */
    uint32_t npix;
    int d709;          /* matrix_coeffs == 1 */
    uint32_t minVR, maxVR;
    int shift, shift_right;
};

/* k_fir_fused (h2y_fir_fused.hip): a wave's unit of work is (frame, segment of chroma rows, strip of 240 columns) */
struct firf_args {
    const frame_io *frames;
    int n_frames;
    uint32_t width, height;
    uint32_t wq;              /* width / 4 */
    uint32_t n_strips;        /* ceil(wq / 60) */
    uint32_t n_seg, seg_rows; /* segments per frame, chroma rows per segment (the last may be shorter): the even cut */
    const uint32_t *unit_rows; /* [total_units]: first chroma row | one past the last << 16 of every unit, or NULL for the even cut.
                                  Strips are independent of each other, so every (frame, strip) column may be cut its own way:
                                  the host gives the units that run on slower XCDs fewer rows */
    unsigned long long *block_clock; /* as fused_args.block_clock */
    uint32_t mix_xcds;        /* 1 (grid a multiple of 8): block b works as block h2y_firf_vblock(b), so that the segments of one
                                 (frame, strip) column land on XCDs of both halves of the card and of both parities */
    uint32_t units_per_frame; /* n_seg * n_strips */
    uint32_t total_units;     /* n_frames * units_per_frame */
    uint32_t sync_mask;       /* the block's waves meet at a barrier every sync_mask + 1 steps (a power of two); ~0u: never */
    const void *table, *table1;
    const float *lut16;       /* FF_TIER_LUT16: PQ of every half in [0, 2) */
    h2y::t1_sens sn;
    float *partial;           /* [n_frames][units_per_frame][6] */
    uint32_t *redo_count;     /* [n_frames][units_per_frame] */
    uint32_t *low_flag;       /* [n_frames] or NULL (see fused_args) */
    const assumed_stats *assumed;
    h2y::pix_params pp;
};

/* the upsampling forms of k_up444 / k_inverse420(_batch): up_args.algorithm.  The entries map the public `algorithm` (0, or any other
 * value for the FIR) and the context's inverse chroma siting onto these */
enum { UP_REPLICATE = 0, UP_FIR = 1, UP_FIR_TL = 2 };
struct up_args { /* k_up444: one or two chroma planes, (width/2 x height/2) -> (width x height) */
    const uint16_t *src0, *src1; /* src1 may be NULL (one plane) */
    uint16_t *dst0, *dst1;
    int width, height;           /* of the 4:4:4 result; both even */
    int algorithm;               /* UP_REPLICATE, UP_FIR_TL, else the reference's FIR pair */
    float fmin, fmax;            /* (float) of minCV / maxCV, convert.cpp:1932-1934 */
};

struct inv420_args { /* k_inverse420: Subsample420to444 of both chroma planes and matrix_inverse in one pass */
    up_args up;       /* src0/src1 = the 4:2:0 Cb/Dz and Cr/Dx planes; dst0/dst1 unused; width, height, algorithm, fmin, fmax */
    inverse_args inv; /* in[0] = the luma plane (in[1], in[2] unused), out[3] = G, B, R */
};

/* one frame of k_inverse420_batch / k_inverse_batch: Y, Cb/Dz, Cr/Dx in (chroma at half size each way for 4:2:0), G, B, R out */
struct inv_frame {
    const uint16_t *in[3];
    uint16_t *out[3];
};

#ifdef H2Y_BLOCK_TIMES
void h2y_dump_block_times(const char *path); /* timing experiments only */
void h2y_dump_ff_block_times(const char *path);
#endif
int h2y_fused_threads(const fused_variant &v);
const char *h2y_fused_name(const fused_variant &v);
bool h2y_fused_grouped(const fused_variant &v); /* does the kernel honour fused_args.groups? */
int h2y_fused_blocks_per_cu(const fused_variant &v);
hipError_t h2y_launch_fused(const fused_variant &v, int grid, hipStream_t st, const fused_args &a);
hipError_t h2y_launch_build_lut16(hipStream_t st, const void *table, float *lut);
hipError_t h2y_launch_stats(int in_kind, int grid, hipStream_t st, const stats_args &a);
hipError_t h2y_launch_stats_final(int n_frames, hipStream_t st, const final_args &a);
hipError_t h2y_launch_fir420(hipStream_t st, const fir_args &a);
hipError_t h2y_launch_fir420_tl(hipStream_t st, const fir_args &a); /* k_fir420_tl (h2y_siting.hip): the same arguments, top-left sited */
hipError_t h2y_launch_inverse(int grid, hipStream_t st, const inverse_args &a);
hipError_t h2y_launch_fir_fused(int in_kind, int mode, bool ident, bool lut16, int grid, hipStream_t st, const firf_args &a);
hipError_t h2y_launch_up444(hipStream_t st, const up_args &a);
hipError_t h2y_launch_inverse420(hipStream_t st, const inv420_args &a);
/* the batch forms: frames[n_frames] in device memory; every frame takes base's sizes and arithmetic, its own planes */
hipError_t h2y_launch_inverse420_batch(int grid, hipStream_t st, const inv420_args &base, const inv_frame *frames, int n_frames);
hipError_t h2y_launch_inverse_batch(int grid, hipStream_t st, const inverse_args &base, const inv_frame *frames, int n_frames);
int h2y_inverse420_tiles(int width, int height); /* k_inverse420(_batch) tiles of one frame */
hipError_t h2y_launch_yuvp2_420(bool fir, hipStream_t st, const yuvp2_args &a);
void h2y_yuvp2_lin_table(uint16_t *lin); /* host: the 65 536 entries of yuvp2_args.lin */
hipError_t h2y_launch_box420(hipStream_t st, const uint16_t *src, uint16_t *dst, int W, int H);

/* one frame of a decode kernel (k_dpx_decode, k_tiff_decode, k_exr_decode): its payload in, the planes G, B, R out, each
 * plane of the kernel's own element type (DPX float, TIFF u16, EXR half) */
struct payload_frame {
    const void *payload;
    void *plane[3];
};

/* k_dpx_decode (h2y_dpx.hip): dpx_read()'s per-pixel loop on the device; the payload is interleaved R,G,B, the planes come out in
 * muxed_dpx_to_planar_float_buf's order */
enum { H2Y_DPX_10 = 0, H2Y_DPX_16 = 1, H2Y_DPX_F32 = 2 };
uint32_t h2y_dpx_chunks(int fmt, uint32_t npix); /* k_dpx_decode's units of 256 threads per frame */
hipError_t h2y_launch_dpx_decode(int fmt, bool swap, int grid, hipStream_t st, uint32_t npix, const payload_frame *frames, int n_frames);

/* k_tiff_decode and k_rgb_interleave (h2y_tiff.hip): read_tiff()'s and write_tiff()'s per-pixel work on the device */
struct tiff_geom { /* the decoded picture within `height` packed rows of row_bytes */
    uint32_t width, height, x0, row_bytes;
};
/* one frame: planes G, B, R in, interleaved R,G,B u16 out */
struct rgb_frame {
    const uint16_t *plane[3];
    uint16_t *rgb;
};
uint32_t h2y_tiff_chunks(uint32_t width, uint32_t height); /* k_tiff_decode's units of 256 threads per frame */
uint32_t h2y_rgb_chunks(uint32_t npix);                    /* k_rgb_interleave's */
/* k_tiff_decode's payload: packed rows of interleaved R,G,B u16 */
hipError_t h2y_launch_tiff_decode(bool swap, bool clamp, int grid, hipStream_t st, const tiff_geom &g, const payload_frame *frames, int n_frames);
hipError_t h2y_launch_rgb_interleave(int grid, hipStream_t st, uint32_t npix, const rgb_frame *frames, int n_frames);

/* k_exr_decode (h2y_exr.hip): read_exr()'s scanline decode on the device, from h2y_exr_unpack's payload */
struct exr_geom { /* what k_exr_decode takes of an h2y_exr_info */
    uint32_t width, height, lines_per_chunk, n_chunks, n_channels, line_bytes, flags_bytes, all_half;
    int32_t type[3], offset[3]; /* planes G, B, R: H2Y_EXR_* pixel type (-1 missing), byte offset within a line */
};
hipError_t h2y_launch_exr_decode(int grid, hipStream_t st, const exr_geom &g, const payload_frame *frames, int n_frames);

/* k_compare and k_compare_sum (h2y_compare.hip): two frames of u16 planes reduced per plane to exact integer stats */
struct cmp_geom {
    uint32_t n[3];              /* samples per plane */
    uint32_t width[3];          /* plane width (first_over's x, y are the host's) */
    uint32_t a_off[3], b_off[3]; /* plane start in samples from the frame base, per side */
    uint32_t shift[3];          /* a_off & 7 where both sides share it (16-byte groups), else 0 */
    uint32_t vec;               /* bit p: plane p takes 16-byte loads */
    uint32_t chunks[3];         /* k_compare's units per frame and plane */
    uint32_t sigma;
};
struct cmp_frame { /* one pair; bases 16-byte aligned */
    const uint16_t *a, *b;
};
struct cmp_partial { /* one k_compare unit (at most 16384 samples: its sad and over fit 32 bits) */
    uint64_t sse;
    uint32_t sad, max_abs, over, first; /* first: plane index of the unit's first over-sigma sample, 0xFFFFFFFF when none */
};
struct h2y_compare_stats;
uint32_t h2y_compare_chunks(uint32_t n, uint32_t shift); /* k_compare's units for a plane of n samples */
/* k_compare over (frame, plane, chunk) units into partials[frame x units per frame + unit], then k_compare_sum into stats[frame] */
hipError_t h2y_launch_compare(int grid, hipStream_t st, const cmp_geom &g, const cmp_frame *frames, int n_frames, cmp_partial *partials,
                              h2y_compare_stats *stats);

/* k_histogram and k_histogram_finish (h2y_histogram.hip): code-value bins and legal-range counts of u16 frames, per plane */
struct hist_geom {
    uint32_t n[3];      /* samples per plane */
    uint32_t off[3];    /* plane start in samples from the frame base */
    uint32_t shift[3];  /* off & 7: the 16-byte groups follow the plane's start */
    uint32_t vec;       /* bit p: plane p takes 16-byte loads */
    uint32_t units[3];  /* k_histogram's units per frame and plane */
    uint32_t lo[3], hi[3]; /* the legal range per plane */
    uint32_t nbins, down;  /* 2^bits; bin = min(code >> down, nbins - 1) */
};
struct hist_frame { /* one frame; base 16-byte aligned */
    const uint16_t *base;
};
struct hist_acc { /* one (frame, plane): zeroed before k_histogram */
    uint32_t nmin; /* 65535 - min */
    uint32_t max, below, above, at_low, at_high;
};
struct h2y_histogram_stats;
uint32_t h2y_histogram_units(uint32_t n, uint32_t shift); /* k_histogram's units for a plane of n samples */
size_t h2y_histogram_lds(uint32_t nbins);                 /* its dynamic LDS bytes */
int h2y_histogram_grid(int n_cu, const hist_geom &g, int n_frames);
/* k_histogram over n_frames frames into acc[frame x 3 + plane] and bins[(frame x 3 + plane) x nbins] (both zeroed by the caller),
 * then k_histogram_finish into stats[frame] */
hipError_t h2y_launch_histogram(int grid, hipStream_t st, const hist_geom &g, const hist_frame *frames, int n_frames, hist_acc *acc,
                                uint32_t *bins, h2y_histogram_stats *stats);

/* k_ssim and k_ssim_sum (h2y_ssim.hip): SSIM of two frames of u16 planes, per plane, from exact integer window sums */
struct ssim_geom {
    uint32_t pw[3], ph[3];       /* plane width and height (at least 8 x 8) */
    uint32_t a_off[3], b_off[3]; /* plane start in samples from the frame base, per side */
    uint32_t strips[3], units[3]; /* k_ssim's strips and units (strips x segments) per frame and plane */
    uint32_t wide;               /* bit depth above 12: block sums ss and s12 in 64 bits */
    double c1, c2;               /* the host's constants */
};
struct h2y_ssim_stats;
uint32_t h2y_ssim_strips(uint32_t plane_width);    /* k_ssim's strips of a plane */
uint32_t h2y_ssim_segments(uint32_t plane_height); /* and its segments */
int h2y_ssim_grid(int n_cu, const ssim_geom &g, int n_frames);
/* k_ssim over n_frames pairs into partials[frame x units per frame + unit], then k_ssim_sum into stats[frame] */
hipError_t h2y_launch_ssim(int grid, hipStream_t st, const ssim_geom &g, const cmp_frame *frames, int n_frames, int64_t *partials,
                           h2y_ssim_stats *stats);

/* k_regions and k_regions_sum (h2y_regions.hip): the error of flat and of busy 8x8 tiles, and over- and undershoot, of two frames of
 * u16 planes, per plane, as exact integer sums */
struct regions_geom {
    uint32_t pw[3], ph[3];        /* plane width and height */
    uint32_t a_off[3], b_off[3];  /* plane start in samples from the frame base, per side */
    uint32_t strips[3], units[3]; /* k_regions' strips and units (strips x segments) per frame and plane */
    uint32_t flat_var, radius;    /* a tile is flat when act <= flat_var x n x n; the window's radius, 1..4 */
};
struct regions_partial { /* one k_regions unit: every tile's sums, and the flat tiles' */
    uint64_t sse_all, sse_flat, sad_all, sad_flat, over_sum, under_sum;
    uint32_t tiles_all, tiles_flat, samples_all, samples_flat, over, under, over_max, under_max;
};
struct h2y_regions_stats;
uint32_t h2y_regions_strips(uint32_t plane_width);    /* k_regions' strips of a plane */
uint32_t h2y_regions_segments(uint32_t plane_height); /* and its segments */
int h2y_regions_grid(int n_cu, const regions_geom &g, int n_frames);
/* k_regions over n_frames pairs into partials[frame x units per frame + unit], then k_regions_sum into stats[frame] */
hipError_t h2y_launch_regions(int grid, hipStream_t st, const regions_geom &g, const cmp_frame *frames, int n_frames, regions_partial *partials,
                              h2y_regions_stats *stats);

/* k_light (h2y_light.hip): the content light of frames of the forward conversion's input (include/hdr2yuv_hip.h, h2y_light_stats) */
struct light_frame { /* one frame: its G, B, R planes (16-byte aligned) and the floor / ceiling its conversion used */
    const void *in[3];
    const assumed_stats *assumed;
};
struct light_acc { /* one frame: zeroed before k_light */
    unsigned long long key; /* max over pixels of (m bits << 32) | ~index: the largest m, the first pixel on ties */
    unsigned long long sum; /* sum over pixels of rint(m x 2^32) */
};
struct light_args {
    uint32_t npix;           /* pixels per frame (< 2^28) */
    uint32_t n4;             /* npix / 4: 4-pixel groups read by vector loads; the rest one by one */
    const void *table;       /* the source transfer's table (tfn_build_table; NULL for a LINEAR source) */
    h2y::pix_params pp;      /* derive_params() of the descriptor, src_fn / tf_ext[0] of the source stage set; offset / range per frame */
};
int h2y_light_grid(uint32_t npix, int n_frames); /* blocks per frame */
/* k_light over n_frames frames into acc[frame] (zeroed by the caller) */
hipError_t h2y_launch_light(int in_kind, int grid, hipStream_t st, const light_args &a, const light_frame *frames, int n_frames, light_acc *acc);

/* k_lightdist (h2y_lightdist.hip): the light distribution of the same frames (include/hdr2yuv_hip.h, h2y_lightdist_stats), with
 * k_light's frame table and arguments */
struct lightdist_acc { /* one frame: zeroed before k_lightdist */
    unsigned long long sum; /* sum over pixels of rint(m x 2^32) */
    uint32_t maxscl[3];     /* the largest L of planes G, B, R, as bits */
    uint32_t below;         /* pixels with m <= 0.01f */
};
int h2y_lightdist_grid(uint32_t npix, int n_frames); /* blocks per frame */
/* k_lightdist over n_frames frames into acc[frame] and bins[frame x H2Y_LIGHTDIST_BINS] (both zeroed by the caller) */
hipError_t h2y_launch_lightdist(int in_kind, int grid, hipStream_t st, const light_args &a, const light_frame *frames, int n_frames,
                                lightdist_acc *acc, uint32_t *bins);

/* k_codelight (h2y_codelight.hip): content light and the light distribution of frames of three u16 PQ code planes, 4:4:4
 * (include/hdr2yuv_hip.h, "light of PQ code planes") */
struct codelight_frame { /* one frame: Y, Cb, Cr (or G, B, R), width x height codes each */
    const uint16_t *p[3];
};
struct codelight_args {
    uint32_t npix;           /* pixels per frame (< 2^28) */
    uint32_t n8;             /* npix / 8: 8-pixel groups; the rest one by one */
    uint32_t vec;            /* bit p: plane p of every frame starts 16-byte aligned and takes 16-byte loads */
    float sub[2], div[2];    /* the normalisation of [0] Y (and of G, B, R planes), [1] Cb and Cr: (code - sub) / div */
    const void *table;       /* PQ10000_f's table (tfn_build_table of H2Y_TFN_PQ_F) */
    h2y::pix_params pp;      /* what light1<true> reads: src_tf PQ, src_fn H2Y_TFN_PQ_F, tf_ext[0], norm_identity 1 */
};
int h2y_codelight_grid(uint32_t npix, int n_frames); /* blocks per frame */
/* k_codelight over n_frames frames into acc[frame] and, where dacc is not NULL, dacc[frame] and bins[frame x H2Y_LIGHTDIST_BINS]
 * (all zeroed by the caller); matrix: H2Y_MATRIX_GBR, _BT709, _BT2020NC or _ICTCP */
hipError_t h2y_launch_codelight(int matrix, int grid, hipStream_t st, const codelight_args &a, const codelight_frame *frames, int n_frames,
                                light_acc *acc, lightdist_acc *dacc, uint32_t *bins);

/* k_gamutcheck (h2y_gamutcheck.hip): the gamut containment check of the same frames (include/hdr2yuv_hip.h, "gamut containment of PQ
 * code planes"), with k_codelight's frame table */
struct gamutcheck_acc { /* one frame and set: zeroed before k_gamutcheck */
    unsigned long long key; /* max over pixels of (e bits << 32) | ~index: the largest excursion, the first pixel on ties */
    unsigned long long sum; /* sum over pixels of rint(e x 2^32) */
    uint32_t outside;       /* pixels with e > 0 */
    uint32_t beyond;        /* pixels with e > t m and e > a */
};
struct gamutcheck_frame_acc { /* one frame: its sets' accumulators (H2Y_GAMUTCHECK_MAX_SETS of them, the first n_sets used) */
    gamutcheck_acc set[2];
};
struct gamutcheck_args {
    codelight_args c;        /* k_codelight's */
    uint32_t n_sets;         /* 1 or 2 */
    float m[2][9];           /* per set h2y_gamut_matrix(file, set): row-major, on (R, G, B) columns */
    float t, a;              /* the ratio, and the floor in units of 10000 cd/m2 */
};
/* k_gamutcheck over n_frames frames into acc[frame] (zeroed by the caller), on a grid of h2y_codelight_grid's blocks per frame; matrix: H2Y_MATRIX_GBR, _BT709, _BT2020NC or _ICTCP */
hipError_t h2y_launch_gamutcheck(int matrix, int grid, hipStream_t st, const gamutcheck_args &a, const codelight_frame *frames, int n_frames,
                                 gamutcheck_frame_acc *acc);

/* k_scenesig and k_codescenesig (h2y_scenesig.hip): the scene signature (include/hdr2yuv_hip.h, h2y_scenesig) of the frames k_lightdist
 * and k_codelight measure, with their frame tables and arguments */
struct scenesig_geom {
    uint32_t width, height;
    uint32_t rows; /* rows of a block's band */
};
/* the geometry of a launch of n_frames frames read in groups of `group` pixels (4: k_scenesig, 8: k_codescenesig) */
scenesig_geom h2y_scenesig_geom(uint32_t width, uint32_t height, uint32_t group, int n_frames);
/* over n_frames frames into sig[frame x 144] (zeroed by the caller): cell cy x 16 + cx */
hipError_t h2y_launch_scenesig(int in_kind, hipStream_t st, const light_args &a, const scenesig_geom &g, const light_frame *frames, int n_frames,
                               unsigned long long *sig);
hipError_t h2y_launch_codescenesig(int matrix, hipStream_t st, const codelight_args &a, const scenesig_geom &g, const codelight_frame *frames,
                                   int n_frames, unsigned long long *sig);

/* k_linearize (h2y_linearize.hip): the three lights of every pixel of such frames as binary32 planes G, B, R
 * (include/hdr2yuv_hip.h, "linearised PQ code planes"); k_codelight's arguments */
struct linearize_frame { /* one frame: its code planes as codelight_frame has them, and the three output planes (16-byte aligned) */
    const uint16_t *p[3];
    float *out[3];
};
int h2y_linearize_grid(uint32_t npix, int n_frames); /* blocks per frame */
hipError_t h2y_launch_linearize(int matrix, int grid, hipStream_t st, const codelight_args &a, const linearize_frame *frames, int n_frames);

/* k_deltae (h2y_deltae.hip): Delta E ITP of pairs of such frames (include/hdr2yuv_hip.h, "Delta E ITP of PQ code planes") */
struct deltae_frame { /* one pair: the planes of A and of B as codelight_frame has them */
    const uint16_t *a[3], *b[3];
};
struct deltae_acc { /* one pair: zeroed before k_deltae */
    unsigned long long key;  /* max over pixels of (d bits << 32) | ~index: the largest d, the first pixel on ties */
    unsigned long long sum;  /* sum over pixels of rint(d x 2^20) */
    unsigned long long over; /* pixels with d > threshold */
};
struct deltae_args {
    codelight_args c;        /* k_codelight's, for both sides (vec: plane p of A and of B alike); pp also carries what code1 reads:
                                dst_tf PQ, dst_fn H2Y_TFN_PQ_R, tf_ext[1] */
    const void *table_r;     /* PQ10000_r's table (tfn_build_table of H2Y_TFN_PQ_R) */
    float threshold;
};
int h2y_deltae_grid(uint32_t npix, int n_frames); /* blocks per pair */
/* k_deltae over n_frames pairs into acc[pair] (zeroed by the caller); matrix: H2Y_MATRIX_GBR, _BT709, _BT2020NC or _ICTCP */
hipError_t h2y_launch_deltae(int matrix, int grid, hipStream_t st, const deltae_args &a, const deltae_frame *frames, int n_frames, deltae_acc *acc);

/* k_gamut (h2y_gamut.hip): the conversion between colour primaries of include/hdr2yuv_hip.h on frames of three float or half
 * planes G, B, R; dst may be src (in place) */
struct gamut_frame {
    const void *src[3];
    void *dst[3];
};
struct gamut_args {
    uint32_t npix; /* pixels per frame (< 2^28) */
    uint32_t clip; /* 1: results that are not above 0 become +0.0 */
    float m[9];    /* row-major, on (R, G, B) columns */
};
uint32_t h2y_gamut_chunks(int in_kind, uint32_t npix); /* k_gamut's units of 256 threads per frame */
hipError_t h2y_launch_gamut(int in_kind, int grid, hipStream_t st, const gamut_args &a, const gamut_frame *frames, int n_frames);

/* k_gamut_compress (h2y_gamut_compress.hip): the gamut compression pass of include/hdr2yuv_hip.h on frames of three float or half
 * planes G, B, R, k_gamut's frame table and units (dst may be src: in place) */
struct gamut_compress_consts {
    float m[9];       /* row-major, on (R, G, B) columns: h2y_gamut_matrix's */
    float t;          /* the threshold */
    float q;          /* at least 1 - t (1 - 2^-20): a pixel whose smallest channel is fl(a q) or more is inside the threshold */
    float l[3], k[3]; /* per channel R, G, B: the limit (a curve where it is above 1) and the table's scale */
};
struct gamut_compress_args {
    uint32_t npix; /* pixels per frame (< 2^28) */
    gamut_compress_consts c;
    const float *tables; /* device: 3 x H2Y_GAMUT_COMPRESS_NODES entries, R's, G's, B's */
};
hipError_t h2y_launch_gamut_compress(int in_kind, int grid, hipStream_t st, const gamut_compress_args &a, const gamut_frame *frames,
                                     int n_frames);

/* k_tonemap (h2y_tonemap.hip): the tone curve of include/hdr2yuv_hip.h on frames of three float or half planes G, B, R in linear
 * light, k_gamut's frame table (dst may be src: in place) */
struct tonemap_args {
    uint32_t npix;     /* pixels per frame (< 2^28) */
    float cap;         /* no sample leaves the pass above it */
    const float *gain; /* device: H2Y_LIGHTDIST_BINS gains, h2y_tonemap_curve's */
};
int h2y_tonemap_grid(int n_cu, uint64_t units); /* blocks for so many of k_gamut's units (h2y_gamut_chunks per frame) */
hipError_t h2y_launch_tonemap(int in_kind, int grid, hipStream_t st, const tonemap_args &a, const gamut_frame *frames, int n_frames);

/* k_lut3d (h2y_lut3d.hip): the 3D LUT pass of include/hdr2yuv_hip.h on frames of three float or half planes G, B, R, k_gamut's
 * frame table; in planes mode the destination planes have the source's type (dst may be src: in place), in signal mode they are
 * float (dst may be src for float planes) */
struct alignas(16) lut3d_node {
    float r, g, b, pad; /* 16 bytes: one corner is one access */
};
struct lut3d_consts {
    uint32_t n;                   /* nodes per axis, 2..128 */
    float last;                   /* float(n - 1) */
    float lo[3], s[3];            /* per channel r, g, b: the domain's lower end, (n - 1) / (hi - lo) rounded once */
    float mulY, addY, mulC, addC; /* signal mode: the conversion's scale step (derive_params) */
};
struct lut3d_args {
    uint32_t npix; /* pixels per frame (< 2^28) */
    lut3d_consts c;
    const lut3d_node *nodes; /* device: n^3 nodes, r fastest, then g, then b */
};
/* lds 1 (n <= H2Y_LUT3D_LDS_MAX_N only): k_lut3d_lds, blocks of H2Y_LUT3D_LDS_THREADS threads that read the table from their copy in LDS */
enum { H2Y_LUT3D_LDS_MAX_N = 17, H2Y_LUT3D_LDS_THREADS = 1024 };
uint32_t h2y_lut3d_chunks(int lds, int in_kind, uint32_t npix); /* the kernel's units per frame */
int h2y_lut3d_grid(int n_cu, int lds, uint64_t units);          /* blocks for so many units */
/* interp 0 trilinear, 1 tetrahedral; signal 0 planes, 1 signal */
hipError_t h2y_launch_lut3d(int in_kind, int interp, int signal, int lds, int grid, hipStream_t st, const lut3d_args &a,
                            const gamut_frame *frames, int n_frames);

/* k_hlg (h2y_hlg.hip): the HLG pass of include/hdr2yuv_hip.h on frames of three float or half planes G, B, R of display light,
 * k_gamut's frame table; the destination planes are float (dst may be src for float planes: in place) */
struct hlg_consts {
    float k;                      /* 10000 / L_W rounded once, or 1 */
    float mulY, addY, mulC, addC; /* the conversion's scale step (derive_params) */
};
struct hlg_args {
    uint32_t npix;            /* pixels per frame (< 2^28) */
    hlg_consts c;
    const float *gain, *oetf; /* device: H2Y_LIGHTDIST_BINS entries each, h2y_hlg_tables' */
};
enum { H2Y_HLG_THREADS = 512 };
uint32_t h2y_hlg_chunks(int in_kind, uint32_t npix); /* k_hlg's units of H2Y_HLG_THREADS threads per frame */
int h2y_hlg_grid(int n_cu, uint64_t units);           /* blocks for so many units */
hipError_t h2y_launch_hlg(int in_kind, int grid, hipStream_t st, const hlg_args &a, const gamut_frame *frames, int n_frames);

/* k_ictcp (h2y_ictcp.hip): the ICtCp pass of include/hdr2yuv_hip.h on frames of three float or half planes G, B, R of display
 * light, k_gamut's frame table; the destination planes are float (dst may be src for float planes: in place) */
struct ictcp_args {
    uint32_t npix;          /* pixels per frame (< 2^28) */
    float oY, aY, oC, aC;   /* H.273's scale of dst_bit_depth and dst_full_range */
    float top;              /* 2^n - 1 */
    const void *table_r;    /* PQ10000_r's table (tfn_build_table of H2Y_TFN_PQ_R) */
    h2y::pix_params pp;     /* what code1 reads: dst_tf PQ, dst_fn H2Y_TFN_PQ_R, tf_ext[1] */
};
enum { H2Y_ICTCP_THREADS = 512 };
uint32_t h2y_ictcp_chunks(int in_kind, uint32_t npix); /* k_ictcp's units of H2Y_ICTCP_THREADS threads per frame */
int h2y_ictcp_grid(int n_cu, uint64_t units);           /* blocks for so many units */
hipError_t h2y_launch_ictcp(int in_kind, int grid, hipStream_t st, const ictcp_args &a, const gamut_frame *frames, int n_frames);

/* k_hlg_linearize (h2y_hlgsrc.hip): the display light of frames of three u16 HLG code planes as binary32 planes G, B, R
 * (include/hdr2yuv_hip.h, "light of HLG code planes"); k_linearize's frame table */
struct hlgsrc_args {
    codelight_args c;        /* npix, n8, vec, sub, div (table and pp are not read) */
    float kappa;             /* L_W / 10000 rounded once */
    const float *ootf, *inv; /* device: H2Y_LIGHTDIST_BINS entries each, h2y_hlg_inverse_tables' */
};
int h2y_hlg_linearize_grid(int n_cu, uint32_t npix, int n_frames); /* blocks per frame */
hipError_t h2y_launch_hlg_linearize(int matrix, int grid, hipStream_t st, const hlgsrc_args &a, const linearize_frame *frames, int n_frames);

/* k_sdr_linearize (h2y_sdrsrc.hip): the light of frames of three u16 SDR (BT.1886) code planes as binary32 planes G, B, R
 * (include/hdr2yuv_hip.h, "light of SDR code planes"); k_linearize's frame table */
struct sdrsrc_args {
    codelight_args c;        /* k_linearize's, with the BT.1886 stage in place of PQ's: table is H2Y_TFN_G24's, pp carries src_tf
                                H2Y_TF_BT1886, src_fn H2Y_TFN_G24, tf_ext[0], norm_identity 1 */
    float kappa;             /* W / 10000 rounded once */
};
int h2y_sdr_linearize_grid(uint32_t npix, int n_frames); /* blocks per frame */
hipError_t h2y_launch_sdr_linearize(int matrix, int grid, hipStream_t st, const sdrsrc_args &a, const linearize_frame *frames, int n_frames);

/* k_code_signal (h2y_sigsrc.hip): the signal G', B', R' in [+0, 1] of frames of three u16 code planes as binary32 planes, no transfer
 * applied (include/hdr2yuv_hip.h, "signal of code planes"); k_linearize's frame table; of a it reads npix, n8, vec, sub and div
 * (table and pp are not read) */
int h2y_code_signal_grid(uint32_t npix, int n_frames); /* blocks per frame */
hipError_t h2y_launch_code_signal(int matrix, int grid, hipStream_t st, const codelight_args &a, const linearize_frame *frames, int n_frames);
/* the same arithmetic on 4:4:4 planes in host memory (h2y_code_signal_planes); false for a matrix other than 0, 1 or 9 */
bool h2y_code_signal_host(int matrix, const codelight_args &a, size_t npix, const uint16_t *const src[3], float *const dst[3]);

/* k_scale (h2y_scale.hip): the Lanczos resampler of include/hdr2yuv_hip.h on frames of three u16 planes.  One axis' table on the
 * device: first[d] and count[d] (int32), then d rows of H2Y_SCALE_MAX_TAPS int16 coefficients (zero past count). */
enum { H2Y_SCALE_MAX_TAPS = 32, H2Y_SCALE_TILE_W = 64, H2Y_SCALE_TILE_H = 32, H2Y_SCALE_STAGE_ROWS = 16 };
struct scale_axis {
    const int32_t *first, *count;
    const int16_t *coef;
};
struct scale_plane {
    uint32_t sw, sh, dw, dh;       /* the plane's source and destination size */
    uint32_t src_off, dst_off;     /* plane start in samples from the frame base, per side */
    uint32_t tiles_x, tiles;       /* tiles of H2Y_SCALE_TILE_W x H2Y_SCALE_TILE_H outputs: per row, in all */
    int32_t lo, hi;                /* the clamp */
    scale_axis h, v;
};
struct scale_geom {
    scale_plane p[3];
    uint32_t h_rows;   /* rows of the LDS tile of horizontal sums: the most source rows a tile of the call needs */
    uint32_t src_cols; /* samples per staged source row (a multiple of 8): the widest segment a tile needs, plus its alignment shift */
};
struct scale_frame { /* one frame; bases 16-byte aligned */
    const uint16_t *src;
    uint16_t *dst;
};
size_t h2y_scale_lds(const scale_geom &g); /* k_scale's dynamic LDS bytes */
/* k_scale over (frame, plane, tile) units */
hipError_t h2y_launch_scale(int grid, hipStream_t st, const scale_geom &g, const scale_frame *frames, int n_frames);

/* k_dither (h2y_dither.hip): the reduction to the output bit depth of include/hdr2yuv_hip.h ("dither") on frames of three u16
 * planes; a frame's dst may be its src (in place).  Plane p holds n samples in rows of w, off samples from both bases. */
struct dither_plane {
    uint32_t w, n, off;
    uint32_t chunks; /* k_dither's units of the plane */
    uint32_t lo, hi; /* the clamp at the destination depth */
    uint32_t div_m, div_k; /* (i x div_m) >> div_k = i / w for a plane index i < 2^28 */
};
struct dither_args {
    dither_plane p[3];
    uint32_t shift;    /* s = W - D, 1..8 */
    uint32_t key;      /* seed ^ 0x9E3779B9 */
    uint32_t temporal; /* 1: the frame number enters the keys */
    uint32_t first;    /* the number of the launch's first frame */
};
struct dither_frame { /* one frame; bases 16-byte aligned for 16-byte accesses */
    const uint16_t *src;
    uint16_t *dst;
};
/* plane of `rows` rows of w samples (w x rows < 2^28), off samples from the frame bases, clamped to lo..hi: its units and reciprocal */
dither_plane h2y_dither_plane(uint32_t w, uint32_t rows, uint32_t off, uint32_t lo, uint32_t hi);
/* k_dither<mode> over (frame, plane, chunk) units; mode: H2Y_DITHER_CUT, _ORDERED or _NOISE (h2y_dither1.h) */
hipError_t h2y_launch_dither(int mode, int grid, hipStream_t st, const dither_args &a, const dither_frame *frames, int n_frames);

/* k_pack / k_unpack (h2y_pack.hip): the sample packings of include/hdr2yuv_hip.h between a frame of three u16 planes ("planar")
 * and its packed form.  A job is one plane that becomes bytes or words, or the two chroma planes that become one block of
 * (P1, P2) pairs; offsets count samples from the planar base and elements (bytes, P010: words) from the packed base. */
struct pack_job {
    uint32_t n;       /* the plane's samples, or the chroma block's pairs */
    uint32_t pl, pl2; /* planar: where the plane starts (a chroma block: P1 and P2) */
    uint32_t pk;      /* packed: where its elements start */
    uint32_t sh;      /* indices of the first group that lie before the job */
    uint32_t vec;     /* whole groups lie on 16-byte boundaries on every side: 16-byte accesses */
    uint32_t chunks;  /* the kernels' units of the job */
};
struct pack_args {
    pack_job j[3];  /* PLANAR8: the three planes; NV12, P010: plane 0 and the chroma block (j[2] empty) */
    uint32_t maxv;  /* M = 2^D - 1 */
    uint32_t shift; /* P010: 16 - D; else 0 */
};
struct pack_frame { /* one frame; both bases 16-byte aligned */
    const void *planar, *packed; /* k_pack writes packed, k_unpack planar */
};
/* the jobs of a w x h frame (w x h < 2^28) of a legal (chroma, bit_depth, packing) whose planar planes start off[] samples from
 * the planar base (one after the other in a frame; padded apart in an inverse ring's slot) */
pack_args h2y_pack_args(uint32_t w, uint32_t h, int chroma, int bit_depth, int packing, const uint32_t off[3]);
/* k_pack<packing> or k_unpack<packing> over (frame, job, chunk) units */
hipError_t h2y_launch_pack(int packing, bool unpack, int grid, hipStream_t st, const pack_args &a, const pack_frame *frames, int n_frames);

#endif
