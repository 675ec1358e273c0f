/*
 * hdr2yuv_hip.h -- C-ABI of the MI355X (gfx950) conversion hot path.
 *
 * This is the drop-in boundary for the in-memory convert path of hdr2yuv:
 *
 *     pic_stats()       /root/reference/common.cpp:66   (hdr.h:439)
 *  -> matrix_convert()  /root/reference/convert.cpp:879 (hdr.h:422)
 *  -> convert()         /root/reference/convert.cpp:513 (hdr.h:420)
 *  -> write_yuv()       /root/reference/tiff.cpp:368    (hdr.h:421), the
 *                       per-sample shift + range clamp only; the file write
 *                       stays with the caller.
 *
 * The reference calls those four functions back to back from main()
 * (hdr2yuv.cpp:797-928) on one planar picture.  h2y_convert_frame() replaces
 * that whole sequence; the per-stage entry points below it exist so that a
 * maintainer can swap one stage at a time (the reference's own precedent for
 * that is the compile-time OPENCV_ENABLED switch at hdr2yuv.cpp:892-896).
 *
 * Plain C: pointers, sizes and one POD descriptor.  No C++ or torch types.
 * The library never calls exit(); every entry returns 0 on success and a
 * non-zero H2Y_E* code otherwise (the reference returns 0/1 and exit()s,
 * convert.cpp:1196, common.cpp:231); h2y_last_error() gives the text.
 */
#ifndef HDR2YUV_HIP_H
#define HDR2YUV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define H2Y_ABI_VERSION 1
/* set in h2y_abi_version() by a timing-experiment build of the library (-DH2Y_EXPERIMENT: its kernels may write wrong bytes) */
#define H2Y_ABI_EXPERIMENT 0x40000000

/* ---- enums: integer values are the reference's CLI contract ------------ */

/* pic_t.pic_buffer_type, hdr.h:297-298; F16 is the EXR case (exr.cpp:233,
 * half widened to float before anything else happens). */
#define H2Y_SAMPLE_U16 1
#define H2Y_SAMPLE_F32 2
#define H2Y_SAMPLE_F16 3

/* chroma_format_idc, hdr.h:14-17 */
#define H2Y_CHROMA_420 1
#define H2Y_CHROMA_444 3

/* transfer_characteristics, hdr.h:108-138 */
#define H2Y_TRANSFER_LINEAR 8
#define H2Y_TRANSFER_PQ 16

/* matrix_coeffs, hdr.h:172-193 */
#define H2Y_MATRIX_GBR 0
#define H2Y_MATRIX_BT709 1
#define H2Y_MATRIX_BT2020NC 9
#define H2Y_MATRIX_YDZDX 11
#define H2Y_MATRIX_YDZDX_Y500 12
#define H2Y_MATRIX_YDZDX_Y100 13
/* "YUVPrime2" (hdr.h:190), destination only.  The reference's experimental Y'u'v' coding:
 *  - 4:4:4: matrix_convert() passes G, B, R through (convert.cpp:1191-1194), adds Half - 1 to the two
 *    chroma planes (:1200-1201) unless source and destination matrices are equal, and clamps to maxCV.
 *  - 4:2:0 (convert.cpp:533-800): Y' is copied; per 4:2:0 site the chroma planes carry CIE 1976 u', v'
 *    of X = Cr, Z = Cb and Y = the linearised Y' (RHO_GAMMA_f), each subsampled by the box or the FIR,
 *    clipped to [0, 1] and written as (unsigned short)(u' * 65535.0) whatever the bit depth.  The
 *    reference computes u''v'' and then overwrites them with u'v' (its "HACK", :732-734); that is what
 *    it emits.  Chroma resamplers 0 and 1 only: with any other value the reference reads uninitialised
 *    memory, and the descriptor is refused. */
#define H2Y_MATRIX_YUVPRIME2 15
/* H.273's matrix_coeffs 14, ICtCp (Rec. ITU-R BT.2100, PQ).  Accepted in h2y_codelight_desc.matrix_coeffs only ("light of ICtCp code
 * planes" below): the reference's 14 is "YUVPrime1" (hdr.h:189), its unbuilt Y'u'v' variant, so h2y_desc_check goes on refusing it as a
 * destination, and an ICtCp rung is written by the ICtCp pass ("ICtCp" below) on a passthrough descriptor. */
#define H2Y_MATRIX_ICTCP 14

/* error codes */
#define H2Y_OK 0
#define H2Y_EINVAL 1       /* descriptor / argument rejected            */
#define H2Y_EUNSUPPORTED 2 /* valid for the reference, not on this path */
#define H2Y_EHIP 3         /* a HIP runtime call failed                 */
#define H2Y_ENOMEM 4

/*
 * Picture-pair descriptor: the attribute set of pic_t (hdr.h:363-378) for the
 * source and destination pictures plus user_args_t.chroma_resampler_type
 * (hdr.h:275).  Source and destination have the same width/height (the
 * reference's convert() never resizes either; resizing is cv.cpp, compiled
 * out).  The source is always 4:4:4 (matrix_convert() refuses anything else,
 * convert.cpp:886).
 */
typedef struct h2y_desc {
    int32_t width;
    int32_t height;
    int32_t in_sample_type;        /* H2Y_SAMPLE_*                              */
    int32_t src_bit_depth;         /* used for U16 input only (hdr2yuv.cpp:805) */
    int32_t dst_bit_depth;         /* 8..16                                     */
    int32_t src_transfer;          /* --src_transfer_characteristics            */
    int32_t dst_transfer;          /* --dst_transfer_characteristics            */
    int32_t src_matrix;            /* --src_matrix_coeffs                       */
    int32_t dst_matrix;            /* --dst_matrix_coeffs                       */
    int32_t src_primaries;         /* --src_colour_primaries                    */
    int32_t dst_primaries;         /* --dst_colour_primaries                    */
    int32_t dst_full_range;        /* --dst_video_full_range_flag               */
    int32_t dst_chroma_format_idc; /* H2Y_CHROMA_420 or H2Y_CHROMA_444          */
    int32_t chroma_resampler_type; /* 0 = 2x2 box, non-zero = FIR (convert.cpp:807) */
    /* 0: take floor/ceiling from the frame like pic_stats() does
     * (common.cpp:135-136); 1: use the values below instead (the caller
     * already knows them). */
    int32_t stats_override;
    int32_t floor[3];
    int32_t ceiling[3];
} h2y_desc;

typedef struct h2y_ctx h2y_ctx;

/* Bytes of one output frame in .yuv layout: Y plane, then Cb, then Cr, each
 * row-major little-endian uint16 with no padding (tiff.cpp:457-551).
 * Returns 0 for an invalid descriptor. */
size_t h2y_frame_bytes(const h2y_desc *d);
/* Bytes of one input plane (width*height*sizeof(sample)). */
size_t h2y_plane_bytes(const h2y_desc *d);

/* Validate a descriptor for this path. H2Y_OK / H2Y_EINVAL / H2Y_EUNSUPPORTED.
 * `why` (may be NULL) receives a static string. */
int h2y_desc_check(const h2y_desc *d, const char **why);

int h2y_abi_version(void);

/* Create a context on HIP device `device`. Owns streams, device scratch and
 * the PQ coefficient table. Fails (H2Y_EHIP) when no device is present:
 * there is no CPU fallback in this library. */
int h2y_ctx_create(int device, h2y_ctx **out);
void h2y_ctx_destroy(h2y_ctx *ctx);
const char *h2y_last_error(const h2y_ctx *ctx); /* ctx may be NULL: global error */

/* Tuning and test knobs of one context, as strings (the library reads nothing from the environment):
 *   "t1" "0"|"1"|"always" (binary32 first tier; "always": never steered away from it), "groups" "0"|"1".."64" (frame groups; 0: by the frame's size), "cols8" "0"|"1"
 *   (8-column tiles for half input), "balance" "adaptive"|"xcd"|"off"|"<xcd mask>,<ratio>" (slices by measured block / XCD speed),
 *   "tail" "auto"|"on"|"off" (the last frame of a frame group dealt dynamically), "fir" "auto"|"twopass"|"fused" (how chroma_resampler_type != 0 runs), "firsync" "auto"|"0".."1024" (the one-pass
 *   FIR kernel's waves meet at a barrier every so many steps).  None changes a byte of output.
 * The reference has no counterpart (its only knobs are the command-line flags in h2y_desc). */
int h2y_ctx_set_option(h2y_ctx *ctx, const char *name, const char *value);

/* Use the caller's HIP stream (hipStream_t passed as void*) for every launch
 * of this context; NULL restores the context's own stream. */
int h2y_ctx_set_stream(h2y_ctx *ctx, void *hip_stream);

/*
 * Whole path on HOST buffers: replaces pic_stats + matrix_convert + convert +
 * write_yuv's arithmetic (hdr2yuv.cpp:797-928).
 *   in_planes[3]  planar source samples in the reference's plane order
 *                 0=G/Y, 1=B/Z, 2=R/X (convert.cpp:980-982)
 *   out_yuv       h2y_frame_bytes() bytes, .yuv layout
 * Copies in, runs the device path, copies out, synchronises.
 */
int h2y_convert_frame(h2y_ctx *ctx, const h2y_desc *d,
                      const void *const in_planes[3], uint16_t *out_yuv);

/*
 * Whole path on DEVICE buffers, n_frames independent frames in one call
 * (the reference runs one process per frame and appends, tiff.cpp:440).
 *   d_in[f*3 + c]  device pointer to plane c of frame f
 *   d_out[f]       device pointer to h2y_frame_bytes() bytes for frame f
 * The arrays of pointers themselves are host memory.  Asynchronous on the
 * context's stream except for one small status read-back at the end, after
 * which every frame is final.
 */
int h2y_convert_batch(h2y_ctx *ctx, const h2y_desc *d, int n_frames,
                      const void *const *d_in, uint16_t *const *d_out);

/* As h2y_convert_batch but enqueue-only: no host synchronisation and no
 * status read-back.  h2y_batch_finish() must be called before the outputs
 * are consumed: it waits for the OLDEST batch in flight, checks the per-frame
 * floor/ceiling the kernels measured against the ones they assumed, and
 * re-runs any frame where they differ.  Returns the number of frames re-run
 * through *n_redone.
 * Up to TWO batches may be in flight: enqueue k+1 before finishing k and the
 * next launch is already queued behind the running one (no idle gap between
 * them).  A batch's input and output buffers belong to the library until its
 * own h2y_batch_finish() returns; batches finish in the order enqueued.
 * h2y_convert_batch() finishes everything in flight, its own batch last. */
int h2y_convert_batch_enqueue(h2y_ctx *ctx, const h2y_desc *d, int n_frames,
                              const void *const *d_in, uint16_t *const *d_out);
int h2y_batch_finish(h2y_ctx *ctx, int *n_redone);

/* ---- per-stage entries (device buffers), for stage-at-a-time swaps ------ */

/* pic_stats() F32/F16/U16 branch (common.cpp:74-139): per-plane min/max and
 * the derived estimated_floor/ceiling.  fminmax[6] = {min0,max0,min1,...} as
 * float (integers for U16), floor_ceiling[6] likewise as int. */
int h2y_pic_stats(h2y_ctx *ctx, const h2y_desc *d, const void *const d_in[3],
                  float fminmax[6], int32_t floor_ceiling[6]);

/* matrix_convert() (convert.cpp:879-1221), F32/F16/U16 in -> U16 4:4:4 out.
 * d->floor/ceiling are used (stats_override is ignored: caller ran stats). */
int h2y_matrix_convert(h2y_ctx *ctx, const h2y_desc *d, const void *const d_in[3],
                       uint16_t *const d_out444[3]);

/* convert() chroma part (convert.cpp:802-859): one U16 plane 4:4:4 -> 4:2:0,
 * box (resampler 0) or FIR. bit_depth gives the clamp (clip->maxCV). */
int h2y_subsample_420(h2y_ctx *ctx, int width, int height, int bit_depth,
                      int chroma_resampler_type, const uint16_t *d_src,
                      uint16_t *d_dst);

/* matrix_inverse() (hdr.h:423, convert.cpp:1320-1867): the .yuv -> .tiff flow of
 * hdr2yuv.cpp:818-819.  U16 4:4:4 planes Y', Cb/Dz, Cr/Dx in, U16 planes G, B, R out, on the device,
 * 8-byte aligned.  Byte-exact with the compiled reference, including its oddities: Half/Full are those
 * of 12 bits at any bit depth, only matrix_coeffs 1 (BT.709) takes the Y'CbCr equations -- every other
 * value, BT.2020 included, the Y'DzDx ones --, matrix_coeffs 0 is refused (the reference exits), the
 * result is clamped to the INPUT picture's video (or full) range and shifted to out_bit_depth.
 * The function indexes all three planes at full resolution: 4:2:0 input goes through h2y_upsample_444 first
 * (h2y_inverse_420 does both). */
int h2y_matrix_inverse(h2y_ctx *ctx, int width, int height, int in_bit_depth, int in_full_range,
                       int in_matrix_coeffs, int out_bit_depth, const uint16_t *const d_in[3],
                       uint16_t *const d_out[3]);

/* Subsample420to444() (convert.cpp:1869-1986; the same function is yuv2tiff.cpp:575-692, called at :341-342;
 * in convert.cpp only its call site :1576-1577 is under #if 0): one U16 chroma plane of (width/2) x (height/2)
 * samples -> width x height, on the device.  algorithm 0 replicates samples (:1871-1881); any other value runs
 * the FIR pair (:1882-1983): vertical (3 -16 67 227 -32 7)/256 per row parity into a U16 intermediate, then
 * even samples copied and odd samples (21 -52 159 159 -52 21)/256; edges replicate; every stage clamps to
 * [min_cv, max_cv] and truncates.  width and height even (for odd sizes the reference reads rows of its
 * intermediate that it never wrote); d_dst 4-byte aligned. */
int h2y_upsample_444(h2y_ctx *ctx, int width, int height, int algorithm, unsigned min_cv, unsigned max_cv,
                     const uint16_t *d_src, uint16_t *d_dst);

/* The .yuv 4:2:0 -> RGB flow (yuv2tiff.cpp:341-342 followed by its pixel loop = matrix_inverse()):
 * d_in = Y (width x height), Cb/Dz and Cr/Dx (width/2 x height/2); both chroma planes are upsampled with
 * minCV 0 / maxCV 2^in_bit_depth - 1 (yuv2tiff.cpp:92-93,142-154) into scratch the context owns, then
 * h2y_matrix_inverse() runs on the three full planes.  width a multiple of 4, height even. */
int h2y_inverse_420(h2y_ctx *ctx, int width, int height, int in_bit_depth, int in_full_range, int in_matrix_coeffs,
                    int out_bit_depth, int algorithm, const uint16_t *const d_in[3], uint16_t *const d_out[3]);

/* The same flow on HOST buffers, one frame: what main() does between read_planar_integer_file() (hdr2yuv.cpp:582-656) and
 * write_tiff() (tiff.cpp:559-652: the `<< (out depth - in depth)` of its sample loop is part of out_bit_depth here) when a
 * .yuv is read for a .tiff (hdr2yuv.cpp:818-819).  in_planes = Y, Cb/Dz, Cr/Dx as the file holds them: all three width x height
 * for in_chroma_format_idc 3 (h2y_matrix_inverse), chroma at half size each way for 1 (h2y_inverse_420 with `algorithm`);
 * out_planes = G, B, R, width x height each.  Copies in, runs the device path, copies out, synchronises. */
int h2y_inverse_frame(h2y_ctx *ctx, int width, int height, int in_chroma_format_idc, int in_bit_depth, int in_full_range,
                      int in_matrix_coeffs, int out_bit_depth, int algorithm, const uint16_t *const in_planes[3],
                      uint16_t *const out_planes[3]);

/* Frames per launch of h2y_inverse_batch: longer batches are split into launches of at most this many frames. */
#define H2Y_INVERSE_FRAMES_PER_LAUNCH 64

/* The .yuv -> G,B,R flow of h2y_inverse_420 (in_chroma_format_idc 1) or h2y_matrix_inverse (3) on n_frames frames of one size in
 * one call, device buffers: what main() does per frame between read_planar_integer_file() (hdr2yuv.cpp:582-656) and write_tiff()
 * (hdr2yuv.cpp:818-819), for a whole sequence.
 *   d_in[f*3 + c]   Y, Cb/Dz, Cr/Dx of frame f (chroma width/2 x height/2 for in_chroma_format_idc 1)
 *   d_out[f*3 + c]  G, B, R of frame f, width x height each
 * The arrays of pointers themselves are host memory; each frame's planes may lie anywhere.  Limits as the single-frame entries:
 * width a multiple of 4 and height even for 4:2:0, planes 4-byte (4:2:0) or 8-byte (4:4:4) aligned.  The frames run in
 * launches of up to H2Y_INVERSE_FRAMES_PER_LAUNCH (k_inverse420_batch / k_inverse_batch: every launch deals all its frames'
 * tiles over one persistent grid); h2y_last_kernel_ms() sums them.  Synchronous: every frame is final on return. */
int h2y_inverse_batch(h2y_ctx *ctx, int width, int height, int in_chroma_format_idc, int in_bit_depth, int in_full_range,
                      int in_matrix_coeffs, int out_bit_depth, int algorithm, int n_frames, const uint16_t *const *d_in,
                      uint16_t *const *d_out);

/* ---- host <-> device pipeline --------------------------------------------
 * The reference reads a frame, converts it and appends it to the .yuv, one after the other
 * (hdr2yuv.cpp:582-656 reader, :797-928, tiff.cpp:457-551 writer).  Here the upload of frame
 * k+1, the conversion of frame k and the download of frame k-1 overlap, through a ring of
 * `depth` pinned host slots that the caller fills and drains in place:
 *
 *     h2y_stream_open(ctx, &desc, 3);
 *     for each frame:  h2y_stream_input(ctx, planes);   read the file into planes[0..2]
 *                      h2y_stream_submit(ctx);
 *                      if (frames in flight == depth - 1) { h2y_stream_output(ctx, &yuv); write yuv; }
 *     drain:           h2y_stream_output(ctx, &yuv) for the frames still in flight
 *     h2y_stream_close(ctx);
 *
 * planes[c] hold h2y_plane_bytes() each, yuv h2y_frame_bytes(); the pointer h2y_stream_output
 * returns stays valid until the next h2y_stream_output / h2y_stream_close.  Frames come out in
 * submission order.  No other entry of the context may be used while a stream is open. */
int h2y_stream_open(h2y_ctx *ctx, const h2y_desc *d, int depth /* 2..16 slots */);
/* The same ring for the .yuv -> G,B,R flow (h2y_inverse_frame's arguments; hdr2yuv.cpp:818-819 frame after frame): each slot
 * does one H2D copy of its three input planes, the kernel, one D2H copy of its three output planes.  h2y_stream_input hands out
 * Y, Cb/Dz, Cr/Dx (chroma width/2 x height/2 for in_chroma_format_idc 1, else width x height), h2y_stream_output returns
 * G | B | R, width x height uint16 each, contiguous in that order.  h2y_stream_submit / _close as above; while it is open,
 * h2y_stream_open and every other entry are refused, as they are while a forward stream is open. */
int h2y_inverse_stream_open(h2y_ctx *ctx, int width, int height, int in_chroma_format_idc, int in_bit_depth, int in_full_range,
                            int in_matrix_coeffs, int out_bit_depth, int algorithm, int depth /* 2..16 slots */);
int h2y_stream_input(h2y_ctx *ctx, void *planes[3]);
int h2y_stream_submit(h2y_ctx *ctx);
int h2y_stream_output(h2y_ctx *ctx, const uint16_t **yuv);
int h2y_stream_close(h2y_ctx *ctx);

/* ---- DPX input (dpx_read(), dpx.cpp:209-520, then muxed_dpx_to_planar_float_buf(), common.cpp:14-27) ------------------
 * The header and the file read stay on the host; the per-pixel loop runs on the device (k_dpx_decode).  What a DPX file is
 * to the reference: 2048 header bytes; the first four read as a native little-endian int are 0x53445058 (bytes "XPDS": no byte
 * swap) or 0x58504453 ("SDPX": every 32-bit word, or every 16-bit word of a 16-bit file, byte-swapped); the pixels start at
 * the u32 at byte 4; width and height are the u32 at 772 and 776, narrowed to short; the element bit size is the byte at 803
 * (10: one 32-bit word per pixel, R = w >> 22, G = (w >> 12) & 1023, B = (w >> 2) & 1023, each (float)(c / 1023.0); 16: R, G,
 * B u16, (float)(u / 65535.0); 32: R, G, B binary32, copied as they are).  Descriptor, packing and end-of-line padding are
 * ignored: the payload is width x height interleaved R,G,B pixels in one block.  The decoded planes are G, B, R (the
 * reference's fbuf[0..2]) of an F32 4:4:4 picture. */
typedef struct h2y_dpx_info {
    int32_t width;          /* 1..32767 */
    int32_t height;         /* 1..32767 */
    int32_t bit_size;       /* 10, 16 or 32 */
    int32_t swap;           /* 1: big-endian file ("SDPX"), words byte-swapped */
    uint64_t data_offset;   /* first payload byte in the file */
    uint64_t payload_bytes; /* width * height * (4, 6 or 12) */
} h2y_dpx_info;

/* Parse a DPX header: `header` holds the file's first n bytes, file_bytes is the file's size.  Host only: no device, no
 * context.  Refuses (H2Y_EINVAL, `why` a static string) where the reference aborts -- a bad magic, a bit size other than 10,
 * 16 or 32 -- and, where the reference would read memory it never initialised, a header shorter than 2048 bytes and a payload
 * that runs past the end of the file (data_offset + payload_bytes > file_bytes); also a width or height outside 1..32767
 * after the narrowing to short. */
int h2y_dpx_parse(const void *header, size_t n, uint64_t file_bytes, h2y_dpx_info *out, const char **why);

/* Frames per launch of h2y_dpx_decode_batch: longer batches are split into launches of at most this many frames. */
#define H2Y_DPX_FRAMES_PER_LAUNCH 64

/* The per-pixel loop of dpx_read() and the demux on n_frames payloads of one geometry and format, device buffers:
 *   d_payload[f]       device pointer to frame f's payload_bytes, 4-byte aligned
 *   d_planes[f*3 + c]  device pointers to frame f's float planes G, B, R (width x height each), 4-byte aligned
 * The arrays of pointers themselves are host memory.  16-byte accesses where a frame's payload and planes allow them.  Runs in
 * launches of up to H2Y_DPX_FRAMES_PER_LAUNCH; synchronous: every plane is final on return.  Chain it with h2y_convert_batch
 * (d->in_sample_type H2Y_SAMPLE_F32) for the whole .dpx -> .yuv flow on device buffers. */
int h2y_dpx_decode_batch(h2y_ctx *ctx, const h2y_dpx_info *info, int n_frames, const void *const *d_payload,
                         float *const *d_planes);

/* The h2y_stream_* ring of h2y_stream_open on DPX payloads: each slot does one H2D copy of payload_bytes, k_dpx_decode into the
 * slot's device float planes, the forward conversion of d (in_sample_type H2Y_SAMPLE_F32, width and height those of info), and
 * one D2H copy of the .yuv frame.  h2y_stream_input hands out planes[0] = the pinned payload (payload_bytes; fill it with the
 * file's bytes from data_offset on), planes[1] = planes[2] = NULL; h2y_stream_submit / _output / _close and the exclusivity
 * rules are those of the forward stream. */
int h2y_dpx_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_dpx_info *info, int depth /* 2..16 slots */);

/* ---- 16-bit RGB TIFF input and output (read_tiff(), tiff.cpp:54-362; write_tiff(), tiff.cpp:559-652) -----------------------
 * The IFD and the file I/O stay on the host; the per-pixel work runs on the device (k_tiff_decode, k_rgb_interleave).  What a
 * TIFF is to read_tiff: uncompressed strips of interleaved u16 R, G, B read raw (TIFFReadRawStrip), strip s = row s; a row is
 * bc[0] = 6 x ImageWidth bytes.  Geometry, with stripsize = bc[0] in uint32 arithmetic:
 *   start = 0; if stripsize > 960*6: start = (stripsize - 3840*6)/2, 0 when that wraps past stripsize; then --cutout_hd:
 *   (stripsize - 1920*6)/2, --cutout_qhd: (stripsize - 960*6)/2 (qhd wins); rows: stripStart = (N - 1080)/2 (hd) or
 *   (N - 540)/2 (qhd) of the N rows; width = (stripsize - start)/6 - start/6, height = N - 2 stripStart.
 * A picture wider than 3840 is centre-cropped to 3840; the cutouts centre-crop to 1920x1080 / 960x540.  Each sample is
 * clamped to [4096, 60160] when the input picture is video range; planes G, B, R.  Extensions over the reference: any number of
 * rows (it exits unless N is 1080 or 2160), RowsPerStrip > 1 (row r at StripOffsets[r / RPS] + (r % RPS) x 6W), and "MM" files
 * decoded with the bytes of each sample exchanged (the reference reads them unswapped). */
#define H2Y_TIFF_CUTOUT_HD 1  /* --cutout_hd 1 */
#define H2Y_TIFF_CUTOUT_QHD 2 /* --cutout_qhd 1; with both bits set qhd wins, as in read_tiff */

typedef struct h2y_tiff_info {
    int32_t file_width;     /* ImageWidth */
    int32_t file_height;    /* ImageLength */
    int32_t rows_per_strip; /* RowsPerStrip (ImageLength where the tag is absent or larger) */
    int32_t swap;           /* 1: an "MM" (big-endian) file: the bytes of every sample are exchanged */
    int32_t width;          /* the decoded picture: pixels x0 .. x0 + width - 1 of rows y0 .. y0 + height - 1 */
    int32_t height;
    int32_t x0;
    int32_t y0;
    uint64_t row_bytes;     /* 6 x file_width: one file row */
    uint64_t payload_bytes; /* height x row_bytes: the decoded rows, whole, one after the other */
    uint64_t data_offset;   /* file offset of row y0 */
    int32_t contiguous;     /* 1: the decoded rows lie back to back in the file from data_offset on (one read fills a slot) */
    int32_t reserved;       /* 0 */
} h2y_tiff_info;

/* Parse a classic TIFF held whole in memory (file: file_bytes bytes) for read_tiff's decode with `cutout` (H2Y_TIFF_CUTOUT_*
 * bits).  Host only: no device, no context.  row_offsets (may be NULL) receives the file offset of each decoded row; it needs
 * room for info.height entries (row_capacity).  Refuses (H2Y_EINVAL, `why` a static string): a file that is not a classic TIFF,
 * BigTIFF, Compression other than 1, BitsPerSample other than 16 for any sample, SamplesPerPixel other than 3, PlanarConfig
 * 2, SampleFormat other than 1, a strip or an array past the end of the file, a truncated IFD, a one-row strip whose byte count
 * is not 6 x ImageWidth, a horizontal crop that starts inside a pixel (odd ImageWidth: the reference misaligns the channels),
 * and a cutout larger than the picture (the reference's uint32 arithmetic wraps). */
int h2y_tiff_parse(const void *file, size_t file_bytes, int cutout, h2y_tiff_info *out, uint64_t *row_offsets, int row_capacity,
                   const char **why);

/* The bytes of a TIFF file that go before (head: 8) and after (tail: *tail_bytes) the 6 x width x height bytes of interleaved
 * R,G,B u16 samples: head + samples + tail is, byte for byte, the file libtiff 4.3 writes for write_tiff's call sequence
 * (SamplesPerPixel 3, BitsPerSample 16, PlanarConfig 1, ImageWidth, ImageLength, RowsPerStrip 1, Photometric 2, one raw strip
 * per row): the strips from offset 8 on, then the IFD with its ten entries (Compression 1 included) and its out-of-line
 * arrays.  tail NULL: *tail_bytes receives the size only; otherwise *tail_bytes is tail's capacity on entry and the size on
 * return.  Refuses a size < 1 and a file that would need BigTIFF (4 GiB or more). */
int h2y_tiff_layout(int width, int height, uint8_t head[8], uint8_t *tail, size_t *tail_bytes);

/* Frames per launch of h2y_tiff_decode_batch and h2y_rgb_interleave_batch. */
#define H2Y_TIFF_FRAMES_PER_LAUNCH 64

/* read_tiff's per-pixel loop on n_frames payloads of one geometry, device buffers:
 *   d_payload[f]       device pointer to frame f's payload_bytes (the decoded rows, whole, as h2y_tiff_parse laid them out),
 *                      2-byte aligned
 *   d_planes[f*3 + c]  device pointers to frame f's u16 planes G, B, R (width x height each), 2-byte aligned
 * clamp_video_range: 1 for a video-range input picture ([4096, 60160]), 0 to keep the samples.  16-byte accesses where a
 * frame's payload, row_bytes and x0 (and its planes) allow them.  Synchronous.  Chain it with h2y_convert_batch
 * (in_sample_type H2Y_SAMPLE_U16, src_bit_depth 16) for the .tiff -> .yuv flow on device buffers. */
int h2y_tiff_decode_batch(h2y_ctx *ctx, const h2y_tiff_info *info, int clamp_video_range, int n_frames,
                          const void *const *d_payload, uint16_t *const *d_planes);

/* write_tiff's interleave on n_frames of width x height: d_planes[f*3 + c] = frame f's u16 planes G, B, R, d_rgb[f] its
 * 3 x width x height interleaved R,G,B u16 output (device pointers, 2-byte aligned).  Synchronous. */
int h2y_rgb_interleave_batch(h2y_ctx *ctx, int width, int height, int n_frames, const uint16_t *const *d_planes,
                             uint16_t *const *d_rgb);

/* The h2y_stream_* ring of h2y_stream_open on TIFF rows: each slot does one H2D copy of payload_bytes, k_tiff_decode into the
 * slot's device u16 planes, the forward conversion of d (in_sample_type H2Y_SAMPLE_U16, src_bit_depth 16, width and height
 * the info's decoded ones) and one D2H copy of the .yuv frame.  clamp_video_range as for h2y_tiff_decode_batch (the input
 * picture's range flag: h2y_desc has none).  h2y_stream_input hands out planes[0] = the pinned payload (fill it with the
 * decoded rows: payload_bytes from data_offset when contiguous, else row by row from the parse's row offsets), planes[1] =
 * planes[2] = NULL; the rest and the exclusivity rules are those of the forward stream. */
int h2y_tiff_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_tiff_info *info, int clamp_video_range,
                         int depth /* 2..16 slots */);

/* The inverse ring of h2y_inverse_stream_open with write_tiff's interleave after the inverse kernel: h2y_stream_output returns
 * width x height x 3 u16, R, G, B per pixel -- the samples between h2y_tiff_layout's head and tail. */
int h2y_tiff_inverse_stream_open(h2y_ctx *ctx, int width, int height, int in_chroma_format_idc, int in_bit_depth, int in_full_range,
                                 int in_matrix_coeffs, int out_bit_depth, int algorithm, int depth);

/* ---- scanline OpenEXR input (read_exr(), exr.cpp:138-255) ---------------------------------------------------------------
 * read_exr() opens an RgbaInputFile, takes the size from the data window and stores every pixel's half R, G, B as planes
 * G, B, R (alpha ignored).  Half -> float is exact, so the picture is three half planes for the H2Y_SAMPLE_F16 forward path.
 * The container and the decompression stay on the host (h2y_exr_parse, h2y_exr_unpack: zlib, RLE); the predictor, the byte
 * reorder and the scanline-to-plane decode run on the device (k_exr_decode).  What the subset is, as RgbaInputFile (OpenEXR
 * 2.x) reads it:
 *   channels  R, G, B are read (A and every other channel take their space in each line and are skipped); a missing R, G or
 *             B reads +0.0.  A line holds `width` samples of each channel, in the order of the channel names (sorted).
 *   types     HALF is taken bit for bit; FLOAT through floatToHalf (a finite |f| > 65504 becomes +-inf before rounding,
 *             otherwise round to nearest even; a NaN keeps its top 10 mantissa bits, 1 if they are all 0); UINT through
 *             uintToHalf (u > 65504: +inf, otherwise half((float)u)).
 *   chunks    NONE, RLE, ZIPS: one line each, ZIP: 16 (the last one may hold fewer).  A chunk whose size is its lines'
 *             uncompressed bytes is stored raw, whatever the compression.
 * Refused (H2Y_EINVAL, `why` naming the cause): tiled, multi-part and deep files; PIZ, PXR24, B44, B44A, DWAA, DWAB;
 * luminance/chroma files (Y, RY, BY); a channel with x or y sampling other than 1; an offset table that is broken or points
 * past the end of the file (OpenEXR would rebuild it by scanning the chunks); a chunk whose y is not its table slot's, or whose
 * size exceeds its uncompressed bytes. */
#define H2Y_EXR_NONE 0 /* the file's compression codes this reader takes */
#define H2Y_EXR_RLE 1
#define H2Y_EXR_ZIPS 2
#define H2Y_EXR_ZIP 3
#define H2Y_EXR_UINT 0 /* pixel types */
#define H2Y_EXR_HALF 1
#define H2Y_EXR_FLOAT 2
#define H2Y_EXR_MISSING (-1)
#define H2Y_EXR_CHUNK_RAW 0     /* payload flag byte of a chunk: its lines as the file would hold them uncompressed */
#define H2Y_EXR_CHUNK_ENCODED 1 /* its bytes before the predictor and the reorder (RLE or ZIP expanded) */
#define H2Y_EXR_FRAMES_PER_LAUNCH 64

typedef struct h2y_exr_info {
    int32_t width;           /* the data window: width x height pixels from (x_min, y_min) */
    int32_t height;
    int32_t x_min;
    int32_t y_min;
    int32_t compression;     /* H2Y_EXR_NONE .. H2Y_EXR_ZIP */
    int32_t line_order;      /* 0 INCREASING_Y, 1 DECREASING_Y (the chunks' order in the file only) */
    int32_t lines_per_chunk; /* 1, 16 for ZIP */
    int32_t n_chunks;        /* ceil(height / lines_per_chunk): the offset table's entries */
    int32_t n_channels;      /* every channel of the file, the skipped ones included */
    int32_t all_half;        /* 1: every channel is HALF (k_exr_decode's fast path) */
    int32_t channel_type[3]; /* planes G, B, R (channels G, B, R): H2Y_EXR_UINT/HALF/FLOAT, or H2Y_EXR_MISSING */
    int32_t channel_offset[3]; /* planes G, B, R: byte offset of the channel's `width` samples within a line; -1 missing */
    int32_t line_bytes;      /* one line of every channel */
    int32_t reserved;        /* 0 */
    uint64_t flags_bytes;    /* the payload's head: one flag byte per chunk, padded to 256 bytes */
    uint64_t payload_bytes;  /* flags_bytes + height x line_bytes: the unpacked lines follow the flags in row order */
} h2y_exr_info;

typedef struct h2y_exr_chunk { /* one entry of the offset table, checked */
    uint64_t offset;       /* file offset of the chunk: int32 y, int32 size, then `size` packed bytes */
    uint32_t packed_bytes; /* its size field */
    int32_t row;           /* its first line: y - y_min */
} h2y_exr_chunk;

/* Parse a scanline OpenEXR file held whole in memory (file: file_bytes bytes).  Host only: no device, no context.  chunks
 * (may be NULL) receives the n_chunks checked table entries, indexed by increasing y; it needs room for info.n_chunks
 * (capacity).  Refuses what the block above lists, and a truncated header or table. */
int h2y_exr_parse(const void *file, size_t file_bytes, h2y_exr_info *out, h2y_exr_chunk *chunks, int capacity, const char **why);

/* Unpack chunks [first_chunk, first_chunk + n_chunks) of a parsed file into payload (info.payload_bytes, host memory): chunk c's
 * lines go to flags_bytes + chunks[c].row x line_bytes and its flag to payload[c].  A NONE chunk or one stored raw is copied
 * (H2Y_EXR_CHUNK_RAW); an RLE, ZIPS or ZIP chunk is expanded (H2Y_EXR_CHUNK_ENCODED) and must fill its lines exactly.  The
 * bytes between the flags and flags_bytes are zeroed by the call that unpacks chunk 0.  Host only; disjoint ranges of one
 * frame may run on separate threads. */
int h2y_exr_unpack(const h2y_exr_info *info, const h2y_exr_chunk *chunks, const void *file, int first_chunk, int n_chunks,
                   void *payload, const char **why);

/* k_exr_decode on n_frames payloads of one info, device buffers, in launches of H2Y_EXR_FRAMES_PER_LAUNCH:
 *   d_payload[f]       device pointer to frame f's payload (h2y_exr_unpack's layout), 2-byte aligned
 *   d_planes[f*3 + c]  device pointers to frame f's half planes G, B, R (width x height u16 each), 2-byte aligned
 * Synchronous.  Chain it with h2y_convert_batch (in_sample_type H2Y_SAMPLE_F16) for the .exr -> .yuv flow on device buffers. */
int h2y_exr_decode_batch(h2y_ctx *ctx, const h2y_exr_info *info, int n_frames, const void *const *d_payload,
                         uint16_t *const *d_planes);

/* The h2y_stream_* ring of h2y_stream_open on EXR payloads: each slot does one H2D copy of payload_bytes, k_exr_decode into
 * the slot's device half planes, the forward conversion of d (in_sample_type H2Y_SAMPLE_F16, width and height the data
 * window's) and one D2H copy of the .yuv frame.  h2y_stream_input hands out planes[0] = the pinned payload (fill it with
 * h2y_exr_unpack), planes[1] = planes[2] = NULL; the rest and the exclusivity rules are those of the forward stream. */
int h2y_exr_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_exr_info *info, int depth /* 2..16 slots */);

/* ---- comparison with a reference (--ref_filename / --sigma_compare; hdr2yuv.cpp:91-100, :827-833 leaves it a TODO) ------
 * Two frames A and B of u16 samples, three planes each, reduced per plane to exact integers: how many samples, the sum of
 * squared and of absolute differences, the largest |a - b|, how many samples have |a - b| > sigma and where the first of them
 * is.  Plane geometry: 4:2:0 (chroma_format_idc 1) Y width x height, Cb and Cr (width >> 1) x (height >> 1), the planes one
 * after the other as h2y_frame_bytes lays them out; 4:4:4 (3, also the G | B | R planes of the inverse flow) three planes of
 * width x height.  The reductions run on the device (k_compare, then k_compare_sum over its per-block partials: no atomics,
 * so every figure is independent of the order of the work). */
#define H2Y_COMPARE_FRAMES_PER_LAUNCH 64

typedef struct h2y_compare_stats {
    uint64_t samples[3];    /* per plane: samples compared */
    uint64_t sse[3];        /* sum of (a - b)^2 */
    uint64_t sad[3];        /* sum of |a - b| */
    uint64_t over[3];       /* samples with |a - b| > sigma */
    int64_t first_over[3];  /* plane index y x plane_width + x of the first such sample in raster order, -1 when none */
    uint32_t max_abs[3];    /* largest |a - b| */
    uint32_t first_a[3];    /* a and b at first_over (0 when none) */
    uint32_t first_b[3];
    uint32_t reserved;      /* 0 */
} h2y_compare_stats;

/* n_frames pairs of device frames, each frame's three planes contiguous from a 16-byte aligned base (H2Y_EINVAL otherwise):
 * out[f] (host memory) receives the stats of d_a[f] against d_b[f].  chroma_format_idc 1 or 3, sigma >= 0.  Launches of up to
 * H2Y_COMPARE_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them); synchronous. */
int h2y_compare_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int sigma, int n_frames,
                      const uint16_t *const *d_a, const uint16_t *const *d_b, h2y_compare_stats *out);

/* Arm an open ring (forward, DPX, TIFF, EXR, inverse, TIFF inverse) after its *_stream_open and before its first input: every
 * submitted frame is then compared on the device with a reference frame the caller supplies.  The reference is laid out as the
 * ring's output: a .yuv frame (h2y_frame_bytes) on the forward rings, the G | B | R planes (width x height each) on the inverse
 * rings -- on the TIFF inverse ring the planes before the interleave.  keep_output 0: the frame itself stays on the device (no
 * download; the TIFF inverse ring skips the interleave too) and h2y_stream_output returns *yuv = NULL. */
int h2y_stream_compare(h2y_ctx *ctx, int sigma, int keep_output);
/* The pinned slot that receives the reference of the frame about to be submitted (call it before each h2y_stream_submit of an
 * armed ring); h2y_stream_submit uploads it on the upload stream and runs k_compare on the slot's device output after the
 * conversion. */
int h2y_stream_reference(h2y_ctx *ctx, void **ref);
/* The stats of the frame that h2y_stream_output returned last. */
int h2y_stream_compare_result(h2y_ctx *ctx, h2y_compare_stats *out);
/* A compare-only ring: no conversion.  h2y_stream_input lends A's three planes (planes of the geometry above, one after the
 * other), h2y_stream_reference B's frame in the same layout; h2y_stream_output returns *yuv = NULL and
 * h2y_stream_compare_result the stats. */
int h2y_compare_stream_open(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int sigma, int depth /* 2..16 slots */);

/* ---- code-value histograms and the legal-range check ("hist", "check video range": hdr2yuv.cpp:658, :797 leave them a TODO) --
 * A frame of u16 samples, three planes in the comparison's geometry (4:2:0 Y, Cb, Cr; 4:4:4 Y, Cb, Cr or G, B, R), counted per
 * plane on the device (k_histogram, then k_histogram_finish): 2^bits bins, bin = code >> (bit_depth - bits) (a code above
 * 2^bit_depth - 1 counts in the last bin), and, from the samples themselves, min, max and the samples below, above and at the
 * limits of the legal range of set_pic_clip() (common.cpp:300-327) at bit_depth: [0, maxCV] in full range; in video range
 * [minVR, maxVR] for plane 0 and for every plane of a G, B, R frame (gbr 1), [minVRC, maxVRC] for planes 1 and 2 of a YCbCr frame
 * -- write_yuv()'s per-plane clamp (tiff.cpp:469-478).  Every figure is an exact integer. */
#define H2Y_HISTOGRAM_FRAMES_PER_LAUNCH 64

typedef struct h2y_histogram_stats {
    uint64_t samples[3]; /* per plane: samples counted */
    uint64_t below[3];   /* samples < lo */
    uint64_t above[3];   /* samples > hi */
    uint64_t at_low[3];  /* samples == lo */
    uint64_t at_high[3]; /* samples == hi */
    uint32_t min[3];     /* smallest and largest sample (0 and 0 for a plane of no samples) */
    uint32_t max[3];
    uint32_t lo[3];      /* the legal range the counts are of */
    uint32_t hi[3];
    uint32_t nbins;      /* 2^bits: bins per plane */
    uint32_t shift;      /* bit_depth - bits */
} h2y_histogram_stats;

/* n_frames device frames (d_frames[f]: the three planes one after the other from a 16-byte aligned base): out_stats[f] (host)
 * receives frame f's stats and, when out_bins (host) is not NULL, out_bins[(f x 3 + plane) x 2^bits + bin] its bins.
 * chroma_format_idc 1 or 3 (2: H2Y_EUNSUPPORTED), bit_depth 8..16, bits 1..bit_depth, full_range and gbr 0 or 1.  Launches of up
 * to H2Y_HISTOGRAM_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them); synchronous. */
int h2y_histogram_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int bit_depth, int full_range, int gbr, int bits,
                        int n_frames, const uint16_t *const *d_frames, h2y_histogram_stats *out_stats, uint32_t *out_bins);

/* Arm an open ring (forward, DPX, TIFF, EXR, inverse, TIFF inverse; with or without h2y_stream_compare) after its *_stream_open
 * and before its first input: every submitted frame is then counted on the device, after its conversion, on the kernel stream;
 * the output bytes do not change.  What is counted: on the forward rings the .yuv frame (dst_bit_depth, dst_full_range, YCbCr
 * limits), on the inverse rings the G, B, R planes before any interleave (out_bit_depth, in_full_range, G/B/R limits).  bits
 * 1..that bit depth; 0 takes the bit depth itself. */
int h2y_stream_histogram(h2y_ctx *ctx, int bits);
/* The same with the frame's bit depth (8..16), range and limits given: required on a compare-only ring (h2y_compare_stream_open),
 * whose frame A it counts; on the other rings -1 for each takes the ring's own, as h2y_stream_histogram does. */
int h2y_stream_histogram_ex(h2y_ctx *ctx, int bits, int bit_depth, int full_range, int gbr);
/* The stats (and, out_bins not NULL, the 3 x 2^bits bins) of the frame that h2y_stream_output returned last. */
int h2y_stream_histogram_result(h2y_ctx *ctx, h2y_histogram_stats *out_stats, uint32_t *out_bins);
/* A histogram-only ring: no conversion.  h2y_stream_input lends the frame's three planes one after the other; h2y_stream_output
 * returns *yuv = NULL and h2y_stream_histogram_result the counts. */
int h2y_histogram_stream_open(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int bit_depth, int full_range, int gbr,
                              int bits, int depth /* 2..16 slots */);

/* ---- SSIM beside the comparison ("SNR, etc. computation on orig vs. decoded": hdr2yuv.cpp:826 leaves it a TODO) ---------------
 * SSIM on code values, per plane, of two frames in the comparison's geometry, as x264 and FFmpeg define it: 4x4 blocks at (4i, 4j)
 * (columns and rows past the last whole block ignored), one window per 2x2 group of neighbouring blocks (8x8 samples at a stride
 * of 4), with exact integer sums S1 = sum a, S2 = sum b, SS = sum a^2 + sum b^2, S12 = sum ab.  At bit depth d, M = 2^d - 1,
 * c1 = ((0.01 * 0.01) * M) * M * 64 and c2 = (((0.03 * 0.03) * M) * M * 64) * 63 (binary64, left to right), each window in binary64
 * with separate roundings:
 *   vars = ((SS * 64) - S1 * S1) - S2 * S2,  covar = (S12 * 64) - S1 * S2,
 *   s = (((2 * S1) * S2 + c1) * ((2 * covar) + c2)) / (((S1 * S1 + S2 * S2) + c1) * (vars + c2)),
 * added to sum_q as rint(s x 2^32) (half to even) in int64, so every figure is independent of the order of the work.
 * ssim[p] = (sum_q x 2^-32) / windows; all = ((ssim0 n0 + ssim1 n1) + ssim2 n2) / (n0 + n1 + n2), n the planes' sample counts.
 * Every plane needs at least 8 x 8 samples (4:2:0: width and height of at least 16). */
#define H2Y_SSIM_FRAMES_PER_LAUNCH 64

typedef struct h2y_ssim_stats {
    uint64_t windows[3]; /* per plane: ((plane_width >> 2) - 1) x ((plane_height >> 2) - 1) */
    int64_t sum_q[3];    /* sum over the windows of rint(s x 2^32) */
    double ssim[3];      /* (sum_q x 2^-32) / windows */
    double all;          /* the planes' values weighted by their sample counts */
} h2y_ssim_stats;

/* n_frames pairs of device frames in h2y_compare_batch's layout and alignment: out[f] (host memory) receives the SSIM of d_a[f] against
 * d_b[f].  chroma_format_idc 1 or 3 (2: H2Y_EUNSUPPORTED), bit_depth 8..16, n_frames >= 1.  Launches of up to
 * H2Y_SSIM_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them, h2y_last_kernel_name "k_ssim"); synchronous. */
int h2y_ssim_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int bit_depth, int n_frames, const uint16_t *const *d_a,
                   const uint16_t *const *d_b, h2y_ssim_stats *out);

/* Arm a ring that h2y_stream_compare (or h2y_compare_stream_open) has armed, before its first input: k_ssim then runs on the kernel
 * stream after k_compare, on the same device frame and reference; the output bytes and the compare stats do not change.
 * bit_depth -1 takes the ring's own (dst_bit_depth on the forward rings, out_bit_depth on the inverse rings); a compare-only ring
 * needs it given (8..16).  H2Y_EINVAL when the ring is not armed for comparison. */
int h2y_stream_ssim(h2y_ctx *ctx, int bit_depth);
/* The SSIM of the frame that h2y_stream_output returned last. */
int h2y_stream_ssim_result(h2y_ctx *ctx, h2y_ssim_stats *out);

/* ---- PSNR of flat and of busy areas, over- and undershoot ("measure undershoot and overshoot", "measure PSNR on flat areas
 * separate from busy areas": entries 2 and 3 of the reference's NOTES) -------------------------------------------------------------
 * Two frames A and B of u16 samples in the comparison's geometry and layout, measured per plane: A is the produced or decoded
 * picture, B the reference (k_compare's a and b).  chroma_format_idc 1 or 3.
 * Tiles and classes.  A plane is cut into 8x8 tiles at (8i, 8j); the last column and row of tiles are cut to the plane, so a tile
 * has n = tw x th samples, 1 <= tw, th <= 8, and every sample belongs to exactly one tile.  From B alone, in uint64:
 *   S = sum b,  SS = sum b^2,  act = n x SS - S x S          (n^2 times the tile's variance; below 2^45 at 16 bits)
 * and the tile is flat (class 0) when act <= flat_var x n x n, busy (class 1) otherwise; flat_var is in squared code values.  Per
 * plane and class c: tiles[c], samples[c], sse[c] = sum (a - b)^2 and sad[c] = sum |a - b| over the class's tiles.  Summed over
 * the two classes, samples, sse and sad equal h2y_compare_stats' samples, sse and sad of the same pair.
 * Over- and undershoot.  For a sample at (x, y), m and M are the smallest and the largest b over the window
 * [x - r, x + r] x [y - r, y + r] cut to the plane, r = radius (1..4); o = max(a - M, 0), u = max(m - a, 0).  Per plane: over the
 * samples with o > 0, over_sum the sum of o, over_max the largest o; under, under_sum, under_max the same for u.
 * Every figure is an exact integer: nothing depends on how the work is dealt. */
#define H2Y_REGIONS_FRAMES_PER_LAUNCH 64

typedef struct h2y_regions_stats {
    uint64_t tiles[3][2], samples[3][2], sse[3][2], sad[3][2];   /* [plane][0 flat, 1 busy] */
    uint64_t over[3], over_sum[3], under[3], under_sum[3];
    uint32_t over_max[3], under_max[3];
    uint32_t flat_var, radius;                                    /* what the figures are of */
} h2y_regions_stats;

/* The figures of one pair of frames in host memory (each frame's planes one after the other), in plain C++ on the CPU: the twin of
 * k_regions, as h2y_dither_offsets is k_dither's.  H2Y_EINVAL: a size below 1 or of 2^28 samples or more, chroma_format_idc other
 * than 1, 2 or 3, radius outside 1..4, a null pointer; H2Y_EUNSUPPORTED: chroma_format_idc 2. */
int h2y_regions_host(int width, int height, int chroma_format_idc, uint32_t flat_var, int radius, const uint16_t *a, const uint16_t *b,
                     h2y_regions_stats *out);

/* n_frames pairs of device frames in h2y_compare_batch's layout and alignment: out[f] (host memory) receives the figures of d_a[f]
 * against d_b[f].  chroma_format_idc 1 or 3 (2: H2Y_EUNSUPPORTED), radius 1..4, n_frames >= 1.  Launches of up to
 * H2Y_REGIONS_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them, h2y_last_kernel_name "k_regions"); synchronous. */
int h2y_regions_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, uint32_t flat_var, int radius, int n_frames,
                      const uint16_t *const *d_a, const uint16_t *const *d_b, h2y_regions_stats *out);

/* Arm a ring that h2y_stream_compare (or h2y_compare_stream_open) has armed, before its first input, beside h2y_stream_ssim,
 * h2y_stream_deltae and h2y_stream_histogram: k_regions then runs on the kernel stream after k_compare, on the same device frame and
 * reference; the output bytes and every other stage's results do not change.  H2Y_EINVAL when the ring is not armed for
 * comparison, when it is armed for this already, after the first input, or for a radius outside 1..4. */
int h2y_stream_regions(h2y_ctx *ctx, uint32_t flat_var, int radius);
/* The figures of the frame that h2y_stream_output returned last. */
int h2y_stream_regions_result(h2y_ctx *ctx, h2y_regions_stats *out);

/* ---- content light level (MaxCLL / MaxFALL, CTA-861.3) of a forward conversion to PQ ------------------------------------------
 * Scope: dst_transfer 16 (PQ), src_transfer another transfer the conversion linearises (8 LINEAR, 18 RHO_GAMMA, 1/6/14/15
 * BT.1886), src_matrix 0 (G, B, R); anything else is H2Y_EUNSUPPORTED.  Light is taken where matrix_convert() defines it
 * (convert.cpp:930-1040), per frame, with the offset and range the conversion used for that frame (the frame's own pic_stats
 * floor and ceiling, or the descriptor's stats_override):
 *   per sample  L_c = the binary32 value matrix_convert() hands to PQ10000_r: v' = (v - offset[c]) / range[c] (binary32 subtract,
 *               IEEE divide; v itself when every offset is 0 and every range 1), then L_c = tf_to_linear(src transfer, v') (v' itself
 *               for LINEAR).  A NaN counts as 0; L_c is clamped to [0, 1], what the output can carry.  PQ maps L = 1 to 10000 cd/m2.
 *   per pixel   m = max(L_G, L_B, L_R)
 *   per frame   max_bits = the largest m as a binary32 bit pattern, (x, y) the first pixel in raster order that holds it;
 *               sum_q = sum over the pixels of rint(m x 2^32) (half to even) in uint64 -- exact, whatever the order of the work
 *               (an 8K frame stays below 2^58); cll = 10000 x m_max and fall = ((10000 x (double)sum_q) x 2^-32) / pixels, binary64,
 *               in that order.
 * MaxCLL and MaxFALL of a sequence are the largest cll and fall of its frames (the hdr2yuv CLI rounds them to whole cd/m2). */
#define H2Y_LIGHT_FRAMES_PER_LAUNCH 64

typedef struct h2y_light_stats {
    uint32_t max_bits; /* the largest m of the frame, as binary32 bits */
    uint32_t x, y;     /* the first pixel in raster order that holds it */
    uint32_t reserved; /* 0 */
    uint64_t sum_q;    /* sum over the pixels of rint(m x 2^32) */
    uint64_t pixels;   /* width x height */
    double cll;        /* 10000 x m_max, cd/m2 */
    double fall;       /* ((10000 x sum_q) x 2^-32) / pixels, cd/m2 */
} h2y_light_stats;

/* The light of n_frames device frames of d (d_planes[f x 3 + c]: plane c = G, B, R of frame f, 16-byte aligned, in the layout
 * h2y_convert_batch reads): out[f] (host memory).  Floor and ceiling as h2y_convert_batch takes them: the descriptor's override,
 * or pic_stats of each frame (k_stats, run here).  Launches of up to H2Y_LIGHT_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums
 * them, h2y_last_kernel_name "k_light"); synchronous. */
int h2y_light_batch(h2y_ctx *ctx, const h2y_desc *d, int n_frames, const void *const *d_planes, h2y_light_stats *out);

/* Arm an open forward ring (h2y_stream_open, h2y_dpx_stream_open, h2y_tiff_stream_open, h2y_exr_stream_open, h2y_pqcode_stream_open; with or without
 * h2y_stream_compare and h2y_stream_histogram) before its first input: k_light then runs on every frame's decoded planes, on the
 * kernel stream after the conversion, with the floor and ceiling the conversion used; the output bytes do not change.
 * H2Y_EUNSUPPORTED for a descriptor out of the scope above, H2Y_EINVAL on any other ring. */
int h2y_stream_light(h2y_ctx *ctx);
/* The light of the frame that h2y_stream_output returned last. */
int h2y_stream_light_result(h2y_ctx *ctx, h2y_light_stats *out);

/* ---- light distribution (SMPTE ST 2094-40, "HDR10+" dynamic metadata) of a forward conversion to PQ ------------------------------
 * A second measurement on the samples of the content-light section above, in its scope, word for word: dst_transfer 16, a source
 * transfer the conversion linearises (8, 18, 1/6/14/15), src_matrix 0; anything else is H2Y_EUNSUPPORTED.
 *   per sample  L_c as above: normalised with the frame's floor and ceiling, through the source transfer by the conversion's own
 *               tiers, a NaN as 0, clamped to [+0, 1].
 *   per pixel   m = max(L_G, L_B, L_R)
 *   per frame, all exact integers, independent of the order of the work:
 *     maxscl_bits[c]  the largest L_c of plane c (0 G, 1 B, 2 R) as a binary32 bit pattern (L >= +0 orders as its bits)
 *     max_bits        the largest m = the largest of the three maxscl_bits; sum_q = sum over the pixels of rint(m x 2^32) (half to
 *                     even) in uint64; pixels = width x height: h2y_light_stats' figures, equal to h2y_light_batch's on the same frame
 *     below_100       the pixels with m <= 0.01f (bits 0x3C23D70A: 100 cd/m2)
 *     the histogram   H2Y_LIGHTDIST_BINS = 8706 uint32 bins of m by its bit pattern e: bin 0 when e < 0x37000000 (m < 2^-17, below
 *                     0.08 cd/m2), otherwise bin = ((e - 0x37000000) >> 14) + 1: 512 bins per binade (0.2 % wide) over the 17
 *                     binades [2^-17, 1), bins 1..8704; m = 1 alone lands in bin 8705
 *     pct_bits[i]     for p = H2Y_LIGHTDIST_PCT[i] hundredths of a percent (1, 5, 10, 25, 50, 75, 90, 95, 99 and 99.98 %): the
 *                     percentile's bin is the smallest k with cum(k) x 10000 >= p x pixels (uint64; cum(k) the count in bins 0..k),
 *                     and pct_bits[i] that bin's lower edge as binary32 bits: 0 for bin 0, 0x37000000 + ((k - 1) << 14) otherwise.
 *                     A percentile never exceeds max_bits; a 1 x 1 frame returns its own bin's edge for every p.
 * k_lightdist counts the bins on the device; the percentiles are found on the host from the downloaded bins.
 * Units of the HDR10+ file are 0.1 cd/m2 as integers: u(L) = rint(100000 x (double)L), half to even, 0..100000; the average is
 * rint(((100000 x (double)sum_q) x 2^-32) / pixels), in fall's order of operations. */
#define H2Y_LIGHTDIST_BINS 8706
#define H2Y_LIGHTDIST_FIRST_BITS 0x37000000u /* 2^-17: the lower edge of bin 1 */
#define H2Y_LIGHTDIST_PERCENTILES 10
#define H2Y_LIGHTDIST_PCT {100, 500, 1000, 2500, 5000, 7500, 9000, 9500, 9900, 9998}
#define H2Y_LIGHTDIST_FRAMES_PER_LAUNCH 64

typedef struct h2y_lightdist_stats {
    uint32_t maxscl_bits[3]; /* the largest L of planes G, B, R, as binary32 bits */
    uint32_t max_bits;       /* the largest m of the frame */
    uint64_t sum_q;          /* sum over the pixels of rint(m x 2^32) */
    uint64_t pixels;         /* width x height */
    uint64_t below_100;      /* pixels with m <= 0.01f */
    uint32_t pct_bits[H2Y_LIGHTDIST_PERCENTILES]; /* the percentiles' bin edges, as binary32 bits */
} h2y_lightdist_stats;

/* The light distribution of n_frames device frames of d: planes, alignment and floor / ceiling (stats_override, or k_stats run
 * here) exactly as h2y_light_batch takes them.  out[f] (host memory); bins_out may be NULL, otherwise it receives n_frames x
 * H2Y_LIGHTDIST_BINS uint32.  Launches of up to H2Y_LIGHTDIST_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them,
 * h2y_last_kernel_name "k_lightdist"); synchronous. */
int h2y_lightdist_batch(h2y_ctx *ctx, const h2y_desc *d, int n_frames, const void *const *d_planes, h2y_lightdist_stats *out,
                        uint32_t *bins_out);

/* Arm an open forward ring before its first input, beside any other stage (after h2y_stream_gamut it sees the converted planes):
 * k_lightdist then runs on every frame's decoded planes, on the kernel stream after the conversion, with the floor and ceiling the
 * conversion used; the output bytes and every other stage's results do not change.  H2Y_EUNSUPPORTED / H2Y_EINVAL exactly where
 * h2y_stream_light returns them. */
int h2y_stream_lightdist(h2y_ctx *ctx);
/* The light distribution of the frame that h2y_stream_output returned last. */
int h2y_stream_lightdist_result(h2y_ctx *ctx, h2y_lightdist_stats *out);

/* The HDR10+ JSON (the file x265 takes as --dhdr10-info) of n_frames frames in one scene, SceneId 0, the first of them frame
 * first_frame_index of the sequence.  Host only: no device, no context.  Writes at most cap - 1 bytes and a terminating 0 into buf
 * (buf may be NULL when cap is 0) and returns the bytes the whole text needs, the terminator not counted; 0 for a null stats, n_frames
 * < 1, a negative first_frame_index or a frame without pixels.  Layout, one SceneInfo entry per frame and line:
 *   {"JSONInfo": {"HDR10plusProfile": "A", "Version": "1.0"}, "SceneInfo": [ENTRY, ...],
 *    "SceneInfoSummary": {"SceneFirstFrameIndex": [first], "SceneFrameNumbers": [n]}, "ToolInfo": {"Tool": "hdr2yuv", "Version": "1.0"}}
 *   ENTRY = {"LuminanceParameters": {"AverageRGB": A, "LuminanceDistributions": {"DistributionIndex": [1, 5, 10, 25, 50, 75, 90, 95, 99],
 *            "DistributionValues": [9 integers]}, "MaxScl": [R, G, B]}, "NumberOfWindows": 1,
 *            "TargetedSystemDisplayMaximumLuminance": 400, "SceneFrameIndex": k, "SceneId": 0, "SequenceFrameIndex": first + k}
 * in 0.1 cd/m2 (u(L) above).  The DistributionValues slots follow the HDR10+ convention: slot "1" and slots "25".."99" carry those
 * percentiles, slot "5" the 99.98th percentile, slot "10" the whole percentage of pixels at or below 100 cd/m2,
 * floor(100 x below_100 / pixels).  The layout is written from x265's documentation; no encoder's parser has checked it. */
size_t h2y_lightdist_json(const h2y_lightdist_stats *stats, int n_frames, long first_frame_index, char *buf, size_t cap);

/* ---- light of PQ code planes: MaxCLL / MaxFALL and the HDR10+ figures of a finished PQ master, from its codes (--light_only 1) ---
 * The two sections above see the light of a conversion.  This one measures a picture that is PQ already: a PQ Y'CbCr .yuv, a
 * decoded stream, a 16-bit PQ .rgb.  It is the project's own definition, as gamut and siting are: the reference's matrix_inverse
 * treats BT.2020 as Y'DzDx and hard-codes 12-bit constants, so it defines no bytes here.
 * Frame: three u16 code planes at bit_depth n (8..16), video or full range; matrix_coeffs 0 (G, B, R planes), 1 (BT.709) or 9
 *   (BT.2020nc); chroma_format_idc 3, or 1 with even sizes (not with matrix 0).  The transfer is PQ, always.
 *   1. Chroma at every pixel.  4:4:4 planes are used as they are.  4:2:0 planes are first upsampled by what the .yuv -> RGB flow
 *      uses: k_up444 with the clip [0, 2^n - 1], in the form `algorithm` and the context's inverse chroma siting select (algorithm
 *      0 replication; otherwise the reference's FIR pair, or under h2y_ctx_set_inverse_chroma_siting(2) the top-left form; siting 2
 *      with algorithm 0 is H2Y_EUNSUPPORTED), into a scratch area the context owns.  Two passes.
 *   2. Normalise, in binary32: the codes are integers and so exact; each step is one subtraction and one IEEE division.  With
 *      s = 2^(n-8):  video range  y = (Y - 16 s) / (219 s),  cb = (Cb - 128 s) / (224 s),  cr likewise;
 *                    full range   y = Y / (2^n - 1),         cb = (Cb - 2^(n-1)) / (2^n - 1),  cr likewise.
 *      Matrix 0: all three planes are normalised as Y is.
 *   3. Matrix, every product and sum rounded by itself to binary32 (no fused multiply-add), the constants being these decimal
 *      values rounded once to binary32:
 *        matrix 9:  R' = y + 1.4746 cr;  B' = y + 1.8814 cb;  G' = (y - 0.16455313 cb) - 0.57135313 cr
 *        matrix 1:  R' = y + 1.5748 cr;  B' = y + 1.8556 cb;  G' = (y - 0.18732427 cb) - 0.46812427 cr
 *        matrix 0:  none.
 *      No subnormal arises: the smallest non-zero |v'| over all 10-bit (Y, Cb) pairs is 1.16e-6.
 *   4. Clamp before the transfer: v' = v > 0 ? min(v, 1) : +0; L_c = PQ10000_f(v') by the conversion's tiers (the table, the
 *      full-range table, the careful tier), then the clamp to [+0, 1] of the sections above.  The clamp in front is part of the
 *      definition: PQ10000_f of a negative argument is a NaN, and every near-black pixel with a little chroma would otherwise
 *      take the careful tier.
 *   5. From here on nothing is new: m = max(L_G, L_B, L_R), and per frame h2y_light_stats and h2y_lightdist_stats word for word.
 * Anchors (10-bit video range, Cb = Cr = 512): Y 64 -> 0; Y 940 and 1023 -> 1.0 (10000 cd/m2); Y 509 -> 99.9128 cd/m2; Y 723 ->
 * 1004.19 cd/m2. */
#define H2Y_CODELIGHT_FRAMES_PER_LAUNCH 8 /* a launch's 4:2:0 scratch: 2 planes x 2 bytes x width x height x 8 frames -- 253 MiB at 3840 x 2160 */

typedef struct h2y_codelight_desc {
    int width, height, chroma_format_idc, bit_depth, full_range, matrix_coeffs, algorithm;
} h2y_codelight_desc;

/* The light of n_frames device frames of d.  d_frames[f] holds the frame's three planes one after the other from a 16-byte
 * aligned base, as h2y_histogram_batch takes them (4:2:0: Y, then two chroma planes of (width / 2) x (height / 2)).  out[f]
 * (host memory) always; dist_out (n_frames entries) and bins_out (n_frames x H2Y_LIGHTDIST_BINS uint32) may each be NULL: with
 * either given, the one pass yields both structs, and their max_bits and sum_q agree.  Launches of up to
 * H2Y_CODELIGHT_FRAMES_PER_LAUNCH frames, each k_up444 per 4:2:0 frame and then one k_codelight (h2y_last_kernel_ms sums them,
 * upsampling included; h2y_last_kernel_name "k_codelight"; the variant names the matrix, DIST and the upsampling form, e.g.
 * "k_codelight<BT2020NC,DIST,FIR>"); synchronous.
 * H2Y_EUNSUPPORTED: chroma_format_idc 2, a matrix other than 0, 1, 9 and 14 (ICtCp, below), siting 2 with replication.  H2Y_EINVAL: a bad size (4:2:0:
 * odd, or above 32766), depth or alignment, full_range not 0 or 1, matrix 0 with 4:2:0. */
int h2y_codelight_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int n_frames, const uint16_t *const *d_frames, h2y_light_stats *out,
                        h2y_lightdist_stats *dist_out, uint32_t *bins_out);

/* A ring that only measures light: h2y_stream_input lends the frame's three planes (contiguous, as above), h2y_stream_output
 * returns *yuv = NULL, h2y_stream_light_result the frame's light and, when want_dist is 1, h2y_stream_lightdist_result its
 * distribution.  The inverse chroma siting is read when the ring opens.  Every arming entry (h2y_stream_compare, _ssim, _histogram,
 * _histogram_ex, _light, _lightdist, _scale, _gamut) but h2y_stream_scenesig and h2y_stream_gamutcheck is H2Y_EINVAL on this ring.  Refusals as h2y_codelight_batch; want_dist other
 * than 0 or 1 and depth outside 2..16 are H2Y_EINVAL. */
int h2y_codelight_stream_open(h2y_ctx *ctx, const h2y_codelight_desc *d, int want_dist, int depth);

/* ---- scene signature and scene cuts: per-scene HDR10+ metadata of a conversion or of a PQ master (--scene_detect 1, --scene_cuts) ----
 * HDR10+ metadata is scene-based: a display adapts its tone curve per scene.  This section is the project's own definition (the
 * reference has none): a spatial signature of a frame's light, counted on the device; a distance between two signatures and the
 * cuts it gives; the figures of a scene, merged exactly from its frames' figures and bins; and the scene-based JSON.
 *
 * Signature of a frame.  m = max(L_G, L_B, L_R) of a pixel exactly as the light sections above define it: on the forward flow
 *   light1 with the frame's floor and ceiling, a NaN as 0, the clamp ("light distribution"); on PQ code frames steps 1-4 of "light of
 *   PQ code planes".  Its log-light value is the bin index of the light distribution, b = bin_of(bits(m)), 0..8705, 512 to a stop.
 *   The frame is divided into a fixed grid of H2Y_SCENESIG_COLS x H2Y_SCENESIG_ROWS cells: pixel (x, y) of a W x H frame belongs to
 *   cell (cy, cx) = ((y x 9) / H, (x x 16) / W), by integer division.  Every pixel has exactly one cell; a frame narrower than 16 or
 *   lower than 9 leaves some cells empty.  cell[cy x 16 + cx] is the sum of b over the cell's pixels, pixels = W x H.  All figures
 *   are integer sums: exact whatever the order of the work and the number of GPUs.
 * Distance.  S = the sum over the cells of |a.cell - b.cell|, an exact uint64; D = (double)S / (512.0 x (double)a.pixels): the mean
 *   absolute change of the cells' mean log light, in stops (weighted by the cells' sizes).
 * Cuts.  Frame 0 opens scene 0; frame f opens a new scene when the distance between frames f - 1 and f exceeds the threshold.
 * Figures of a scene.  maxscl_bits and max_bits: the maxima over the scene's frames; the 128-bit sum of the frames' sum_q; pixels
 *   and below_100: sums; pct_bits from the frames' bins summed in uint64, by the rule of "light distribution": the smallest k with
 *   cum(k) x 10000 >= p x pixels, all in uint64.  The scene's average in 0.1 cd/m2 is rint(((100000 x (double)S128) x 2^-32) /
 *   (double)pixels), half to even, in that order, (double)S128 being the correctly rounded conversion of the 128-bit sum: it is
 *   h2y_lightdist_json's order of operations.
 *   Invariant: a scene of one frame carries exactly that frame's figures, and its entry in h2y_lightdist_json_scenes' text has the
 *   LuminanceParameters of that frame's entry in h2y_lightdist_json's.
 * The threshold the hdr2yuv CLI takes by default (0.5 stops) is a choice, not a measurement. */
#define H2Y_SCENESIG_COLS 16
#define H2Y_SCENESIG_ROWS 9
#define H2Y_SCENESIG_FRAMES_PER_LAUNCH 64

typedef struct h2y_scenesig {
    uint64_t cell[H2Y_SCENESIG_COLS * H2Y_SCENESIG_ROWS]; /* row-major, cy*16+cx: sum of b over the cell's pixels */
    uint64_t pixels;                                      /* W x H */
} h2y_scenesig;

typedef struct h2y_scene_stats {
    int64_t  first_frame, n_frames;
    uint32_t maxscl_bits[3], max_bits;              /* maxima over the scene's frames */
    uint64_t sum_q_hi, sum_q_lo;                    /* the 128-bit sum of the frames' sum_q */
    uint64_t pixels, below_100;                     /* sums */
    uint32_t pct_bits[H2Y_LIGHTDIST_PERCENTILES];   /* from the summed bins, by the header's own rule */
} h2y_scene_stats;

/* The signatures of n_frames device frames of d: scope, planes, alignment and floor / ceiling exactly as h2y_lightdist_batch takes
 * them; out[f] (host memory).  Launches of up to H2Y_SCENESIG_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them,
 * h2y_last_kernel_name "k_scenesig"); synchronous. */
int h2y_scenesig_batch(h2y_ctx *ctx, const h2y_desc *d, int n_frames, const void *const *d_planes, h2y_scenesig *out);

/* The signatures of n_frames device frames of PQ codes: scope, layout and refusals exactly as h2y_codelight_batch takes them (4:2:0
 * chroma upsampled by k_up444 into the same scratch); out[f] (host memory).  Launches of up to H2Y_CODELIGHT_FRAMES_PER_LAUNCH
 * frames (h2y_last_kernel_name "k_codescenesig"); synchronous. */
int h2y_codescenesig_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int n_frames, const uint16_t *const *d_frames, h2y_scenesig *out);

/* Arm an open ring before its first input: a forward ring wherever h2y_stream_lightdist is accepted, with its return values
 * (k_scenesig then runs after k_lightdist on the same decoded planes: behind h2y_stream_gamut / _tonemap the converted ones), or the
 * ring of h2y_codelight_stream_open (k_codescenesig on the planes k_codelight read).  Any other ring is H2Y_EINVAL.  The output
 * bytes and every other stage's results do not change. */
int h2y_stream_scenesig(h2y_ctx *ctx);
/* The signature of the frame that h2y_stream_output returned last. */
int h2y_stream_scenesig_result(h2y_ctx *ctx, h2y_scenesig *out);
/* The H2Y_LIGHTDIST_BINS bins of the frame that h2y_stream_output returned last, on a ring armed with h2y_stream_lightdist or opened
 * by h2y_codelight_stream_open with want_dist (they come down with the frame for its percentiles); H2Y_EINVAL on a ring that does
 * not measure the distribution. */
int h2y_stream_lightdist_bins(h2y_ctx *ctx, uint32_t *bins);

/* The four functions below are host only: no device, no context. */

/* D of two signatures; -1 for a null argument, zero pixels or differing pixels. */
double h2y_scene_distance(const h2y_scenesig *a, const h2y_scenesig *b);
/* scene_id[f] of n frames from their signatures; returns the number of scenes, 0 for n < 1, a null pointer, or a threshold that is
 * negative or not finite (a pair whose distance is -1 opens no scene). */
int h2y_scene_cuts(const h2y_scenesig *sig, int n, double threshold, int32_t *scene_id);
/* The figures of the scenes of n_frames frames: stats[f] and bins[f x H2Y_LIGHTDIST_BINS] as h2y_lightdist_batch returns them,
 * scene_id[f] as h2y_scene_cuts does (0 first, then equal to the frame before or one more).  Returns the number of scenes and writes
 * the first min(that, cap) of them to out (out may be NULL when cap is 0); 0 for a null stats, bins or scene_id, n_frames < 1, a
 * negative cap, scene ids of any other form, or a frame without pixels. */
int h2y_scene_merge(const h2y_lightdist_stats *stats, const uint32_t *bins, const int32_t *scene_id, int n_frames, h2y_scene_stats *out,
                    int cap);
/* h2y_lightdist_json's text for scenes: its layout and slot convention, one SceneInfo entry per frame and line, every entry of scene
 * s carrying the scene's figures with "SceneId": s, "SceneFrameIndex" counting from 0 inside the scene, "SequenceFrameIndex" running
 * on from first_frame_index, and "SceneFirstFrameIndex" / "SceneFrameNumbers" listing every scene.  Sizing and refusals as
 * h2y_lightdist_json (0 for null scenes, n_scenes < 1, a negative first_frame_index, a scene without pixels or frames); scenes that do
 * not tile [0, N) in order return 0.  As there, no encoder's parser has checked the layout. */
size_t h2y_lightdist_json_scenes(const h2y_scene_stats *scenes, int n_scenes, long first_frame_index, char *buf, size_t cap);

/* ---- linearised PQ code planes: a finished PQ master as a LINEAR G,B,R F32 source of the forward flow (--linearize 1) ------------
 * Nothing in the arithmetic is new.  The output is three binary32 planes G, B, R of width x height that hold L_G, L_B, L_R exactly as
 * steps 1-4 of "light of PQ code planes" above define them, in that order: 4:2:0 chroma upsampled by k_up444 in the form `algorithm`
 * and the context's inverse chroma siting select; the normalisation; the matrix, every operation rounded by itself; the clamp to
 * [+0, 1]; PQ10000_f through light1<true>'s tiers; the clamp again.  Where k_codelight keeps m = max(L_G, L_B, L_R) of a pixel,
 * k_linearize writes the three lights (both call the one function of h2y_codepixel.h).  The values lie in [+0, 1], 1.0 = 10000
 * cd/m2: what k_gamut, k_tonemap, k_light and the forward kernels take as a LINEAR (transfer 8) G,B,R (matrix 0) F32 source.  Their
 * floor and ceiling are 0 and 1 by stats_override: measured pic_stats of such planes are 0 / 0 whenever no sample reaches 1.0. */
#define H2Y_LINEARIZE_FRAMES_PER_LAUNCH 8 /* h2y_codelight_batch's rule: the launch's 4:2:0 scratch is the same one */

/* n_frames device frames of d, taken as h2y_codelight_batch takes them, into d_planes_out[f x 3 + c]: plane c = G, B, R of frame
 * f, width x height binary32 each, 16-byte aligned, the layout h2y_light_batch, h2y_gamut_batch and h2y_convert_batch read.
 * Launches of up to H2Y_LINEARIZE_FRAMES_PER_LAUNCH frames, each k_up444 per 4:2:0 frame and then one k_linearize
 * (h2y_last_kernel_ms sums them, upsampling included; h2y_last_kernel_name "k_linearize"; the variant names the matrix and the
 * upsampling form, e.g. "k_linearize<BT2020NC,FIR>"); synchronous.  Refusals word for word h2y_codelight_batch's, and H2Y_EINVAL
 * for an output plane that is null or not 16-byte aligned. */
int h2y_linearize_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int n_frames, const uint16_t *const *d_frames, void *const *d_planes_out);

/* A forward ring whose decode is the linearisation, beside h2y_dpx_stream_open, h2y_tiff_stream_open and h2y_exr_stream_open:
 * h2y_stream_input lends planes[0] for the code frame of src (its three planes one after the other, as above), the device runs
 * k_up444 (4:2:0; one scratch of the context serves every slot) and k_linearize into the slot's three planes, and from there the
 * ring is h2y_stream_open's on an F32 source: every arming entry works on it as on the DPX ring.  The inverse chroma siting is read
 * when the ring opens.  Refusals: src as h2y_codelight_batch; H2Y_EINVAL unless d describes that source -- in_sample_type
 * H2Y_SAMPLE_F32, src_transfer 8, src_matrix 0, width and height of src, stats_override 1 with floor 0 and ceiling 1 -- and for a
 * depth outside 2..16. */
int h2y_pqcode_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_codelight_desc *src, int depth);

/* ---- Delta E ITP of PQ code planes: the visible difference (Rec. ITU-R BT.2124) of a PQ picture from a reference (--delta_e 1) -----
 * PSNR and SSIM judge code values; this judges what is seen: 720 x the Euclidean distance in ICtCp with T = Ct / 2, where 1.0 is about
 * one just-noticeable difference.  The reference has nothing here: it is the project's own definition, every step in binary32.
 * Two frames A and B of one geometry, each exactly what h2y_codelight_desc describes: three u16 code planes at bit depth 8..16, video or
 * full range, matrix_coeffs 0, 1 or 9, chroma_format_idc 3, or 1 with even sizes, `algorithm` for the 4:2:0 upsampler.  The transfer is
 * PQ; the planes are taken as BT.2020 primaries (the entries take no primaries: the caller checks them).
 * Per pixel, for A and for B alike:
 *   1. Steps 1-4 of "light of PQ code planes" give L_G, L_B, L_R in [+0, 1] (code_lights<MATRIX>, h2y_codepixel.h), 4:2:0 chroma first
 *      upsampled by k_up444 in the form `algorithm` and the context's inverse chroma siting select.
 *   2. LMS (BT.2100), every product and every sum rounded by itself to binary32, left to right, no fused multiply-add; the constants
 *      are k / 4096, exact in binary32; with R = L_R, G = L_G, B = L_B:
 *        l = ((1688/4096) R + (2146/4096) G) + (262/4096) B
 *        m = ((683/4096) R + (2951/4096) G) + (462/4096) B
 *        s = ((99/4096) R + (309/4096) G) + (3688/4096) B
 *      each then v > 0 ? min(v, 1) : +0.  Every row adds up to 4096/4096 and the inputs are <= 1, so by monotone rounding no value exceeds
 *      1; the clamp is kept so that the table tiers never see anything else.
 *   3. l' = PQ10000_r(l), m' and s' likewise: the binary32 value the forward conversion's own tiers give for that argument (the
 *      H2Y_TFN_PQ_R table, the full-range table, the careful tier: pixel_fast()'s destination stage).  PQ10000_r(+0) = 7.3e-7, not 0.
 *   4. ITP, every constant exact in binary32, every product and sum rounded by itself, left to right:
 *        I = 0.5 l' + 0.5 m'
 *        T = ((6610/8192) l' - (13613/8192) m') + (7003/8192) s'      (= Ct / 2)
 *        P = ((17933/4096) l' - (17390/4096) m') - (543/4096) s'      (= Cp)
 *   5. dI = I_A - I_B, dT and dP likewise;  d = 720 x sqrt((dI dI + dT dT) + dP dP), every operation rounded by itself, the square
 *      root the correctly rounded IEEE one.  d is finite, never negative, and below 2^13.
 * Per frame, all exact integers, independent of the order of the work and of the GPU count:
 *   pixels = width x height;  sum_q = the sum over the pixels of rint(d x 2^20) (the product is exact; a term is at most 2^33, a 2^28-
 *   pixel frame stays below 2^61) in uint64;  max_bits = the largest d as a binary32 bit pattern and (max_x, max_y) the first pixel in
 *   raster order that holds it;  over = the pixels with d > threshold, strictly, threshold a binary32 of the caller's.
 *   mean = ((double)sum_q x 2^-20) / pixels and max = (double)d_max are conveniences computed on the host in binary64.
 * Anchors (10-bit video range, Cb = Cr = 512): Y against Y + 1 gives d = 0.822 (720 / 876) anywhere on the scale; Y 64 against Y 940
 * gives 720. */
#define H2Y_DELTAE_FRAMES_PER_LAUNCH 4 /* a launch's 4:2:0 scratch: 4 planes x 2 bytes x width x height x 4 pairs -- 253 MiB at 3840 x 2160 */

typedef struct h2y_deltae_stats {
    uint32_t max_bits;     /* the largest d of the frame, as binary32 bits */
    uint32_t max_x, max_y; /* the first pixel in raster order that holds it */
    float threshold;       /* the caller's */
    uint64_t sum_q;        /* sum over the pixels of rint(d x 2^20) */
    uint64_t pixels;       /* width x height */
    uint64_t over;         /* pixels with d > threshold */
    double mean;           /* (sum_q x 2^-20) / pixels */
    double max;            /* the largest d */
} h2y_deltae_stats;

/* Delta E ITP of n_frames pairs of device frames of d: d_a[f] and d_b[f] each hold a frame's three planes one after the other from a
 * 16-byte aligned base, as h2y_codelight_batch takes them; out[f] (host memory).  Launches of up to H2Y_DELTAE_FRAMES_PER_LAUNCH
 * pairs, each k_up444 twice per 4:2:0 pair (four upsampled chroma planes a pair, in a scratch area the context owns) and then one
 * k_deltae (h2y_last_kernel_ms sums them, upsampling included; h2y_last_kernel_name "k_deltae"; the variant names the matrix and the
 * upsampling form, e.g. "k_deltae<BT2020NC,FIR>"); synchronous.  Refusals word for word h2y_codelight_batch's, and H2Y_EINVAL for a
 * threshold that is NaN or negative. */
int h2y_deltae_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, float threshold, int n_frames, const uint16_t *const *d_a,
                     const uint16_t *const *d_b, h2y_deltae_stats *out);

/* Arm a ring that h2y_stream_compare or h2y_compare_stream_open has armed, before its first input, beside h2y_stream_ssim and the
 * histogram: k_deltae then runs on every slot's device frame (A) and its reference twin (B), on the kernel stream after k_compare and
 * k_ssim; the output bytes and every other stage's results do not change.  d must agree with the ring's frame -- size and chroma
 * format, and where the ring knows them bit depth, range and matrix_coeffs 0 exactly where its planes are G, B, R -- otherwise
 * H2Y_EINVAL.  The stage owns one scratch for the four upsampled planes (stream order makes one enough); the inverse chroma siting is
 * read here.  H2Y_EINVAL on a ring not armed for comparison (the histogram-only and scale-only rings among them) and on the light-only
 * ring; d's and the threshold's refusals as h2y_deltae_batch. */
int h2y_stream_deltae(h2y_ctx *ctx, const h2y_codelight_desc *d, float threshold);
/* Delta E ITP of the frame that h2y_stream_output returned last. */
int h2y_stream_deltae_result(h2y_ctx *ctx, h2y_deltae_stats *out);

/* ---- scaling: an exact Lanczos resampler (--dst_pic_width / --dst_pic_height; the reference's cv.cpp is compiled out) ------------
 * The reference plugs a per-plane Lanczos cv::resize in at hdr2yuv.cpp:892-896, in a file that does not compile; it defines no
 * bytes.  This is the project's own definition, in integers, so that a restatement checks every output byte.
 * Frame and target: three u16 planes in the comparison's geometry (4:2:0 Y, Cb, Cr; 4:4:4 Y, Cb, Cr or G, B, R).  Every plane
 * is resampled on its own from (sw, sh) to (dw, dh); the chroma planes of a 4:2:0 frame from (sw/2, sh/2) to (dw/2, dh/2).  Sample
 * centres are aligned (the 2x2-centre siting of the box filter is kept; chroma_sample_loc_type is not consulted).
 * Tap table of one axis, s source samples -> d output samples, a in {2, 3, 4} lobes, all in binary64 on the host:
 *   f = max(1, s/d), r = a f, and for output o the centre c = ((o + 0.5) x s) / d - 0.5 (the product, exact, then one division);
 *   taps: the integers i with ceil(c - r) <= i <= floor(c + r) and |i - c| < r;
 *   w_i = sinc(t) sinc(t/a) with t = (i - c)/f, sinc(x) = sin(pi x)/(pi x), sinc(0) = 1;  S = the w_i added left to right;
 *   q_i = rint(w_i 16384 / S) (the product first, then the division);  16384 - sum q_i is added to the largest q_i (the first one
 *   on ties);
 *   edges replicate: the q_i of a tap outside [0, s-1] is added to the tap at the clamped index; `first` is the lowest clamped
 *   index; the row is first, the tap count n and n int16 coefficients.
 *   A row whose stored coefficients have sum |q| > 32767 makes the call fail with H2Y_EUNSUPPORTED (none occurs in the
 *   tested ratios).
 * Pixel:  H(y, x) = sum_i qh[x][i] src(y, first_h[x] + i), an exact int32 (sum |q| x 65535 < 2^31);
 *         V(y, x) = sum_j qv[y][j] H(first_v[y] + j, x) in int64;
 *         output = clamp((V + 2^27) >> 28, lo, hi), an arithmetic shift: one rounding per sample, none in between, so the answer
 *         does not depend on tiling or on the order of the passes.
 *   lo..hi is set_pic_clip()'s range of the plane at the frame's depth -- write_yuv()'s per-plane clamp, the rule
 *   h2y_histogram_batch documents: [0, maxCV] in full range; in video range [minVR, maxVR] for plane 0 and every plane of a G, B, R
 *   frame (gbr 1), [minVRC, maxVRC] for planes 1 and 2 of a YCbCr frame.
 * Limits: each axis ratio s/d in [1/4, 4] (at most 32 taps); widths and heights 2..10000, even for 4:2:0, on both sides;
 * chroma_format_idc 1 or 3 (2: H2Y_EUNSUPPORTED); bit_depth 8..16; a 2..4. */
#define H2Y_SCALE_FRAMES_PER_LAUNCH 64
#define H2Y_SCALE_TAPS 32 /* coefficients per row of h2y_scale_taps' table */

/* The table of one axis.  Host only: no device, no context.  first[o], count[o] (dst entries each) and coef[o x 32 + i] (dst x 32;
 * zero past count[o]); *max_taps (may be NULL) the largest count.  H2Y_EINVAL for sizes, a ratio or an `a` out of the limits. */
int h2y_scale_taps(int src, int dst, int a, int32_t *first, int32_t *count, int16_t *coef /* dst x 32 */, int *max_taps);

/* Bytes of one frame of three u16 planes of this geometry (0 for an unsupported one). */
size_t h2y_scale_frame_bytes(int width, int height, int chroma_format_idc);

/* k_scale on n_frames device frames in h2y_compare_batch's layout (three planes one after the other from a 16-byte aligned base):
 * d_dst[f] receives d_src[f] resampled from src_w x src_h to dst_w x dst_h.  The tables are built on the host and uploaded once
 * per call.  Launches of up to H2Y_SCALE_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them, h2y_last_kernel_name
 * "k_scale"); synchronous. */
int h2y_scale_batch(h2y_ctx *ctx, int src_w, int src_h, int dst_w, int dst_h, int chroma_format_idc, int bit_depth, int full_range,
                    int gbr, int a, int n_frames, const uint16_t *const *d_src, uint16_t *const *d_dst);

/* Arm an open forward ring (h2y_stream_open, h2y_dpx_stream_open, h2y_tiff_stream_open, h2y_exr_stream_open) before its first
 * input: after the conversion of a slot k_scale runs on the slot's device output, on the kernel stream, and the scaled frame
 * (dst_w x dst_h, the descriptor's dst_chroma_format_idc, dst_bit_depth and dst_full_range, YCbCr limits) is what goes down and
 * what h2y_stream_output returns.  h2y_stream_light beside it is unaffected.  H2Y_EINVAL on an inverse, compare-only,
 * histogram-only or scale-only ring; H2Y_EUNSUPPORTED on a ring armed with h2y_stream_compare / _histogram / _ssim, as is arming any
 * of those on a scale-armed ring. */
int h2y_stream_scale(h2y_ctx *ctx, int dst_w, int dst_h, int a);

/* A scale-only ring: no conversion.  h2y_stream_input lends the frame's three planes one after the other, h2y_stream_output
 * returns the scaled frame. */
int h2y_scale_stream_open(h2y_ctx *ctx, int src_w, int src_h, int chroma_format_idc, int bit_depth, int full_range, int gbr, int dst_w,
                          int dst_h, int a, int depth /* 2..16 slots */);

/* ---- dither: the reduction to the output bit depth (--dither; "TEMPORAL DITHERING -- dither" is an open entry of the reference's
 * to-do list, and the reference itself only cuts: (unsigned int) in matrix_convert(), a plain >> in write_yuv()) --------------------
 * There are no bytes of the reference to match: this is the project's own definition, in integers, so that a restatement checks
 * every output bit.
 * A frame of three u16 planes at a working depth W is reduced to depth D; the geometry is h2y_scale_batch's (4:2:0 or 4:4:4,
 * planes one after the other).  The shift is s = W - D with 1 <= s <= 8 and 8 <= D < W <= 16.  All arithmetic is uint32 with
 * wrap-around.  For sample v at (x, y) of plane p (coordinates within that plane) of frame number n:
 *   mix(a):  a ^= a >> 16;  a *= 0x7FEB352D;  a ^= a >> 15;  a *= 0x846CA68B;  a ^= a >> 16
 *   fi = temporal ? n : 0
 *   kf = mix((seed ^ 0x9E3779B9) + fi)
 *   kp = mix(kf + p)
 *   mode 0 (library only, "cut"):  t = 0
 *   mode 1 (ordered):  ox = kp & 15,  oy = (kp >> 4) & 15
 *                      t = B((x + ox) & 15, (y + oy) & 15) >> (8 - s)
 *   mode 2 (noise):    t = mix(mix(kp + y) + x) & (2^s - 1)
 *   out = min(max((uint32(v) + t) >> s, lo), hi)
 * B is the 16 x 16 ordered matrix, defined without a table: with a = x ^ y, bit i (0..3) of a goes to bit 2 (3 - i) + 1 of B and
 * bit i of y to bit 2 (3 - i).  Anchors: mix(0) = 0, mix(1) = 0x688990C0; rows y = 0..3, columns x = 0..3 of B are
 * 0 128 32 160 / 192 64 224 96 / 48 176 16 144 / 240 112 208 80.
 * lo..hi is write_yuv()'s per-plane clamp at depth D, the rule h2y_scale_batch documents: [0, 2^D - 1] in full range; in video
 * range [16 << (D-8), 235 << (D-8)] for plane 0 and every plane of a G, B, R frame (gbr 1), [16 << (D-8), 240 << (D-8)] for planes
 * 1 and 2 otherwise.
 * Ordered mode: every aligned 16 x 16 tile of B holds 0..255 once, and B >> (8 - s) each of the 2^s levels 256 / 2^s times, so on a
 * constant plane v the outputs of any 16 x 16 tile add up to exactly 256 v / 2^s: the mean is kept exactly.  Noise mode is uniform
 * and keeps the mean in expectation.  The value of a W-bit code is taken as v / 2^s: in full range 65535 >> 6 is 1023, and 2^16
 * does not map onto 2^10 - 1 exactly; that is the definition, not a defect.
 * For a U16 source the reference converts at the source's depth and shifts: the conversion with dst_bit_depth = W followed by
 * mode 0 to D (gbr 0) is byte for byte the conversion with dst_bit_depth = D.  For float and half sources no such identity holds
 * (at 16 bits the matrix's +0.5 rounds before the floor): there the definition is "the frame converted at 16 bits, then reduced". */
#define H2Y_DITHER_FRAMES_PER_LAUNCH 64

/* t of every sample of one plane, t[y x width + x].  Host only: no device, no context; the CPU-testable twin of k_dither.
 * H2Y_EINVAL for a mode outside 0..2, a shift outside 1..8, temporal not 0 / 1, a plane outside 0..2, sizes below 1, a null t. */
int h2y_dither_offsets(int mode, int shift, int temporal, uint32_t seed, uint32_t frame, int plane, int width, int height, uint16_t *t);

/* k_dither on n_frames device frames in h2y_scale_batch's layout (three planes one after the other from a 16-byte aligned base):
 * d_dst[f] receives d_src[f] reduced from src_depth to dst_depth as frame number first_frame + f; d_dst[f] may be d_src[f] (in
 * place; no other overlap).  Launches of up to H2Y_DITHER_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them,
 * h2y_last_kernel_name "k_dither", the variant "k_dither<ordered>", "<noise>" or "<cut>"); synchronous.  H2Y_EUNSUPPORTED for
 * 4:2:2; H2Y_EINVAL for depths outside 8 <= dst < src <= 16 or more than 8 bits apart, odd 4:2:0 sizes, sizes below 1 or of 2^28
 * pixels and more, null or misaligned frames, while a batch is pending or a stream open. */
int h2y_dither_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int src_depth, int dst_depth, int full_range, int gbr,
                     int mode, int temporal, uint32_t seed, uint32_t first_frame, int n_frames, const uint16_t *const *d_src,
                     uint16_t *const *d_dst);

/* Arm an open forward ring (plain, DPX, TIFF, EXR, PQ code) before its first input: after a slot's conversion -- and after
 * k_scale on a ring armed with h2y_stream_scale before this call, at the scaled size -- k_dither reduces the frame that would go
 * down, from the descriptor's dst_bit_depth to dst_depth with the YCbCr limits (gbr 0), into a frame of its own, which goes down
 * and is what h2y_stream_output returns.  The k-th submitted frame has number first_frame + k.  H2Y_EUNSUPPORTED on a ring armed
 * with h2y_stream_compare / _histogram / _ssim / _deltae, as is arming any of those afterwards (they would see the undithered
 * frame), and on dst_matrix_coeffs 15; H2Y_EINVAL on every other kind of ring, after the first input, on a ring armed already, and
 * for h2y_stream_scale after this call. */
int h2y_stream_dither(h2y_ctx *ctx, int dst_depth, int mode, int temporal, uint32_t seed, uint32_t first_frame);

/* A dither-only ring: no conversion.  h2y_stream_input lends the frame's three planes one after the other, h2y_stream_output
 * returns the reduced frame. */
int h2y_dither_stream_open(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int src_depth, int dst_depth, int full_range, int gbr,
                           int mode, int temporal, uint32_t seed, uint32_t first_frame, int depth /* 2..16 slots */);

/* ---- sample packings: byte and semi-planar frames (--dst_pack, --src_pack) ----------------------------------------------------------
 * Every raw frame above is the reference's write_yuv() form: three planes of 16-bit little-endian words ("planar16").  Encoders and
 * hardware codecs read other forms of the same samples; these are the project's own definitions of three of them, in integers.
 * A frame is three planes P0, P1, P2 of u16 codes at bit depth D, M = 2^D - 1.  P0 is w x h; P1 and P2 are cw x ch with
 * cw = w >> 1, ch = h >> 1 for 4:2:0 and cw = w, ch = h for 4:4:4 (h2y_scale_batch's layout: the planes one after the other).
 * 4:2:2 is refused as everywhere.
 *   0  H2Y_PACK_PLANAR16  every depth and format: the form above.  Packing and unpacking refuse it (H2Y_EINVAL); the command line
 *                         reads it as "no packing".
 *   1  H2Y_PACK_PLANAR8   D = 8, 4:2:0 or 4:4:4: P0, P1, P2, one byte a sample, rows without padding: w h + 2 cw ch bytes
 *   2  H2Y_PACK_NV12      D = 8, 4:2:0: P0 as bytes, then ch rows of cw byte pairs (P1[i], P2[i]): w h + 2 cw ch bytes
 *   3  H2Y_PACK_P010      D = 10..16, 4:2:0: P0 as little-endian u16 words, then ch rows of cw word pairs (P1[i], P2[i]), the sample
 *                         in a word's high bits: 2 (w h + 2 cw ch) bytes
 * Pack: the byte is min(v, M); P010's word is min(v, M) << (16 - D).  The library's own frames never exceed M; a caller's buffer
 * may, and here such a code saturates.  Unpack: v = the byte; for P010 v = word >> (16 - D), the low 16 - D bits ignored (decoders
 * differ in what they leave there).  So unpack(pack(x)) = min(x, M); pack(unpack(y)) = y for packings 1 and 2, and y with the low
 * 16 - D bits of every word cleared for packing 3.
 * As an ffmpeg -pix_fmt (the command line's banner): packing 1 is yuv420p or yuv444p, packing 2 nv12, packing 3 p010le, p012le or
 * p016le at D = 10, 12, 16 and has no such name at the other depths; planar16 is yuv420p10le and the like. */
enum { H2Y_PACK_PLANAR16 = 0, H2Y_PACK_PLANAR8 = 1, H2Y_PACK_NV12 = 2, H2Y_PACK_P010 = 3 };
#define H2Y_PACK_FRAMES_PER_LAUNCH 64

/* The bytes of one packed frame (the table's last column); 0 for packing 0, an unknown packing, a chroma format the packing does
 * not take (4:2:2 among them) and sizes below 1.  The depth does not enter. */
size_t h2y_pack_frame_bytes(int width, int height, int chroma_format_idc, int packing);

/* One frame on the host: no device, no context; the CPU-testable twins of k_pack and k_unpack, compiled from the same per-sample
 * lines.  src and dst must not overlap.  H2Y_EINVAL for a null pointer, sizes below 1 or of 2^28 pixels and more, packing 0 and
 * every (chroma format, bit_depth, packing) the table does not list; H2Y_EUNSUPPORTED for 4:2:2. */
int h2y_pack_frame(int width, int height, int chroma_format_idc, int bit_depth, int packing, const uint16_t *src, void *dst);
int h2y_unpack_frame(int width, int height, int chroma_format_idc, int bit_depth, int packing, const void *src, uint16_t *dst);

/* k_pack / k_unpack on n_frames device frames: d_dst[f] receives d_src[f] packed (unpacked).  The planar16 side is in
 * h2y_scale_batch's layout; both frames start on 16-byte boundaries (the planes inside them need not: the kernels take no access
 * wider than its address's alignment).  A frame's source and destination must not overlap; that is not checked.  Launches of up to
 * H2Y_PACK_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them, h2y_last_kernel_name "k_pack" / "k_unpack", the variant
 * "k_pack<PLANAR8>", "<NV12>" or "<P010>"); synchronous.  The refusals of h2y_pack_frame, and H2Y_EINVAL for n_frames below 1, null
 * or misaligned frames, while a batch is pending or a stream open. */
int h2y_pack_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int bit_depth, int packing, int n_frames,
                   const uint16_t *const *d_src, void *const *d_dst);
int h2y_unpack_batch(h2y_ctx *ctx, int width, int height, int chroma_format_idc, int bit_depth, int packing, int n_frames,
                     const void *const *d_src, uint16_t *const *d_dst);

/* Arm an open ring that hands out a u16 .yuv frame, before its first input: a forward ring (plain, DPX, TIFF, EXR, code), the
 * scale-only ring or the dither-only ring.  The ring's last stage, after h2y_stream_scale's and h2y_stream_dither's: k_pack packs
 * the frame that would go down -- the conversion's, the scale stage's or the dither stage's, at that frame's depth D -- into a frame
 * of the stage's own, which goes down and is what h2y_stream_output returns: the pointer's type stays, and on such a ring it points
 * to h2y_pack_frame_bytes bytes.  H2Y_EINVAL for packing 0 or an unknown one, a packing the frame's depth or chroma format does not
 * take, after the first input, on a ring armed already, and for h2y_stream_scale / h2y_stream_dither after this call;
 * H2Y_EUNSUPPORTED on a ring armed with h2y_stream_compare / _histogram / _ssim / _deltae, as is arming any of those afterwards
 * (compare or count the written file instead), on dst_matrix_coeffs 15, and on every ring whose output is no .yuv frame (inverse,
 * compare-only, histogram-only, light-only). */
int h2y_stream_pack(h2y_ctx *ctx, int packing);

/* Arm an open ring whose h2y_stream_input lends u16 code planes, before its first input: the inverse rings, the planes rings
 * (compare-only, histogram-only, scale-only, dither-only, h2y_codelight_stream_open) and the three code rings (h2y_pqcode_ /
 * h2y_hlgcode_ / h2y_sdrcode_stream_open).  From then on h2y_stream_input lends one packed frame (h2y_pack_frame_bytes bytes) in
 * planes[0], planes[1] = planes[2] = null, as the payload rings do; only those bytes go up, and k_unpack writes the planes where the
 * upload would have put them, before the ring's producer and every stage: all that follows sees the same planes.  On the
 * compare-only ring the reference h2y_stream_reference lends is packed the same way.  D is the ring's input depth.  H2Y_EINVAL for
 * packing 0 or an unknown one, a packing the ring's input depth or chroma format does not take, H2Y_PACK_P010 on a compare-only ring
 * (whose depth is unknown: h2y_stream_unpack_ex takes it), after the first input, on a ring armed already, and on rings whose input is not u16 code planes (float
 * and half forward rings, DPX / TIFF / EXR rings); H2Y_EUNSUPPORTED on a forward ring opened on U16 planes (the reference's integer
 * .yuv -> .yuv flow stays the reference's). */
int h2y_stream_unpack(h2y_ctx *ctx, int packing);

/* The same with the frames' bit depth given: what a compare-only ring, which does not know it, needs for H2Y_PACK_P010 (A and the
 * reference are both shifted down by 16 - bit_depth, so the comparison sees codes of that depth).  bit_depth 0: the ring's own, as
 * h2y_stream_unpack.  H2Y_EINVAL for a negative bit_depth and for one that differs from the depth a ring knows. */
int h2y_stream_unpack_ex(h2y_ctx *ctx, int packing, int bit_depth);

/* ---- conversion between colour primaries, in linear light, before the forward conversion (--gamut_convert 1) ---------------------
 * The reference parses --src_colour_primaries / --dst_colour_primaries and never converts between them: matrix_to_primaries() is an
 * empty function (convert.cpp:1991), and the two values only choose between the identity and the colour-difference branch of
 * matrix_convert() (convert.cpp:1159-1160).  That behaviour is kept, bit for bit, by everything above.  This is the project's own
 * definition of the missing step: a pass over the decoded source planes, after which the unchanged forward conversion writes the
 * bytes it would write had the source file held the converted planes.
 * Primaries (colour_primaries codes, hdr.h:95-105, and H.273's 12), CIE 1931 x/y:
 *    1        BT.709   R .640/.330  G .300/.600  B .150/.060
 *    8 and 9  BT.2020  R .708/.292  G .170/.797  B .131/.046
 *   12        P3-D65   R .680/.320  G .265/.690  B .150/.060
 *   10        XYZ      the planes hold X, Y, Z: the normalised primary matrix is the identity
 *   The RGB sets share the D65 white .3127/.3290; there is no chromatic adaptation.  Any other code is H2Y_EUNSUPPORTED (11, P3 with
 *   the DCI white, included); a pair of equal chromaticities (s == d, or 8 and 9) is H2Y_EINVAL: there is nothing to convert.
 * Matrix: M = NPM(dst)^-1 NPM(src), row-major, on column vectors (R, G, B) -- (X, Y, Z) for code 10.  NPM is the normalised primary
 *   matrix of SMPTE RP 177: its columns are the XYZ of the primaries, scaled so that R = G = B = 1 gives the white with Y = 1.
 *   Each of the nine entries is the exact rational value rounded to nearest binary32; an entry whose exact value is 0 is +0.0 (709 and
 *   P3 share the blue primary).  So the matrix does not depend on how it is computed.
 * Pixel: planes 0 = G (Y), 1 = B (Z), 2 = R (X), so v = (p2, p0, p1).  A half is widened to binary32 (exact).
 *   o_i = ((m[i][0] v0) + (m[i][1] v1)) + (m[i][2] v2): every multiply and add its own binary32 round-to-nearest operation, in that
 *   order, no fused multiply-add; subnormal inputs and results are kept.
 *   clip 1: o_i = o_i > 0 ? o_i : +0.0 (negatives, -0.0 and NaN become +0.0; +inf stays).  clip 0: the sums as they are; a NaN result
 *   is some NaN.
 *   p0' = o_1, p1' = o_2, p2' = o_0.  F32 is stored as is; F16 is rounded to nearest even (overflow gives inf).  The sample type
 *   does not change. */
#define H2Y_GAMUT_FRAMES_PER_LAUNCH 64

/* The matrix of a pair of primaries.  Host only: no device, no context.  `why` (may be NULL) receives a static string. */
int h2y_gamut_matrix(int src_primaries, int dst_primaries, float m[9], const char **why);

/* k_gamut on n_frames device frames of width x height: d_src[f*3 + c] / d_dst[f*3 + c] are plane c = G, B, R of frame f, 16-byte
 * aligned; a d_dst entry may equal its d_src entry (in place; no other overlap).  sample_type H2Y_SAMPLE_F32 or H2Y_SAMPLE_F16
 * (H2Y_SAMPLE_U16: H2Y_EUNSUPPORTED), clip 0 or 1.  Launches of up to H2Y_GAMUT_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums
 * them, h2y_last_kernel_name "k_gamut"); synchronous. */
int h2y_gamut_batch(h2y_ctx *ctx, int width, int height, int sample_type, int src_primaries, int dst_primaries, int clip, int n_frames,
                    const void *const *d_src, void *const *d_dst);

/* Arm an open forward ring whose decoded planes are float or half (h2y_stream_open with F32 or F16 planes, h2y_dpx_stream_open,
 * h2y_exr_stream_open) before its first input: k_gamut then runs in place on every slot's decoded device planes, on the context's
 * stream, after the decode and before pic_stats, so the floor, the ceiling, the conversion and h2y_stream_light beside it see the
 * converted planes.  The primaries are the arguments, not the descriptor's: no field of h2y_desc changes meaning.
 * H2Y_EUNSUPPORTED where the planes are U16 (the TIFF ring, a U16 plain ring), where src_transfer is not 8 (LINEAR) or src_matrix not
 * 0 (G, B, R), and for unsupported primaries; H2Y_EINVAL on an inverse, compare-only, histogram-only or scale-only ring, after the
 * first input, on a ring armed already, for equal chromaticities and a clip other than 0 or 1. */
int h2y_stream_gamut(h2y_ctx *ctx, int src_primaries, int dst_primaries, int clip);

/* ---- gamut compression: out-of-gamut colours rolled off, not clipped (--gamut_convert 1 --gamut_compress 1) ------------------------
 * The conversion above clips at 0: a saturated colour of the source loses the detail of its smallest channels, and its hue moves,
 * because one channel stops while the other two go on.  This pass does the same matrix and, in the same trip through memory, brings
 * the channels that the matrix left far below the pixel's largest channel back above 0 along a smooth curve.  It stands where
 * h2y_stream_gamut's pass stands, in its place.  The reference has no such step: this is the project's own definition, as the
 * conversion, tone mapping and the LUT are.
 * The model is the distance-from-achromatic form of the ACES 1.3 Reference Gamut Compression: per pixel a = max(R, G, B) is the
 * achromatic axis, per channel d = (a - c) / a is the distance from it (0 on the axis, 1 at the destination gamut's boundary, above
 * 1 outside), and a curve C brings the distances t .. l onto t .. 1 while those below t stay.  The limits l come from the source
 * primaries, not from camera gamuts.
 * Parameters, both binary32: the threshold t, 0.5 <= t <= 0.95, and the power p, 1 <= p <= 4; every formula below takes their
 *   exact values.  H2Y_GAMUT_COMPRESS_THRESHOLD and _POWER are the defaults: choices in the range ACES uses, no measurements.
 * Host, in binary64; each operation as written, pow is the C library's:
 *   1. M = h2y_gamut_matrix(src, dst), nine binary32 entries, widened.
 *   2. Limits.  For each of the six corners x of the source cube, in the order (1,0,0) (0,1,0) (0,0,1) (0,1,1) (1,0,1) (1,1,0):
 *      o_i = ((m[i][0] x0) + (m[i][1] x1)) + (m[i][2] x2), a = max(o0, o1, o2), d_i = (a - o_i) / a.  The limit of channel i is the
 *      largest d_i of the six, rounded once to binary32: l_i.  From here on l_i is that binary32 value, widened.
 *   3. A channel with l_i <= 1 has no curve: its scale and its table are zeros, and the pixel rule clips it at 0 as k_gamut does.
 *   4. For a channel with a curve: w = l - t,  s = w / pow(pow((1 - t) / w, -p) - 1, 1 / p),
 *      C(u) = t + u / pow(1 + pow(u / s, p), 1 / p) for a distance t + u, so that C(0) = t and C(w) = 1.
 *   5. Table: H2Y_GAMUT_COMPRESS_NODES = 1025 binary32 entries, T[k] = C((w k) / 1024) rounded once, but T[0] = t and T[1024] = 1
 *      exactly.  Scale: k = 1024 / w, rounded once to binary32.
 *   XYZ (code 10) on either side is H2Y_EUNSUPPORTED: a cube of XYZ has no gamut to take limits from.
 * Pixel, in binary32; a half is widened first (exact).  Every product, sum, difference and quotient is one round-to-nearest
 *   operation in the order written, no fused multiply-add; subnormals are kept:
 *   1. o_i as h2y_gamut_batch's pixel computes them, without its clip.
 *   2. An o_i that is a NaN becomes +0.0, one that is +inf becomes the largest finite binary32 (-inf stays: it is a negative).
 *   3. a = max(max(o_0, o_1), o_2).  Where a is not above 0, all three outputs are +0.0.
 *   4. Otherwise, per channel, d = (a - o_i) / a:
 *      d <= t: the output is o_i, bit for bit (the largest channel has d = 0: it never changes);
 *      otherwise, a channel without a curve: o_i where o_i > 0, else +0.0 -- the clip;
 *      otherwise, d >= l_i: +0.0;
 *      otherwise x = (d - t) k_i, n = min((int)x, 1023), f = x - n, cd = T_i[n] + (T_i[n + 1] - T_i[n]) f, v = a - cd a,
 *      and the output is v where v > 0, else +0.0.
 *   p0' = out_1, p1' = out_2, p2' = out_0.  F32 is stored as is; F16 is rounded to nearest even.  The sample type does not change.
 * What follows: no output is negative or a NaN, whatever the input; greys and every colour within the threshold keep their bits;
 *   max(R, G, B) of a pixel is what h2y_gamut_batch with clip 1 leaves (but for step 2: there +inf stays +inf); each channel's map is
 *   continuous at t and at l and does not decrease.  The six corners are not the extremes of d over the whole cube: between two
 *   corners d passes l (0.8 % of uniformly random BT.2020 pixels going to BT.709 in a numpy prototype), and such a channel is +0.0,
 *   continuously, as the clip leaves it.  Where no channel has a curve (BT.709 -> BT.2020) the pass equals h2y_gamut_batch with
 *   clip 1 but for step 2's +inf: a NaN becomes +0.0 in both, a sum of +inf stays there and is the largest finite binary32 here (in
 *   an F16 plane that is +inf again).
 * With the defaults the interpolated table stays within 2^-18 of C on every channel of 9 -> 1, 12 -> 1 and 9 -> 12. */
#define H2Y_GAMUT_COMPRESS_NODES 1025
#define H2Y_GAMUT_COMPRESS_THRESHOLD 0.8f
#define H2Y_GAMUT_COMPRESS_POWER 1.2f
#define H2Y_GAMUT_COMPRESS_FRAMES_PER_LAUNCH 64

typedef struct h2y_gamut_compress_tables {
    float m[9];                                /* h2y_gamut_matrix's */
    float threshold, power;                    /* as given */
    float limit[3];                            /* R, G, B: l_i; a curve where it is above 1 */
    float scale[3];                            /* k_i; 0 without a curve */
    float table[3][H2Y_GAMUT_COMPRESS_NODES];  /* T_i; zeros without a curve */
} h2y_gamut_compress_tables;

/* The matrix, the limits, the scales and the tables of a pair of primaries.  Host only: no device, no context.  `why` (may be NULL)
 * receives a static string.  H2Y_EINVAL for a null out, a threshold or power out of range or not finite and for what
 * h2y_gamut_matrix refuses so; H2Y_EUNSUPPORTED for XYZ on either side and for what h2y_gamut_matrix refuses so. */
int h2y_gamut_compress_curve(int src_primaries, int dst_primaries, float threshold, float power, h2y_gamut_compress_tables *out,
                             const char **why);

/* The pass on host planes, k_gamut_compress' CPU twin: src[c] / dst[c] are plane c = G, B, R of npix samples of sample_type
 * H2Y_SAMPLE_F32 or H2Y_SAMPLE_F16 (anything else: H2Y_EUNSUPPORTED); dst[c] may be src[c].  Host only. */
int h2y_gamut_compress_planes(int src_primaries, int dst_primaries, float threshold, float power, int sample_type, size_t npix,
                              const void *const src[3], void *const dst[3]);

/* k_gamut_compress on n_frames device frames of width x height, as h2y_gamut_batch takes them: d_src[f*3 + c] / d_dst[f*3 + c] are
 * plane c = G, B, R of frame f, 16-byte aligned; a d_dst entry may equal its d_src entry (in place; no other overlap).  sample_type
 * H2Y_SAMPLE_F32 or H2Y_SAMPLE_F16 (H2Y_SAMPLE_U16: H2Y_EUNSUPPORTED).  Launches of up to H2Y_GAMUT_COMPRESS_FRAMES_PER_LAUNCH frames
 * (h2y_last_kernel_ms sums them, h2y_last_kernel_name "k_gamut_compress"); synchronous. */
int h2y_gamut_compress_batch(h2y_ctx *ctx, int width, int height, int sample_type, int src_primaries, int dst_primaries, float threshold,
                             float power, int n_frames, const void *const *d_src, void *const *d_dst);

/* Arm an open forward ring as h2y_stream_gamut arms it, on the same kinds of ring, with k_gamut_compress in k_gamut's place: in
 * place on every slot's decoded device planes, after the decode, before h2y_stream_tonemap's, h2y_stream_lut3d's, h2y_stream_hlg's
 * and h2y_stream_ictcp's passes, pic_stats and the conversion.  A ring takes one of the two gamut stages: H2Y_EINVAL on a ring armed
 * with either already, and after the first input.  Otherwise h2y_stream_gamut's refusals, and h2y_gamut_compress_curve's. */
int h2y_stream_gamut_compress(h2y_ctx *ctx, int src_primaries, int dst_primaries, float threshold, float power);

/* ---- gamut containment of PQ code planes: how much of a finished PQ master lies outside a narrower primaries set (--light_only 1
 * --gamut_check 1) -------------------------------------------------------------------------------------------------------------------
 * An HDR10 file is coded in BT.2020 primaries and is almost always required to stay inside P3-D65, the mastering display's gamut;
 * before an SDR rung is cut the same question is asked of BT.709.  This section counts, per frame, the pixels whose colour lies
 * outside a check set, and by how much.  It is the project's own definition: the reference has nothing to match.
 * Frame: exactly what "light of PQ code planes" takes: h2y_codelight_desc, matrix_coeffs 0, 1, 9 and 14, 4:4:4 or 4:2:0 with the
 *   context's inverse chroma siting.  The file's primaries F are 1, 8 / 9 or 12.  Between one and H2Y_GAMUTCHECK_MAX_SETS check sets
 *   C_s, each one of 1, 8 / 9, 12, with chromaticities different from F's and from each other's.  XYZ (10) on either side is
 *   H2Y_EUNSUPPORTED; everything else is refused as h2y_gamut_matrix refuses it.
 *   1. Steps 1-4 of "light of PQ code planes" give L_G, L_B, L_R in [+0, 1]; m = max(L_G, L_B, L_R), as there.
 *   2. Per set, M = h2y_gamut_matrix(F, C_s).  For i in R, G, B: v_i = (M[3i] L_R + M[3i+1] L_G) + M[3i+2] L_B, every product and
 *      sum rounded to binary32 by itself: k_gamut's row form.
 *   3. lo = min(v_R, v_G, v_B); the excursion is e = lo < 0 ? -lo : +0.  No NaN can arise.  For the known sets the negative entries
 *      of a row sum to at least -0.67, so e < 1, e x 2^32 is exact and rint(e x 2^32) <= 2^32.
 *   4. Two classes.  A pixel is outside when e > 0.  It is beyond when e > t m (one binary32 product) and e > a, where t = (float)T
 *      and a = (float)(A / 10000.0), the division done in binary64 and rounded once.  T is `ratio`, 0 <= T <= 1, by default
 *      H2Y_GAMUTCHECK_RATIO; A is `floor` in cd/m2, A >= 0, by default H2Y_GAMUTCHECK_FLOOR.
 *   5. Per frame and set, every figure an exact integer, whatever the order of the work: pixels, outside, beyond; the largest e as
 *      its binary32 bits with the first pixel that holds it (the key (bits(e) << 32) | ~index, as content light keeps its peak; the
 *      position is (-1, -1) when outside is 0); sum_q = the sum over all pixels of rint(e x 2^32).  The host finishes, in binary64:
 *      max_cdm2 = 10000 x e_max, mean_cdm2 = ((10000 x (double)sum_q) x 2^-32) / pixels (over all the frame's pixels), beyond_share =
 *      beyond / pixels.
 * Why two classes.  A strict count is useless on real files: colours that lie exactly on the BT.709 or P3-D65 boundary, expressed in
 *   BT.2020 and coded as 10-bit video-range BT.2020nc, come back strictly outside their own gamut about half of the time, by
 *   quantisation alone -- by up to 0.68 cd/m2 at 10-100 cd/m2 and 5.9 cd/m2 at 100-1000 cd/m2, yet by no more than 1.9 % of the
 *   pixel's largest channel above 1 cd/m2 and no more than 0.016 cd/m2 below it.  Hence a relative tolerance and an absolute floor,
 *   and the strict count reported beside the tolerant one.  With the defaults none of such boundary colours is beyond its own set
 *   (tests/test_gamutcheck_host.py repeats the experiment on the binary32 path), and the BT.2020 primaries, cyan and magenta are
 *   beyond P3-D65 and BT.709 at 1, 100 and 1000 cd/m2.  BT.2020 yellow sits 1.7 % from P3-D65's yellow edge: it is outside P3-D65 and
 *   not beyond it.  The defaults are choices from that experiment; they have not been tuned on real programmes.
 * The out-of-gamut pixels that 4:2:0 chroma upsampling itself creates at saturated edges are counted, as they are in the picture a
 *   display shows. */
#define H2Y_GAMUTCHECK_MAX_SETS 2
#define H2Y_GAMUTCHECK_RATIO 0.02
#define H2Y_GAMUTCHECK_FLOOR 0.02

typedef struct h2y_gamutcheck_set {
    int32_t  primaries;          /* the check set's code, as given */
    int32_t  max_x, max_y;       /* the first pixel, in raster order, that holds the largest excursion; (-1, -1) when outside is 0 */
    uint32_t max_bits;           /* the largest excursion, as binary32 bits (units of 10000 cd/m2) */
    uint64_t outside, beyond;    /* pixels with e > 0; with e > t m and e > a */
    uint64_t sum_q;              /* sum over the frame's pixels of rint(e x 2^32) */
    double   max_cdm2, mean_cdm2, beyond_share;
} h2y_gamutcheck_set;

typedef struct h2y_gamutcheck_stats {
    uint64_t pixels;             /* width x height */
    int32_t  n_sets, reserved;
    h2y_gamutcheck_set set[H2Y_GAMUTCHECK_MAX_SETS]; /* the first n_sets, in the order given; the rest zeros */
} h2y_gamutcheck_stats;

/* The check from step 2 on, on host light planes such as h2y_linearize_batch writes: lights[c] is plane c = G, B, R of width x height
 * binary32 samples in [+0, 1]; a sample outside that range, a NaN included, is H2Y_EINVAL (step 3's e < 1 rests on it), and *out is
 * then left as it was.  k_gamutcheck's CPU twin.  Host only: no device, no context.  H2Y_EINVAL for n_sets outside
 * 1..H2Y_GAMUTCHECK_MAX_SETS, a set of the file's chromaticities or listed twice, a ratio that is not finite or outside [0, 1], a
 * floor that is negative or not finite, a bad size and null arguments; H2Y_EUNSUPPORTED for XYZ (10), code 11 and every other
 * unknown code. */
int h2y_gamutcheck_planes(int file_primaries, int n_sets, const int *sets, double ratio, double floor, int width, int height,
                          const float *const lights[3], h2y_gamutcheck_stats *out);

/* The check of n_frames device frames of d, laid out and refused exactly as h2y_codelight_batch takes them; out[f] (host memory).
 * Launches of up to H2Y_CODELIGHT_FRAMES_PER_LAUNCH frames, each k_up444 per 4:2:0 frame and then one k_gamutcheck (h2y_last_kernel_ms
 * sums them, upsampling included; h2y_last_kernel_name "k_gamutcheck"; the variant names the matrix, the number of sets and the
 * upsampling form, e.g. "k_gamutcheck<BT2020NC,2,FIR>"); synchronous.  The check's own refusals as h2y_gamutcheck_planes. */
int h2y_gamutcheck_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int file_primaries, int n_sets, const int *sets, double ratio,
                         double floor, int n_frames, const uint16_t *const *d_frames, h2y_gamutcheck_stats *out);

/* Arm the ring of h2y_codelight_stream_open before its first input: k_gamutcheck then runs directly behind k_codelight, on the planes
 * that kernel read (the slot's upsampled chroma included).  Every other ring is H2Y_EINVAL, and so is arming twice.  The light, the
 * distribution and the scene signature of the ring do not change. */
int h2y_stream_gamutcheck(h2y_ctx *ctx, int file_primaries, int n_sets, const int *sets, double ratio, double floor);
/* The check of the frame that h2y_stream_output returned last. */
int h2y_stream_gamutcheck_result(h2y_ctx *ctx, h2y_gamutcheck_stats *out);

/* ---- tone mapping: the light of an HDR master brought down to a target peak, in linear light (--tone_map 1) ----------------------
 * The reference has no tone mapper (its README sends the user to ctlrender), so there are no bytes to match: this is the project's
 * own definition, as scaling, primaries, siting and the light figures are.  A pass over the decoded source planes, after
 * h2y_stream_gamut where both are armed, after which the unchanged forward conversion writes the bytes it would write had the
 * source file held the mapped planes.
 * The curve is the EETF of Rep. ITU-R BT.2390 with both black levels at 0, applied to m = max(R, G, B); the three samples of a
 * pixel are scaled by one gain, so their ratios (the hue) are kept.  A source sample of 1.0 is 10000 cd/m2, as the PQ path assumes.
 * Parameters: integers S (the source's mastering peak) and D (the target's peak) in cd/m2, 100 <= D < S <= 10000, and `relative`:
 *   1: the output is display-referred, 1.0 = D (for BT.1886 / rho-gamma destinations); 0: it stays in units of 10000 cd/m2 (PQ).
 * The curve, in binary64 on the host.  N is the ST 2084 inverse EOTF,
 *     N(L) = ((c1 + c2 L^m1) / (1 + c3 L^m1))^m2,   N^-1(V) = (max(V^(1/m2) - c1, 0) / (c2 - c3 V^(1/m2)))^(1/m1),
 *     m1 = 2610/16384, m2 = 2523/4096 x 128, c1 = 3424/4096, c2 = 2413/4096 x 32, c3 = 2392/4096 x 32.
 *   W = N(S/10000), maxLum = N(D/10000) / W, KS = 1.5 maxLum - 0.5.  For a light e:
 *     E1 = min(N(e) / W, 1);
 *     E2 = E1 where E1 < KS; otherwise, with t = (E1 - KS) / (1 - KS), the Hermite spline
 *          E2 = (2t^3 - 3t^2 + 1) KS + (t^3 - 2t^2 + t) (1 - KS) + (-2t^3 + 3t^2) maxLum;
 *     T(e) = N^-1(E2 W);   u = D/10000 if relative, else 1;   1/u is computed as 10000.0 / D (relative) or is 1;
 *     the gain g(e) = 1/u where E1 < KS -- exactly the identity below the knee, no round trip through pow -- and
 *     g(e) = T(e) / (e u) elsewhere.
 * The table: H2Y_LIGHTDIST_BINS = 8706 binary32 gains on the nodes of the light distribution's bins (above): entry 0 is 1/u
 *   (everything below 2^-17 is far below any knee: the lowest, S = 10000 and D = 100, lies near 6 cd/m2); entry k, 1 <= k <= 8705,
 *   is g at the float whose bits are H2Y_LIGHTDIST_FIRST_BITS + ((k - 1) << 14), so entry 8705 is g(1.0); each is rounded once to
 *   binary32.  cap = 1.0f if relative, else D/10000 rounded once.
 * Pixel, in binary32; a half is widened first (exact).  Every product, difference and sum is one round-to-nearest operation, no
 *   fused multiply-add:
 *   1. for each of G, B, R: c' = c > 0 ? min(c, 1) : +0.0 (NaN, -0.0 and negatives become +0.0, +inf becomes 1);
 *   2. m = max(max(G', B'), R'), its bits e, k = the bin of e: 0 when e < 0x37000000, else min(((e - 0x37000000) >> 14) + 1, 8705);
 *   3. gain = table[0] for k = 0, table[8705] for k = 8705; otherwise, with t = float(e & 0x3FFF) x 2^-14 (exact),
 *      gain = table[k] + (table[k + 1] - table[k]) t;
 *   4. out_c = min(c' gain, cap).  In binary64 m g(m) reaches 1 + 1e-9 at the peak: the min is part of the definition.
 *   F32 is stored as is; F16 is rounded to nearest even.  The sample type does not change.
 * On (S, D) = (1000, 100), (4000, 1000), (10000, 100), (1000, 600) T is monotone, the gains do not increase with e, and the
 * interpolation between nodes stays within 1e-6 (relative) of the exact curve; the binary32 pixel arithmetic adds its roundings. */
#define H2Y_TONEMAP_FRAMES_PER_LAUNCH 64

/* The table and the cap of a pair of peaks.  Host only: no device, no context.  gain receives H2Y_LIGHTDIST_BINS floats; `why` (may
 * be NULL) receives a static string.  H2Y_EINVAL for a null gain or cap, peaks outside 100 <= dst_peak < src_peak <= 10000 and a
 * `relative` other than 0 or 1. */
int h2y_tonemap_curve(int src_peak, int dst_peak, int relative, float gain[H2Y_LIGHTDIST_BINS], float *cap, const char **why);

/* k_tonemap on n_frames device frames of width x height: d_src[f*3 + c] / d_dst[f*3 + c] are plane c = G, B, R of frame f, 16-byte
 * aligned; a d_dst entry may equal its d_src entry (in place; no other overlap).  sample_type H2Y_SAMPLE_F32 or H2Y_SAMPLE_F16
 * (H2Y_SAMPLE_U16: H2Y_EUNSUPPORTED); a bad size, null or unaligned planes, peaks or `relative` out of range, a pending batch or an
 * open stream: H2Y_EINVAL.  Launches of up to H2Y_TONEMAP_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them,
 * h2y_last_kernel_name "k_tonemap", the variant "k_tonemap<F32,RELATIVE>" .. "k_tonemap<F16,ABSOLUTE>"); synchronous. */
int h2y_tonemap_batch(h2y_ctx *ctx, int width, int height, int sample_type, int src_peak, int dst_peak, int relative, int n_frames,
                      const void *const *d_src, void *const *d_dst);

/* Arm an open forward ring whose decoded planes are float or half (h2y_stream_open with F32 or F16 planes, h2y_dpx_stream_open,
 * h2y_exr_stream_open) before its first input, once: k_tonemap then runs in place on every slot's decoded device planes, on the
 * context's stream, after the decode and after h2y_stream_gamut's or h2y_stream_gamut_compress' pass where one of the two is armed
 * (whichever was armed first) -- so it sees the converted, clipped or compressed planes, and no channel leaves [0, cap] in the
 * destination's primaries -- and before the conversion;
 * h2y_stream_light and h2y_stream_lightdist beside it measure the mapped light.
 * The ring must have been opened with stats_override 1, floor 0 and ceiling 1 on all three planes (H2Y_EINVAL otherwise): mapped
 * planes are referred to their target by definition, and the measured pic_stats of such a frame -- (int)max, 0 below 1.0 -- would
 * normalise them by a zero range.
 * H2Y_EUNSUPPORTED where the planes are U16 (the TIFF ring, a U16 plain ring) and where src_transfer is not 8 (LINEAR) or src_matrix
 * not 0 (G, B, R); H2Y_EINVAL on an inverse, compare-only, histogram-only, scale-only or light-only ring, after the first input, on
 * a ring armed already, and for peaks or a `relative` out of range. */
int h2y_stream_tonemap(h2y_ctx *ctx, int src_peak, int dst_peak, int relative);

/* ---- 3D LUT: a .cube table applied to the decoded source planes (--lut3d FILE.cube) ------------------------------------------------
 * The reference has no LUT step, so there are no bytes to match: this is the project's own definition, as primaries, tone mapping,
 * scaling and dither are.  A pass over the decoded source planes, after h2y_stream_gamut's and h2y_stream_tonemap's where those are
 * armed and before h2y_stream_hlg's / h2y_stream_ictcp's, after which the unchanged forward conversion writes the bytes it would
 * write had the source file held the planes this pass leaves.
 * The table: N nodes per axis, 2 <= N <= 128; per channel c of (r, g, b) a domain lo_c < hi_c, finite binary32; N^3 nodes of three
 *   finite binary32 values in .cube file order, r fastest, then g, then b.  On the host, per channel,
 *   s_c = (N - 1) / (hi_c - lo_c), evaluated in binary64 and rounded once to binary32.
 * Pixel, in binary32.  Planes are 0 = G, 1 = B, 2 = R, so x_r = p2, x_g = p0, x_b = p1; a half is widened first (exact).  Every
 *   difference, product and sum is one round-to-nearest operation, never contracted into a fused multiply-add:
 *   1. t_c = (x_c - lo_c) s_c; then t_c = t_c > 0 ? min(t_c, float(N - 1)) : +0.0 (NaN, -0.0 and everything below the domain go to
 *      the first node, +inf and everything above to the last);
 *   2. i_c = (int)t_c (truncation, 0 .. N - 1), j_c = min(i_c + 1, N - 1), f_c = t_c - float(i_c) (exact, in [0, 1)).  The upper
 *      neighbour is clamped, not the cell: an input exactly on a node, the last one included, has f = 0 and returns that node's
 *      values exactly (i = min((int)t, N - 2) does not at the domain's maximum);
 *   3. interp 1, tetrahedral (the default): the path is chosen by these comparisons exactly as written, ties take the else -- in
 *      rounded arithmetic the paths differ, so the comparisons are part of the definition:
 *          f_r > f_g ? (f_g > f_b ? rgb : (f_r > f_b ? rbg : brg))
 *                    : (f_b > f_g ? bgr : (f_b > f_r ? gbr : grb))
 *      for a path (a1, a2, a3): P0 is the node (i_r, i_g, i_b), P1 is P0 with axis a1 moved to its j, P2 is P1 with a2 moved too, P3
 *      is (j_r, j_g, j_b); per output channel v = ((P0 + (P1 - P0) f_a1) + (P2 - P1) f_a2) + (P3 - P2) f_a3.
 *      interp 0, trilinear, with lerp(a, b, w) = a + (b - a) w: four lerps along r, two along g, one along b;
 *   4. signal 0 ("planes"): o_c = v_c.  The sample type does not change: F32 is stored as is, F16 is rounded to nearest even.  The
 *      LUT's output stands where the source file's samples stood, in the source's transfer and normalisation;
 *   5. signal 1 ("signal"): the LUT's output is the destination's R'G'B' signal in [0, 1]: v_c = v_c > 0 ? min(v_c, 1) : +0.0, then
 *      step 6 of "HLG" below with the same four constants mulY, addY, mulC, addC, derived the same way from dst_bit_depth,
 *      dst_full_range and dst_matrix (0 or 9): o_G = v_g mulY + addY, o_B = v_b mulC + addC, o_R = v_r mulC + addC, product first, then
 *      sum.  The outputs are F32 whatever the input type.  The ring is the passthrough one (equal transfers), which takes
 *      code-valued planes straight to its matrix (convert.cpp:930, :1012);
 *   6. p0' = o_g, p1' = o_b, p2' = o_r.
 * With M = max |node| and D = the largest difference between neighbouring nodes, either interpolation stays within
 * 2^-24 (16 M + 12 (N - 1) D) of its evaluation in binary64: at most 15 rounded operations of magnitude <= M on the value path, and
 * three index roundings of relative 2^-24 on each of three axes. */
#define H2Y_LUT3D_FRAMES_PER_LAUNCH 64

typedef struct h2y_lut3d h2y_lut3d; /* a parsed table; host memory only */

/* Parse the `len` bytes of a .cube file.  Host only: no device, no context.  Read: '#' comments, blank lines, LF or CRLF, blanks and
 * tabs; TITLE "...", DOMAIN_MIN r g b, DOMAIN_MAX r g b (default 0 0 0 and 1 1 1), LUT_3D_SIZE N, Resolve's LUT_3D_INPUT_RANGE lo hi
 * (the same domain on all three channels), then N^3 rows of three numbers, scientific notation included, values outside [0, 1]
 * allowed.  Refused, with `why` (may be NULL) receiving a reason that stays valid until the calling thread's next call:
 * LUT_1D_SIZE / LUT_1D_INPUT_RANGE (1D LUTs and shaper + 3D files: H2Y_EUNSUPPORTED); H2Y_EINVAL for an unknown keyword, a keyword
 * after the first row, a missing or repeated size, N outside 2..128, too few or too many rows, a row with other than three numbers,
 * a value that is not finite, and hi_c <= lo_c.  On success *lut owns the table until h2y_lut3d_free. */
int h2y_lut3d_parse(const char *text, size_t len, h2y_lut3d **lut, const char **why);
void h2y_lut3d_free(h2y_lut3d *lut);
/* N, the domain (lo_r, lo_g, lo_b, hi_r, hi_g, hi_b) and the title (the table's own memory); each may be NULL */
int h2y_lut3d_info(const h2y_lut3d *lut, int *n, float domain[6], const char **title);
/* the 3 N^3 node values as parsed, in file order */
int h2y_lut3d_nodes(const h2y_lut3d *lut, float *rgb);

/* The pass on npix pixels in host memory: k_lut3d's host twin, compiled from the same per-pixel lines.  src[c] / dst[c] are plane
 * c = G, B, R; sample_type H2Y_SAMPLE_F32 or H2Y_SAMPLE_F16 (else H2Y_EUNSUPPORTED); dst holds the source's type in planes mode
 * and floats in signal mode.  dst_bit_depth (8..16), dst_full_range and dst_matrix (0 or 9) are read in signal mode only. */
int h2y_lut3d_planes(const h2y_lut3d *lut, int interp, int signal, int dst_bit_depth, int dst_full_range, int dst_matrix, int sample_type,
                     size_t npix, const void *const src[3], void *const dst[3]);

/* k_lut3d on n_frames device frames of width x height: d_src[f*3 + c] / d_dst[f*3 + c] are plane c = G, B, R of frame f, 16-byte
 * aligned; a d_dst entry may equal its d_src entry (in place; no other overlap) but for F16 planes in signal mode, whose float
 * output needs room of its own.  The table is uploaded once per call.  sample_type H2Y_SAMPLE_F32 or H2Y_SAMPLE_F16
 * (H2Y_SAMPLE_U16: H2Y_EUNSUPPORTED); a bad size, null or unaligned planes, a null lut, an interp or signal other than 0 or 1, a
 * pending batch or an open stream: H2Y_EINVAL.  Launches of up to H2Y_LUT3D_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums
 * them, h2y_last_kernel_name "k_lut3d", the variant "k_lut3d<F32,TETRA,PLANES>" .. "k_lut3d<F16,TRILINEAR,SIGNAL>", or "k_lut3d_lds<...>" for a
 * table of up to 17 nodes per axis, which the blocks read from a copy in LDS unless h2y_ctx_set_option "lut3d_lds" is "0": the
 * same bytes either way); synchronous. */
int h2y_lut3d_batch(h2y_ctx *ctx, int width, int height, int sample_type, const h2y_lut3d *lut, int interp, int signal, int dst_bit_depth,
                    int dst_full_range, int dst_matrix, int n_frames, const void *const *d_src, void *const *d_dst);

/* Arm an open forward ring whose decoded planes are float or half (h2y_stream_open with F32 or F16 planes, h2y_dpx_stream_open,
 * h2y_exr_stream_open, h2y_pqcode_stream_open, h2y_hlgcode_stream_open) before its first input, once: k_lut3d then runs in place on
 * every slot's decoded device planes, on the context's stream, after h2y_stream_gamut's and h2y_stream_tonemap's passes where those
 * are armed (whichever was armed first), before h2y_stream_hlg's / h2y_stream_ictcp's, before pic_stats and the conversion;
 * h2y_stream_light and h2y_stream_lightdist beside it measure what the LUT left.  The table is copied to the device here; `lut` may
 * be freed once the call returns.
 * The ring must have src_matrix 0 (H2Y_EUNSUPPORTED otherwise) and stats_override 1, floor 0 and ceiling 1 on all three planes
 * (H2Y_EINVAL otherwise), for h2y_stream_tonemap's reason.  signal 1 takes the ring's dst_bit_depth, dst_full_range and dst_matrix
 * and also needs F32 planes and equal transfers (the passthrough descriptor; H2Y_EUNSUPPORTED otherwise); it conflicts with
 * h2y_stream_hlg and h2y_stream_ictcp in either arming order (H2Y_EINVAL), because each of them leaves code values.
 * H2Y_EUNSUPPORTED where the planes are U16; H2Y_EINVAL on an inverse, compare-only, histogram-only, scale-only, dither-only or
 * light-only ring, after the first input, and on a ring armed already. */
int h2y_stream_lut3d(h2y_ctx *ctx, const h2y_lut3d *lut, int interp, int signal);

/* ---- HLG: display light written as a Hybrid Log-Gamma signal (ARIB STD-B67, Rec. ITU-R BT.2100; --hlg 1) --------------------------
 * The reference has no HLG transfer (its transfer list ends at TRANSFER_RHO_GAMMA, and its code 18 is that, not H.273's HLG), so
 * there are no bytes to match: this is the project's own definition, as tone mapping's is.  It is Rep. ITU-R BT.2408's conversion
 * of display light to HLG at a nominal peak: the inverse OOTF with the system gamma of that peak and no black lift, then the OETF,
 * both from BT.2100, non-constant luminance.  A pass over the decoded source planes, after h2y_stream_gamut's and
 * h2y_stream_tonemap's where those are armed, which leaves CODE-VALUED floats: the conversion's own scale step is part of the pass.
 * The ring is opened with equal transfers, and the unchanged forward conversion then takes the planes straight to its matrix
 * (convert.cpp:930, :1012), the chroma resampler and write_yuv, as it does for any source whose transfer is the destination's.
 * Input: planes G, B, R of display light in BT.2020 primaries.
 * Parameters: an integer peak L_W in cd/m2, 400 <= L_W <= 2000 -- the range over which BT.2100 gives
 *   gamma = 1.2 + 0.42 log10(L_W / 1000); outside it the Recommendation uses another formula, so other peaks are refused --,
 *   `relative`: 1: the planes are display-referred, 1.0 = L_W (what h2y_stream_tonemap leaves for a destination that is not PQ);
 *   0: 1.0 = 10000 cd/m2,
 *   and four binary32 scale constants mulY, addY, mulC, addC: the conversion's own, what it derives from the descriptor's
 *   dst_bit_depth, dst_full_range and dst_matrix for its scale step (convert.cpp:1123-1145).  The HLG rung therefore has the scale
 *   step of the PQ rungs, the reference's habit of scaling B' and R' by the chroma range in video range included: that
 *   is kept here on purpose, so that an HLG rung and a PQ rung of one run differ in the transfer alone.
 * Host, binary64: gamma as above, p = (1 - gamma) / gamma; k = 10000 / L_W rounded once to binary32 (`relative` 0), or 1;
 *   the OETF's constants a = 0.17883277, b = 1 - 4a, c = 0.5 - a ln(4a).
 *   Two tables of H2Y_LIGHTDIST_BINS = 8706 binary32 entries on the nodes tone mapping uses: node j >= 1 is the float whose bits
 *   are H2Y_LIGHTDIST_FIRST_BITS + ((j - 1) << 14); every entry is rounded once to binary32:
 *     gain[j] = node_j^p for j >= 1, and gain[0] = 256^-p: the factor of the reads below the first node, where the table is read
 *       at 256 Y, since Y^p = (256 Y)^p 256^-p.  The nodes then reach down to 2^-25 of L_W (3e-5 cd/m2 at 1000): a pure blue of
 *       2^-17 has Y = 2^-21.1.  The inverse OOTF's gain grows without bound towards black; below 2^-25 of L_W it is held constant.
 *       That is part of the definition.
 *     oetf[j] = a ln(12 node_j - b) + c for every node >= 2^-4, and 0 below (never read: the logarithmic branch starts above 1/12);
 *       oetf[8705] rounds to 1.0f.
 * Pixel, in binary32; a half is widened first (exact).  Every product, sum and difference is one round-to-nearest operation, never
 *   contracted into a fused multiply-add:
 *   1. for each of G, B, R: c' = c > 0 ? min(c, 1) : +0.0 (NaN, -0.0 and negatives become +0.0, +inf becomes 1), then
 *      s = min(c' k, 1);
 *   2. Y = ((0.2627f s_R) + (0.6780f s_G)) + (0.0593f s_B);
 *   3. the table read R(x) at x's bits e, x >= 2^-17, is tone mapping's steps 2-3: the bin is min(((e - 0x37000000) >> 14) + 1,
 *      8705); R = gain[8705] in bin 8705, otherwise, with t = float(e & 0x3FFF) x 2^-14 (exact),
 *      R = gain[bin] + (gain[bin + 1] - gain[bin]) t.  For Y >= 2^-17 (its bits >= 0x37000000) g = R(Y).  Otherwise Y' = 256 Y
 *      (exact), g' = R(Y') where Y' >= 2^-17 and gain[1] below, and g = g' gain[0], one more product;
 *   4. E_c = min(s_c g, 1).  The min is part of the definition: display light such as pure blue at the peak has a scene light of
 *      1.6 and lies outside what an HLG signal can carry;
 *   5. E'_c = sqrt(3.0f E_c), the correctly rounded square root, for E_c <= 1/12 (the binary32 nearest to it); otherwise oetf
 *      interpolated at E_c's bits the same way; then min(E'_c, 1);
 *   6. out_G = E'_G mulY + addY, out_B = E'_B mulC + addC, out_R = E'_R mulC + addC: the product, then the sum.
 *   The outputs are F32 whatever the source's sample type: a half cannot hold code-valued samples.
 * Accuracy: for greys, the three primaries and the three secondaries whose plane value runs over [2^-17, 1] (both modes; peaks
 * 400, 1000 and 2000) E' stays within 0.012 of a 16-bit video-range luma step, 1 / (219 x 256), of the BT.2100 formulas evaluated
 * in binary64 (tests/test_hlg_host.py holds it to half a step). */
#define H2Y_HLG_FRAMES_PER_LAUNCH 64
#define H2Y_HLG_PEAK_MIN 400
#define H2Y_HLG_PEAK_MAX 2000

/* The two tables, k and gamma of a peak.  Host only: no device, no context.  gain and oetf receive H2Y_LIGHTDIST_BINS floats each;
 * `why` (may be NULL) receives a static string.  H2Y_EINVAL for a null gain, oetf, k or gamma, a peak outside 400..2000 and a
 * `relative` other than 0 or 1. */
int h2y_hlg_tables(int peak, int relative, float gain[H2Y_LIGHTDIST_BINS], float oetf[H2Y_LIGHTDIST_BINS], float *k, double *gamma,
                   const char **why);

/* The pixel function on planes in host memory: the host twin of k_hlg, which compiles the same lines (csrc/h2y_hlg1.h).  Host only.
 * src[c] / dst[c]: plane c = G, B, R of npix samples, sample_type H2Y_SAMPLE_F32 or H2Y_SAMPLE_F16 in, binary32 out; a dst plane
 * may be its F32 src plane.  The scale constants are those of (dst_bit_depth 8..16, dst_full_range 0 / 1, dst_matrix 0 / 9).
 * H2Y_EINVAL for null planes and parameters out of range, H2Y_EUNSUPPORTED for another sample type or dst_matrix. */
int h2y_hlg_planes(int peak, int relative, int dst_bit_depth, int dst_full_range, int dst_matrix, int sample_type, size_t npix,
                   const void *const src[3], float *const dst[3]);

/* k_hlg on n_frames device frames of width x height: d_src[f*3 + c] / d_dst[f*3 + c] are plane c = G, B, R of frame f, 16-byte
 * aligned; the destination planes are F32.  With H2Y_SAMPLE_F32 a d_dst entry may equal its d_src entry (in place; no other
 * overlap); with H2Y_SAMPLE_F16 the planes are widened, and in place is refused (H2Y_EINVAL).  H2Y_SAMPLE_U16 and a dst_matrix
 * other than 0 (G,B,R) and 9 (BT.2020nc): H2Y_EUNSUPPORTED; a bad size, null or unaligned planes, a peak, `relative`,
 * dst_bit_depth (8..16) or dst_full_range out of range, a pending batch or an open stream: H2Y_EINVAL.  Launches of up to
 * H2Y_HLG_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them, h2y_last_kernel_name "k_hlg", the variant
 * "k_hlg<F32,RELATIVE>" .. "k_hlg<F16,ABSOLUTE>"); synchronous. */
int h2y_hlg_batch(h2y_ctx *ctx, int width, int height, int sample_type, int peak, int relative, int dst_bit_depth, int dst_full_range,
                  int dst_matrix, int n_frames, const void *const *d_src, void *const *d_dst);

/* Arm an open forward ring whose decoded planes are F32 (h2y_stream_open with F32 planes, h2y_dpx_stream_open,
 * h2y_pqcode_stream_open) before its first input, once: k_hlg then runs in place on every slot's decoded device planes, on the
 * context's stream, after h2y_stream_gamut's and h2y_stream_tonemap's passes where those are armed (whichever was armed first), and
 * before the conversion.  The scale constants are the ring's descriptor's.
 * The descriptor must be the passthrough flow's: src_matrix 0, dst_matrix 0 or 9, src_transfer == dst_transfer == 8, and
 * stats_override 1 with floor 0 and ceiling 1 on all three planes (what h2y_stream_tonemap beside it needs of the source side).
 * (dst_matrix 0 goes with src_primaries == dst_primaries: no ring opens on another such descriptor, h2y_desc_check refuses it as
 * the reference does, "can't determine color difference to use", convert.cpp:1195-1197.)
 * h2y_stream_light and h2y_stream_lightdist refuse such a ring: their light is PQ's, and its dst_transfer is not 16.
 * H2Y_EUNSUPPORTED where the planes are F16 or U16 (the EXR ring, .f16 planes, the TIFF ring: a half cannot hold code-valued
 * samples) and for other transfers or matrices; H2Y_EINVAL on the other ring kinds, after the first input, on a ring armed
 * already, without that statistics override, and for a peak or a `relative` out of range. */
int h2y_stream_hlg(h2y_ctx *ctx, int peak, int relative);

/* ---- light of HLG code planes: a finished HLG master as a LINEAR G,B,R F32 source of the forward flow (--linearize 1 --src_hlg 1) ---
 * The way back from the section above: the OETF's inverse and the OOTF of Rec. ITU-R BT.2100 at a stated display peak, non-constant
 * luminance, no black lift.  The project's own definition, as "HLG" is: the reference has no HLG transfer, so there are no bytes to
 * match.  With a PQ destination it is Rep. ITU-R BT.2408's conversion of HLG to PQ (at 1000 cd/m2: --src_hlg_peak 1000).
 * Frame: exactly what h2y_codelight_desc describes ("light of PQ code planes" above): three u16 code planes at bit_depth 8..16,
 *   video or full range; matrix_coeffs 0, 1 or 9; chroma_format_idc 3, or 1 with even sizes (not with matrix 0); `algorithm` and the
 *   context's inverse chroma siting select the upsampler.  The transfer is HLG, always.
 * Parameter: an integer display peak L_W in cd/m2, H2Y_HLG_PEAK_MIN <= L_W <= H2Y_HLG_PEAK_MAX; gamma = 1.2 + 0.42 log10(L_W / 1000)
 *   as above, in binary64.
 * Host, binary64, every entry rounded once to binary32: two tables of H2Y_LIGHTDIST_BINS entries on the nodes of "HLG",
 *     ootf[j] = node_j^(gamma - 1) for j >= 1, and ootf[0] = 256^-(gamma - 1), the factor of the reads below the first node;
 *     inv[j] = (exp((node_j - c) / a) + b) / 12 for every node >= 2^-1 -- 513 entries, from node index 16 x 512 + 1 = 8193 up -- and 0
 *       below (never read: the exponential branch starts above 0.5).  inv[8193] is the binary32 nearest to 1/12, which is also
 *       (0.5f x 0.5f) / 3.0f, so the two branches meet; inv[8705] is 1.0f;
 *   kappa = L_W / 10000 rounded once to binary32.
 * Steps 1-3 are steps 1-3 of "light of PQ code planes", word for word: k_up444 for 4:2:0; the normalisation, one subtraction and one
 *   IEEE division; the matrix, every product and sum rounded by itself.  Then per pixel, in binary32, every product, sum and
 *   difference one round-to-nearest operation, never contracted:
 *   4h. for each of G', B', R': v' = v > 0 ? min(v, 1) : +0.0.  Super-whites above the nominal peak are clipped: that is part of the
 *       definition.
 *   5h. the OETF's inverse: for v' <= 0.5f E_c = (v' v') / 3.0f, the product first, then the IEEE division; otherwise E_c = inv read
 *       at the bits of v' by the table read of "HLG", step 3.
 *   6h. Y_s = ((0.2627f E_R) + (0.6780f E_G)) + (0.0593f E_B); g = the OOTF's gain at Y_s, read from ootf exactly as "HLG" step 3
 *       reads the inverse OOTF's gain: below 2^-17 at 256 Y_s, times entry 0; below 2^-25 the gain is held at ootf[1] ootf[0].
 *       The exponent gamma - 1 is positive, so the held gain OVERSTATES a light that is already below 2^-25 of the peak (3e-5 cd/m2 at
 *       1000): that is part of the definition.
 *   7h. L_c = (E_c g) kappa, the product with g first.  The results lie in [+0, kappa]; 1.0 = 10000 cd/m2; the planes are G, B, R:
 *       what k_linearize leaves for a PQ master, so everything behind it -- k_gamut, k_tonemap, k_hlg, k_light, the forward kernels,
 *       with floor 0 and ceiling 1 by stats_override -- is untouched.
 * Anchors (10-bit video range, Cb = Cr = 512, L_W = 1000): Y 64 -> 0; Y 502 (E' = 0.5) -> 50.697 cd/m2; Y 721 (75 %, BT.2408's
 *   reference white) -> 203.152 cd/m2; Y 940 and 1023 -> 1000.0 cd/m2.
 * Accuracy: for greys, the three primaries and the three secondaries whose E' runs over [0, 1] on a grid of 2^18 + 1 values, at peaks
 *   400, 1000 and 2000, wherever Y_s >= 2^-25, L_c stays within 5.01e-6 of BT.2100's formulas in binary64 (relative; measured with the
 *   host twin's arithmetic; 3.89e-6 at 400, 4.52e-6 at 1000, the worst at 2000), of which (2^-10 / a)^2 / 8 = 3.7e-6 is the linear
 *   interpolation of exp over a step of 2^-10; tests/test_hlg_source_host.py holds it to 1e-5, a fourteenth of a 16-bit PQ code step
 *   (1.4e-4 relative).  Below Y_s = 2^-25 only the absolute error is bounded: the worst absolute error over the whole grid is
 *   9.65e-7 of 10000 cd/m2 (at 2000, near the top of the scale), and below the hold 1.4e-10 (at 400), where the light itself is at
 *   most (2^-25 / 0.0593) (2^-25)^(gamma - 1) kappa = 1.1e-8. */

/* The two tables, kappa and gamma of a peak.  Host only: no device, no context.  ootf and inv receive H2Y_LIGHTDIST_BINS floats
 * each; `why` (may be NULL) receives a static string.  H2Y_EINVAL for a null ootf, inv, kappa or gamma and a peak outside 400..2000. */
int h2y_hlg_inverse_tables(int peak, float ootf[H2Y_LIGHTDIST_BINS], float inv[H2Y_LIGHTDIST_BINS], float *kappa, double *gamma,
                           const char **why);

/* Steps 4h-7h on planes in host memory: the host twin of k_hlg_linearize, which compiles the same lines (csrc/h2y_hlg1.h).  Host
 * only.  src[c] / dst[c]: plane c = G', B', R' in, G, B, R out, npix binary32 samples each; the primes may be clamped or not; a dst
 * plane may be its src plane.  H2Y_EINVAL for null planes and a peak out of range. */
int h2y_hlg_inverse_planes(int peak, size_t npix, const float *const src[3], float *const dst[3]);

/* h2y_linearize_batch for HLG codes at a display peak of `peak` cd/m2: the layout, the scratch, the launches of up to
 * H2Y_LINEARIZE_FRAMES_PER_LAUNCH frames (k_up444 per 4:2:0 frame, then one k_hlg_linearize) and the refusals are that entry's; a
 * peak outside 400..2000 is H2Y_EINVAL.  h2y_last_kernel_name "k_hlg_linearize"; the variant names the matrix and the upsampling
 * form, e.g. "k_hlg_linearize<BT2020NC,FIR>". */
int h2y_hlg_linearize_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int peak, int n_frames, const uint16_t *const *d_frames,
                            void *const *d_planes_out);

/* h2y_pqcode_stream_open with this decode: a forward ring on HLG code frames of src, which the device takes through k_up444 (4:2:0)
 * and k_hlg_linearize at `peak` into the slot's three planes.  Every arming entry behaves as on the PQ code ring, h2y_stream_hlg among
 * them (an HLG master re-written at another nominal peak is a legitimate run).  Refusals as h2y_pqcode_stream_open, and H2Y_EINVAL
 * for a peak outside 400..2000. */
int h2y_hlgcode_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_codelight_desc *src, int peak, int depth);

/* ---- ICtCp: display light written as a PQ ICtCp signal (Rec. ITU-R BT.2100; H.273 matrix_coeffs 14; --ictcp 1) -----------------------
 * The reference has no ICtCp (its matrix 14 is its unbuilt Y'u'v' variant), so there are no bytes to match: this is the project's own
 * definition, as HLG's is.  PQ constants only: BT.2100's HLG form of ICtCp has other coefficients and stays out.  A pass over the decoded
 * source planes, after h2y_stream_gamut's and h2y_stream_tonemap's where those are armed, which leaves CODE-VALUED floats with the
 * rounding half already added.  The ring is opened on the passthrough descriptor "HLG" uses with matrix 0 -- src_transfer ==
 * dst_transfer == 8, src_matrix == dst_matrix == 0, equal primaries, stats_override 1 with floor 0 and ceiling 1 -- and the unchanged
 * forward conversion then does the cast (convert.cpp:1159-1166), the chroma resampler on planes 1 and 2, top-left siting where set, and
 * write_yuv.
 * Input: planes G, B, R of display light in BT.2020 primaries, 1.0 = 10000 cd/m2.  A half is widened first (exact).
 * Pixel, in binary32.  Every product, sum and difference is one round-to-nearest operation, left to right as written, never contracted
 *   into a fused multiply-add:
 *   1. for each of G, B, R: c' = c > 0 ? min(c, 1) : +0.0 (NaN, -0.0 and negatives become +0.0, +inf becomes 1);
 *   2. l, m, s by step 2 of "Delta E ITP of PQ code planes" word for word, its clamp included:
 *        l = clamp(((1688/4096 R) + (2146/4096 G)) + (262/4096 B)), m with 683, 2951, 462, s with 99, 309, 3688;
 *   3. l' = PQ10000_r(l), m' and s' likewise: the forward conversion's own tiers (the table, the full-range table, the careful tier),
 *      exactly as Delta E ITP's step 3;
 *   4. I  = (0.5 l') + (0.5 m')
 *      Ct = ((6610/4096 l') - (13613/4096 m')) + (7003/4096 s')      -- 2 T of Delta E ITP's step 4, bit for bit
 *      Cp = ((17933/4096 l') - (17390/4096 m')) - (543/4096 s')      -- every constant is exact in binary32;
 *   5. H.273's scale for n = dst_bit_depth, s = 2^(n-8): video range oY = 219 s, aY = 16 s, oC = 224 s, aC = 128 s; full range
 *      oY = oC = 2^n - 1, aY = 0, aC = 2^(n-1).  These are NOT the conversion's mulY / addY (its habit of scaling B' and R' by the
 *      chroma range): the ICtCp matrix acts on unscaled primes, and the way back normalises by H.273.
 *        out0 = ((I oY) + aY) + 0.5,  out1 = ((Ct oC) + aC) + 0.5,  out2 = ((Cp oC) + aC) + 0.5,
 *      each then min(max(v, 0), 2^n - 1).  The 0.5 makes the conversion's (unsigned int) cast a rounding; the clamp keeps a negative
 *      from ever reaching that cast.
 *   The outputs are F32 whatever the source's sample type: a half cannot hold code-valued samples.
 * Anchors (10-bit video range): grey of 0 / 100 / 203 / 1000 / 10000 cd/m2 -> I 64 / 509 / 573 / 723 / 940 with Ct = Cp = 512; pure
 *   BT.2020 red, green, blue at 1.0 -> (814, 334, 922), (895, 89, 408), (707, 766, 243) (tests/test_ictcp_host.py). */
#define H2Y_ICTCP_FRAMES_PER_LAUNCH 64

/* k_ictcp on n_frames device frames of width x height: d_src[f*3 + c] / d_dst[f*3 + c] are plane c = G, B, R of frame f, 16-byte
 * aligned; the destination planes are F32 and receive I, Ct, Cp.  With H2Y_SAMPLE_F32 a d_dst entry may equal its d_src entry (in
 * place; no other overlap); with H2Y_SAMPLE_F16 the planes are widened, and in place is refused (H2Y_EINVAL).  H2Y_SAMPLE_U16:
 * H2Y_EUNSUPPORTED; a bad size, null or unaligned planes, dst_bit_depth (8..16) or dst_full_range out of range, a pending batch or an
 * open stream: H2Y_EINVAL.  Launches of up to H2Y_ICTCP_FRAMES_PER_LAUNCH frames (h2y_last_kernel_ms sums them, h2y_last_kernel_name
 * "k_ictcp", the variant "k_ictcp<F32>" or "k_ictcp<F16>"); synchronous. */
int h2y_ictcp_batch(h2y_ctx *ctx, int width, int height, int sample_type, int dst_bit_depth, int dst_full_range, int n_frames,
                    const void *const *d_src, void *const *d_dst);

/* Arm an open forward ring whose decoded planes are F32 (h2y_stream_open with F32 planes, h2y_dpx_stream_open, h2y_pqcode_stream_open,
 * h2y_hlgcode_stream_open) before its first input, once: k_ictcp then runs in place on every slot's decoded device planes, on the
 * context's stream, after h2y_stream_gamut's and h2y_stream_tonemap's passes where those are armed (whichever was armed first), and
 * before the conversion.  The scale is that of the ring's dst_bit_depth and dst_full_range.  The descriptor must be the passthrough
 * flow's as stated above.  h2y_stream_light and h2y_stream_lightdist refuse such a ring (its dst_transfer is not 16): measure the
 * written file ("light of ICtCp code planes").
 * H2Y_EUNSUPPORTED where the planes are F16 or U16, for other transfers, a src_matrix other than 0 and a dst_matrix other than 0;
 * H2Y_EINVAL on the other ring kinds, after the first input, on a ring armed already or armed with h2y_stream_hlg (which in turn
 * refuses a ring armed here), and without that statistics override. */
int h2y_stream_ictcp(h2y_ctx *ctx);

/* ---- light of ICtCp code planes: h2y_codelight_desc.matrix_coeffs 14 (--src_ictcp 1) ----------------------------------------------
 * The way back from the section above, for every entry that takes an h2y_codelight_desc for PQ codes: h2y_codelight_batch,
 * h2y_codescenesig_batch, h2y_linearize_batch, h2y_deltae_batch, h2y_codelight_stream_open, h2y_pqcode_stream_open and
 * h2y_stream_deltae accept matrix_coeffs H2Y_MATRIX_ICTCP, with chroma_format_idc 3, or 1 at even sizes; the variants are named ICTCP
 * ("k_linearize<ICTCP,FIR>").  h2y_hlg_linearize_batch and h2y_hlgcode_stream_open refuse it (H2Y_EUNSUPPORTED): the HLG form of ICtCp
 * is not built.  The project's own definition; every product, sum and difference is rounded by itself to binary32.
 *   Steps 1-2 of "light of PQ code planes" are unchanged: I is normalised as Y is, Ct and Cp as cb and cr.
 *   3i. L' = (I + a Ct) + b Cp;  M' = (I - a Ct) - b Cp;  S' = (I + c Ct) - d Cp, with a = 0.00860903703793, b = 0.111029625003,
 *       c = 0.560031335711, d = 0.320627174987, each rounded once to binary32 (0x3C0D0CEB, 0x3DE36380, 0x3F0F5E37, 0x3EA4293F): the
 *       exact inverse of step 4's matrix above.
 *   4i. each of the three is clamped as step 4 of "light of PQ code planes" clamps and taken through PQ10000_f by the same tiers:
 *       l, m, s.
 *   5i. R = ((3.43660669433 l - 2.50645211866 m) + 0.0698454243232 s)     (0x405BF15D, 0x402069B6, 0x3D8F0B1E)
 *       G = ((1.98360045179 m - 0.791329555599 l) - 0.192270896193 s)     (0x3FFDE69F, 0x3F4A9493, 0x3E44E2A9)
 *       B = ((1.1248636144 s - 0.0259498996906 l) - 0.0989137147117 m)    (0x3F8FFB88, 0x3CD494E2, 0x3DCA9346)
 *       the magnitudes rounded once to binary32: the exact inverse of the k / 4096 LMS matrix.  L_R, L_G, L_B are each
 *       v > 0 ? min(v, 1) : +0.
 *   From there nothing is new: the figures of k_codelight, the planes of k_linearize, the two sides of k_deltae. */

/* ---- light of SDR code planes: a finished SDR master (BT.1886) as a LINEAR G,B,R F32 source of the forward flow (--linearize 1
 * --src_sdr 1) ---------------------------------------------------------------------------------------------------------------------
 * Rep. ITU-R BT.2408's display-referred "direct mapping": an SDR picture placed in absolute light with its reference white at W
 * cd/m2, ready for a PQ or HLG container.  The project's own definition of the flow: the reference has none that leaves the
 * source's transfer for absolute light.  The transfer step, though, is the reference's own function, bt1886_f (convert.cpp:67-75).
 * Frame: exactly what h2y_codelight_desc describes ("light of PQ code planes" above): three u16 code planes at bit_depth 8..16,
 *   video or full range; matrix_coeffs 0, 1 or 9; chroma_format_idc 3, or 1 with even sizes (not with matrix 0); `algorithm` and the
 *   context's inverse chroma siting select the upsampler.  matrix_coeffs 14 is H2Y_EUNSUPPORTED.  The transfer is BT.1886, always.
 * Parameter: an integer reference white W in cd/m2, H2Y_SDR_WHITE_MIN <= W <= H2Y_SDR_WHITE_MAX; H2Y_SDR_WHITE_DEFAULT (203, BT.2408)
 *   where a caller has none; W = 100 is BT.1886's nominal display.  kappa = W / 10000, computed in binary64 and rounded once to
 *   binary32.
 * Steps 1-3 are steps 1-3 of "light of PQ code planes", word for word: k_up444 for 4:2:0; the normalisation, one subtraction and one
 *   IEEE division; the matrix, every product and sum rounded by itself (the file is built -ffp-contract=off).  Then per sample:
 *   4s. for each of G', B', R': v' = v > 0 ? min(v, 1) : +0.0.  A NaN cannot arise from codes.  Super-whites (10-bit Y 941..1019)
 *       are clipped at white: that is part of the definition, as it is for HLG.
 *   5s. E_c = tf_to_linear(BT.1886 class, v'): the binary32 of pow((double)v', (double)2.4f), which is bt1886_f with a = 1 and b = 0.
 *       The exponent is the reference's promoted float, 2.4000000953674316, not 2.4.  It is evaluated by the conversion's own
 *       tiers -- the function's table (H2Y_TFN_G24), its full-range table, the careful tier -- and is therefore the very float the
 *       forward conversion produces for a src_transfer 1 G,B,R sample of value v'.
 *   6s. L_c = E_c x kappa, one rounding.  The results lie in [+0, kappa] and are never -0; 1.0 = 10000 cd/m2; the planes are G, B,
 *       R: what k_linearize leaves for a PQ master, so everything behind it -- k_gamut (BT.709 primaries to BT.2020), k_tonemap,
 *       k_hlg, k_ictcp, k_light, the forward kernels, with floor 0 and ceiling 1 by stats_override -- is untouched.
 * Anchors (10-bit video range, Cb = Cr = 512, W = 203): Y 64 -> 0; Y 502 (v' = 0.5) -> 38.4613 cd/m2; Y 721 -> 101.7755 cd/m2;
 *   Y 940 and 1019 -> 203.0000 cd/m2.  With W = 100, Y 502 -> 18.9465 cd/m2.
 * Accuracy: wherever L_c is a normal number it stays within 2^-22 relative of (W / 10000) x v'^((double)2.4f) in binary64 on the
 *   binary32 v': three roundings of 2^-24 each, E_c, kappa and the product (tests/test_sdr_source_host.py holds it). */
#define H2Y_SDR_WHITE_MIN 80
#define H2Y_SDR_WHITE_MAX 1000
#define H2Y_SDR_WHITE_DEFAULT 203

/* Steps 4s-6s on planes in host memory: the host twin of k_sdr_linearize, step 5s through the careful tier's function
 * (csrc/h2y_math.h), which compiles on the host.  Host only: no device, no context.  src[c] / dst[c]: plane c = G', B', R' in, G, B,
 * R out, npix binary32 samples each; the primes may be clamped or not; a dst plane may be its src plane.  H2Y_EINVAL for null planes
 * and a white out of range. */
int h2y_sdr_inverse_planes(int white, size_t npix, const float *const src[3], float *const dst[3]);

/* h2y_linearize_batch for SDR codes with the reference white at `white` cd/m2: the layout, the scratch, the launches of up to
 * H2Y_LINEARIZE_FRAMES_PER_LAUNCH frames (k_up444 per 4:2:0 frame, then one k_sdr_linearize) and the refusals are that entry's; a
 * white outside 80..1000 is H2Y_EINVAL, matrix_coeffs 14 H2Y_EUNSUPPORTED.  h2y_last_kernel_name "k_sdr_linearize"; the variant
 * names the matrix and the upsampling form, e.g. "k_sdr_linearize<BT709,FIR>" (444, FIR, FIR_TL, REPLICATE). */
int h2y_sdr_linearize_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int white, int n_frames, const uint16_t *const *d_frames,
                            void *const *d_planes_out);

/* h2y_pqcode_stream_open with this decode: a forward ring on SDR code frames of src, which the device takes through k_up444 (4:2:0)
 * and k_sdr_linearize at `white` into the slot's three planes.  Every arming entry behaves as on the PQ code ring.  Refusals as
 * h2y_pqcode_stream_open, H2Y_EINVAL for a white outside 80..1000 and H2Y_EUNSUPPORTED for matrix_coeffs 14. */
int h2y_sdrcode_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_codelight_desc *src, int white, int depth);

/* ---- signal of code planes: a finished master's codes as the R'G'B' signal a signal-domain 3D LUT reads (--linearize 1
 * --src_signal 1 --lut3d FILE.cube --lut3d_signal 1) ---------------------------------------------------------------------------------
 * A colourist's HDR -> SDR trim or a show look is a .cube whose input is non-linear R'G'B' signal in [0, 1].  This decode hands a
 * code master to such a table as what it is: no transfer is applied, so one decode serves PQ, HLG and SDR masters alike, and the
 * table decides what the codes mean.  Nothing in the arithmetic is new: it is "light of PQ code planes" above with its last step
 * taken out.
 * Frame: exactly what h2y_codelight_desc describes: three u16 code planes at bit_depth 8..16, video or full range; matrix_coeffs 0,
 *   1 or 9; chroma_format_idc 3, or 1 with even sizes (not with matrix 0).  matrix_coeffs 14 is H2Y_EUNSUPPORTED: I, Ct, Cp give
 *   L'M'S', not R'G'B'.
 *   Step 1 is step 1 of "light of PQ code planes", unchanged: k_up444 in the form `algorithm` and the context's inverse chroma siting
 *     select.
 *   Steps 2 and 3 are unchanged too: the normalisation, one subtraction and one IEEE division; the matrix, every product and sum
 *     rounded by itself (the file is built -ffp-contract=off).
 *   Last step, for each of G', B', R': v' = v > 0 ? min(v, 1) : +0.0.  Super-whites and sub-blacks are clipped: a .cube's domain
 *     ends there.
 * Output: three binary32 planes G', B', R' in [+0, 1].  Never -0, never NaN (none can arise from codes).
 * Anchors: 10-bit video range with Cb = Cr = 512: Y 64 -> 0, Y 940 -> 1.0, Y 1023 -> 1.0 (clamped), Y 0 -> +0.0.  Full range:
 *   Y 1023 -> 1.0.  (tests/test_signal_source_host.py asserts each.) */

/* Steps 2, 3 and the clamp on 4:4:4 planes in host memory: the host twin of k_code_signal, the same two functions of
 * csrc/h2y_codepixel.h compiled for the host without contraction.  Host only: no device, no context.  src[c]: plane c of the frame
 * (Y, Cb, Cr or G, B, R), npix codes; dst[c]: plane c = G', B', R', npix binary32 samples.  d's chroma_format_idc and `algorithm`
 * describe the file the planes came from and are only checked.  Refusals are the descriptor's, as h2y_codelight_batch states them,
 * H2Y_EUNSUPPORTED for matrix_coeffs 14 and H2Y_EINVAL for null planes. */
int h2y_code_signal_planes(const h2y_codelight_desc *d, size_t npix, const uint16_t *const src[3], float *const dst[3]);

/* h2y_linearize_batch with this decode: the layout, the scratch, the launches of up to H2Y_LINEARIZE_FRAMES_PER_LAUNCH frames (k_up444
 * per 4:2:0 frame, then one k_code_signal) and the refusals are that entry's; matrix_coeffs 14 is H2Y_EUNSUPPORTED.
 * h2y_last_kernel_name "k_code_signal"; the variant names the matrix and the upsampling form, e.g. "k_code_signal<BT709,FIR>" (GBR,
 * BT709, BT2020NC; 444, FIR, FIR_TL, REPLICATE). */
int h2y_code_signal_batch(h2y_ctx *ctx, const h2y_codelight_desc *d, int n_frames, const uint16_t *const *d_frames, void *const *d_planes_out);

/* h2y_pqcode_stream_open with this decode, armed with `lut` in signal mode (h2y_stream_lut3d(ctx, lut, interp, 1)) in the same call:
 * the device takes a code frame of src through k_up444 (4:2:0) and k_code_signal into the slot's three planes, k_lut3d maps them and
 * ends with the conversion's scale step, and the passthrough conversion writes the frame.  Planes in [0, 1] that met no scale step
 * would be written as garbage, so no state exists in which this ring runs without its LUT.  d is the descriptor on which
 * h2y_stream_lut3d(signal 1) arms a PQ code ring: in_sample_type H2Y_SAMPLE_F32, src_matrix 0, src_transfer 8 and dst_transfer 8 (the
 * table is the transfer), dst_matrix 0 or 9, stats_override 1 with floor 0 and ceiling 1, width and height of src.  Anything else
 * gets the code and message of h2y_pqcode_stream_open or of h2y_stream_lut3d, in that order, and leaves no ring open.
 * h2y_stream_lut3d on this ring is H2Y_EINVAL (it applies a LUT already), and so are h2y_stream_hlg, h2y_stream_ictcp,
 * h2y_stream_gamut, h2y_stream_gamut_compress and h2y_stream_tonemap, which act on light.  The arming entries a PQ code ring with a
 * signal-mode LUT takes work on it unchanged (compare, SSIM, histogram, dither, pack, unpack). */
int h2y_sigcode_stream_open(h2y_ctx *ctx, const h2y_desc *d, const h2y_codelight_desc *src, const h2y_lut3d *lut, int interp, int depth);

/* ---- chroma siting: 4:2:0 chroma co-sited with the top-left luma sample (chroma_sample_loc_type 2; HDR10, UHD Blu-ray) -----------
 * The reference carries chroma_sample_loc_type through pic_t and prints it (hdr2yuv.cpp:490, :505); it parses no flag for it and
 * never acts on it.  Its two resamplers site the chroma as they happen to: the 2x2 box in the centre of the block both ways (loc
 * type 1), Subsample444to420_FIR co-sited horizontally (an odd 7-tap filter at the even columns) and centred vertically (an even
 * 12-tap filter, "0.5 sample interval phase shift", convert.cpp:364): loc type 0.  That is kept, bit for bit, by everything above.
 * This is the project's own definition of loc type 2, built from the reference's filter.
 * Input: a chroma plane T of W x H codes (W, H even): matrix_convert's output, not shifted and not yet clamped to the output's
 *   range -- what the two-pass FIR form holds in scratch.  maxCV is the FIR's clip (fir_max; 2^bit_depth - 1 in the stage entry).
 *   1. Horizontal, the reference's stage 1 unchanged: at every row j and every even column i
 *        M[j][i/2] = fir_h(T[j][i-5], T[j][i-3], T[j][i-1], T[j][i], T[j][i+1], T[j][i+3], T[j][i+5]),  columns clamped into 0..W-1;
 *      fir_h in binary32, every product and sum rounded by itself, in this order (convert.cpp:305-317):
 *        acc = (21/512)(m5 + p5) - (52/512)(m3 + p3);  acc = acc + (159/512)(m1 + p1);  acc = acc + (256/512) c;  acc = acc + 0.5
 *      then clamped to [0, maxCV] and truncated to u16.  The 4:2:2 intermediate M is the reference's, bit for bit.
 *   2. Vertical, in exact integers: at every even row j = 2r, the same seven taps down the column,
 *        S = 21 (M[j-5] + M[j+5]) - 52 (M[j-3] + M[j+3]) + 159 (M[j-1] + M[j+1]) + 256 M[j],  rows clamped into 0..H-1,
 *        V = (S + 256) >> 9 (an arithmetic shift: the floor), clamped to [0, maxCV].  |S| < 2^26: int32 holds it.
 *      An integer sum depends on no order of summation at 16-bit codes, where the binary32 form does; up to 14-bit codes it
 *      equals fir_h down the column.
 *   3. write_yuv's shift and per-plane range clamp, as after the reference's FIR (not in the stage entry).
 *   4. Y is untouched.
 * The .yuv -> RGB direction honours it through h2y_ctx_set_inverse_chroma_siting, below ("inverse chroma siting"). */

/* The siting of the 4:2:0 chroma this context's forward conversions write: 0 (the default) as the resampler sites it -- every byte
 * as without this call -- or 2, top-left.  Any other value: H2Y_EINVAL.  H2Y_EINVAL too while a batch is in flight or a ring is
 * open: set it before a ring is opened on the context.  It is read once per batch.  With 2:
 *   - a descriptor with 4:2:0 output and chroma_resampler_type != 0 always runs the two-pass form, k_fir420_tl as its second pass
 *     ("+k_fir420_tl" in h2y_last_kernel_variant); the "fir" option changes nothing then.  4:4:4 output is unaffected;
 *   - h2y_convert_frame, h2y_convert_batch[_enqueue] and every forward ring (plain, DPX, TIFF, EXR) follow it, and what is armed on
 *     a ring (compare, SSIM, histogram, light, gamut) sees the sited frame;
 *   - H2Y_EUNSUPPORTED for 4:2:0 output with chroma_resampler_type 0 (the box is centre sited by construction) or with
 *     dst_matrix_coeffs 15, and for h2y_stream_scale on a 4:2:0 ring of such a context (k_scale aligns sample centres: it would
 *     move the siting again). */
int h2y_ctx_set_chroma_siting(h2y_ctx *ctx, int chroma_sample_loc_type);

/* The stage entry beside h2y_subsample_420: one U16 plane 4:4:4 -> 4:2:0 by the FIR, sited as chroma_sample_loc_type says: 0 the
 * reference's FIR (h2y_subsample_420 with chroma_resampler_type 1), 2 the top-left form above.  maxCV = 2^bit_depth - 1; no
 * write_yuv clamp.  d_src, d_dst: device pointers, 2-byte aligned.  Synchronous; h2y_last_kernel_ms gives the launch's time and
 * h2y_last_kernel_name "k_fir420" or "k_fir420_tl". */
int h2y_subsample_420_sited(h2y_ctx *ctx, int width, int height, int bit_depth, int chroma_sample_loc_type, const uint16_t *d_src,
                            uint16_t *d_dst);

/* ---- inverse chroma siting: upsampling 4:2:0 chroma that is co-sited with the top-left luma sample (chroma_sample_loc_type 2) -----
 * The reference's Subsample420to444 (h2y_upsample_444) takes the chroma as its own FIR wrote it: co-sited horizontally, centred
 * between two luma rows vertically (loc type 0) -- its vertical stage is the quarter-phase pair (3 -16 67 227 -32 7)/256.  On
 * HDR10-style 4:2:0 (what h2y_ctx_set_chroma_siting(2) writes, or any decoded HDR10 stream) that leaves the chroma half a luma row
 * low.  This is the project's own definition of the top-left upsampler; the reference has none, so there are no bytes to match.
 * Input: a chroma plane C of w2 x h2 codes (w2 = width/2, h2 = height/2), sample (r, c) co-sited with luma (2r, 2c); the clip
 *   [minCV, maxCV] (0 and 2^in_bit_depth - 1 in the flow, yuv2tiff.cpp:92-93,142-154).
 *   1. Vertical, in exact integers, into a U16 intermediate M of w2 x height; rows clamped into 0..h2-1:
 *        M[2r][c]   = med3(C[r][c], minCV, maxCV)                                           (a copy)
 *        S          = 21 (C[r-2] + C[r+3]) - 52 (C[r-1] + C[r+2]) + 159 (C[r] + C[r+1])     (the half-phase six-tap, down the column)
 *        M[2r+1][c] = med3((S + 128) >> 8, minCV, maxCV)
 *      The shift is arithmetic (the floor); |S| < 2^25: int32 holds it.  The taps read the unclamped source codes, as the
 *      reference's vertical stage does.  Integers, not binary32: 159 (a + b) passes 2^24 at 16-bit codes.
 *   2. Horizontal, the reference's stage unchanged (convert.cpp:1956-1979): out[y][2c] = M[y][c]; out[y][2c+1] the binary32
 *      (21 -52 159 159 -52 21)/256 of M[y][c-2..c+3], columns clamped, every product and sum rounded by itself, + 0.5, the clamp,
 *      truncation.  Horizontally the reference is co-sited already.
 *   3. matrix_inverse's pixel, unchanged. */

/* The siting of the 4:2:0 chroma this context's .yuv -> RGB entries read: 0 (the default) as the reference's upsampler takes it --
 * every byte as without this call -- or 2, top-left.  Any other value: H2Y_EINVAL.  H2Y_EINVAL too while a batch is pending or a
 * ring is open.  Independent of h2y_ctx_set_chroma_siting.  It is read at each call of h2y_inverse_420, h2y_inverse_frame and
 * h2y_inverse_batch, and when h2y_inverse_stream_open or h2y_tiff_inverse_stream_open opens; what is armed on those rings (compare,
 * SSIM, histogram) sees the G, B, R of the sited upsampling.  With 2:
 *   - 4:2:0 input with `algorithm` != 0 runs the form above ("k_inverse420<FIR_TL>" / "k_inverse420_batch<FIR_TL>" in
 *     h2y_last_kernel_variant; h2y_last_kernel_name stays "k_inverse420" / "k_inverse420_batch").  4:4:4 input is unaffected;
 *   - H2Y_EUNSUPPORTED for 4:2:0 input with `algorithm` 0 (replication is centre sited by construction); nothing is launched. */
int h2y_ctx_set_inverse_chroma_siting(h2y_ctx *ctx, int chroma_sample_loc_type);

/* The stage entry beside h2y_upsample_444: one U16 chroma plane 4:2:0 -> 4:4:4 by the FIR, the source sited as
 * chroma_sample_loc_type says: 0 the reference's FIR pair (h2y_upsample_444 with algorithm 1), 2 the top-left form above.  Any
 * other value: H2Y_EINVAL.  Sizes, the clip and alignment as h2y_upsample_444.  Synchronous. */
int h2y_upsample_444_sited(h2y_ctx *ctx, int width, int height, int chroma_sample_loc_type, unsigned min_cv, unsigned max_cv,
                           const uint16_t *d_src, uint16_t *d_dst);

/* Timing of the last h2y_convert_batch*() (or h2y_inverse_*, h2y_dpx_decode_batch, h2y_tiff_decode_batch,
 * h2y_rgb_interleave_batch, h2y_exr_decode_batch, h2y_compare_batch, h2y_ssim_batch, h2y_regions_batch, h2y_light_batch, h2y_lightdist_batch, h2y_codelight_batch, h2y_scenesig_batch, h2y_codescenesig_batch, h2y_linearize_batch, h2y_hlg_linearize_batch, h2y_sdr_linearize_batch, h2y_code_signal_batch, h2y_scale_batch, h2y_gamut_batch, h2y_tonemap_batch, h2y_hlg_batch, h2y_ictcp_batch, h2y_dither_batch, h2y_pack_batch, h2y_unpack_batch) call measured with HIP events on
 * the stream the kernels ran on: total ms over the main kernels and how many
 * launches that covered. */
int h2y_last_kernel_ms(const h2y_ctx *ctx, float *ms, int *launches);

/* Name of the kernel those launches ran ("k_fused", "k_fused_t1", "k_fused_lut16",
 * "k_fused_narrow"; of the inverse entries "k_inverse", "k_inverse420", "k_inverse_batch", "k_inverse420_batch"; of
 * h2y_dpx_decode_batch "k_dpx_decode"; of h2y_tiff_decode_batch "k_tiff_decode", of h2y_rgb_interleave_batch
 * "k_rgb_interleave"; of h2y_exr_decode_batch "k_exr_decode"; of h2y_compare_batch "k_compare"; of h2y_scale_batch "k_scale"; of h2y_dither_batch "k_dither"; of h2y_pack_batch "k_pack"; of h2y_unpack_batch "k_unpack"; of h2y_gamut_batch "k_gamut"; of h2y_tonemap_batch "k_tonemap"; of h2y_hlg_batch "k_hlg"; of h2y_ictcp_batch "k_ictcp"; of h2y_codelight_batch "k_codelight"; of h2y_scenesig_batch "k_scenesig"; of h2y_codescenesig_batch "k_codescenesig"; of h2y_linearize_batch "k_linearize"; of h2y_hlg_linearize_batch "k_hlg_linearize"; of h2y_sdr_linearize_batch "k_sdr_linearize"; of h2y_code_signal_batch "k_code_signal"): the name to
 * look for in a rocprofv3 kernel trace. */
const char *h2y_last_kernel_name(const h2y_ctx *ctx);
/* The same with its template arguments and launch shape, e.g. "k_fused_t1<F32,420BOX,YCBCR,PQ_IDENT> groups=8 xcd=1";
 * "+k_fir420" after the '>' when the chroma went through the two-pass FIR form ("+k_fir420_tl" with chroma siting 2).  Tests assert on it: which
 * variant a call took must not depend on what ran before. */
const char *h2y_last_kernel_variant(const h2y_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* HDR2YUV_HIP_H */
