/*
 * hdr2yuv (MI355X build) -- host program with the reference's command-line surface (hdr2yuv.cpp:73-263) and its
 * resolution of unset attributes (h2y_cli_args.h) for the in-memory convert path.  It reads raw planar input, hands the
 * planes to the C-ABI (include/hdr2yuv_hip.h) and writes the .yuv frames where write_yuv() would append them
 * (tiff.cpp:440: the file is opened in append mode; planes Y, Cb, Cr, little-endian 16-bit).
 *
 * How the file is laid out: main resolves the command line, scans the source (h2y_cli_sources.h) and checks every file's size,
 * then chooses one of seven flows -- forward, .yuv -> RGB, --compare_only, --histogram_only, --scale_only, --light_only, --dither_only.  A flow is a `flow`: how
 * to open its ring and arm its stages, how frame k gets into a slot's planes, the layout of the reference frame, how frame k is
 * written.  run_block drives every flow the same way (context, source, ring, reference, stages, the fill / submit / drain loop
 * three slots deep, the tail) and tears down through one guard; what the blocks measure is kept in one `results`.
 *
 * Input formats:
 *   .yuv / .rgb  16-bit planar integer (hdr2yuv.cpp:582-656; .rgb is R,G,B in the file, planes 2,0,1 in memory)
 *   .f32 / .f16  raw planar float / half in G,B,R plane order -- what dpx_read() or read_exr() (exr.cpp:233-235) leave in
 *                memory; the attributes those readers force on the input picture are forced here too
 *   .dpx         10-bit, 16-bit or float DPX (dpx_read(), dpx.cpp:209-520): the header is parsed here (h2y_dpx_parse), the
 *                payload read straight into the pinned slot of the DPX ring and decoded on the device; one file is one
 *                frame, and a name with one integer conversion (shot.%06d.dpx) numbers the files of a sequence
 *   .tiff        16-bit R,G,B TIFF (read_tiff(), tiff.cpp:54-362): the file is mapped and its IFD parsed here
 *                (h2y_tiff_parse), the decoded rows read into the pinned slot of the TIFF ring and de-interleaved on the
 *                device; numbered like .dpx
 *   .exr         scanline OpenEXR (read_exr(), exr.cpp:138-255; NONE, RLE, ZIPS or ZIP): the file is mapped, its header and
 *                offset table parsed here (h2y_exr_parse), its chunks inflated or copied straight into the pinned slot of the
 *                EXR ring by a pool of unpack threads (at most 16 across all GPU threads), the predictor, reorder and
 *                scanline-to-plane work done on the device; numbered like .dpx.  Its size is checked against the command
 *                line before anything else, also under --dry_run, as read_exr() takes it from the file
 *   --synthetic N  the seeded test frame of SURVEY 8c (no input file), treated as an .exr-like float input
 * and, from .yuv input, the .yuv -> .tiff flow (hdr2yuv.cpp:818-819, matrix_inverse): .tiff output (write_tiff(),
 * tiff.cpp:559-652; the samples interleaved on the device, the file bytes libtiff would write around them, one truncated
 * file per frame, numbered through a name like shot.%06d.tiff) or the same samples as planes R, G, B in one .rgb.
 *
 * Several GPUs (--gpus N, an addition: the reference converts one frame per process): one host thread per GPU, each with
 * its own context and pinned ring; thread r takes a contiguous block of the frame indices (the split of
 * hdr2yuv_amd/shard.py), reads frame k at its offset in the source (hdr2yuv.cpp:624) and writes it at
 * `size of the file at start + k x frame bytes` -- the bytes N appending runs in frame order would have left (tiff.cpp:440).
 *
 * Comparison (--ref_filename R [--sigma_compare S], or --compare_only 1; h2y_cli_args.h): each GPU thread arms its ring
 * (h2y_stream_compare; with no destination the frames stay on the device) or opens a compare-only ring, reads frame k of R into
 * the reference slot beside the input, and keeps the stats of frame k by its index; the report is printed once every thread is
 * done, so it is the same for any --gpus.  Report on stdout, planes Y Cb Cr for .yuv and G B R for .rgb / .tiff, maxv =
 * 2^bit_depth - 1 of the compared frames (the destination's, or the source's under --compare_only), PSNR of n samples with a sum
 * of squared differences sse printed "%.4f" of 10 * log10((double)maxv * maxv * n / sse) in double arithmetic, or "inf" for
 * sse 0:
 *   frame <k> psnr <P0> <psnr> <P1> <psnr> <P2> <psnr> max_abs <m0> <m1> <m2> over <o0> <o1> <o2>     one line per frame, in order
 *   summary frames <N> mean_psnr <P0> <m> <P1> <m> <P2> <m> global_psnr <P0> <g> <P1> <g> <P2> <g> max_abs <m0> <m1> <m2> over <o0> <o1> <o2>
 *   first_over frame <k> plane <P> x <x> y <y> a <a> b <b>       (or "first_over none")
 * mean_psnr: the mean over frames of the per-frame value, a frame with sse 0 counting 99.99; global_psnr: from the summed sse
 * and samples; max_abs the largest |a - b|, over the count of |a - b| > S (S 0 by default); first_over the first such sample in
 * frame, plane and raster order, a the output's (the source's) sample, b R's.  Exit status 3 when S was given and over > 0.
 *
 * SSIM (--ssim 1 beside a comparison; h2y_cli_args.h): each GPU thread arms its ring for SSIM too (h2y_stream_ssim) and keeps
 * the figures of frame k by its index; the report follows the compare report, so it is the same for any --gpus.  Planes as there,
 * values "%.6f", dB = -10 * log10(1 - x) "%.4f" or "inf" for x = 1:
 *   ssim frame <k> <P0> <v> <P1> <v> <P2> <v> all <v> db <P0> <d> <P1> <d> <P2> <d> all <d>      one line per frame, in order
 *   ssim summary frames <N> <P0> <m> <P1> <m> <P2> <m> all <m> db ...     the means over frames (summed in frame order), dB of them
 *   ssim worst frame <k> all <v>                                          the lowest all, the first such frame on ties
 *
 * Flat and busy areas, over- and undershoot (--regions 1 [--regions_flat_var V] [--regions_radius R] beside a comparison;
 * h2y_cli_args.h): each GPU thread arms its ring for them too (h2y_stream_regions) and keeps the figures of frame k by its index; the
 * report follows the SSIM report, so it is the same for any --gpus.  Planes and PSNR as in the comparison's report, of a class's
 * samples and sse ("-" for a class of no samples); flat_share = flat samples / samples "%.6f"; *_mean = sum / count "%.4f" ("-" for
 * a count of 0); the summary's figures come from the sums over the run:
 *   regions frame <k> flat_share <P0> <s> <P1> <s> <P2> <s> psnr_flat <P0> <v> .. psnr_busy <P0> <v> .. over <c0> <c1> <c2> over_max <m0> <m1> <m2> under <c0> <c1> <c2> under_max <m0> <m1> <m2>
 *   regions summary frames <N> flat_share .. global_psnr_flat .. global_psnr_busy .. over .. over_mean <P0> <x> .. over_max .. under .. under_mean .. under_max ..
 * The exit status is unchanged: the figures gate nothing.
 *
 * Delta E ITP (--delta_e 1 [--delta_e_threshold X] [--delta_e_limit Y] beside a comparison of PQ code frames; h2y_cli_args.h): each GPU
 * thread sets its context's inverse chroma siting where the frames' siting flag says 2 and arms its ring for Delta E too
 * (h2y_stream_deltae) and keeps the figures of frame k by its index; the report follows the SSIM report, so it is the same for any
 * --gpus.  Values "%.6f", the share of the frame's pixels above the threshold in percent "%.4f":
 *   delta_e: frame <k> mean <m> max <d> at <x> <y> over <n> share <s>        one line per frame, in order
 *   delta_e: summary frames <N> mean <m> worst frame <k> mean <m> max <d> frame <k> at <x> <y> over <n> share <s>
 * the summary's mean is the mean of the frames' means (summed in frame order), worst the frame with the largest mean and max the largest
 * max (the first such frame on ties), over and share over all frames.  Exit status 5 when --delta_e_limit Y was given and a frame's mean
 * exceeds Y (3 and 4 before it).
 *
 * Histogram (--histogram FILE [--histogram_bits B] [--check_range 1], or --histogram_only 1; h2y_cli_args.h): each GPU thread arms
 * its ring (h2y_stream_histogram; h2y_stream_histogram_ex on a compare-only ring) or opens a histogram-only ring, keeps the stats
 * of frame k by its index and sums its frames' bins; the report is printed once every thread is done, so it, and FILE, are the
 * same for any --gpus.  Planes P0 P1 P2 are Y Cb Cr, or G B R for .rgb / .tiff; occupied counts the non-zero bins of 2^B:
 *   histogram frame <k> <P0> min <m> max <M> below <b> above <a> at_low <l> at_high <h> occupied <o> <P1> ... <P2> ...
 *   histogram summary frames <N> <P0> min .. occupied <o> <P1> ... <P2> ...   (sums, and bins occupied in the totals)
 *   histogram legal <P0> <lo>..<hi> <P1> <lo>..<hi> <P2> <lo>..<hi> outside <below + above over all planes and frames>
 * FILE (text): "bin,code_lo,code_hi,<P0>,<P1>,<P2>", then one line per bin, code_lo = bin << (depth - B), code_hi = code_lo +
 * 2^(depth - B) - 1, the counts summed over the frames (a code above 2^depth - 1 counts in the last bin).  Exit status 4 under
 * --check_range 1 when outside > 0 (3 before it, when the comparison's status is 3).
 *
 * Content light (--content_light 1 on the forward flow; h2y_cli_args.h): each GPU thread arms its ring (h2y_stream_light) and keeps
 * the figures of frame k by its index; the report is printed once every thread is done, so it is the same for any --gpus.  cd/m2
 * "%.4f"; MaxCLL and MaxFALL rounded to the nearest integer (halves away from zero):
 *   light frame <k> peak <cll> at <x> <y> average <fall>              one line per frame, in order (the first pixel holding the peak)
 *   light summary frames <N> maxcll <CLL> frame <k> maxfall <FALL> frame <k>    the largest of each, the first such frame on ties
 *   light x265 --max-cll "<CLL>,<FALL>"
 *   light svt-av1 --content-light <CLL>,<FALL>
 *
 * Dynamic metadata (--dynamic_metadata FILE on the forward flow; h2y_cli_args.h): each GPU thread arms its ring (h2y_stream_lightdist)
 * and keeps the figures of frame k by its index; the report is printed and FILE written (h2y_lightdist_json: HDR10+ JSON, every frame
 * in scene 0) once every thread is done, so both are the same for any --gpus.  cd/m2 "%.4f" (10000 x L; the percentiles are the lower
 * edges of their bins), the percentiles 1, 5, 10, 25, 50, 75, 90, 95, 99 and 99.98 %, the share in percent:
 *   dynamic_metadata: frame <k> maxscl <R> <G> <B> average <A> percentiles <p1> ... <p99.98> below_100 <share>
 *   dynamic_metadata_written: <N> frames to FILE
 * Scenes (--scene_detect 1 [--scene_threshold T] or --scene_cuts FILE, [--scene_qpfile OUT], beside --dynamic_metadata; h2y_cli_args.h):
 * each GPU thread also arms its ring with h2y_stream_scenesig (the detected case) and keeps frame k's signature and its bins
 * (h2y_stream_lightdist_bins: 34 KB a frame of host memory) by its index; after every thread is done the cuts are decided
 * (h2y_scene_cuts) or taken from FILE, the scenes merged (h2y_scene_merge) and FILE written by h2y_lightdist_json_scenes, the same for
 * any --gpus.  Between the dynamic_metadata: frame lines and dynamic_metadata_written:
 *   scene: frame <k> distance <D>[ cut]                      (the detected case, k from 1)
 *   scene: <s> first <f> frames <n> maxscl <R> <G> <B> average <A> percentiles <p1> ... <p99.98> below_100 <share>
 *   scene: summary scenes <S> frames <N>
 *   scene_qpfile_written: <S> scenes to OUT                  (--scene_qpfile: one line "<frame> I" per scene start)
 *
 * Light of a PQ master (--light_only 1 [--dynamic_metadata FILE]; h2y_cli_args.h): each GPU thread sets its context's inverse chroma
 * siting where --src_chroma_sample_loc_type 2 says so and opens a light-only ring (h2y_codelight_stream_open) on the source's code
 * planes; the figures of frame k are kept by its index and reported by the two reports above, word for word, so the lines and FILE
 * are the same for any --gpus.  The banner carries light_only: and light_only_from:.  With --gamut_check 1 the ring is armed with
 * h2y_stream_gamutcheck too and the run prints the gamut_check: lines (gamutcheck_report); --gamut_check_limit makes the exit status 6.
 *
 * Scaling (--scale 1 [--scale_taps A] with --dst_pic_width / --dst_pic_height on the forward flow; h2y_cli_args.h): each GPU thread
 * arms its ring (h2y_stream_scale), so the frame that comes down is the converted frame resampled on the device to the destination
 * size (include/hdr2yuv_hip.h states the filter); frame k is written at `size of the file at start + k x scaled frame bytes`.
 * --scale_only 1 resamples a .yuv or .rgb source through a scale-only ring (h2y_scale_stream_open) into a file of the same layout.
 *
 * Dither (--dither 1|2 [--dither_temporal 0|1] [--dither_seed N] on the forward flow to .yuv; h2y_cli_args.h): the run's descriptor
 * converts at the working depth (cli_resolve_dither), and each GPU thread arms its ring last (h2y_stream_dither, after
 * h2y_stream_scale) with the destination depth and its block's first frame counted from the run's first, so the frame that comes
 * down is the converted (and scaled) frame reduced on the device, numbered as one thread would number it: any --gpus writes the
 * same file.  --dither_only 1 reduces a .yuv or .rgb source through a dither-only ring (h2y_dither_stream_open) into a file of the
 * same layout.
 *
 * Primaries (--gamut_convert 1 [--gamut_clip 0|1] on the forward flow from .f32, .f16, .exr and .dpx; h2y_cli_args.h): each GPU thread
 * arms its ring (h2y_stream_gamut) with --src_colour_primaries and --dst_colour_primaries, so every slot's decoded planes are
 * converted in place on the device before pic_stats and the conversion: the run writes the bytes it would write had the source
 * held the converted planes, and --content_light beside it measures the converted light.  The banner carries gamut_convert:,
 * gamut_clip: and the nine entries of gamut_matrix: as "%.9g".  With --gamut_compress 1 [--gamut_compress_threshold T]
 * [--gamut_compress_power P] beside it the ring is armed with h2y_stream_gamut_compress instead: the same matrix, and out-of-gamut
 * colours rolled off toward the pixel's largest channel, not clipped; the banner carries gamut_compress:, the two parameters and
 * gamut_compress_limits:.
 *
 * Tone mapping (--tone_map 1 [--tone_map_src_peak S] [--tone_map_dst_peak D] on the forward flow from .f32, .f16, .exr and .dpx;
 * h2y_cli_args.h): each GPU thread opens its ring with floor 0 and ceiling 1 for every frame and arms it (h2y_stream_tonemap), so
 * every slot's decoded planes are mapped in place on the device, after --gamut_convert's pass, before the conversion: the run
 * writes the bytes it would write had the source held the mapped planes, and --content_light and --dynamic_metadata beside it
 * measure the mapped light.  The banner carries tone_map:, tone_map_src_peak:, tone_map_dst_peak: ("(default)" where not given),
 * tone_map_output: relative|absolute and the knee in cd/m2 as tone_map_knee: "%.9g".
 *
 * HLG (--hlg 1 [--hlg_peak L] on the forward flow from .f32 and .dpx, and from a PQ .yuv / .rgb with --linearize 1; h2y_cli_args.h):
 * the run's destination transfer becomes the source's 8, each GPU thread opens its ring with floor 0 and ceiling 1 and arms it
 * (h2y_stream_hlg), so every slot's decoded planes become code-valued HLG samples in place on the device, after --gamut_convert's and
 * --tone_map's passes, and the conversion takes them straight to its matrix.  The banner carries hlg:, hlg_peak: ("(default)" where
 * not given), hlg_gamma: "%.9g", hlg_input: absolute|relative, hlg_note: and hlg_encoder:.
 *
 * 3D LUT (--lut3d FILE.cube [--lut3d_interp 0|1] [--lut3d_signal 0|1] on the forward flow from .f32, .f16, .exr, .dpx and --linearize 1
 * sources; h2y_cli_args.h): the file is read and parsed once (h2y_lut3d_parse), each GPU thread opens its ring with floor 0 and
 * ceiling 1 and arms it (h2y_stream_lut3d), so the table is applied to every slot's decoded planes in place on the device, after
 * --gamut_convert's and --tone_map's passes and before --hlg's / --ictcp's.  In planes mode the run writes the bytes it would write had
 * the source held the planes the LUT leaves; in signal mode the run's destination transfer becomes the source's and the conversion
 * takes the LUT's code values straight to its matrix, as for --hlg 1.  The banner carries lut3d:, lut3d_title:, lut3d_size:,
 * lut3d_domain:, lut3d_interp:, lut3d_signal: and, where --dst_transfer_characteristics was given in signal mode, lut3d_dst_transfer:.
 *
 * ICtCp (--ictcp 1 on the same sources; h2y_cli_args.h): the run's destination matrix and transfer become the passthrough descriptor's
 * 0 and 8 with equal primaries, each GPU thread opens its ring with floor 0 and ceiling 1 and arms it (h2y_stream_ictcp), so every
 * slot's decoded planes become code-valued PQ I, Ct, Cp samples in place on the device, after --gamut_convert's and --tone_map's passes,
 * and the conversion casts, subsamples and writes them.  The banner carries ictcp:, ictcp_scale:, ictcp_note: and ictcp_encoder:.
 * --src_ictcp 1 gives the code frames that --linearize 1, --light_only 1 and --compare_only 1 --delta_e 1 read matrix_coeffs 14 in
 * their h2y_codelight_desc; nothing else in those flows differs.
 *
 * A PQ master as the source (--linearize 1 on the forward flow from a PQ .yuv or .rgb; h2y_cli_args.h): each GPU thread sets its
 * context's inverse chroma siting where --src_chroma_sample_loc_type 2 says so and opens the forward ring that decodes PQ code frames
 * (h2y_pqcode_stream_open): a frame is read whole into the pinned slot, as --light_only reads it, and linearised on the device into
 * the slot's F32 G,B,R planes; everything armed on the ring sees those planes.  One more source kind of the forward flow, not a flow
 * of its own.  The banner carries linearize: and linearize_from:.  With --src_hlg 1 [--src_hlg_peak L] beside it the file's codes
 * are HLG's and the ring is h2y_hlgcode_stream_open's at that display peak; nothing else differs.  The banner then carries src_hlg:,
 * src_hlg_peak:, src_hlg_gamma: and src_hlg_note: too.  With --src_sdr 1 [--src_sdr_white W] beside it the codes are an SDR
 * master's (BT.1886) and the ring is h2y_sdrcode_stream_open's with the reference white at W cd/m2; the banner then carries src_sdr:,
 * src_sdr_white: and src_sdr_gamma:.  With --src_signal 1 --lut3d FILE.cube --lut3d_signal 1 beside it no transfer is applied: the ring
 * is h2y_sigcode_stream_open's, whose decode leaves the codes' R'G'B' signal for the table it arms in the same call; the banner then
 * carries src_signal: and linearize_from: names the signal.
 *
 * Packings (--dst_pack / --src_pack planar8|nv12|p010; h2y_cli_args.h): each GPU thread arms its ring last with h2y_stream_pack, so the
 * frame that comes down is the .yuv frame packed on the device, written at `size of the file at start + k x h2y_pack_frame_bytes`; and
 * right after opening it with h2y_stream_unpack, so a frame of the source (and of R under --compare_only) is read whole, packed, into
 * the pinned slot and unpacked on the device.  The file offsets, the length check and R's frame size are the packed frame's.
 *
 * Chroma siting (--dst_chroma_sample_loc_type 0|2 on the forward flow to .yuv; h2y_cli_args.h): each GPU thread sets its context's
 * siting (h2y_ctx_set_chroma_siting) before it opens its ring, so every frame, and whatever is armed on the ring, has its 4:2:0
 * chroma where the flag says.  The banner carries dst_chroma_sample_loc_type: only when the flag is given, and with 2 it ends with
 * the settings that signal the siting to an encoder:
 *   chroma_siting x265 --chromaloc 2
 *   chroma_siting svt-av1 --chroma-sample-position topleft
 * The way back (--src_chroma_sample_loc_type 0|2 on the .yuv -> .rgb / .tiff flow with 4:2:0 input): each GPU thread sets its
 * context's inverse chroma siting (h2y_ctx_set_inverse_chroma_siting) before it opens its inverse ring, so every frame, and what is
 * armed on the ring, is upsampled from where the flag says the chroma lies.  The banner carries src_chroma_sample_loc_type: only
 * when the flag is given.
 */
#include <array>
#include <cmath>
#include <memory>

#include "h2y_cli_sources.h"

static bool write_at(int fd, const void *buf, size_t n, off_t at)
{
    const char *p = (const char *)buf;
    while (n) {
        ssize_t w = pwrite(fd, p, n, at);
        if (w < 0) {
            if (errno == EINTR) continue;
            return false;
        }
        p += w;
        at += w;
        n -= (size_t)w;
    }
    return true;
}

/* the bytes of one 16-bit planar frame, 4:2:0 or 4:4:4: h2y_scale_frame_bytes states them for every size and chroma format
 * cli_resolve lets through to a flow that reads or writes such frames (1..10000 a side, chroma_format_idc 1 or 3; it is 0 beyond) */
static size_t planar16_bytes(const cli_pic &p)
{
    return h2y_scale_frame_bytes(p.width, p.height, p.chroma_format_idc);
}

/* what every flow's open ends with: the ring just opened (rc 0) takes the source's frames packed where --src_pack says so */
static int opened(int rc, const cli_args &a, h2y_ctx *ctx)
{
    if (rc || !a.src_pack) return rc;
    /* a compare-only ring does not know its frames' depth: --src_bit_depth says it (P010 needs it, and cli_resolve insists on it) */
    return a.compare_only ? h2y_stream_unpack_ex(ctx, a.src_pack, a.in.bit_depth) : h2y_stream_unpack(ctx, a.src_pack);
}

struct block { /* one thread's share: frames [first, first + count) of the run, on `device` */
    int device = 0;
    long first = 0, count = 0;
    std::string err;
    long done = 0;
};

/* frame k of the reference file into a ring's reference slot: the whole frame as the file holds it, or, for a .rgb (planes
 * R, G, B in the file), into the slot's G | B | R order */
static bool read_ref(FILE *f, bool rgb, size_t plane_bytes, size_t frame_bytes, void *ref)
{
    if (!rgb) return fread(ref, 1, frame_bytes, f) == frame_bytes;
    if (frame_bytes != 3 * plane_bytes) return false; /* a .rgb frame is three full planes: nothing else fits the slot */
    char *p = static_cast<char *>(ref);
    return fread(p + 2 * plane_bytes, 1, plane_bytes, f) == plane_bytes && fread(p, 1, 2 * plane_bytes, f) == 2 * plane_bytes;
}

/* What a run measures: the stats of frame k kept by its index, whichever GPU thread took them, so that every report is the same
 * for any --gpus; the histogram's bins summed per GPU thread and added up at the end. */
struct results {
    std::vector<h2y_compare_stats> compare;
    std::vector<h2y_ssim_stats> ssim;
    std::vector<h2y_regions_stats> regions;
    std::vector<h2y_deltae_stats> deltae;
    std::vector<h2y_light_stats> light;
    std::vector<h2y_lightdist_stats> lightdist;
    std::vector<h2y_scenesig> scenesig; /* --scene_detect 1: frame k's signature */
    std::vector<h2y_gamutcheck_stats> gamutcheck; /* --gamut_check 1: frame k's check */
    std::vector<uint32_t> dist_bins;    /* a scene flag: frame k's H2Y_LIGHTDIST_BINS bins, for the scenes' percentiles */
    std::vector<h2y_histogram_stats> hist;
    std::vector<std::array<uint32_t, 3>> occupied; /* the non-zero bins of frame k's planes */
    std::vector<uint32_t> bins;                    /* per GPU thread: one frame's 3 x nbins */
    std::vector<uint64_t> total;                   /* per GPU thread: its sums */
    size_t nbins = 0;
    results(const cli_args &a, long frames)
        : compare(a.ref ? (size_t)frames : 0), ssim(a.ssim ? (size_t)frames : 0), regions(a.regions ? (size_t)frames : 0), deltae(a.delta_e ? (size_t)frames : 0), light(a.light ? (size_t)frames : 0),
          lightdist(a.dynmeta ? (size_t)frames : 0), scenesig(a.scene_detect == 1 ? (size_t)frames : 0),
          gamutcheck(a.gamut_check == 1 ? (size_t)frames : 0),
          dist_bins(a.scenes() ? (size_t)frames * H2Y_LIGHTDIST_BINS : 0), hist(a.hist ? (size_t)frames : 0), occupied(hist.size())
    {
        if (!a.hist) return;
        nbins = (size_t)1 << a.hist_bits;
        bins.assign((size_t)a.gpus * 3 * nbins, 0u);
        total.assign((size_t)a.gpus * 3 * nbins, 0u);
    }
    /* after h2y_stream_output on GPU thread r: frame k's results; false when the library refused one */
    bool take(const cli_args &a, h2y_ctx *ctx, long k, int r)
    {
        if (a.ref && h2y_stream_compare_result(ctx, &compare[k])) return false;
        if (a.ssim && h2y_stream_ssim_result(ctx, &ssim[k])) return false;
        if (a.regions && h2y_stream_regions_result(ctx, &regions[k])) return false;
        if (a.delta_e && h2y_stream_deltae_result(ctx, &deltae[k])) return false;
        if (a.hist) {
            uint32_t *b = &bins[(size_t)r * 3 * nbins];
            uint64_t *t = &total[(size_t)r * 3 * nbins];
            if (h2y_stream_histogram_result(ctx, &hist[k], b)) return false;
            for (int p = 0; p < 3; p++) {
                uint32_t occ = 0;
                for (size_t i = 0; i < nbins; i++) {
                    const uint32_t c = b[p * nbins + i];
                    occ += c != 0u;
                    t[p * nbins + i] += c;
                }
                occupied[k][p] = occ;
            }
        }
        if (a.light && h2y_stream_light_result(ctx, &light[k])) return false;
        if (a.dynmeta && h2y_stream_lightdist_result(ctx, &lightdist[k])) return false;
        if (a.scene_detect == 1 && h2y_stream_scenesig_result(ctx, &scenesig[k])) return false;
        if (a.gamut_check == 1 && h2y_stream_gamutcheck_result(ctx, &gamutcheck[k])) return false;
        if (a.scenes() && h2y_stream_lightdist_bins(ctx, &dist_bins[(size_t)k * H2Y_LIGHTDIST_BINS])) return false;
        return true;
    }
    /* the bins of every thread, summed (the same totals for any split) */
    std::vector<uint64_t> histogram_total() const
    {
        std::vector<uint64_t> sum(3 * nbins, 0u);
        for (size_t i = 0; i < total.size(); i++) sum[i % sum.size()] += total[i];
        return sum;
    }
};

/* the bytes libtiff writes around write_tiff()'s samples (h2y_tiff_layout) */
struct tiff_wrap {
    uint8_t head[8];
    std::vector<uint8_t> tail;
};

/* what main resolved and every block of the run shares */
struct job {
    cli_args a;
    h2y_desc d{};
    scanned src;
    tiff_wrap tw;
    size_t in_frame_bytes = 0, out_frame_bytes = 0;
    int fd_out = -1; /* the one destination file (not .tiff output), frames going in from `base` on */
    off_t base = 0;
};

/* The reader fills the pinned slot of the pipeline directly, the writer drains what comes out of it two frames later: upload,
 * conversion and download of neighbouring frames overlap. */
static constexpr int kRingDepth = 3;

/* What one of the six flows hands to run_block.  open and arm return the library's status; fill and write return "" or the
 * block's error message. */
struct flow {
    /* `first` is the block's first frame, counted from the run's first: the number of the ring's first frame where frames are numbered */
    std::function<int(h2y_ctx *, long first)> open; /* the flow's ring, kRingDepth deep */
    std::function<int(h2y_ctx *, long first)> arm;  /* its stages, once the reference file is open (empty: none) */
    size_t src_frame_bytes = 0;         /* of the one raw source file run_block opens and seeks; 0: the flow has none */
    std::function<std::string(long, FILE *, void *const *)> fill; /* frame k (of that file, where there is one) into the slot's planes */
    bool ref_rgb = false;               /* frame k of --ref_filename, where given, as read_ref takes it */
    size_t ref_plane_bytes = 0, ref_frame_bytes = 0;
    std::function<std::string(long, const uint16_t *)> write; /* frame k as it came down (empty: nothing is written) */
    size_t out_bytes = 0;               /* what write writes */
    bool says_written = false;          /* a written frame prints the --verbose_level line */
};

/* Frames [first, first + count) of the run through one context's pinned ring, the same way for every flow: frame k filled into a
 * slot (and frame k of the reference beside it), submitted, and with two frames in flight the oldest taken out, measured and
 * written.  Returns "" or the block's error; the guard tears down on every way out. */
static std::string run_block(const cli_args &a, const flow &fl, results &res, int r, block *b)
{
    struct guard {
        h2y_ctx *ctx = nullptr;
        FILE *src = nullptr, *ref = nullptr;
        ~guard()
        {
            if (ctx) { h2y_stream_close(ctx); h2y_ctx_destroy(ctx); } /* (closing is a no-op when no ring was opened) */
            if (src) fclose(src);
            if (ref) fclose(ref);
        }
    } g;
    if (h2y_ctx_create(b->device, &g.ctx)) return h2y_last_error(nullptr);
    auto library = [&] { return std::string(h2y_last_error(g.ctx)); };
    if (fl.src_frame_bytes) {
        g.src = fopen(a.src, "rb");
        if (!g.src) return std::string("unable to open file ") + a.src;
        if (fseeko(g.src, (off_t)fl.src_frame_bytes * (off_t)(a.start_frame + b->first), SEEK_SET)) return "seek failed"; /* hdr2yuv.cpp:624 */
    }
    if (fl.open(g.ctx, b->first)) return library();
    if (a.ref) { /* R from its frame 0 on: this block's frames start at `first` */
        g.ref = fopen(a.ref, "rb");
        if (!g.ref || fseeko(g.ref, (off_t)fl.ref_frame_bytes * (off_t)b->first, SEEK_SET)) return std::string("unable to read ") + a.ref;
    }
    if (fl.arm && fl.arm(g.ctx, b->first)) return library();
    long in_flight = 0;
    auto drain_one = [&]() -> std::string {
        const uint16_t *out = nullptr;
        if (h2y_stream_output(g.ctx, &out)) return library();
        const long k = b->first + b->done;
        if (!res.take(a, g.ctx, k, r)) return library();
        if (fl.write) {
            const std::string err = fl.write(k, out);
            if (!err.empty()) return err;
            if (fl.says_written) printf("frame %ld: %zu bytes written to %s (device %d)\n", k, fl.out_bytes, a.dst, b->device);
        }
        b->done++;
        in_flight--;
        return "";
    };
    for (long f = 0; f < b->count; f++) {
        void *planes[3];
        if (h2y_stream_input(g.ctx, planes)) return library();
        std::string err = fl.fill(b->first + f, g.src, planes);
        if (!err.empty()) return err;
        if (g.ref) {
            void *ref = nullptr;
            if (h2y_stream_reference(g.ctx, &ref)) return library();
            if (!read_ref(g.ref, fl.ref_rgb, fl.ref_plane_bytes, fl.ref_frame_bytes, ref)) return std::string("short read from ") + a.ref;
        }
        if (h2y_stream_submit(g.ctx)) return library();
        in_flight++;
        if (in_flight == kRingDepth - 1 && !(err = drain_one()).empty()) return err;
    }
    while (in_flight > 0) {
        const std::string err = drain_one();
        if (!err.empty()) return err;
    }
    return "";
}

/* frame k at `base + k x bytes` of the one destination file */
static std::function<std::string(long, const uint16_t *)> write_plain(const job &j, size_t bytes)
{
    return [&j, bytes](long k, const uint16_t *out) {
        return write_at(j.fd_out, out, bytes, j.base + (off_t)k * (off_t)bytes) ? "" : std::string("short write to ") + j.a.dst;
    };
}

/* the same for a .rgb: planes G, B, R of plane_bytes each -> file order R, G, B (write_tiff: R, G, B per pixel) */
static std::function<std::string(long, const uint16_t *)> write_rgb(const job &j, size_t plane_bytes)
{
    return [&j, plane_bytes](long k, const uint16_t *out) {
        const char *p = reinterpret_cast<const char *>(out);
        const off_t at = j.base + (off_t)k * (off_t)(3 * plane_bytes);
        return write_at(j.fd_out, p + 2 * plane_bytes, plane_bytes, at) && write_at(j.fd_out, p, 2 * plane_bytes, at + (off_t)plane_bytes)
                   ? "" : std::string("short write to ") + j.a.dst;
    };
}

/* forward path: the ring of h2y_stream_open, or for .dpx, .tiff and .exr the ring that decodes on the device what the file holds
 * (frame k is file k of the scan) */
static flow forward_flow(const job &j)
{
    const cli_args &a = j.a;
    const scanned &s = j.src;
    const size_t pb = h2y_plane_bytes(&j.d);
    flow f;
    f.open = [&j, &a, &s](h2y_ctx *ctx, long) {
        if (a.siting && h2y_ctx_set_chroma_siting(ctx, a.siting)) return (int)H2Y_EINVAL; /* before the ring is opened */
        /* the inverse siting serves --linearize's upsampler and --delta_e's (cli_resolve_delta_e has them agree where both upsample) */
        const int inv_siting = a.linearize && a.src_siting ? a.src_siting : a.delta_e ? a.de_siting : 0;
        if (inv_siting && h2y_ctx_set_inverse_chroma_siting(ctx, inv_siting)) return (int)H2Y_EINVAL;
        if (a.linearize) { /* the file's PQ codes, linearised on the device into the planes j.d describes */
            const h2y_codelight_desc code{a.lin.width, a.lin.height, a.lin.chroma_format_idc, a.lin.bit_depth, a.lin.video_full_range_flag,
                                          a.lin.matrix_coeffs, a.resampler};
            if (a.src_hlg == 1) return opened(h2y_hlgcode_stream_open(ctx, &j.d, &code, a.src_hlg_peak, kRingDepth), a, ctx); /* the file's codes are HLG's */
            if (a.src_sdr == 1) return opened(h2y_sdrcode_stream_open(ctx, &j.d, &code, a.src_sdr_white, kRingDepth), a, ctx); /* the file's codes are BT.1886's */
            if (a.src_signal == 1) /* the codes stay signal for the LUT, which this ring arms as it opens */
                return opened(h2y_sigcode_stream_open(ctx, &j.d, &code, a.lut3d_table, a.lut3d_interp, kRingDepth), a, ctx);
            return opened(h2y_pqcode_stream_open(ctx, &j.d, &code, kRingDepth), a, ctx);
        }
        return a.in_type == CLI_IN_DPX    ? h2y_dpx_stream_open(ctx, &j.d, &s.di, kRingDepth)
               : a.in_type == CLI_IN_TIFF ? h2y_tiff_stream_open(ctx, &j.d, &s.ti, a.in.video_full_range_flag == 0, kRingDepth)
               : a.in_type == CLI_IN_EXR  ? h2y_exr_stream_open(ctx, &j.d, &s.xi, kRingDepth)
                                          : h2y_stream_open(ctx, &j.d, kRingDepth);
    };
    f.arm = [&a](h2y_ctx *ctx, long first) {
        return (a.ref && h2y_stream_compare(ctx, a.sigma, a.dst ? 1 : 0)) || (a.ssim && h2y_stream_ssim(ctx, -1)) || (a.regions && h2y_stream_regions(ctx, a.regions_flat_var, a.regions_radius)) ||
               (a.delta_e && h2y_stream_deltae(ctx, &a.de, a.delta_e_threshold)) ||
               (a.hist && h2y_stream_histogram(ctx, a.hist_bits)) || (a.light && h2y_stream_light(ctx)) ||
               (a.dynmeta && h2y_stream_lightdist(ctx)) || (a.scene_detect == 1 && h2y_stream_scenesig(ctx)) ||
               (a.gamut && !a.gamut_compress && h2y_stream_gamut(ctx, a.in.colour_primaries, a.out.colour_primaries, a.gamut_clip)) ||
               (a.gamut && a.gamut_compress && h2y_stream_gamut_compress(ctx, a.in.colour_primaries, a.out.colour_primaries,
                                                                         a.gamut_compress_threshold, a.gamut_compress_power)) ||
               (a.tone_map && h2y_stream_tonemap(ctx, a.tone_src_peak, a.tone_dst_peak, a.tone_relative)) ||
               (a.lut3d_table && a.src_signal != 1 && h2y_stream_lut3d(ctx, a.lut3d_table, a.lut3d_interp, a.lut3d_signal)) ||
               (a.hlg == 1 && h2y_stream_hlg(ctx, a.hlg_peak, a.hlg_relative)) || (a.ictcp == 1 && h2y_stream_ictcp(ctx)) ||
               (a.scale && h2y_stream_scale(ctx, a.out.width, a.out.height, a.scale_taps)) ||
               (a.dithers() && h2y_stream_dither(ctx, a.dither_to, a.dither, a.dither_temporal, a.dither_seed, (uint32_t)first)) || /* after scale */
               (a.dst_pack && h2y_stream_pack(ctx, a.dst_pack));                                                                      /* last */
    };
    if (a.linearize) { /* the code frame whole, as whole_frame_flow reads it: one read, a .rgb with its planes put in G, B, R order */
        const bool rgb = a.lin_type == CLI_IN_RGB;
        const size_t plane = (size_t)a.lin.width * a.lin.height * 2, frame = j.in_frame_bytes;
        f.src_frame_bytes = frame;
        f.fill = [&a, rgb, plane, frame](long, FILE *src, void *const *planes) {
            return read_ref(src, rgb, plane, frame, planes[0]) ? "" : std::string("short read from ") + a.src;
        };
    } else if (a.in_type == CLI_IN_DPX) { /* the payload as the file holds it, straight into the pinned slot */
        f.fill = [&s](long k, FILE *, void *const *planes) -> std::string {
            const dpx_src &src = s.dpx[k];
            FILE *fd = fopen(src.path.c_str(), "rb");
            if (!fd) return "unable to open file " + src.path;
            size_t got = 0;
            if (!fseeko(fd, (off_t)src.offset, SEEK_SET)) got = fread(planes[0], 1, s.di.payload_bytes, fd);
            fclose(fd);
            return got == s.di.payload_bytes ? "" : "only " + std::to_string(got) + " payload bytes read from " + src.path;
        };
    } else if (a.in_type == CLI_IN_TIFF) { /* the decoded rows, whole: one read when they lie back to back, else one per row */
        f.fill = [&s](long k, FILE *, void *const *planes) -> std::string {
            const tiff_src &src = s.tiff[k];
            const int fd = open(src.path.c_str(), O_RDONLY);
            if (fd < 0) return "unable to open file " + src.path;
            bool ok = true;
            char *dst = static_cast<char *>(planes[0]);
            if (src.contiguous) ok = read_at(fd, dst, s.ti.payload_bytes, (off_t)src.rows[0]);
            else
                for (size_t r = 0; ok && r < src.rows.size(); r++) ok = read_at(fd, dst + r * s.ti.row_bytes, s.ti.row_bytes, (off_t)src.rows[r]);
            close(fd);
            return ok ? "" : "short read from " + src.path;
        };
    } else if (a.in_type == CLI_IN_EXR) { /* parsed again (the file may have changed since the scan), unpacked into the slot */
        struct unpacker { /* this block's own (a flow is made per block) */
            unpack_pool pool;
            std::vector<h2y_exr_chunk> chunks;
            unpacker(int threads, int n_chunks) : pool(threads), chunks((size_t)n_chunks) {}
        };
        auto u = std::make_shared<unpacker>(std::max(1, kUnpackThreads / std::max(1, a.gpus)), s.xi.n_chunks);
        f.fill = [&s, u](long k, FILE *, void *const *planes) -> std::string {
            const std::string &path = s.exr[k];
            mapped_file m;
            if (!m.open(path)) return "read_exr() (exr.cpp:146): unable to open or read file " + path;
            h2y_exr_info x2;
            const char *why = nullptr;
            if (h2y_exr_parse(m.p, m.n, &x2, u->chunks.data(), s.xi.n_chunks, &why)) return "read_exr() (exr.cpp): " + path + ": " + why;
            if (memcmp(&x2, &s.xi, sizeof s.xi)) return "read_exr() (exr.cpp): " + path + " no longer has the header the run started with";
            const std::string err = u->pool.run(s.xi, u->chunks.data(), m.p, planes[0]);
            return err.empty() ? err : "read_exr() (exr.cpp): " + path + ": " + err;
        };
    } else if (a.in_type == CLI_IN_SYNTH) {
        f.fill = [&j, &a](long k, FILE *, void *const *planes) {
            synth_fill(j.d, planes, 12345u + (uint32_t)(a.synthetic + a.start_frame + k));
            return std::string();
        };
    } else { /* .yuv, .rgb, .f32, .f16: three planes of the one source file */
        f.src_frame_bytes = 3 * pb;
        f.fill = [&a, pb](long, FILE *src, void *const *planes) -> std::string {
            /* file plane order -> memory planes (0=G/Y, 1=B/Cb, 2=R/Cr); .rgb holds R,G,B (hdr2yuv.cpp:635-637) */
            const int order_rgb[3] = {2, 0, 1}, order_nat[3] = {0, 1, 2};
            const int *ord = a.in_type == CLI_IN_RGB ? order_rgb : order_nat;
            size_t got = 0;
            for (int p = 0; p < 3; p++) got += fread(planes[ord[p]], 1, pb, src);
            return got == 3 * pb ? "" : "only " + std::to_string(got) + " bytes read from " + a.src + ", expecting " + std::to_string(3 * pb);
        };
    }
    f.ref_frame_bytes = h2y_frame_bytes(&j.d);
    f.out_bytes = j.out_frame_bytes; /* what comes down: the converted frame, or under --scale the scaled one */
    if (a.dst) f.write = write_plain(j, f.out_bytes);
    f.says_written = a.verbose > 0;
    return f;
}

/* .yuv -> RGB (matrix_inverse): the inverse ring; .tiff output: the ring with the interleave (h2y_tiff_inverse_stream_open), frame
 * k into its own file, head + samples + tail */
static flow inverse_flow(const job &j)
{
    const cli_args &a = j.a;
    const bool tiff = a.out_type == CLI_OUT_TIFF;
    const size_t luma = (size_t)a.in.width * a.in.height * 2, chroma = (j.in_frame_bytes - luma) / 2, out_frame = j.out_frame_bytes;
    flow f;
    f.open = [&a, tiff](h2y_ctx *ctx, long) {
        if (a.src_siting && h2y_ctx_set_inverse_chroma_siting(ctx, a.src_siting)) return (int)H2Y_EINVAL; /* before the ring is opened */
        return opened((tiff ? h2y_tiff_inverse_stream_open : h2y_inverse_stream_open)(ctx, a.in.width, a.in.height, a.in.chroma_format_idc,
                                                                                     a.in.bit_depth, a.in.video_full_range_flag, a.in.matrix_coeffs,
                                                                                     a.out.bit_depth, a.resampler, kRingDepth), a, ctx);
    };
    f.arm = [&a](h2y_ctx *ctx, long) {
        return (a.ref && h2y_stream_compare(ctx, a.sigma, a.dst ? 1 : 0)) || (a.ssim && h2y_stream_ssim(ctx, -1)) || (a.regions && h2y_stream_regions(ctx, a.regions_flat_var, a.regions_radius)) ||
               (a.hist && h2y_stream_histogram(ctx, a.hist_bits));
    };
    f.src_frame_bytes = j.in_frame_bytes;
    const size_t packed = a.src_pack ? j.in_frame_bytes : 0; /* --src_pack: the slot lends one packed frame */
    f.fill = [&a, luma, chroma, packed](long, FILE *src, void *const *planes) {
        const size_t got = packed ? fread(planes[0], 1, packed, src)
                                  : fread(planes[0], 1, luma, src) + fread(planes[1], 1, chroma, src) + fread(planes[2], 1, chroma, src);
        return got == (packed ? packed : luma + 2 * chroma) ? "" : std::string("short read from ") + a.src;
    };
    f.ref_rgb = true, f.ref_plane_bytes = luma, f.ref_frame_bytes = out_frame;
    f.out_bytes = out_frame;
    if (a.dst && tiff)
        f.write = [&j, &a, out_frame](long k, const uint16_t *gbr) { /* TIFFOpen(filename, "w"): a new file */
            const std::string path = cli_frame_name(a.dst, a.start_frame + k);
            const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
            const bool ok = fd >= 0 && write_at(fd, j.tw.head, sizeof j.tw.head, 0) && write_at(fd, gbr, out_frame, sizeof j.tw.head) &&
                            write_at(fd, j.tw.tail.data(), j.tw.tail.size(), (off_t)(sizeof j.tw.head + out_frame));
            if (fd >= 0) close(fd);
            return ok ? "" : "unable to write " + path;
        };
    else if (a.dst) f.write = write_rgb(j, luma);
    return f;
}

/* the source of the four flows that convert nothing, .yuv or .rgb: the slot's planes lie one after the other, so a frame is
 * one read, a .rgb one with its planes put in G, B, R order */
static flow whole_frame_flow(const job &j)
{
    const cli_args &a = j.a;
    const bool rgb = a.in_type == CLI_IN_RGB;
    const size_t plane = (size_t)a.in.width * a.in.height * 2, frame = j.in_frame_bytes;
    flow f;
    f.src_frame_bytes = frame;
    f.fill = [&a, rgb, plane, frame](long, FILE *src, void *const *planes) {
        return read_ref(src, rgb, plane, frame, planes[0]) ? "" : std::string("short read from ") + a.src;
    };
    f.ref_rgb = rgb, f.ref_plane_bytes = plane, f.ref_frame_bytes = frame; /* --compare_only: R has the source's layout */
    return f;
}

/* --compare_only: the source against the same frames of R through one compare-only ring */
static flow compare_flow(const job &j)
{
    const cli_args &a = j.a;
    flow f = whole_frame_flow(j);
    f.open = [&a](h2y_ctx *ctx, long) {
        if (a.delta_e && a.de_siting && h2y_ctx_set_inverse_chroma_siting(ctx, a.de_siting)) return (int)H2Y_EINVAL; /* before the ring is opened */
        return opened(h2y_compare_stream_open(ctx, a.in.width, a.in.height, a.in.chroma_format_idc, a.sigma, kRingDepth), a, ctx);
    };
    f.arm = [&a](h2y_ctx *ctx, long) {
        return (a.ssim && h2y_stream_ssim(ctx, a.in.bit_depth)) || (a.regions && h2y_stream_regions(ctx, a.regions_flat_var, a.regions_radius)) || (a.delta_e && h2y_stream_deltae(ctx, &a.de, a.delta_e_threshold)) ||
               (a.hist && h2y_stream_histogram_ex(ctx, a.hist_bits, a.hist_depth, a.hist_full, a.hist_gbr));
    };
    return f;
}

/* --histogram_only: the source through one histogram-only ring */
static flow histogram_flow(const job &j)
{
    const cli_args &a = j.a;
    flow f = whole_frame_flow(j);
    f.open = [&a](h2y_ctx *ctx, long) {
        return opened(h2y_histogram_stream_open(ctx, a.in.width, a.in.height, a.in.chroma_format_idc, a.hist_depth, a.hist_full, a.hist_gbr,
                                                a.hist_bits, kRingDepth), a, ctx);
    };
    return f;
}

/* --light_only: the source's PQ code planes through one light-only ring */
static flow light_flow(const job &j)
{
    const cli_args &a = j.a;
    flow f = whole_frame_flow(j);
    f.open = [&a](h2y_ctx *ctx, long) {
        if (a.src_siting && h2y_ctx_set_inverse_chroma_siting(ctx, a.src_siting)) return (int)H2Y_EINVAL; /* before the ring is opened */
        const h2y_codelight_desc d{a.in.width, a.in.height, a.in.chroma_format_idc, a.in.bit_depth, a.in.video_full_range_flag,
                                   a.in.matrix_coeffs, a.resampler};
        return opened(h2y_codelight_stream_open(ctx, &d, a.dynmeta ? 1 : 0, kRingDepth), a, ctx);
    };
    if (a.scene_detect == 1 || a.gamut_check == 1)
        f.arm = [&a](h2y_ctx *ctx, long) {
            return (a.scene_detect == 1 && h2y_stream_scenesig(ctx)) ||
                   (a.gamut_check == 1 && h2y_stream_gamutcheck(ctx, a.in.colour_primaries, a.gamut_check_n_sets, a.gamut_check_sets,
                                                                a.gamut_check_ratio, a.gamut_check_floor));
        };
    return f;
}

/* --scale_only: the source through one scale-only ring into the destination */
static flow scale_flow(const job &j)
{
    const cli_args &a = j.a;
    const bool rgb = a.in_type == CLI_IN_RGB;
    flow f = whole_frame_flow(j);
    f.open = [&a, rgb](h2y_ctx *ctx, long) {
        return opened(h2y_scale_stream_open(ctx, a.in.width, a.in.height, a.in.chroma_format_idc, a.in.bit_depth, a.in.video_full_range_flag,
                                            rgb ? 1 : 0, a.out.width, a.out.height, a.scale_taps, kRingDepth), a, ctx);
    };
    if (a.dst_pack) f.arm = [&a](h2y_ctx *ctx, long) { return h2y_stream_pack(ctx, a.dst_pack); };
    f.out_bytes = j.out_frame_bytes;
    f.write = rgb ? write_rgb(j, (size_t)a.out.width * a.out.height * 2) : write_plain(j, f.out_bytes);
    f.says_written = a.verbose > 0;
    return f;
}

/* --dither_only: the source through one dither-only ring into the destination, the block's frames numbered from its first */
static flow dither_flow(const job &j)
{
    const cli_args &a = j.a;
    const bool rgb = a.in_type == CLI_IN_RGB;
    flow f = whole_frame_flow(j);
    f.open = [&a, rgb](h2y_ctx *ctx, long first) {
        return opened(h2y_dither_stream_open(ctx, a.in.width, a.in.height, a.in.chroma_format_idc, a.dither_from, a.dither_to,
                                             a.in.video_full_range_flag, rgb ? 1 : 0, a.dither, a.dither_temporal, a.dither_seed, (uint32_t)first,
                                             kRingDepth), a, ctx);
    };
    if (a.dst_pack) f.arm = [&a](h2y_ctx *ctx, long) { return h2y_stream_pack(ctx, a.dst_pack); };
    f.out_bytes = j.out_frame_bytes;
    f.write = rgb ? write_rgb(j, (size_t)a.in.width * a.in.height * 2) : write_plain(j, f.out_bytes);
    f.says_written = a.verbose > 0;
    return f;
}

/* the histogram report of the header comment and FILE; returns the exit status (4: --check_range 1 and samples outside) */
static int histogram_report(const cli_args &a, const std::vector<h2y_histogram_stats> &st, const std::vector<std::array<uint32_t, 3>> &occ,
                            const std::vector<uint64_t> &total)
{
    static const char *const kYuv[3] = {"Y", "Cb", "Cr"}, *const kRgb[3] = {"G", "B", "R"};
    const char *const *name = a.hist_gbr ? kRgb : kYuv;
    const size_t nbins = (size_t)1 << a.hist_bits;
    uint64_t below[3] = {0, 0, 0}, above[3] = {0, 0, 0}, at_low[3] = {0, 0, 0}, at_high[3] = {0, 0, 0};
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0, 0, 0};
    auto plane = [&](int p, uint32_t lo, uint32_t hi, uint64_t b, uint64_t ab, uint64_t l, uint64_t h, uint32_t o) {
        printf(" %s min %u max %u below %llu above %llu at_low %llu at_high %llu occupied %u", name[p], lo, hi, (unsigned long long)b,
               (unsigned long long)ab, (unsigned long long)l, (unsigned long long)h, o);
    };
    for (size_t k = 0; k < st.size(); k++) {
        const h2y_histogram_stats &s = st[k];
        printf("histogram frame %zu", k);
        for (int p = 0; p < 3; p++) {
            plane(p, s.min[p], s.max[p], s.below[p], s.above[p], s.at_low[p], s.at_high[p], occ[k][p]);
            below[p] += s.below[p], above[p] += s.above[p], at_low[p] += s.at_low[p], at_high[p] += s.at_high[p];
            if (s.samples[p]) mn[p] = std::min(mn[p], s.min[p]), mx[p] = std::max(mx[p], s.max[p]);
        }
        printf("\n");
    }
    printf("histogram summary frames %zu", st.size());
    uint64_t outside = 0;
    for (int p = 0; p < 3; p++) {
        uint32_t o = 0;
        for (size_t i = 0; i < nbins; i++) o += total[p * nbins + i] != 0u;
        plane(p, mn[p] == 0xFFFFFFFFu ? 0u : mn[p], mx[p], below[p], above[p], at_low[p], at_high[p], o);
        outside += below[p] + above[p];
    }
    printf("\nhistogram legal");
    for (int p = 0; p < 3; p++) printf(" %s %u..%u", name[p], st.empty() ? 0u : st[0].lo[p], st.empty() ? 0u : st[0].hi[p]);
    printf(" outside %llu\n", (unsigned long long)outside);
    FILE *f = fopen(a.hist, "w");
    if (!f) {
        printf("ERROR: unable to write %s\n", a.hist);
        return 1;
    }
    const uint32_t shift = (uint32_t)(a.hist_depth - a.hist_bits);
    fprintf(f, "bin,code_lo,code_hi,%s,%s,%s\n", name[0], name[1], name[2]);
    for (size_t i = 0; i < nbins; i++)
        fprintf(f, "%zu,%zu,%zu,%llu,%llu,%llu\n", i, i << shift, ((i + 1) << shift) - 1, (unsigned long long)total[i],
                (unsigned long long)total[nbins + i], (unsigned long long)total[2 * nbins + i]);
    if (fclose(f)) {
        printf("ERROR: unable to write %s\n", a.hist);
        return 1;
    }
    return a.check_range && outside ? 4 : 0;
}

static std::string psnr_str(uint64_t maxv, uint64_t n, uint64_t sse)
{
    if (sse == 0) return "inf";
    char buf[64];
    snprintf(buf, sizeof buf, "%.4f", 10.0 * log10((double)maxv * maxv * n / sse));
    return buf;
}

/* the report of the header comment; returns the exit status (3: over-sigma samples with --sigma_compare given) */
static int compare_report(const cli_args &a, bool yuv, int bit_depth, const std::vector<h2y_compare_stats> &st)
{
    static const char *const kYuv[3] = {"Y", "Cb", "Cr"}, *const kRgb[3] = {"G", "B", "R"};
    const char *const *name = yuv ? kYuv : kRgb;
    const uint64_t maxv = (1ull << bit_depth) - 1;
    uint64_t n[3] = {0, 0, 0}, sse[3] = {0, 0, 0}, over[3] = {0, 0, 0};
    uint32_t mx[3] = {0, 0, 0};
    double mean[3] = {0, 0, 0};
    long first_f = -1;
    int first_p = -1;
    for (size_t k = 0; k < st.size(); k++) {
        const h2y_compare_stats &s = st[k];
        printf("frame %zu psnr", k);
        for (int p = 0; p < 3; p++) printf(" %s %s", name[p], psnr_str(maxv, s.samples[p], s.sse[p]).c_str());
        printf(" max_abs %u %u %u over %llu %llu %llu\n", s.max_abs[0], s.max_abs[1], s.max_abs[2], (unsigned long long)s.over[0],
               (unsigned long long)s.over[1], (unsigned long long)s.over[2]);
        for (int p = 0; p < 3; p++) {
            n[p] += s.samples[p], sse[p] += s.sse[p], over[p] += s.over[p];
            mx[p] = std::max(mx[p], s.max_abs[p]);
            mean[p] += s.sse[p] ? 10.0 * log10((double)maxv * maxv * s.samples[p] / s.sse[p]) : 99.99;
            if (first_f < 0 && s.over[p]) first_f = (long)k, first_p = p;
        }
    }
    printf("summary frames %zu mean_psnr", st.size());
    for (int p = 0; p < 3; p++) printf(" %s %.4f", name[p], st.empty() ? 0.0 : mean[p] / (double)st.size());
    printf(" global_psnr");
    for (int p = 0; p < 3; p++) printf(" %s %s", name[p], psnr_str(maxv, n[p], sse[p]).c_str());
    printf(" max_abs %u %u %u over %llu %llu %llu\n", mx[0], mx[1], mx[2], (unsigned long long)over[0], (unsigned long long)over[1],
           (unsigned long long)over[2]);
    if (first_f < 0) printf("first_over none\n");
    else {
        const h2y_compare_stats &s = st[(size_t)first_f];
        const bool sub = yuv && a.out.chroma_format_idc == H2Y_CHROMA_420 && first_p > 0;
        const uint64_t w = sub ? (uint64_t)(a.out.width >> 1) : (uint64_t)a.out.width, i = (uint64_t)s.first_over[first_p];
        printf("first_over frame %ld plane %s x %llu y %llu a %u b %u\n", first_f, name[first_p], (unsigned long long)(i % w),
               (unsigned long long)(i / w), s.first_a[first_p], s.first_b[first_p]);
    }
    return a.sigma_given && first_f >= 0 ? 3 : 0;
}

static std::string ssim_db(double x)
{
    if (x >= 1.0) return "inf";
    char s[32];
    snprintf(s, sizeof s, "%.4f", -10.0 * log10(1.0 - x));
    return s;
}

/* the SSIM report of the header comment */
static void ssim_report(bool yuv, const std::vector<h2y_ssim_stats> &st)
{
    static const char *const kYuv[3] = {"Y", "Cb", "Cr"}, *const kRgb[3] = {"G", "B", "R"};
    const char *const *name = yuv ? kYuv : kRgb;
    auto line = [&](const double (&v)[3], double all) {
        for (int p = 0; p < 3; p++) printf(" %s %.6f", name[p], v[p]);
        printf(" all %.6f db", all);
        for (int p = 0; p < 3; p++) printf(" %s %s", name[p], ssim_db(v[p]).c_str());
        printf(" all %s\n", ssim_db(all).c_str());
    };
    double mean[3] = {0, 0, 0}, mean_all = 0;
    size_t worst = 0;
    for (size_t k = 0; k < st.size(); k++) {
        printf("ssim frame %zu", k);
        line(st[k].ssim, st[k].all);
        for (int p = 0; p < 3; p++) mean[p] += st[k].ssim[p];
        mean_all += st[k].all;
        if (st[k].all < st[worst].all) worst = k;
    }
    if (st.empty()) return;
    for (int p = 0; p < 3; p++) mean[p] /= (double)st.size();
    printf("ssim summary frames %zu", st.size());
    line(mean, mean_all / (double)st.size());
    printf("ssim worst frame %zu all %.6f\n", worst, st[worst].all);
}

/* the regions report of the header comment */
static void regions_report(bool yuv, int bit_depth, const std::vector<h2y_regions_stats> &st)
{
    static const char *const kYuv[3] = {"Y", "Cb", "Cr"}, *const kRgb[3] = {"G", "B", "R"};
    const char *const *name = yuv ? kYuv : kRgb;
    const uint64_t maxv = (1ull << bit_depth) - 1;
    auto ratio = [](uint64_t num, uint64_t den, const char *fmt) -> std::string {
        if (!den) return "-";
        char buf[64];
        snprintf(buf, sizeof buf, fmt, (double)num / (double)den);
        return buf;
    };
    auto triple = [](const char *key, const uint64_t (&v)[3]) {
        printf(" %s %llu %llu %llu", key, (unsigned long long)v[0], (unsigned long long)v[1], (unsigned long long)v[2]);
    };
    /* flat_share and the two PSNRs of one set of per-class sums */
    auto classes = [&](const uint64_t (&n)[3][2], const uint64_t (&sse)[3][2], const char *flat, const char *busy) {
        printf(" flat_share");
        for (int p = 0; p < 3; p++) printf(" %s %s", name[p], ratio(n[p][0], n[p][0] + n[p][1], "%.6f").c_str());
        for (int c = 0; c < 2; c++) {
            printf(" %s", c ? busy : flat);
            for (int p = 0; p < 3; p++) printf(" %s %s", name[p], n[p][c] ? psnr_str(maxv, n[p][c], sse[p][c]).c_str() : "-");
        }
    };
    h2y_regions_stats t{};
    for (size_t k = 0; k < st.size(); k++) {
        const h2y_regions_stats &s = st[k];
        printf("regions frame %zu", k);
        classes(s.samples, s.sse, "psnr_flat", "psnr_busy");
        triple("over", s.over);
        printf(" over_max %u %u %u", s.over_max[0], s.over_max[1], s.over_max[2]);
        triple("under", s.under);
        printf(" under_max %u %u %u\n", s.under_max[0], s.under_max[1], s.under_max[2]);
        for (int p = 0; p < 3; p++) {
            for (int c = 0; c < 2; c++) t.samples[p][c] += s.samples[p][c], t.sse[p][c] += s.sse[p][c];
            t.over[p] += s.over[p], t.over_sum[p] += s.over_sum[p], t.under[p] += s.under[p], t.under_sum[p] += s.under_sum[p];
            t.over_max[p] = std::max(t.over_max[p], s.over_max[p]), t.under_max[p] = std::max(t.under_max[p], s.under_max[p]);
        }
    }
    if (st.empty()) return;
    printf("regions summary frames %zu", st.size());
    classes(t.samples, t.sse, "global_psnr_flat", "global_psnr_busy");
    triple("over", t.over);
    printf(" over_mean");
    for (int p = 0; p < 3; p++) printf(" %s %s", name[p], ratio(t.over_sum[p], t.over[p], "%.4f").c_str());
    printf(" over_max %u %u %u", t.over_max[0], t.over_max[1], t.over_max[2]);
    triple("under", t.under);
    printf(" under_mean");
    for (int p = 0; p < 3; p++) printf(" %s %s", name[p], ratio(t.under_sum[p], t.under[p], "%.4f").c_str());
    printf(" under_max %u %u %u\n", t.under_max[0], t.under_max[1], t.under_max[2]);
}

/* the Delta E report of the header comment; returns the exit status (5: --delta_e_limit given and a frame's mean above it) */
static int deltae_report(const cli_args &a, const std::vector<h2y_deltae_stats> &st)
{
    auto share = [](uint64_t over, uint64_t pixels) { return pixels ? 100.0 * (double)over / (double)pixels : 0.0; };
    double mean = 0;
    size_t worst = 0, top = 0;
    uint64_t over = 0, pixels = 0;
    bool beyond = false;
    for (size_t k = 0; k < st.size(); k++) {
        const h2y_deltae_stats &t = st[k];
        printf("delta_e: frame %zu mean %.6f max %.6f at %u %u over %llu share %.4f\n", k, t.mean, t.max, t.max_x, t.max_y,
               (unsigned long long)t.over, share(t.over, t.pixels));
        mean += t.mean;
        over += t.over, pixels += t.pixels;
        if (t.mean > st[worst].mean) worst = k;
        if (t.max > st[top].max) top = k;
        beyond = beyond || t.mean > a.delta_e_limit;
    }
    if (st.empty()) return 0;
    printf("delta_e: summary frames %zu mean %.6f worst frame %zu mean %.6f max %.6f frame %zu at %u %u over %llu share %.4f\n", st.size(),
           mean / (double)st.size(), worst, st[worst].mean, st[top].max, top, st[top].max_x, st[top].max_y, (unsigned long long)over,
           share(over, pixels));
    return a.delta_e_limit_given && beyond ? 5 : 0;
}

/* The gamut containment report (--gamut_check 1): per frame and set the pixels outside and beyond with their shares, the largest
 * excursion in cd/m2 with its pixel and the mean; per set a summary.  Returns the exit status (6: --gamut_check_limit given and the
 * share of pixels beyond --gamut_check_against above it in a frame) */
static int gamutcheck_report(const cli_args &a, const std::vector<h2y_gamutcheck_stats> &st)
{
    bool over = false;
    for (size_t k = 0; k < st.size(); k++)
        for (int s = 0; s < st[k].n_sets; s++) {
            const h2y_gamutcheck_set &t = st[k].set[s];
            printf("gamut_check: frame %zu against %d outside %llu share %.6f beyond %llu share %.6f max %.4f at %d %d mean %.6f\n", k,
                   t.primaries, (unsigned long long)t.outside, (double)t.outside / (double)st[k].pixels, (unsigned long long)t.beyond,
                   t.beyond_share, t.max_cdm2, t.max_x, t.max_y, t.mean_cdm2);
            over = over || (t.primaries == a.gamut_check_against && t.beyond_share > a.gamut_check_limit);
        }
    if (st.empty()) return 0;
    for (int s = 0; s < st[0].n_sets; s++) {
        size_t worst = 0, top = 0, with = 0;
        for (size_t k = 0; k < st.size(); k++) {
            const h2y_gamutcheck_set &t = st[k].set[s];
            with += t.beyond > 0;
            if (t.beyond_share > st[worst].set[s].beyond_share) worst = k;
            if (t.max_bits > st[top].set[s].max_bits) top = k;
        }
        printf("gamut_check: summary against %d frames %zu frames_beyond %zu worst frame %zu share %.6f max %.4f frame %zu at %d %d\n",
               st[0].set[s].primaries, st.size(), with, worst, st[worst].set[s].beyond_share, st[top].set[s].max_cdm2, top,
               st[top].set[s].max_x, st[top].set[s].max_y);
    }
    return a.gamut_check_limit_given && over ? 6 : 0;
}

/* the content light report of the header comment */
static void light_report(const std::vector<h2y_light_stats> &st)
{
    size_t kc = 0, kf = 0;
    for (size_t k = 0; k < st.size(); k++) {
        printf("light frame %zu peak %.4f at %u %u average %.4f\n", k, st[k].cll, st[k].x, st[k].y, st[k].fall);
        if (st[k].cll > st[kc].cll) kc = k;
        if (st[k].fall > st[kf].fall) kf = k;
    }
    if (st.empty()) return;
    const long long cll = llround(st[kc].cll), fall = llround(st[kf].fall);
    printf("light summary frames %zu maxcll %lld frame %zu maxfall %lld frame %zu\n", st.size(), cll, kc, fall, kf);
    printf("light x265 --max-cll \"%lld,%lld\"\n", cll, fall);
    printf("light svt-av1 --content-light %lld,%lld\n", cll, fall);
}

/* `text` into the file `path`; false when it could not be written */
static bool write_text(const char *path, const std::string &text)
{
    FILE *f = fopen(path, "w");
    bool ok = f && fwrite(text.data(), 1, text.size(), f) == text.size();
    if (f && fclose(f)) ok = false;
    return ok;
}

/* The scenes of the run's frames: detected from the signatures (with a line per distance) or as --scene_cuts names them; their
 * figures merged from the frames' and printed; `text` becomes the scene-based JSON, and --scene_qpfile's OUT is written.  0, or 1 */
static int scene_report(const cli_args &a, const results &res, std::string &text)
{
    const std::vector<h2y_lightdist_stats> &st = res.lightdist;
    const int n = (int)st.size();
    std::vector<int32_t> id((size_t)n, 0);
    if (a.scene_detect == 1) {
        if (!h2y_scene_cuts(res.scenesig.data(), n, a.scene_threshold, id.data())) {
            printf("ERROR: the scene cuts could not be found\n");
            return 1;
        }
        for (int k = 1; k < n; k++)
            printf("scene: frame %d distance %.6f%s\n", k, h2y_scene_distance(&res.scenesig[k - 1], &res.scenesig[k]), id[k] != id[k - 1] ? " cut" : "");
    } else {
        if (a.scene_firsts.back() >= n) {
            printf("ERROR: --scene_cuts names frame %ld, the run had %d frames\n", a.scene_firsts.back(), n);
            return 1;
        }
        size_t s = 0;
        for (int k = 0; k < n; k++) {
            if (s + 1 < a.scene_firsts.size() && a.scene_firsts[s + 1] == k) s++;
            id[k] = (int32_t)s;
        }
    }
    std::vector<h2y_scene_stats> sc((size_t)id[n - 1] + 1);
    if (h2y_scene_merge(st.data(), res.dist_bins.data(), id.data(), n, sc.data(), (int)sc.size()) != (int)sc.size()) {
        printf("ERROR: the scenes' figures could not be merged\n");
        return 1;
    }
    auto nits = [](uint32_t bits) {
        float l;
        memcpy(&l, &bits, sizeof l);
        return 10000.0 * (double)l;
    };
    for (size_t s = 0; s < sc.size(); s++) {
        const h2y_scene_stats &t = sc[s];
        const unsigned __int128 q = ((unsigned __int128)t.sum_q_hi << 64) | t.sum_q_lo;
        printf("scene: %zu first %lld frames %lld maxscl %.4f %.4f %.4f average %.4f percentiles", s, (long long)t.first_frame, (long long)t.n_frames,
               nits(t.maxscl_bits[2]), nits(t.maxscl_bits[0]), nits(t.maxscl_bits[1]), ((10000.0 * (double)q) * 0x1p-32) / (double)t.pixels);
        for (int i = 0; i < H2Y_LIGHTDIST_PERCENTILES; i++) printf(" %.4f", nits(t.pct_bits[i]));
        printf(" below_100 %.4f\n", 100.0 * (double)t.below_100 / (double)t.pixels);
    }
    printf("scene: summary scenes %zu frames %d\n", sc.size(), n);
    text.assign(h2y_lightdist_json_scenes(sc.data(), (int)sc.size(), 0, nullptr, 0), '\0');
    if (!text.empty()) {
        text.resize(text.size() + 1);
        h2y_lightdist_json_scenes(sc.data(), (int)sc.size(), 0, &text[0], text.size());
        text.pop_back();
    }
    if (a.scene_qpfile) {
        std::string qp;
        for (const h2y_scene_stats &t : sc) qp += std::to_string(t.first_frame) + " I\n";
        if (!write_text(a.scene_qpfile, qp)) {
            printf("ERROR: unable to write %s\n", a.scene_qpfile);
            return 1;
        }
        printf("scene_qpfile_written: %zu scenes to %s\n", sc.size(), a.scene_qpfile);
    }
    return 0;
}

/* the dynamic metadata report of the header comment, and FILE (with a scene flag the scene report and the scene-based text); 0, or 1
 * when a file could not be written */
static int lightdist_report(const cli_args &a, const results &res)
{
    const std::vector<h2y_lightdist_stats> &st = res.lightdist;
    auto nits = [](uint32_t bits) {
        float l;
        memcpy(&l, &bits, sizeof l);
        return 10000.0 * (double)l;
    };
    for (size_t k = 0; k < st.size(); k++) {
        const h2y_lightdist_stats &t = st[k];
        printf("dynamic_metadata: frame %zu maxscl %.4f %.4f %.4f average %.4f percentiles", k, nits(t.maxscl_bits[2]), nits(t.maxscl_bits[0]),
               nits(t.maxscl_bits[1]), ((10000.0 * (double)t.sum_q) * 0x1p-32) / (double)t.pixels);
        for (int i = 0; i < H2Y_LIGHTDIST_PERCENTILES; i++) printf(" %.4f", nits(t.pct_bits[i]));
        printf(" below_100 %.4f\n", 100.0 * (double)t.below_100 / (double)t.pixels);
    }
    std::string text;
    if (a.scenes()) {
        if (st.empty() || scene_report(a, res, text)) return 1;
    } else {
        text.assign(h2y_lightdist_json(st.data(), (int)st.size(), 0, nullptr, 0), '\0');
        if (!text.empty()) {
            text.resize(text.size() + 1);
            h2y_lightdist_json(st.data(), (int)st.size(), 0, &text[0], text.size());
            text.pop_back();
        }
    }
    if (text.empty() || !write_text(a.dynmeta, text)) {
        printf("ERROR: unable to write %s\n", a.dynmeta);
        return 1;
    }
    printf("dynamic_metadata_written: %zu frames to %s\n", st.size(), a.dynmeta);
    return 0;
}

int main(int argc, char **argv)
{
    job j;
    cli_args &a = j.a;
    scanned &s = j.src;
    cli_parse(a, argc, argv);
    if ((!a.dst && !a.ref && !a.hist && !a.hist_only && !a.light && !a.dynmeta && !a.scale_only && !a.light_only && !a.dither_given && !a.dither_only_given) ||
        (!a.src && a.synthetic < 0)) {
        if (!a.help) cli_help();
        return a.help ? 0 : 1;
    }
    if (cli_resolve(a)) {
        printf("TOO MANY ARGUMENT ERRORS. ABORTING PROGRAM. --help to show options\n\n"); /* hdr2yuv.cpp:567-572 (which exits 0) */
        return 1;
    }
    /* read_exr() runs before anything else is checked and takes the size from the file: a dry run reads the .exr too */
    if (a.in_type == CLI_IN_EXR) {
        if (exr_scan(a, a.n_frames > 0 ? a.n_frames : 1, s.xi, s.exr)) return 1;
        static const char *const kComp[] = {"NONE", "RLE", "ZIPS", "ZIP"};
        printf("exr: %dx%d data window at (%d, %d), %s, %s y, %d channels, %d unpack threads per GPU\n", s.xi.width, s.xi.height, s.xi.x_min,
               s.xi.y_min, kComp[s.xi.compression], s.xi.line_order ? "decreasing" : "increasing", s.xi.n_channels,
               std::max(1, kUnpackThreads / std::max(1, a.gpus)));
        printf("src_picture: matrix_coeffs %d chroma_format_idc %d bit_depth %d video_full_range_flag %d\n", a.in.matrix_coeffs,
               a.in.chroma_format_idc, a.in.bit_depth, a.in.video_full_range_flag);
    }
    const bool scaling = a.scale == 1 || a.scale_only == 1;
    if (!scaling && (a.out.width != a.in.width || a.out.height != a.in.height)) {
        printf("ERROR: resizing is not part of convert() (cv.cpp is compiled out in the reference); --scale 1 resamples the .yuv frames on "
               "the GPU\n");
        return 1;
    }
    cli_make_desc(a, &j.d);
    /* the flow, and the bytes of one frame as it reads and as it writes them */
    flow (*make_flow)(const job &);
    size_t &in_frame_bytes = j.in_frame_bytes, &out_frame_bytes = j.out_frame_bytes;
    if (a.compare_only || a.hist_only || a.scale_only || a.light_only || a.dither_only) { /* two files of one layout, or one */
        make_flow = a.light_only ? light_flow : a.hist_only ? histogram_flow : a.scale_only ? scale_flow : a.dither_only ? dither_flow : compare_flow;
        in_frame_bytes = out_frame_bytes = planar16_bytes(a.in);
    } else if (a.inverse) {
        if (a.out.bit_depth > 16 || a.in.bit_depth > 16) { printf("ERROR: bit depths must be 8..16 on the inverse flow\n"); return 1; }
        if (a.out.bit_depth < a.in.bit_depth) { /* tiff.cpp:564: SR = dst - src depth, then `R << SR` */
            printf("ERROR: dst bit_depth(%d) < src bit_depth(%d): write_tiff() would shift by a negative count (undefined in the reference)\n", a.out.bit_depth, a.in.bit_depth);
            return 1;
        }
        make_flow = inverse_flow;
        in_frame_bytes = planar16_bytes(a.in);
        out_frame_bytes = 3 * (size_t)a.in.width * a.in.height * 2;
    } else {
        const char *why = nullptr;
        if (h2y_desc_check(&j.d, &why)) { printf("ERROR: %s\n", why); return 1; }
        make_flow = forward_flow;
        in_frame_bytes = a.linearize ? planar16_bytes(a.lin) : 3 * h2y_plane_bytes(&j.d);
        out_frame_bytes = h2y_frame_bytes(&j.d);
    }
    if (scaling) out_frame_bytes = h2y_scale_frame_bytes(a.out.width, a.out.height, a.out.chroma_format_idc); /* the scaled frame's */
    if (a.src_pack) { /* the source's frames, and under --compare_only R's, as the file packs them */
        const cli_pic &file = a.linearize ? a.lin : a.in;
        in_frame_bytes = h2y_pack_frame_bytes(file.width, file.height, file.chroma_format_idc, a.src_pack);
        if (a.compare_only) out_frame_bytes = in_frame_bytes;
    }
    if (a.dst_pack) out_frame_bytes = h2y_pack_frame_bytes(a.out.width, a.out.height, a.out.chroma_format_idc, a.dst_pack);

    /* how many frames there are to do: --n_frames, or what the file holds from --src_start_frame on if that is fewer */
    long frames = a.n_frames > 0 ? a.n_frames : 1;
    struct stat st;
    if (a.in_type == CLI_IN_EXR) frames = (long)s.exr.size();
    else if (a.in_type == CLI_IN_TIFF) { /* as .dpx */
        if (!(a.dry_run && stat(cli_frame_name(a.src, a.start_frame).c_str(), &st))) {
            if (tiff_scan(a, frames, s.ti, s.tiff)) return 1;
            frames = (long)s.tiff.size();
            printf("tiff: %dx%d %s-endian, %d rows per strip, decoded %dx%d from (%d, %d), rows %s\n", s.ti.file_width, s.ti.file_height,
                   s.ti.swap ? "big" : "little", s.ti.rows_per_strip, s.ti.width, s.ti.height, s.ti.x0, s.ti.y0,
                   s.ti.contiguous ? "contiguous" : "scattered");
        }
        printf("src_picture: matrix_coeffs %d chroma_format_idc %d bit_depth %d video_full_range_flag %d\n", a.in.matrix_coeffs,
               a.in.chroma_format_idc, a.in.bit_depth, a.in.video_full_range_flag);
    } else if (a.in_type == CLI_IN_DPX) { /* one file per frame; a dry run may name a file that is not there */
        if (!(a.dry_run && stat(cli_frame_name(a.src, a.start_frame).c_str(), &st))) {
            if (dpx_scan(a, frames, s.di, s.dpx)) return 1;
            frames = (long)s.dpx.size();
            printf("dpx: %dx%d %d-bit %s-endian, payload %llu bytes\n", s.di.width, s.di.height, s.di.bit_size, s.di.swap ? "big" : "little",
                   (unsigned long long)s.di.payload_bytes);
        }
        printf("src_picture: matrix_coeffs %d chroma_format_idc %d bit_depth %d video_full_range_flag %d\n", a.in.matrix_coeffs,
               a.in.chroma_format_idc, a.in.bit_depth, a.in.video_full_range_flag);
    } else if (a.in_type != CLI_IN_SYNTH && !(a.dry_run && stat(a.src, &st))) { /* (a dry run may name a file that is not there) */
        if (stat(a.src, &st)) { printf("ERROR: unable to open file %s\n", a.src); return 1; }
        const long have = (long)((st.st_size - (off_t)in_frame_bytes * a.start_frame) / (off_t)in_frame_bytes);
        if (st.st_size < (off_t)in_frame_bytes * (a.start_frame + 1)) {
            printf("ERROR: only %lld bytes in %s, expecting %zu from frame %d on\n", (long long)st.st_size, a.src, in_frame_bytes, a.start_frame);
            return 1;
        }
        if (frames > have) frames = have;
    }
    if (a.gpus < 1) a.gpus = 1;
    if (a.devices.empty()) {
        if (a.gpus == 1) a.devices.push_back(a.device);
        else for (int r = 0; r < a.gpus; r++) a.devices.push_back(r);
    }
    if ((int)a.devices.size() != a.gpus) { printf("ERROR: --devices names %zu devices, --gpus %d\n", a.devices.size(), a.gpus); return 1; }
    printf("gpus: %d (devices", a.gpus);
    for (int dv : a.devices) printf(" %d", dv);
    printf(")\nframes: %ld\nframe_bytes: %zu\n", frames, out_frame_bytes);
    /* R in the layout of what the run produces: a whole number of frames, at least as many as the run has */
    const bool cmp_yuv = a.compare_only ? a.in_type == CLI_IN_YUV : a.out_type == CLI_OUT_YUV;
    if (a.ref) {
        if (!stat(a.ref, &st)) {
            if (st.st_size % (off_t)out_frame_bytes) {
                printf("WARNING: reference file (%s): %lld bytes is not a whole number of %zu-byte frames\n", a.ref, (long long)st.st_size,
                       out_frame_bytes);
                return 1;
            }
            if (st.st_size / (off_t)out_frame_bytes < frames) {
                printf("WARNING: reference file (%s) holds %lld frames, the run produces %ld\n", a.ref,
                       (long long)(st.st_size / (off_t)out_frame_bytes), frames);
                return 1;
            }
        } else if (!a.dry_run) { printf("ERROR: unable to open file %s\n", a.ref); return 1; }
        printf("compare: %s %dx%d chroma_format_idc %d bit_depth %d planes %s, %ld frames against %s, sigma %d, output %s\n",
               cmp_yuv ? "yuv" : "rgb", a.out.width, a.out.height, cmp_yuv ? a.out.chroma_format_idc : H2Y_CHROMA_444, a.out.bit_depth,
               cmp_yuv ? "Y,Cb,Cr" : "G,B,R", frames, a.ref, a.sigma, a.compare_only ? "none (compare only)" : a.dst ? "kept" : "none (not written)");
    }
    tiff_wrap &tw = j.tw;
    if (a.out_type == CLI_OUT_TIFF) {
        if (frames > 1 && cli_frame_pattern(a.dst) != 1) {
            printf("ERROR: %ld frames into one .tiff: a .tiff holds one frame; name them with one integer conversion (shot.%%06d.tiff)\n",
                   frames);
            return 1;
        }
        size_t tb = 0;
        if (h2y_tiff_layout(a.in.width, a.in.height, tw.head, nullptr, &tb)) { printf("ERROR: %s\n", h2y_last_error(nullptr)); return 1; }
        tw.tail.resize(tb);
        if (h2y_tiff_layout(a.in.width, a.in.height, tw.head, tw.tail.data(), &tb)) { printf("ERROR: %s\n", h2y_last_error(nullptr)); return 1; }
        printf("tiff_file_bytes: %zu\n", sizeof tw.head + out_frame_bytes + tb);
    }
    if (a.siting == 2) printf("chroma_siting x265 --chromaloc 2\nchroma_siting svt-av1 --chroma-sample-position topleft\n");
    if (a.dry_run) return 0;

    /* tiff.cpp:440 opens ios::ate | ios::app: what is in the file stays, frames go behind it (.tiff: one file per frame) */
    if (a.dst && a.out_type != CLI_OUT_TIFF) {
        j.fd_out = open(a.dst, O_WRONLY | O_CREAT, 0644);
        if (j.fd_out < 0) { printf("ERROR: unable to open %s\n", a.dst); return 1; }
        j.base = lseek(j.fd_out, 0, SEEK_END);
    }

    /* contiguous blocks of frame indices, the first `frames % gpus` one longer (hdr2yuv_amd/shard.py) */
    std::vector<block> blocks(a.gpus);
    long at = 0;
    for (int r = 0; r < a.gpus; r++) {
        blocks[r].device = a.devices[r];
        blocks[r].first = at;
        blocks[r].count = frames / a.gpus + (r < frames % a.gpus ? 1 : 0);
        at += blocks[r].count;
    }
    results res(a, frames);
    auto work = [&](int r) { /* one GPU thread: its own flow (an .exr source keeps its unpack threads there), context and ring */
        if (blocks[r].count > 0) blocks[r].err = run_block(a, make_flow(j), res, r, &blocks[r]);
    };
    if (a.gpus == 1) work(0);
    else {
        std::vector<std::thread> th;
        for (int r = 0; r < a.gpus; r++) th.emplace_back(work, r);
        for (auto &t : th) t.join();
    }
    if (j.fd_out >= 0) close(j.fd_out);
    int rc = 0;
    for (int r = 0; r < a.gpus; r++)
        if (!blocks[r].err.empty()) {
            printf("ERROR (device %d, frames %ld..%ld): %s\n", blocks[r].device, blocks[r].first, blocks[r].first + blocks[r].count - 1, blocks[r].err.c_str());
            rc = 1;
        }
    const bool ran = !rc;
    const bool compared = !rc && a.ref;
    if (compared) rc = compare_report(a, cmp_yuv, a.out.bit_depth, res.compare);
    if (compared && a.ssim) ssim_report(cmp_yuv, res.ssim);
    if (compared && a.regions) regions_report(cmp_yuv, a.out.bit_depth, res.regions);
    if ((!rc || rc == 3) && a.hist) {
        const int hrc = histogram_report(a, res.hist, res.occupied, res.histogram_total());
        if (hrc == 1 || !rc) rc = hrc;
    }
    if (ran && a.delta_e) {
        const int drc = deltae_report(a, res.deltae);
        if (!rc) rc = drc;
    }
    if (ran && a.light) light_report(res.light);
    if (ran && a.dynmeta && lightdist_report(a, res)) rc = 1;
    if (ran && a.gamut_check == 1) {
        const int grc = gamutcheck_report(a, res.gamutcheck);
        if (!rc) rc = grc;
    }
    return rc;
}
