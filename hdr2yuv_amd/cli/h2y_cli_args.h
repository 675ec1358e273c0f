/*
 * h2y_cli_args.h -- the command line of hdr2yuv and how its values are resolved, restated from the reference's
 * behaviour (no HIP here: `hdr2yuv --dry_run` prints the resolved attributes without touching a device, and
 * tests/test_host_logic.py checks them on the CPU against the rules below).
 *
 * What the reference does, in its order (hdr2yuv.cpp):
 *   :765-766  in_pic and out_pic are zeroed: every source attribute that is not given is 0 -- range 0 (video), primaries 0,
 *             matrix 0 (GBR), transfer 0, chroma_format_idc 0, bit depth 0, width/height 0
 *   :61-62    the destination's chroma format, range, transfer, matrix and primaries start at -1
 *   :73-263   flags overwrite (unknown flags warn and are skipped, :258)
 *   :265-318  what the destination leaves unset is copied from the source AS PARSED (depth, width, height: 0 means unset)
 *   :321-372  input type by extension; float types (.exr/.dpx) force the INPUT chroma format to 4:4:4 -- after the copy above
 *   :386-440  output type by extension; integer depth outside [10,16] only warns
 *   :519-572  sanity checks: width/height in [2,10000], src depth in [8,32], input 4:4:4, dst likewise; any failure:
 *             "TOO MANY ARGUMENT ERRORS", exit
 *   read_file :662-756: .rgb forces the input matrix to GBR (:677-680); .dpx forces GBR, 4:4:4, 32 bits (:729-734); .exr forces
 *             4:4:4, 32 bits, GBR and FULL RANGE on the input picture (exr.cpp:172-183).  The destination keeps what :265-318 gave it.
 *   read_planar_integer_file :592-610: integer input needs a depth in [10,16]
 *   .dpx: dpx_read() (dpx.cpp:209-520) aborts on --src_half_float_flag 1 (:232-236); the picture's size comes from the header,
 *             and main() refuses a header size that differs from --src_pic_width/--src_pic_height (the reference would hand
 *             convert() two different sizes)
 *   .tiff: an integer input type at :321-372; read_tiff() (tiff.cpp:54-362) then forces bit depth 16, 4:4:4 and GBR on the
 *             input picture with a warning each, keeps the range flag, and applies --cutout_hd / --cutout_qhd (ignored for every
 *             other input, as there); the decoded size must be the command line's, as for .dpx
 *   .exr: read_exr() (exr.cpp:138-255) takes the size from the data window (refused here when it differs from
 *             --src_pic_width/--src_pic_height, also under --dry_run) and forces the input picture as above
 *   .tiff output: write_tiff() (tiff.cpp:559-652) from .yuv input only (hdr2yuv.cpp:818-819, 931-933); the file is opened "w"
 * --ref_filename R / --sigma_compare S (hdr2yuv.cpp:91-100 parses them, :442-457 types R, :827-833 leaves the comparison a TODO):
 *             R holds what the run produces -- .yuv for .yuv output (the destination's size, chroma format and depth), planar
 *             .rgb (R, G, B planes, as this program writes .rgb) for .rgb or .tiff output -- and output frame k is compared with
 *             frame k of R on the device.  Refused before anything runs (exit 1): R a .tiff, .exr or .dpx, R of another type than
 *             the output, R holding fewer frames than the run produces or not a whole number of frames.  With R the destination
 *             may be left out: the run converts and compares and writes nothing, its output type taken from R.
 *             --compare_only 1 (an addition) compares --src_filename (.yuv or .rgb, read with the --src_* size, depth and chroma
 *             format -- 1 or 3 for .yuv, 3 for .rgb --, from --src_start_frame on) with R (same layout, from its frame 0), --n_frames of each; no conversion.
 * --ssim 1 (an addition: the "SNR, etc." hdr2yuv.cpp:826 leaves a TODO): SSIM of every compared frame beside its PSNR, on the
 *             frames the comparison reads (8x8 windows at a stride of 4 on code values, include/hdr2yuv_hip.h).  Refused (exit 1)
 *             without a comparison, for 4:2:2 frames and for a plane under 8x8 samples.
 * --regions 1 [--regions_flat_var V] [--regions_radius R] (an addition: "measure undershoot and overshoot" and "measure PSNR on flat
 *             areas separate from busy areas" of the reference's NOTES): of every compared frame, on the frames the comparison reads,
 *             the PSNR of its flat and of its busy 8x8 tiles -- a tile of the reference is flat when its variance is at most V squared
 *             code values -- and the samples that lie above (below) the reference's largest (smallest) sample within R samples
 *             (include/hdr2yuv_hip.h, h2y_regions_stats).  R is 1..4, 1 by default; V is 4 x 4^(d - 8) by default at the compared
 *             frames' bit depth d (a standard deviation of two 8-bit steps: a choice, not tuned on programmes; the report's flat_share
 *             is there to tune it by).  Accepted wherever a comparison runs (--ref_filename with or without --dst_filename,
 *             --compare_only 1), beside --ssim, --delta_e and --histogram, for any --gpus; the exit status does not change.  Refused
 *             (exit 1, also under --dry_run): a value other than 0 or 1, --regions_flat_var or --regions_radius without --regions 1, R
 *             outside 1..4, V negative or above 2^32 - 1, no comparison in the run, 4:2:2 frames.
 * --histogram FILE [--histogram_bits B] [--check_range 1] [--histogram_only 1] (additions: the "hist" and "check video range" the
 *             reference leaves a TODO at hdr2yuv.cpp:658 and :797): every frame the run produces is counted on the device -- the .yuv
 *             frames (destination depth and range, Y,Cb,Cr limits), the G,B,R planes of the inverse flow (destination depth, source
 *             range, G,B,R limits), the source frames of --compare_only -- into 2^B bins (B: 1..depth, the depth by default) and the
 *             legal range of set_pic_clip() at that depth.  Without --dst_filename nothing is written; without it and without
 *             --ref_filename the run is the .yuv flow.  --histogram_only 1 counts a .yuv (4:2:0 or 4:4:4) or .rgb (4:4:4) source
 *             read as --compare_only reads it, without conversion.  --check_range 1: exit status 4 when a counted sample lies
 *             outside the legal range (refused in full range, which has no such samples to find).
 * --content_light 1 (an addition): MaxCLL and MaxFALL (CTA-861.3) of the forward flow, measured on the device from the linear light
 *             the conversion hands to PQ10000_r (include/hdr2yuv_hip.h states every step), with or without --dst_filename, beside
 *             --ref_filename and --histogram.  Refused (exit 1, also under --dry_run) unless the destination transfer is PQ (16), the
 *             source transfer is not PQ and the source matrix is G,B,R (0); refused on the .yuv -> RGB flow, with --compare_only 1
 *             and with --histogram_only 1.
 * --dynamic_metadata FILE (an addition): the HDR10+ (SMPTE ST 2094-40) dynamic metadata of the forward flow, measured on the device on
 *             the samples --content_light 1 measures (include/hdr2yuv_hip.h, "light distribution", states every step): per frame the
 *             largest R, G and B, the average and ten percentiles of max(R, G, B) and the share of pixels at or below 100 cd/m2,
 *             printed per frame and written to FILE as the JSON x265 takes as --dhdr10-info (all frames in one scene).  Accepted
 *             wherever --content_light 1 is, beside it, for any --gpus; refused (exit 1, also under --dry_run) wherever that flag
 *             is, and for a FILE that cannot be created.
 * --scene_detect 1 [--scene_threshold T] | --scene_cuts FILE, [--scene_qpfile OUT] (additions): HDR10+ metadata is scene-based, and with
 *             one of the two scene flags the JSON of --dynamic_metadata FILE is: every frame's entry carries its scene's figures,
 *             merged exactly from the frames' figures and bins (include/hdr2yuv_hip.h, "scene signature and scene cuts", states every
 *             step).  --scene_detect 1 measures a 16 x 9 grid signature of every frame's light on the device and opens a scene where
 *             the distance between two frames' signatures exceeds T stops (0.5 by default: a choice, not tuned on real programmes;
 *             every distance is printed); --scene_cuts FILE names the scenes' first frames instead (decimal indices relative to the
 *             run's first frame, one a line, strictly ascending, 0 optional, '#' comments and blank lines ignored) and runs no
 *             signature kernel.  --scene_qpfile OUT writes one line "<frame> I" per scene start, the form x265's --qpfile is
 *             documented to take.  Accepted wherever --dynamic_metadata FILE is (the forward flow and --light_only 1), and only
 *             beside it, for any --gpus.  Refused (exit 1, also under --dry_run): a --scene_detect value other than 0 or 1, either
 *             scene flag without --dynamic_metadata, both together, --scene_threshold without --scene_detect 1 or negative or not
 *             finite, --scene_qpfile without a scene flag, a cuts file that is unreadable, malformed, not ascending or names a frame
 *             >= --n_frames, and an OUT that cannot be created.  Without the flags not a line or byte changes.
 * --scale 1 [--scale_taps 2|3|4] (an addition; the reference parses --dst_pic_width / --dst_pic_height for a Lanczos cv::resize in
 *             cv.cpp, which is compiled out and does not compile): with it a destination size that differs from the source's is
 *             legal on the forward flow to .yuv, and every converted frame is resampled on the device by the exact Lanczos
 *             filter include/hdr2yuv_hip.h defines (3 lobes by default) before it is written.  Without it a size mismatch still
 *             ends the run.  Refused (exit 1, also under --dry_run): --scale_taps without --scale / --scale_only or outside
 *             2..4, an axis ratio outside [1/4, 4], odd sizes with 4:2:0, chroma_format_idc 2, --scale beside --ref_filename,
 *             --histogram, --ssim, --compare_only or --histogram_only, and on the .yuv -> RGB flow.
 * --scale_only 1 (an addition): a .yuv (4:2:0 or 4:4:4) or .rgb source resampled into a destination of the same extension, no
 *             conversion; depth, chroma format and range are the source's, read as --histogram_only reads them; the destination
 *             size is --dst_pic_width / --dst_pic_height.
 * --dither 1|2 [--dither_temporal 0|1] [--dither_seed N] (an addition; the reference's to-do list names "TEMPORAL DITHERING -- dither",
 *             and the reference itself only cuts: (unsigned int) in matrix_convert(), a plain >> in write_yuv()): on the forward flow
 *             to .yuv the run converts at a working depth W -- 16 bits from float and half planes, --src_bit_depth from .tiff, .rgb
 *             and .yuv sources -- and every frame that would be written is reduced to --dst_bit_depth D on the device, 1 by a 16 x 16
 *             ordered pattern, 2 by uniform noise (include/hdr2yuv_hip.h, "dither", states every step in integers), with the plane's
 *             legal-range clamp at D.  0 is the run without the flag.  The pattern is the same in every frame unless
 *             --dither_temporal 1 (0 by default: a still pattern costs an encoder nothing); --dither_seed (0 by default) moves it.
 *             cli_resolve_dither runs first: it keeps D and rewrites the run's destination depth to W, so every later resolver and
 *             the ring's descriptor see a W-bit conversion (--scale then resamples at W bits).  Each GPU thread arms its ring with its
 *             block's first frame counted from the run's first, so any --gpus writes the same file.  From every input type, beside
 *             --linearize, --tone_map, --gamut_convert, --scale, --dst_chroma_sample_loc_type, --content_light, --dynamic_metadata
 *             and the scene flags, appending included.  The banner ends with dither: <1 (ordered)|2 (noise)>, dither_depth: W -> D,
 *             dither_temporal: and dither_seed:.  Refused (exit 1, also under --dry_run): a value outside 0..2, --dither_temporal or
 *             --dither_seed without --dither 1|2, a --dither_temporal other than 0 / 1, D >= W or W - D > 8 or D < 8, no
 *             --dst_filename, a .rgb / .tiff destination and the .yuv -> RGB flow, --dst_matrix_coeffs 15, chroma_format_idc 2,
 *             --ref_filename, --histogram, --ssim, --delta_e (compare or count the written file) and every other *_only flag.
 * --dither_only 1 (an addition): a .yuv (4:2:0 or 4:4:4) or planar .rgb source at --src_bit_depth W reduced into a destination of the
 *             same extension at --dst_bit_depth D, no conversion, with --dither 1|2 required; it honours the source range flag, takes
 *             the G,B,R limits for a .rgb, numbers the frames from --src_start_frame on as 0, 1, ... and works for any --gpus.  It
 *             prints dither_only: 1 and the four lines above.  Refused as above, and for a source that is not .yuv / .rgb, differing
 *             extensions, and a destination size other than the source's.
 * --hlg 1 [--hlg_peak L] (an addition; the reference's transfer list ends at TRANSFER_RHO_GAMMA, its code 18, which in H.273 is HLG): the
 *             forward flow writes a Hybrid Log-Gamma rung (ARIB STD-B67 / BT.2100, non-constant luminance).  The decoded source
 *             planes, display light in BT.2020 primaries after --gamut_convert's and --tone_map's passes where those are given, go
 *             through BT.2100's inverse OOTF at a nominal peak of L cd/m2 and its OETF on the device (include/hdr2yuv_hip.h, "HLG",
 *             states every step), and the unchanged forward conversion takes it from the matrix on.  L is --tone_map_dst_peak beside
 *             --tone_map 1, else 1000; beside --tone_map 1 the planes are taken as display-referred (1.0 = L), without it 1.0 is
 *             10000 cd/m2.  The flag replaces the destination transfer: the run's becomes the source's 8 with floor 0 and ceiling 1,
 *             and --dst_transfer_characteristics beside it is refused whatever its value (18 is RHO_GAMMA in this program).  From
 *             .f32 and .dpx, and with --linearize 1 from a PQ .yuv / .rgb; beside --tone_map, --gamut_convert, --scale,
 *             --dst_chroma_sample_loc_type 2, --dither, --ref_filename, --ssim and --histogram, for any --gpus, with or without
 *             --dst_filename.  The banner carries hlg:, hlg_peak:, hlg_gamma:, hlg_input:, hlg_note: and hlg_encoder:.  Refused (exit
 *             1, also under --dry_run): a value other than 0 or 1, --hlg_peak without --hlg 1 or outside 400..2000 or other than
 *             --tone_map_dst_peak, .f16, .exr, .tiff, .rgb and .yuv input, a source transfer other than 8 or matrix other than 0,
 *             primaries other than 8 / 9 at the pass, --dst_matrix_coeffs other than 0 / 9 (and 0 with primaries codes that
 *             differ: the library refuses that descriptor as the reference does, convert.cpp:1195), .rgb / .tiff destinations and the .yuv ->
 *             RGB flow, every *_only flow, --content_light, --dynamic_metadata and the scene flags (their light is PQ's), --delta_e.
 * --lut3d FILE.cube [--lut3d_interp 0|1] [--lut3d_signal 0|1] (an addition; the reference has no LUT step): the decoded source planes,
 *             after --gamut_convert's and --tone_map's passes where those are given, go through the .cube table on the device
 *             (include/hdr2yuv_hip.h, "3D LUT", states every step), tetrahedral (1, the default) or trilinear (0).  --lut3d_signal 0
 *             (planes, the default): the result stands where the source's samples stood, in the source's transfer and normalisation,
 *             and the unchanged forward conversion follows.  --lut3d_signal 1 (signal): the result is the destination's R'G'B' signal
 *             in [0, 1]; the run becomes the passthrough flow, the way --hlg 1 makes it one: its destination transfer becomes the
 *             source's, and a --dst_transfer_characteristics given is only printed, as lut3d_dst_transfer:.  Either way the run
 *             takes floor 0 and ceiling 1 for every frame.  On the forward flow to .yuv from .f32, .f16, .exr, .dpx and --linearize 1
 *             sources, beside every flag the --tone_map path accepts, for any --gpus, with or without --dst_filename.  The banner
 *             carries lut3d:, lut3d_title:, lut3d_size:, lut3d_domain:, lut3d_interp: and lut3d_signal:.  Refused (exit 1, also
 *             under --dry_run): an unreadable or malformed file, with the parser's reason; the sub-flags without --lut3d or other
 *             than 0 / 1; .tiff, .rgb or .yuv input without --linearize 1; a source matrix other than 0; the .yuv -> RGB flow and
 *             every *_only flag; --lut3d_signal 1 beside --hlg 1, --ictcp 1, --content_light 1, --dynamic_metadata, a half source,
 *             or a --dst_matrix_coeffs other than 0 / 9.
 * --ictcp 1 (an addition; the reference's matrix list has MATRIX_YUVPRIME1 at H.273's code 14, which is ICtCp): the forward flow writes a PQ
 *             ICtCp rung (Rec. ITU-R BT.2100).  The decoded source planes, display light in BT.2020 primaries with 1.0 = 10000 cd/m2
 *             after --gamut_convert's and --tone_map's passes where those are given (the mapper's output is then absolute), become
 *             code-valued I, Ct, Cp on the device (include/hdr2yuv_hip.h, "ICtCp", states every step), and the unchanged forward
 *             conversion casts, subsamples and writes them.  The flag IS the destination's matrix and transfer: the run's become the
 *             passthrough descriptor's 0 and 8 with floor 0 and ceiling 1 and the source's primaries the destination's;
 *             --dst_matrix_coeffs beside it is refused whatever its value, --dst_transfer_characteristics unless it is 16.  Accepted
 *             and refused where --hlg 1 is, and refused beside --hlg 1; --content_light, --dynamic_metadata, the scene flags and
 *             --delta_e on the same run are refused with the command that measures the written file.  The banner carries ictcp:,
 *             ictcp_scale: (H.273's oY aY oC aC), ictcp_note: and ictcp_encoder:.
 * --src_ictcp 1 (an addition), beside --linearize 1, --light_only 1 or --compare_only 1 --delta_e 1, on a .yuv (4:2:0 or 4:4:4): the file's
 *             codes are PQ I, Ct, Cp (include/hdr2yuv_hip.h, "light of ICtCp code planes").  It replaces --src_matrix_coeffs, which is
 *             refused beside it; --src_transfer_characteristics must be 16 and --src_colour_primaries 8 or 9; with --linearize 1 the
 *             destination's matrix must be given (or --ictcp 1).  Everything else those flows accept and refuse stays so, and
 *             linearize_from:, light_only_from: and delta_e_from: name matrix_coeffs 14 (ICtCp).  Refused: a value other than 0 or 1,
 *             .rgb sources, --src_hlg 1 beside it, the flag without one of the three flows.
 * --gamut_convert 1 [--gamut_clip 0|1] (an addition; the reference's matrix_to_primaries() is empty, convert.cpp:1991, and the two
 *             colour_primaries values only pick a branch of matrix_convert()): the decoded source planes are converted on the device
 *             from --src_colour_primaries to --dst_colour_primaries, in linear light, before the unchanged forward conversion
 *             (include/hdr2yuv_hip.h states the matrix and every rounding); results that are not above 0 are clipped to +0.0 unless
 *             --gamut_clip 0.  On the forward flow from .f32, .f16, .exr and .dpx to .yuv, with or without --dst_filename, beside
 *             --content_light, --ref_filename, --histogram, --ssim and --scale; neither primaries flag changes what it did.  Refused
 *             (exit 1, also under --dry_run): a value other than 0 or 1, --gamut_clip without --gamut_convert 1, a source transfer
 *             other than 8 (LINEAR), a source matrix other than 0 (G,B,R), primaries other than 1, 8, 9, 10 and 12 or a pair of equal
 *             chromaticities, .rgb, .tiff and .yuv input, the .yuv -> RGB flow, --compare_only, --histogram_only and --scale_only.
 * --gamut_compress 1 [--gamut_compress_threshold T] [--gamut_compress_power P] (an addition, beside --gamut_convert 1, wherever that is
 *             valid): the pass does the same matrix and, in the same trip through memory, rolls the channels that it left far below
 *             the pixel's largest channel off toward 0 along a curve, not into a clip (include/hdr2yuv_hip.h, "gamut compression":
 *             the distance-from-achromatic form of the ACES 1.3 Reference Gamut Compression, limits from the source primaries).  T,
 *             0.5 .. 0.95, 0.8 by default: the distance from the largest channel up to which a channel keeps its bits; P, 1 .. 4, 1.2
 *             by default: the curve's power.  The banner carries gamut_compress:, both parameters and gamut_compress_limits: (none
 *             for a channel without a curve, which is clipped at 0).  Refused (exit 1, also under --dry_run): a value other than 0 or
 *             1, the flag without --gamut_convert 1, a parameter without the flag, out of range or not a number, --gamut_clip beside
 *             the flag (the pass has its own rule at 0), XYZ (primaries 10) on either side.
 * --tone_map 1 [--tone_map_src_peak S] [--tone_map_dst_peak D] (an addition; the reference has no tone mapper, its README sends the
 *             user to ctlrender): the decoded source planes, after --gamut_convert's pass where that is given, are brought from a
 *             mastering peak of S cd/m2 (1000 by default) down to a target peak of D cd/m2 (100 by default) on the device by the
 *             BT.2390 curve on max(R, G, B), one gain per pixel (include/hdr2yuv_hip.h, "tone mapping", states every step), before
 *             the unchanged forward conversion.  For --dst_transfer_characteristics 16 the output stays in units of 10000 cd/m2
 *             (absolute); for every other destination transfer it is display-referred, 1.0 = D (relative).  With the flag the run
 *             takes floor 0 and ceiling 1 for every frame instead of its pic_stats: mapped planes are referred to their target.
 *             On the forward flow from .f32, .f16, .exr and .dpx to .yuv, with or without --dst_filename, with any --gpus, beside
 *             --gamut_convert, --scale, --dst_chroma_sample_loc_type, --ref_filename, --ssim and --histogram, and for a PQ
 *             destination beside --content_light and --dynamic_metadata, which then measure the mapped light.  Refused (exit 1,
 *             also under --dry_run): a value other than 0 or 1, a peak flag without --tone_map 1, peaks outside 100 <= D < S <=
 *             10000, a source transfer other than 8 (LINEAR), a source matrix other than 0 (G,B,R), a destination transfer of 8,
 *             .rgb, .tiff and .yuv input, the .yuv -> RGB flow and every *_only flow.
 * --dst_chroma_sample_loc_type 0|2 (an addition; the reference carries chroma_sample_loc_type through pic_t and prints it,
 *             hdr2yuv.cpp:490 and :505, parses no flag for it and never acts on it): 2 writes the 4:2:0 chroma co-sited with the
 *             top-left luma sample of every 2x2 block, as HDR10 and UHD Blu-ray assume (include/hdr2yuv_hip.h states every step); 0
 *             is the FIR resampler's own siting, the bytes written without the flag.  On the forward flow to .yuv from every
 *             input type, with any --gpus, with or without --dst_filename, beside --ref_filename, --ssim, --histogram,
 *             --content_light and --gamut_convert.  Refused (exit 1, also under --dry_run): any other value (1 is the box
 *             resampler's siting), 2 with --chroma_resampler_type 0, with --dst_chroma_format_idc 3, with --dst_matrix_coeffs 15,
 *             with --scale 1 or --scale_only 1, on the .yuv -> RGB flow, with --compare_only 1 and with --histogram_only 1.
 * --src_chroma_sample_loc_type 0|2 (an addition, the way back of the flag above): 2 reads the 4:2:0 chroma of a .yuv as co-sited with
 *             the top-left luma sample (HDR10, UHD Blu-ray; what --dst_chroma_sample_loc_type 2 writes) and upsamples it accordingly
 *             (include/hdr2yuv_hip.h, "inverse chroma siting", states every step); 0 is the reference's upsampler, the bytes written
 *             without the flag.  On the .yuv -> .rgb / .tiff flow with --src_chroma_format_idc 1, with any --gpus, with or without
 *             --dst_filename, beside --ref_filename, --ssim and --histogram.  Refused (exit 1, also under --dry_run): any other
 *             value (1 is replication's siting), 2 with --chroma_resampler_type 0, 2 with --src_chroma_format_idc 3, every forward
 *             flow, --compare_only 1, --histogram_only 1 and --scale_only 1.
 * --light_only 1 (an addition): the light of a finished PQ master, from its codes, without a conversion (include/hdr2yuv_hip.h, "light
 *             of PQ code planes", states every step): MaxCLL / MaxFALL of a .yuv (--src_chroma_format_idc 1 or 3, --src_matrix_coeffs
 *             0, 1 or 9) or a .rgb (4:4:4, matrix 0) read as --histogram_only reads it, with --src_bit_depth 8..16, the source range
 *             flag and --src_transfer_characteristics 16; it prints the lines --content_light 1 prints and, with --dynamic_metadata
 *             FILE, the dynamic_metadata: lines and the HDR10+ JSON.  4:2:0 chroma is upsampled as the .yuv -> RGB flow does it:
 *             --chroma_resampler_type 0 replication, otherwise the FIR, with --src_chroma_sample_loc_type 2 its top-left form.  Any
 *             --gpus gives the same lines and FILE.  Refused (exit 1, also under --dry_run): a value other than 0 or 1, a transfer
 *             other than 16, any other matrix, matrix 0 with 4:2:0, 4:2:2, a source that is not .yuv / .rgb, --dst_filename,
 *             --ref_filename, --histogram, --ssim, --scale, --gamut_convert, --content_light or another *_only flag beside it, and
 *             --src_chroma_sample_loc_type 2 with --chroma_resampler_type 0 or with 4:4:4.
 * --gamut_check 1 [--gamut_check_ratio T] [--gamut_check_floor A] [--gamut_check_against P] [--gamut_check_limit S] (additions), beside
 *             --light_only 1: how much of every frame of the PQ master lies outside a primaries set narrower than the file's own
 *             (include/hdr2yuv_hip.h, "gamut containment of PQ code planes", states every step).  The checked sets follow from
 *             --src_colour_primaries: 8 / 9 (BT.2020) gives 12 (P3-D65) and 1 (BT.709), 12 gives 1.  T (0..1, 0.02 by default) is the
 *             tolerance relative to the pixel's largest channel, A (cd/m2, 0.02 by default) the absolute floor.  The banner carries
 *             gamut_check: and gamut_check_from:; the run prints one "gamut_check: frame" line per frame and set and one "gamut_check:
 *             summary" line per set.  --gamut_check_limit S (0..1) makes the exit status 6 when the share of pixels beyond set P exceeds
 *             S in any frame; P is --gamut_check_against, by default the widest checked set.  Accepted beside --dynamic_metadata, the
 *             scene flags and --src_ictcp 1, for any --gpus.  Refused (exit 1, also under --dry_run): the flag or a sub-flag, whatever its value, without --light_only 1 on any flow,
 *             a value other than 0 or 1, a sub-flag without it, --src_colour_primaries 1, unset or unknown (nothing narrower is known), P
 *             not among the checked sets, T, A or S out of range or not finite.
 * --linearize 1 (an addition): a finished PQ master as the source of the forward flow to .yuv (include/hdr2yuv_hip.h, "linearised PQ code
 *             planes", states every step): a .yuv (--src_chroma_format_idc 1 or 3, --src_matrix_coeffs 1 or 9) or a .rgb (4:4:4, matrix
 *             0, its planes assigned to G, B, R as the .rgb forward reader assigns them) with --src_bit_depth 8..16, the source range flag
 *             and --src_transfer_characteristics 16 is read as --light_only reads it and linearised on the device into F32 G,B,R planes
 *             in units of 10000 cd/m2.  4:2:0 chroma is upsampled as --light_only does it (--chroma_resampler_type, which also selects
 *             the destination's subsampler as always; --src_chroma_sample_loc_type 0|2).  Destination attributes that are not given
 *             take the source's as parsed, as always; from there on the run is a run from a .f32 LINEAR (8) G,B,R (0) 4:4:4 source with
 *             floor 0 and ceiling 1 for every frame: --gamut_convert, --tone_map and its peaks, --content_light, --dynamic_metadata,
 *             --scale, --dst_chroma_sample_loc_type, --ref_filename, --ssim and --histogram are accepted and refused exactly as for
 *             .f32, for any --gpus, with or without --dst_filename.  The banner carries linearize: and linearize_from:.  Refused (exit
 *             1, also under --dry_run): a value other than 0 or 1, a source that is not .yuv / .rgb, a transfer other than 16, another
 *             matrix, 4:2:2, matrix 0 with 4:2:0 or with a .yuv, a .rgb with another matrix, odd 4:2:0 sizes, a .rgb / .tiff destination
 *             (the .yuv -> RGB flow), every *_only flag, --src_chroma_sample_loc_type 2 with --chroma_resampler_type 0 or with 4:4:4.
 *             Without the flag nothing changes: .yuv 4:4:4 -> .yuv stays the reference's integer flow.
 * --src_hlg 1 [--src_hlg_peak L] (an addition), beside --linearize 1 only: the file's codes are HLG's (include/hdr2yuv_hip.h, "light of HLG
 *             code planes"): the device turns them into display light at a peak of L cd/m2 (400..2000, 1000 by default) instead of
 *             reading them as PQ.  The flag is the source's transfer: --src_transfer_characteristics beside it is refused whatever its
 *             value (18 is RHO_GAMMA here, as for --hlg 1), and the destination's transfer must be given (or --hlg 1).  Everything else
 *             --linearize 1 accepts and refuses stays so.  The banner carries src_hlg:, src_hlg_peak: ("(default)" where not given),
 *             src_hlg_gamma: "%.4f", src_hlg_note:, and linearize_from: names HLG codes.  Refused (exit 1, also under --dry_run): a
 *             value other than 0 or 1, --src_hlg_peak without --src_hlg 1 or outside 400..2000, --src_hlg 1 without --linearize 1 or
 *             beside --light_only, --compare_only, --delta_e (those read PQ codes) or --dither_only.
 * --src_sdr 1 [--src_sdr_white W] (an addition), beside --linearize 1 only: the file's codes are an SDR master's, coded with the BT.1886
 *             transfer (include/hdr2yuv_hip.h, "light of SDR code planes"): the device places them in absolute light with the reference
 *             white at W cd/m2 (80..1000, 203 by default: Rep. ITU-R BT.2408's display-referred direct mapping) instead of reading them
 *             as PQ.  --src_transfer_characteristics may be left out or be one of this program's BT.1886 codes (1, 6, 14, 15); the
 *             destination's transfer must be given (or --hlg 1 / --ictcp 1): it must not silently inherit BT.1886.  Everything else
 *             --linearize 1 accepts and refuses stays so.  The banner carries src_sdr:, src_sdr_white: ("(default)" where not given),
 *             src_sdr_gamma: 2.4, and linearize_from: names SDR (BT.1886) codes.  Refused (exit 1, also under --dry_run): a value
 *             other than 0 or 1, --src_sdr_white without --src_sdr 1 or outside 80..1000, --src_sdr 1 without --linearize 1, beside
 *             --src_hlg 1 or --src_ictcp 1, beside any *_only flag, a source transfer that is given and is not 1, 6, 14 or 15, no
 *             destination transfer.
 * --src_signal 1 (an addition), beside --linearize 1 --lut3d FILE.cube --lut3d_signal 1 only: the file's codes reach the table as the
 *             non-linear R'G'B' signal they are (include/hdr2yuv_hip.h, "signal of code planes"): normalised, through the matrix,
 *             clamped to [0, 1], and no transfer applied.  A trim built on PQ signal is so applied to the HDR10 .yuv it was built for;
 *             the table decides what the codes mean, so PQ, HLG and SDR masters go the same way.  --src_transfer_characteristics and
 *             --dst_transfer_characteristics are labels and are not checked (the latter is printed as lut3d_dst_transfer:).
 *             Everything else --linearize 1 with a signal-mode LUT accepts and refuses stays so.  The banner carries src_signal: 1
 *             and linearize_from: names "signal (no transfer applied)".  Refused (exit 1, also under --dry_run): a value other than
 *             0 or 1, --src_signal 1 without --linearize 1, without --lut3d or with --lut3d_signal 0 (unscaled signal cannot reach a
 *             passthrough conversion), beside --src_hlg 1, --src_sdr 1 or --src_ictcp 1, beside --tone_map 1 or --gamut_convert 1
 *             (they act on light), beside any *_only flag.  Without the flag --linearize 1 --lut3d F --lut3d_signal 1 keeps feeding
 *             the table linear light.
 * --delta_e 1 [--delta_e_threshold X] [--delta_e_limit Y] (an addition): Delta E ITP (Rec. ITU-R BT.2124; include/hdr2yuv_hip.h, "Delta E
 *             ITP of PQ code planes", states every step) of every compared frame against the reference's, beside the PSNR, wherever a
 *             comparison runs on PQ code frames of BT.2020 primaries: with --compare_only 1 on two .yuv files (--src_chroma_format_idc
 *             1 or 3, --src_matrix_coeffs 1 or 9) or two .rgb files (matrix 0), --src_transfer_characteristics 16,
 *             --src_colour_primaries 8 or 9, --src_bit_depth 8..16 and the source range flag, --chroma_resampler_type and
 *             --src_chroma_sample_loc_type 0|2 choosing the 4:2:0 upsampler as for --light_only; or with --ref_filename on a forward run
 *             to a PQ .yuv (--dst_transfer_characteristics 16, --dst_colour_primaries 8 or 9, --dst_matrix_coeffs 0, 1 or 9, 4:2:0 with
 *             1 or 9 only), with or without --dst_filename, --linearize, --tone_map and --gamut_convert runs included, where
 *             --dst_chroma_sample_loc_type 2 selects the top-left upsampler.  Beside --ssim and --histogram, same lines for any --gpus.
 *             X (1 by default) is the threshold of the per-frame count `over` (d > X, strictly); --delta_e_limit Y makes the exit
 *             status 5 when a frame's mean exceeds Y (status 3 and 4 keep precedence).  Refused (exit 1, also under --dry_run): a value
 *             other than 0 or 1, the threshold or limit flag without --delta_e 1 or negative, no comparison in the run, a transfer other
 *             than 16, primaries other than 8 / 9 (BT.709-primaries PQ would need --gamut_convert's pass first), matrix 11-15 or any
 *             other, 4:2:2, matrix 0 with 4:2:0, the .yuv -> RGB flow, --histogram_only, --scale_only and --light_only, siting 2 with
 *             --chroma_resampler_type 0, and with --linearize 1 a 4:2:0 source and destination whose sitings differ (one context siting
 *             serves both upsamplers).  Without the flag not a line changes.
 * --dst_pack NAME, --src_pack NAME (additions): how the samples of a .yuv file are packed, NAME one of planar16 (the default, the
 *             reference's write_yuv() form: nothing changes), planar8 (8 bits: one byte a sample, ffmpeg's yuv420p / yuv444p), nv12
 *             (8 bits, 4:2:0: Cb and Cr interleaved) and p010 (10..16 bits, 4:2:0: 16-bit words, the sample in the high bits, Cb and Cr
 *             interleaved; p010le / p012le / p016le at 10, 12, 16 bits); include/hdr2yuv_hip.h, "sample packings", states them.  The
 *             repack runs on the device (h2y_stream_pack, h2y_stream_unpack), and only the packed bytes cross the bus.  --dst_pack goes
 *             with every flow that writes a .yuv through a ring: the forward flow from every input type, with --linearize, --scale,
 *             --dither and the passes in front, --scale_only 1 and --dither_only 1, for any --gpus and appending (frame k lies at
 *             base + k x h2y_pack_frame_bytes); its depth is --dst_bit_depth.  --src_pack goes wherever a .yuv is the source of the
 *             .yuv -> .rgb / .tiff flow, --compare_only (R is packed the same way; the ring learns the depth from --src_bit_depth, which
 *             p010 needs: h2y_stream_unpack_ex), --histogram_only, --light_only, --scale_only,
 *             --dither_only and --linearize 1 (with or without --src_hlg / --src_sdr / --src_ictcp); --src_start_frame and the
 *             file-length check use the packed frame's size.  With --scale_only / --dither_only the two flags are independent.  The
 *             banner ends with src_pack: NAME (ffmpeg -pix_fmt X) and / or dst_pack: ..., only when the flag is given (p010 at 11, 13,
 *             14 or 15 bits has no such name, and the line says so).  Refused (exit 1, also under --dry_run): an unknown NAME, a packing
 *             the side's depth or chroma format does not take, a file on that side that is not a .yuv, --dst_pack without
 *             --dst_filename, beside --ref_filename, --histogram, --ssim or --delta_e, or with --dst_matrix_coeffs 15, --src_pack on
 *             the integer .yuv -> .yuv flow without --linearize 1, and --compare_only 1 --src_pack p010 without --src_bit_depth.
 * Only user_args_t.chroma_resampler_type has no defined default there (never initialised): FIR here, as in
 * make.sh's example.  The reference calls exit(0) on its argument errors; this program returns 1.
 */
#ifndef H2Y_CLI_ARGS_H
#define H2Y_CLI_ARGS_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <strings.h>
#include <sys/stat.h>
#include <unistd.h>
#include <string>
#include <vector>

#include "../../include/hdr2yuv_hip.h"

enum { CLI_IN_NONE = 0, CLI_IN_YUV, CLI_IN_RGB, CLI_IN_F32, CLI_IN_F16, CLI_IN_SYNTH, CLI_IN_DPX, CLI_IN_TIFF, CLI_IN_EXR };
enum { CLI_OUT_NONE = 0, CLI_OUT_YUV, CLI_OUT_RGB, CLI_OUT_CODEC, CLI_OUT_TIFF };

struct cli_pic { /* the attribute set of pic_t that the command line fills (hdr.h:363-378) */
    int width, height, bit_depth, half_float_flag, chroma_format_idc, video_full_range_flag;
    int colour_primaries, transfer_characteristics, matrix_coeffs;
};

struct cli_args {
    const char *src = nullptr, *dst = nullptr;
    cli_pic in{}, out{};
    int start_frame = 0, n_frames = 1, verbose = 0;
    int resampler = 1;
    int cutout = 0; /* H2Y_TIFF_CUTOUT_* bits of --cutout_hd / --cutout_qhd (read_tiff only) */
    /* additional flags of this build */
    int synthetic = -1, device = 0, gpus = 1, dry_run = 0, help = 0;
    /* the comparison: --ref_filename, --sigma_compare (exit status 3 on a sample beyond it only when it was given), --compare_only */
    const char *ref = nullptr;
    int sigma = 0, compare_only = 0;
    bool sigma_given = false;
    /* --ssim 1: SSIM beside the comparison */
    int ssim = 0;
    bool ssim_given = false;
    /* --regions 1: flat and busy areas, over- and undershoot beside the comparison; --regions_flat_var (-1: the default of the compared
     * frames' depth, resolved by cli_resolve_regions), --regions_radius */
    int regions = 0, regions_radius = 1;
    long long regions_flat_var_arg = -1;
    uint32_t regions_flat_var = 0;
    bool regions_given = false, regions_flat_var_given = false, regions_radius_given = false;
    /* --content_light 1: MaxCLL / MaxFALL of the forward flow */
    int light = 0;
    bool light_given = false;
    /* --dynamic_metadata FILE: the HDR10+ JSON of the forward flow */
    const char *dynmeta = nullptr;
    /* scenes of the dynamic metadata: --scene_detect 1 [--scene_threshold T] or --scene_cuts FILE, and --scene_qpfile OUT; resolved by
     * cli_resolve_scenes: scene_firsts, the first frames --scene_cuts names (0 among them) */
    int scene_detect = 0;
    bool scene_detect_given = false, scene_threshold_given = false;
    double scene_threshold = 0.5;
    const char *scene_cuts = nullptr, *scene_qpfile = nullptr;
    std::vector<long> scene_firsts;
    bool scenes() const { return scene_detect == 1 || scene_cuts; }
    /* --gamut_convert 1: the source planes go from the source's to the destination's primaries; --gamut_clip (1 by default) */
    int gamut = 0, gamut_clip = 1;
    bool gamut_given = false, gamut_clip_given = false;
    /* --gamut_compress 1 beside --gamut_convert 1: out-of-gamut colours are rolled off, not clipped; the threshold and the power
     * as given (strtof leaves a text that is no number at NaN's place: gamut_compress_*_bad) */
    int gamut_compress = 0;
    bool gamut_compress_given = false, gamut_compress_threshold_given = false, gamut_compress_power_given = false;
    bool gamut_compress_threshold_bad = false, gamut_compress_power_bad = false;
    float gamut_compress_threshold = H2Y_GAMUT_COMPRESS_THRESHOLD, gamut_compress_power = H2Y_GAMUT_COMPRESS_POWER;
    bool gamut_compress_any() const { return gamut_compress_given || gamut_compress_threshold_given || gamut_compress_power_given; }
    /* --tone_map 1: the source planes go from a mastering peak of tone_src_peak cd/m2 down to tone_dst_peak; tone_relative, resolved:
     * the output is display-referred (1.0 = tone_dst_peak) for every destination transfer but PQ */
    int tone_map = 0, tone_src_peak = 1000, tone_dst_peak = 100, tone_relative = 1;
    bool tone_map_given = false, tone_src_peak_given = false, tone_dst_peak_given = false;
    /* --hlg 1 [--hlg_peak L]: the rung is HLG at a nominal peak of hlg_peak cd/m2; resolved: hlg_relative (the planes are
     * display-referred, after --tone_map 1) and hlg_dst_transfer, what --dst_transfer_characteristics gave before the flag replaced
     * it (-1: not given) */
    int hlg = 0, hlg_peak = 1000, hlg_relative = 0, hlg_dst_transfer = -1;
    bool hlg_given = false, hlg_peak_given = false;
    /* --lut3d FILE.cube [--lut3d_interp 0|1] [--lut3d_signal 0|1]: the table is applied to the decoded source planes; resolved:
     * lut3d_table (parsed by cli_resolve_lut3d, the run's until it ends) and lut3d_dst_transfer, what --dst_transfer_characteristics
     * gave before signal mode replaced it with the source's (-1: not given) */
    const char *lut3d = nullptr;
    int lut3d_interp = 1, lut3d_signal = 0, lut3d_dst_transfer = -1;
    bool lut3d_interp_given = false, lut3d_signal_given = false;
    h2y_lut3d *lut3d_table = nullptr;
    /* --dst_chroma_sample_loc_type: 0 as the resampler sites the 4:2:0 chroma, 2 top-left */
    int siting = 0;
    bool siting_given = false;
    /* --src_chroma_sample_loc_type: how the .yuv -> RGB flow takes the 4:2:0 chroma, 0 as the reference's upsampler, 2 top-left */
    int src_siting = 0;
    bool src_siting_given = false;
    /* the histogram: --histogram FILE, --histogram_bits (0: the counted frames' depth), --histogram_only, --check_range; what is
     * counted, resolved by cli_resolve_histogram: depth, range, G,B,R limits, chroma format */
    const char *hist = nullptr;
    int hist_bits = 0, hist_only = 0, check_range = 0;
    bool hist_bits_given = false;
    int hist_depth = 0, hist_full = 0, hist_gbr = 0, hist_chroma = 0;
    /* scaling: --scale 1 (the forward flow's frames), --scale_only 1 (a .yuv or .rgb, no conversion), --scale_taps (lobes) */
    int scale = 0, scale_only = 0, scale_taps = 3;
    bool scale_given = false, scale_taps_given = false;
    /* --light_only 1: the light of a PQ .yuv or .rgb from its codes, no conversion */
    int light_only = 0;
    bool light_only_given = false;
    /* --gamut_check 1 beside it: the gamut containment check; resolved: the checked sets (gamut_check_sets, the widest first) and the
     * set the limit judges (gamut_check_against) */
    int gamut_check = 0, gamut_check_against = 0, gamut_check_n_sets = 0, gamut_check_sets[H2Y_GAMUTCHECK_MAX_SETS] = {0, 0};
    double gamut_check_ratio = H2Y_GAMUTCHECK_RATIO, gamut_check_floor = H2Y_GAMUTCHECK_FLOOR, gamut_check_limit = 0.0;
    bool gamut_check_given = false, gamut_check_ratio_given = false, gamut_check_floor_given = false, gamut_check_against_given = false,
         gamut_check_limit_given = false;
    bool gamut_check_any() const
    {
        return gamut_check_given || gamut_check_ratio_given || gamut_check_floor_given || gamut_check_against_given || gamut_check_limit_given;
    }
    /* --linearize 1: a PQ .yuv or .rgb linearised on the device as the forward flow's source; resolved: `lin` and lin_type keep the
     * file's own attributes and type, while `in` and in_type become those of the F32 LINEAR G,B,R planes the ring decodes */
    int linearize = 0;
    bool linearize_given = false;
    cli_pic lin{};
    int lin_type = CLI_IN_NONE;
    /* --src_hlg 1 [--src_hlg_peak L], beside --linearize 1: the file's codes are HLG's, linearised at a display peak of src_hlg_peak
     * cd/m2; src_transfer_given: --src_transfer_characteristics was on the command line (refused beside the flag) */
    int src_hlg = 0, src_hlg_peak = 1000;
    /* --src_sdr 1 [--src_sdr_white W], beside --linearize 1: the file's codes are BT.1886's, placed with the reference white at
     * src_sdr_white cd/m2 */
    int src_sdr = 0, src_sdr_white = H2Y_SDR_WHITE_DEFAULT;
    bool src_sdr_given = false, src_sdr_white_given = false;
    /* --src_signal 1, beside --linearize 1 --lut3d FILE --lut3d_signal 1: the file's codes stay signal for the table, no transfer applied */
    int src_signal = 0;
    bool src_signal_given = false;
    /* --ictcp 1: the rung is PQ ICtCp (H.273 matrix_coeffs 14); resolved: ictcp_dst_transfer and ictcp_dst_matrix, what
     * --dst_transfer_characteristics and --dst_matrix_coeffs gave before the flag replaced them with the passthrough descriptor's 8 and
     * 0 (-1: not given).  --src_ictcp 1: the codes --linearize 1, --light_only 1 or --compare_only 1 --delta_e 1 read are PQ I, Ct, Cp */
    int ictcp = 0, ictcp_dst_transfer = -1, ictcp_dst_matrix = -1, src_ictcp = 0;
    bool ictcp_given = false, src_ictcp_given = false, src_matrix_given = false;
    bool src_hlg_given = false, src_hlg_peak_given = false, src_transfer_given = false;
    /* --delta_e 1: Delta E ITP beside the comparison; --delta_e_threshold (the `over` count), --delta_e_limit (exit status 5);
     * resolved by cli_resolve_delta_e: the compared frames as PQ code planes, and the inverse chroma siting their upsampler takes */
    int delta_e = 0;
    bool delta_e_given = false, delta_e_threshold_given = false, delta_e_limit_given = false;
    float delta_e_threshold = 1.0f;
    double delta_e_limit = 0.0;
    h2y_codelight_desc de{};
    int de_siting = 0;
    /* --dither 1|2 (ordered, noise) [--dither_temporal 0|1] [--dither_seed N]: the frames that go into the .yuv are reduced from a
     * working depth to --dst_bit_depth on the device; --dither_only 1: a .yuv or .rgb reduced into a file of the same layout.
     * Resolved by cli_resolve_dither: dither_from (W) and dither_to (D); the run's destination depth becomes W */
    int dither = 0, dither_temporal = 0, dither_only = 0;
    uint32_t dither_seed = 0;
    bool dither_given = false, dither_temporal_given = false, dither_seed_given = false, dither_only_given = false;
    int dither_from = 0, dither_to = 0;
    bool dithers() const { return dither == 1 || dither == 2; }
    /* --dst_pack / --src_pack NAME: how the .yuv written / read packs its samples; resolved by cli_resolve_pack: H2Y_PACK_* (0, planar16:
     * no packing).  src_depth_given: --src_bit_depth was on the command line */
    const char *dst_pack_name = nullptr, *src_pack_name = nullptr;
    int dst_pack = 0, src_pack = 0;
    bool src_depth_given = false;
    std::vector<int> devices;
    /* resolved */
    int in_type = CLI_IN_NONE, out_type = CLI_OUT_NONE;
    bool inverse = false; /* .yuv -> RGB (.rgb or .tiff): matrix_inverse() instead of matrix_convert() (hdr2yuv.cpp:818-819) */
};

static inline const char *cli_ext_of(const char *fn)
{
    const char *dot = fn ? strrchr(fn, '.') : nullptr;
    return dot ? dot + 1 : "";
}

/* A file name with one printf integer conversion (%d, %i or %u, optionally with a 0 flag and a width: shot.%06d.dpx)
 * numbers a sequence of files (.dpx or .tiff input, .tiff output).  1: one such conversion and no other (a literal %% aside);
 * 0: no conversion; -1: any other use of '%' (the name is then refused rather than handed to printf). */
static inline int cli_frame_pattern(const char *fn)
{
    int convs = 0;
    for (const char *p = fn ? fn : ""; *p; p++) {
        if (*p != '%') continue;
        if (p[1] == '%') { p++; continue; }
        const char *q = p + 1;
        if (*q == '0') q++;
        while (*q >= '0' && *q <= '9') q++;
        if ((*q != 'd' && *q != 'i' && *q != 'u') || q - p > 4) return -1;
        convs++;
        p = q;
    }
    return convs == 0 ? 0 : convs == 1 ? 1 : -1;
}

/* the file name of frame k of a numbered sequence (cli_frame_pattern(fn) == 1), or fn itself */
static inline std::string cli_frame_name(const char *fn, long k)
{
    if (cli_frame_pattern(fn) != 1) return fn;
    char buf[4096];
    snprintf(buf, sizeof buf, fn, (int)k);
    return buf;
}

static inline void cli_help()
{
    printf("hdr2yuv (gfx950): --src_filename F --dst_filename F.yuv --src_pic_width W --src_pic_height H --src_bit_depth N\n"
           "  [--dst_bit_depth N] [--src_half_float_flag 0|1] [--src_chroma_format_idc 3] [--dst_chroma_format_idc 1|3]\n"
           "  [--src_start_frame K] [--n_frames N] [--verbose_level L]\n"
           "  [--src_colour_primaries P] [--dst_colour_primaries P] [--src_matrix_coeffs M] [--dst_matrix_coeffs M]\n"
           "  [--src_transfer_characteristics T] [--dst_transfer_characteristics T]\n"
           "  [--src_video_full_range_flag 0|1] [--dst_video_full_range_flag 0|1] [--chroma_resampler_type 0|1]\n"
           "  unset source attributes are 0, unset destination attributes take the source's (as the reference resolves them)\n"
           "  additional: [--synthetic SEEDFRAME] [--device D] [--gpus N [--devices d0,d1,..]] [--dry_run 1]\n"
           "  compare: [--ref_filename R.yuv|R.rgb [--sigma_compare S]] (the output against R, frame by frame; without\n"
           "  --dst_filename nothing is written), [--compare_only 1] (--src_filename against R, no conversion), [--ssim 1] (SSIM\n"
           "  beside the PSNR), [--regions 1 [--regions_flat_var V] [--regions_radius R]] (PSNR of flat and of busy 8x8 tiles, a tile\n"
           "  being flat up to a variance of V squared codes; samples beyond the reference's range within R samples, 1..4),\n"
           "  [--delta_e 1 [--delta_e_threshold X] [--delta_e_limit Y]] (Delta E ITP, BT.2124, of compared PQ BT.2020\n"
           "  frames: per frame the mean, the max and the pixels above X, 1 by default; exit status 5 when a frame's mean exceeds Y)\n"
           "  histogram: [--histogram FILE [--histogram_bits B] [--check_range 1]] (code values of every frame the run produces,\n"
           "  totals into FILE; exit status 4 on a sample outside the legal range), [--histogram_only 1] (--src_filename, no conversion)\n"
           "  content light: [--content_light 1] (MaxCLL and MaxFALL of a conversion to PQ, per frame and for the run; without\n"
           "  --dst_filename nothing is written)\n"
           "  dynamic metadata: [--dynamic_metadata FILE] (HDR10+, SMPTE ST 2094-40: per frame maxSCL, the average and percentiles of\n"
           "  max(R,G,B) of a conversion to PQ, written to FILE as the JSON of x265 --dhdr10-info)\n"
           "  scenes: beside --dynamic_metadata, [--scene_detect 1 [--scene_threshold T]] (scene cuts from a 16x9 signature of every frame's\n"
           "  light, measured on the GPU: a cut where the mean change of the cells' log light exceeds T stops, 0.5 by default; FILE then\n"
           "  carries per-scene figures) or [--scene_cuts FILE] (the scenes' first frames, one a line), [--scene_qpfile OUT] (one line\n"
           "  \"<frame> I\" per scene start, for x265 --qpfile)\n"
           "  light of a PQ master: [--light_only 1] (--src_filename, a PQ .yuv -- 4:2:0 or 4:4:4, --src_matrix_coeffs 1 or 9 -- or .rgb,\n"
           "  --src_transfer_characteristics 16: MaxCLL / MaxFALL from its codes, no conversion; with --dynamic_metadata FILE the HDR10+\n"
           "  JSON too; --src_chroma_sample_loc_type 2 for top-left sited 4:2:0 chroma)\n"
           "  gamut containment of a PQ master: beside --light_only 1, [--gamut_check 1 [--gamut_check_ratio T] [--gamut_check_floor A]\n"
           "  [--gamut_check_against P] [--gamut_check_limit S]] (per frame the pixels outside P3-D65 and BT.709 for --src_colour_primaries\n"
           "  8 / 9, outside BT.709 for 12, counted on the GPU: strictly, and beyond a tolerance of T of the pixel's largest channel, 0.02\n"
           "  by default, and A cd/m2, 0.02 by default; exit status 6 when the share of pixels beyond set P exceeds S in any frame)\n"
           "  a PQ master as the source: [--linearize 1] (--src_filename, a PQ .yuv or .rgb as --light_only takes it, linearised on the\n"
           "  GPU into float G,B,R planes in linear light; from there the run is one from a .f32: --tone_map, --gamut_convert, --scale,\n"
           "  --content_light, --dynamic_metadata, --dst_chroma_sample_loc_type, --ref_filename, --ssim and --histogram apply)\n"
           "  an HLG master as the source: [--linearize 1 --src_hlg 1 [--src_hlg_peak L]] (the .yuv / .rgb holds Hybrid Log-Gamma codes:\n"
           "  the OETF's inverse and the OOTF at a display peak of L cd/m2, 400..2000, 1000 by default, on the GPU; it replaces\n"
           "  --src_transfer_characteristics, whose 18 is RHO_GAMMA in this program; to PQ it is BT.2408's HLG -> PQ conversion)\n"
           "  an SDR master as the source: [--linearize 1 --src_sdr 1 [--src_sdr_white W]] (the .yuv / .rgb holds BT.709 or BT.2020 SDR\n"
           "  codes of the BT.1886 transfer, --src_transfer_characteristics 1, 6, 14, 15 or left out: gamma 2.4 and the reference white\n"
           "  at W cd/m2, 80..1000, 203 by default, on the GPU; BT.2408's display-referred mapping of SDR into a PQ or HLG container;\n"
           "  give --dst_transfer_characteristics or --hlg 1 / --ictcp 1, and --gamut_convert 1 for BT.709 primaries)\n"
           "  a code master into a signal-domain LUT: [--linearize 1 --src_signal 1 --lut3d FILE.cube --lut3d_signal 1] (the .yuv / .rgb's\n"
           "  codes reach the table as the R'G'B' signal they are, in [0, 1], with no transfer applied: a trim built on PQ signal applied\n"
           "  to the HDR10 .yuv it was built for; the transfer flags are labels; not with --tone_map 1 or --gamut_convert 1)\n"
           "  primaries: [--gamut_convert 1 [--gamut_clip 0|1]] (float or half G,B,R source planes in linear light converted from\n"
           "  --src_colour_primaries to --dst_colour_primaries on the GPU before the conversion; 1 BT.709, 8 / 9 BT.2020, 12 P3-D65,\n"
           "  10 XYZ; what is not above 0 is clipped to 0 unless --gamut_clip 0)\n"
           "  gamut compression: beside --gamut_convert 1, [--gamut_compress 1 [--gamut_compress_threshold T] [--gamut_compress_power P]]\n"
           "  (out-of-gamut colours are rolled off toward the pixel's largest channel in the same pass, not clipped; T 0.5 .. 0.95, 0.8 by\n"
           "  default; P 1 .. 4, 1.2 by default; not with --gamut_clip, not with XYZ)\n"
           "  tone mapping: [--tone_map 1 [--tone_map_src_peak S] [--tone_map_dst_peak D]] (float or half G,B,R source planes in linear\n"
           "  light brought from a mastering peak of S cd/m2, 1000 by default, down to D, 100 by default, on the GPU by the BT.2390\n"
           "  curve on max(R,G,B) before the conversion: the SDR rung of an HDR master, or a 1000 cd/m2 PQ rung of a 4000 cd/m2 one)\n"
           "  ICtCp: [--ictcp 1] (the rung is PQ I, Ct, Cp, BT.2100 / H.273 matrix_coeffs 14, from float G,B,R planes of display light;\n"
           "  it replaces --dst_matrix_coeffs and --dst_transfer_characteristics); [--src_ictcp 1] beside --linearize 1, --light_only 1 or\n"
           "  --compare_only 1 --delta_e 1 (the .yuv holds PQ I, Ct, Cp codes; it replaces --src_matrix_coeffs)\n"
           "  3D LUT: [--lut3d FILE.cube [--lut3d_interp 0|1] [--lut3d_signal 0|1]] (a .cube table applied to the float or half G,B,R\n"
           "  source planes on the GPU, after --gamut_convert's and --tone_map's passes, 1 tetrahedral by default, 0 trilinear; signal 0:\n"
           "  the result stands where the source's samples stood and the conversion follows; signal 1: it is the destination's R'G'B'\n"
           "  signal in [0, 1], float sources only, and the destination's transfer is the LUT's)\n"
           "  HLG: [--hlg 1 [--hlg_peak L]] (the rung is Hybrid Log-Gamma, ARIB STD-B67 / BT.2100: float G,B,R source planes of display light\n"
           "  in BT.2020 primaries through the inverse OOTF at a nominal peak of L cd/m2, 400..2000, 1000 by default, and the OETF on the\n"
           "  GPU; it replaces --dst_transfer_characteristics, whose 18 is RHO_GAMMA in this program, not H.273's HLG)\n"
           "  chroma siting: [--dst_chroma_sample_loc_type 0|2] (2: 4:2:0 chroma co-sited with the top-left luma sample, as HDR10\n"
           "  assumes -- x265 --chromaloc 2, SVT-AV1 --chroma-sample-position topleft; needs the FIR resampler; 0: as without the flag)\n"
           "  [--src_chroma_sample_loc_type 0|2] (.yuv -> .rgb / .tiff with --src_chroma_format_idc 1; 2: the 4:2:0 chroma is co-sited\n"
           "  with the top-left luma sample and is upsampled so; needs the FIR resampler; 0: as without the flag)\n"
           "  scaling: [--scale 1 [--scale_taps A]] (with --dst_pic_width / --dst_pic_height: every .yuv frame resampled on the GPU by\n"
           "  an exact Lanczos filter of A = 2, 3 or 4 lobes, 3 by default; each axis ratio within 1/4 .. 4), [--scale_only 1] (a .yuv or\n"
           "  .rgb source into a destination of the same extension, no conversion)\n"
           "  dither: [--dither 1|2 [--dither_temporal 0|1] [--dither_seed N]] (the .yuv frames are converted at a working depth -- 16 bits\n"
           "  from float and half sources, --src_bit_depth from 16-bit ones -- and reduced to --dst_bit_depth on the GPU, 1 by a 16x16\n"
           "  ordered pattern, 2 by uniform noise, where the program otherwise cuts the low bits; at most 8 bits; the pattern is the same\n"
           "  in every frame unless --dither_temporal 1), [--dither_only 1] (a .yuv or .rgb source at --src_bit_depth into a destination\n"
           "  of the same extension at --dst_bit_depth, no conversion)\n"
           "  packings: [--dst_pack planar16|planar8|nv12|p010] [--src_pack ...] (how the .yuv written / read packs its samples: 16-bit planar\n"
           "  words as the reference writes them, bytes (8 bits: yuv420p / yuv444p), NV12 (8 bits, 4:2:0), P010 (10..16 bits, 4:2:0,\n"
           "  samples in the words' high bits); repacked on the GPU)\n"
           "input by extension: .yuv .rgb (16-bit planar), .f32 .f16 (raw planar float / half, plane order G,B,R: what\n"
           "  dpx_read() / read_exr() leave in memory), .dpx (10-bit, 16-bit or float DPX) and .tiff (16-bit R,G,B, uncompressed; centre-cropped\n"
           "  to 3840 wide, [--cutout_hd 1] 1920x1080, [--cutout_qhd 1] 960x540) and .exr (scanline OpenEXR: NONE, RLE, ZIPS or ZIP;\n"
           "  half, float or uint R, G, B), decoded on the GPU, one file per frame, shot.%%06d.dpx / .tiff / .exr numbering them\n"
           "  from --src_start_frame on; output: .yuv, or from .yuv input .tiff (16-bit R,G,B;\n"
           "  one file per frame, shot.%%06d.tiff for several) or .rgb (planar R,G,B: the .tiff's samples)\n");
}

/* hdr2yuv.cpp:73-263 */
static inline void cli_parse(cli_args &a, int argc, char **argv)
{
    memset(&a.in, 0, sizeof a.in);   /* :765 */
    memset(&a.out, 0, sizeof a.out); /* :766 */
    a.out.chroma_format_idc = a.out.video_full_range_flag = -1; /* :61 */
    a.out.transfer_characteristics = a.out.matrix_coeffs = a.out.colour_primaries = -1; /* :62 */
    for (int i = 1; i < argc; i++) {
        auto is = [&](const char *n) { return !strcmp(argv[i], n); };
        auto val = [&]() -> const char * { return (i + 1 < argc) ? argv[++i] : "0"; };
        if (is("--help")) { cli_help(); a.help = 1; } /* :82-85: prints and carries on */
        else if (is("--src_filename")) a.src = val();
        else if (is("--dst_filename")) a.dst = val();
        else if (is("--ref_filename")) a.ref = val();
        else if (is("--sigma_compare")) { a.sigma = atoi(val()); a.sigma_given = true; }
        else if (is("--compare_only")) a.compare_only = atoi(val());
        else if (is("--ssim")) { a.ssim = atoi(val()); a.ssim_given = true; }
        else if (is("--regions")) { a.regions = atoi(val()); a.regions_given = true; }
        else if (is("--regions_flat_var")) { a.regions_flat_var_arg = strtoll(val(), nullptr, 10); a.regions_flat_var_given = true; }
        else if (is("--regions_radius")) { a.regions_radius = atoi(val()); a.regions_radius_given = true; }
        else if (is("--delta_e")) { a.delta_e = atoi(val()); a.delta_e_given = true; }
        else if (is("--delta_e_threshold")) { a.delta_e_threshold = strtof(val(), nullptr); a.delta_e_threshold_given = true; }
        else if (is("--delta_e_limit")) { a.delta_e_limit = strtod(val(), nullptr); a.delta_e_limit_given = true; }
        else if (is("--content_light")) { a.light = atoi(val()); a.light_given = true; }
        else if (is("--light_only")) { a.light_only = atoi(val()); a.light_only_given = true; }
        else if (is("--linearize")) { a.linearize = atoi(val()); a.linearize_given = true; }
        else if (is("--gamut_check")) { a.gamut_check = atoi(val()); a.gamut_check_given = true; }
        else if (is("--gamut_check_ratio")) { a.gamut_check_ratio = strtod(val(), nullptr); a.gamut_check_ratio_given = true; }
        else if (is("--gamut_check_floor")) { a.gamut_check_floor = strtod(val(), nullptr); a.gamut_check_floor_given = true; }
        else if (is("--gamut_check_against")) { a.gamut_check_against = atoi(val()); a.gamut_check_against_given = true; }
        else if (is("--gamut_check_limit")) { a.gamut_check_limit = strtod(val(), nullptr); a.gamut_check_limit_given = true; }
        else if (is("--dynamic_metadata")) a.dynmeta = val();
        else if (is("--scene_detect")) { a.scene_detect = atoi(val()); a.scene_detect_given = true; }
        else if (is("--scene_threshold")) { a.scene_threshold = strtod(val(), nullptr); a.scene_threshold_given = true; }
        else if (is("--scene_cuts")) a.scene_cuts = val();
        else if (is("--scene_qpfile")) a.scene_qpfile = val();
        else if (is("--gamut_convert")) { a.gamut = atoi(val()); a.gamut_given = true; }
        else if (is("--gamut_clip")) { a.gamut_clip = atoi(val()); a.gamut_clip_given = true; }
        else if (is("--gamut_compress")) { a.gamut_compress = atoi(val()); a.gamut_compress_given = true; }
        else if (is("--gamut_compress_threshold")) {
            const char *v = val();
            char *end = nullptr;
            a.gamut_compress_threshold = strtof(v, &end);
            a.gamut_compress_threshold_bad = end == v || *end != 0;
            a.gamut_compress_threshold_given = true;
        }
        else if (is("--gamut_compress_power")) {
            const char *v = val();
            char *end = nullptr;
            a.gamut_compress_power = strtof(v, &end);
            a.gamut_compress_power_bad = end == v || *end != 0;
            a.gamut_compress_power_given = true;
        }
        else if (is("--tone_map")) { a.tone_map = atoi(val()); a.tone_map_given = true; }
        else if (is("--tone_map_src_peak")) { a.tone_src_peak = atoi(val()); a.tone_src_peak_given = true; }
        else if (is("--tone_map_dst_peak")) { a.tone_dst_peak = atoi(val()); a.tone_dst_peak_given = true; }
        else if (is("--src_hlg")) { a.src_hlg = atoi(val()); a.src_hlg_given = true; }
        else if (is("--src_hlg_peak")) { a.src_hlg_peak = atoi(val()); a.src_hlg_peak_given = true; }
        else if (is("--src_sdr")) { a.src_sdr = atoi(val()); a.src_sdr_given = true; }
        else if (is("--src_sdr_white")) { a.src_sdr_white = atoi(val()); a.src_sdr_white_given = true; }
        else if (is("--src_signal")) { a.src_signal = atoi(val()); a.src_signal_given = true; }
        else if (is("--hlg")) { a.hlg = atoi(val()); a.hlg_given = true; }
        else if (is("--ictcp")) { a.ictcp = atoi(val()); a.ictcp_given = true; }
        else if (is("--src_ictcp")) { a.src_ictcp = atoi(val()); a.src_ictcp_given = true; }
        else if (is("--hlg_peak")) { a.hlg_peak = atoi(val()); a.hlg_peak_given = true; }
        else if (is("--lut3d")) a.lut3d = val();
        else if (is("--lut3d_interp")) { a.lut3d_interp = atoi(val()); a.lut3d_interp_given = true; }
        else if (is("--lut3d_signal")) { a.lut3d_signal = atoi(val()); a.lut3d_signal_given = true; }
        else if (is("--dst_chroma_sample_loc_type")) { a.siting = atoi(val()); a.siting_given = true; }
        else if (is("--src_chroma_sample_loc_type")) { a.src_siting = atoi(val()); a.src_siting_given = true; }
        else if (is("--histogram")) a.hist = val();
        else if (is("--histogram_bits")) { a.hist_bits = atoi(val()); a.hist_bits_given = true; }
        else if (is("--histogram_only")) a.hist_only = atoi(val());
        else if (is("--check_range")) a.check_range = atoi(val());
        else if (is("--scale")) { a.scale = atoi(val()); a.scale_given = true; }
        else if (is("--scale_only")) a.scale_only = atoi(val());
        else if (is("--scale_taps")) { a.scale_taps = atoi(val()); a.scale_taps_given = true; }
        else if (is("--dither")) { a.dither = atoi(val()); a.dither_given = true; }
        else if (is("--dither_temporal")) { a.dither_temporal = atoi(val()); a.dither_temporal_given = true; }
        else if (is("--dither_seed")) { a.dither_seed = (uint32_t)strtoul(val(), nullptr, 0); a.dither_seed_given = true; }
        else if (is("--dither_only")) { a.dither_only = atoi(val()); a.dither_only_given = true; }
        else if (is("--alpha_channel")) (void)val(); /* (read_tiff ignores alpha too) */
        else if (is("--cutout_hd")) a.cutout = atoi(val()) ? (a.cutout | H2Y_TIFF_CUTOUT_HD) : (a.cutout & ~H2Y_TIFF_CUTOUT_HD);
        else if (is("--cutout_qhd")) a.cutout = atoi(val()) ? (a.cutout | H2Y_TIFF_CUTOUT_QHD) : (a.cutout & ~H2Y_TIFF_CUTOUT_QHD);
        else if (is("--src_pic_width")) a.in.width = atoi(val());
        else if (is("--src_pic_height")) a.in.height = atoi(val());
        else if (is("--dst_pic_width")) a.out.width = atoi(val());
        else if (is("--dst_pic_height")) a.out.height = atoi(val());
        else if (is("--src_bit_depth")) { a.in.bit_depth = atoi(val()); a.src_depth_given = true; }
        else if (is("--dst_pack")) a.dst_pack_name = val();
        else if (is("--src_pack")) a.src_pack_name = val();
        else if (is("--dst_bit_depth")) a.out.bit_depth = atoi(val());
        else if (is("--src_half_float_flag")) a.in.half_float_flag = atoi(val());
        else if (is("--dst_half_float_flag")) a.out.half_float_flag = atoi(val());
        else if (is("--src_chroma_format_idc")) a.in.chroma_format_idc = atoi(val());
        else if (is("--dst_chroma_format_idc")) a.out.chroma_format_idc = atoi(val());
        else if (is("--src_start_frame")) a.start_frame = atoi(val());
        else if (is("--n_frames")) a.n_frames = atoi(val());
        else if (is("--verbose_level")) a.verbose = atoi(val());
        else if (is("--src_colour_primaries")) a.in.colour_primaries = atoi(val());
        else if (is("--dst_colour_primaries")) a.out.colour_primaries = atoi(val());
        else if (is("--src_matrix_coeffs")) { a.in.matrix_coeffs = atoi(val()); a.src_matrix_given = true; }
        else if (is("--dst_matrix_coeffs")) a.out.matrix_coeffs = atoi(val());
        else if (is("--src_transfer_characteristics")) { a.in.transfer_characteristics = atoi(val()); a.src_transfer_given = true; }
        else if (is("--dst_transfer_characteristics")) a.out.transfer_characteristics = atoi(val());
        else if (is("--src_video_full_range_flag")) a.in.video_full_range_flag = atoi(val());
        else if (is("--dst_video_full_range_flag")) a.out.video_full_range_flag = atoi(val());
        else if (is("--chroma_resampler_type")) a.resampler = atoi(val());
        else if (is("--synthetic")) a.synthetic = atoi(val());
        else if (is("--device")) a.device = atoi(val());
        else if (is("--gpus")) a.gpus = atoi(val());
        else if (is("--dry_run")) a.dry_run = atoi(val());
        else if (is("--devices")) {
            a.devices.clear();
            for (const char *p = val(); *p;) {
                a.devices.push_back(atoi(p));
                p = strchr(p, ',');
                if (!p) break;
                p++;
            }
        } else printf("WARNING: argument (%s) unrecongized\n", argv[i]);
    }
}

/* The reference file's type against the output's: 0, or a warning printed and 1 */
static inline int cli_ref_check(const cli_args &a)
{
    const char *ext = cli_ext_of(a.ref);
    if (!strcasecmp(ext, "tiff") || !strcasecmp(ext, "exr") || !strcasecmp(ext, "dpx")) {
        printf("WARNING: reference file (%s): .%s is not read for a comparison; give the samples as .rgb (planar R, G, B)\n", a.ref, ext);
        return 1;
    }
    const bool yuv = a.compare_only ? a.in_type == CLI_IN_YUV : a.out_type == CLI_OUT_YUV;
    if (strcasecmp(ext, yuv ? "yuv" : "rgb")) {
        printf("WARNING: reference file (%s) must be a .%s: it holds frames in the layout of the %s\n", a.ref, yuv ? "yuv" : "rgb",
               a.compare_only ? "source" : "output");
        return 1;
    }
    return 0;
}

/* --compare_only 1: two files of one layout, no conversion; returns the number of argument errors */
static inline int cli_resolve_compare(cli_args &a)
{
    int arg_errors = 0;
    const char *ext = cli_ext_of(a.src);
    if (!strcasecmp(ext, "yuv")) a.in_type = CLI_IN_YUV;
    else if (!strcasecmp(ext, "rgb")) a.in_type = CLI_IN_RGB;
    else {
        printf("WARNING: --compare_only reads .yuv or .rgb; source file (%s) is a .%s\n", a.src ? a.src : "(none)", ext);
        arg_errors++;
    }
    if (a.dst) { printf("WARNING: --compare_only writes nothing: leave out --dst_filename\n"); arg_errors++; }
    if (!a.ref) { printf("WARNING: --compare_only needs --ref_filename\n"); arg_errors++; }
    else if (a.in_type != CLI_IN_NONE) arg_errors += cli_ref_check(a);
    printf("compare_only: 1\nsrc_filename: %s\nref_filename: %s\n", a.src ? a.src : "(none)", a.ref ? a.ref : "(none)");
    printf("src_pic_width: %d\nsrc_pic_height: %d\nsrc_chroma_format_idc: %d\nsrc_bit_depth: %d\nsrc_start_frame: %d\nn_frames: %d\n",
           a.in.width, a.in.height, a.in.chroma_format_idc, a.in.bit_depth, a.start_frame, a.n_frames);
    printf("sigma_compare: %d%s\n", a.sigma, a.sigma_given ? "" : " (default)");
    if (a.in.width < 1 || a.in.width > 10000) { printf("WARNING: pic_width(%d) outside range [1,10000]\n", a.in.width); arg_errors++; }
    if (a.in.height < 1 || a.in.height > 10000) { printf("WARNING: pic_height(%d) outside range [1,10000]\n", a.in.height); arg_errors++; }
    if (a.in.bit_depth < 8 || a.in.bit_depth > 16) { printf("WARNING: src bit_depth(%d) outside range [8,16]\n", a.in.bit_depth); arg_errors++; }
    if (a.in.chroma_format_idc != H2Y_CHROMA_420 && a.in.chroma_format_idc != H2Y_CHROMA_444) {
        printf("WARNING: chroma_format_idc(%d) not %d or %d\n", a.in.chroma_format_idc, H2Y_CHROMA_420, H2Y_CHROMA_444);
        arg_errors++;
    } else if (a.in_type == CLI_IN_RGB && a.in.chroma_format_idc != H2Y_CHROMA_444) { /* three full planes R, G, B */
        printf("WARNING: a .rgb holds three planes of width x height: --compare_only of .rgb files takes chroma_format_idc %d, not %d\n",
               H2Y_CHROMA_444, a.in.chroma_format_idc);
        arg_errors++;
    }
    if (a.sigma < 0) { printf("WARNING: sigma_compare(%d) is negative\n", a.sigma); arg_errors++; }
    a.out = a.in;
    return arg_errors;
}

/* --histogram_only 1: one file counted, no conversion; returns the number of argument errors */
static inline int cli_resolve_histogram_only(cli_args &a)
{
    int arg_errors = 0;
    const char *ext = cli_ext_of(a.src);
    if (!strcasecmp(ext, "yuv")) a.in_type = CLI_IN_YUV;
    else if (!strcasecmp(ext, "rgb")) a.in_type = CLI_IN_RGB;
    else {
        printf("WARNING: --histogram_only reads .yuv or .rgb; source file (%s) is a .%s\n", a.src ? a.src : "(none)", ext);
        arg_errors++;
    }
    if (a.dst) { printf("WARNING: --histogram_only writes no frames: leave out --dst_filename\n"); arg_errors++; }
    if (a.ref || a.compare_only) { printf("WARNING: --histogram_only reads one file: leave out --ref_filename and --compare_only\n"); arg_errors++; }
    printf("histogram_only: 1\nsrc_filename: %s\n", a.src ? a.src : "(none)");
    printf("src_pic_width: %d\nsrc_pic_height: %d\nsrc_chroma_format_idc: %d\nsrc_bit_depth: %d\nsrc_video_full_range_flag: %d\n"
           "src_start_frame: %d\nn_frames: %d\n", a.in.width, a.in.height, a.in.chroma_format_idc, a.in.bit_depth,
           a.in.video_full_range_flag, a.start_frame, a.n_frames);
    if (a.in.width < 1 || a.in.width > 10000) { printf("WARNING: pic_width(%d) outside range [1,10000]\n", a.in.width); arg_errors++; }
    if (a.in.height < 1 || a.in.height > 10000) { printf("WARNING: pic_height(%d) outside range [1,10000]\n", a.in.height); arg_errors++; }
    if (a.in.bit_depth < 8 || a.in.bit_depth > 16) { printf("WARNING: src bit_depth(%d) outside range [8,16]\n", a.in.bit_depth); arg_errors++; }
    if (a.in.video_full_range_flag != 0 && a.in.video_full_range_flag != 1) {
        printf("WARNING: video_full_range_flag(%d) not 0 or 1\n", a.in.video_full_range_flag);
        arg_errors++;
    }
    if (a.in.chroma_format_idc != H2Y_CHROMA_420 && a.in.chroma_format_idc != H2Y_CHROMA_444) {
        printf("WARNING: chroma_format_idc(%d) not %d or %d\n", a.in.chroma_format_idc, H2Y_CHROMA_420, H2Y_CHROMA_444);
        arg_errors++;
    } else if (a.in_type == CLI_IN_RGB && a.in.chroma_format_idc != H2Y_CHROMA_444) { /* three full planes R, G, B */
        printf("WARNING: a .rgb holds three planes of width x height: --histogram_only of a .rgb takes chroma_format_idc %d, not %d\n",
               H2Y_CHROMA_444, a.in.chroma_format_idc);
        arg_errors++;
    }
    a.out = a.in;
    return arg_errors;
}

/* What --histogram counts, printed; returns the number of argument errors */
static inline int cli_resolve_histogram(cli_args &a)
{
    if (!a.hist) {
        printf("WARNING: --histogram_bits, --histogram_only and --check_range need --histogram FILE\n");
        return 1;
    }
    if (a.compare_only || a.hist_only) { /* the source frames, as read */
        a.hist_depth = a.in.bit_depth, a.hist_full = a.in.video_full_range_flag;
        a.hist_gbr = a.in_type == CLI_IN_RGB, a.hist_chroma = a.in.chroma_format_idc;
    } else if (a.inverse) { /* the G, B, R planes of matrix_inverse(), clamped in the source's range */
        a.hist_depth = a.out.bit_depth, a.hist_full = a.in.video_full_range_flag, a.hist_gbr = 1, a.hist_chroma = H2Y_CHROMA_444;
    } else { /* the .yuv frames, clamped by write_yuv() */
        a.hist_depth = a.out.bit_depth, a.hist_full = a.out.video_full_range_flag, a.hist_gbr = 0, a.hist_chroma = a.out.chroma_format_idc;
    }
    if (!a.hist_bits_given) a.hist_bits = a.hist_depth;
    printf("histogram: %s\nhistogram_bits: %d%s\nhistogram_frames: %s bit_depth %d %s range, planes %s\ncheck_range: %d\n", a.hist,
           a.hist_bits, a.hist_bits_given ? "" : " (default)", a.compare_only || a.hist_only ? "source" : "output", a.hist_depth,
           a.hist_full ? "full" : "video", a.hist_gbr ? "G,B,R" : "Y,Cb,Cr", a.check_range);
    int arg_errors = 0;
    if (a.hist_depth < 8 || a.hist_depth > 16) {
        printf("WARNING: --histogram counts frames of bit_depth 8..16, not %d\n", a.hist_depth);
        arg_errors++;
    } else if (a.hist_bits < 1 || a.hist_bits > a.hist_depth) {
        printf("WARNING: histogram_bits(%d) outside range [1,%d]\n", a.hist_bits, a.hist_depth);
        arg_errors++;
    }
    if (a.check_range && a.hist_full) {
        printf("WARNING: --check_range 1 in full range: every code 0..2^bit_depth-1 is legal, there is no range to check\n");
        arg_errors++;
    }
    return arg_errors;
}

/* hdr2yuv.cpp:265-572 and the attribute overrides of read_file(), then what --histogram counts; returns the number of argument
 * errors */
static inline int cli_resolve_convert(cli_args &a);
static inline int cli_resolve_ssim(cli_args &a);
static inline int cli_resolve_regions(cli_args &a);
static inline int cli_resolve_light(cli_args &a);
static inline int cli_resolve_dynmeta(cli_args &a);
static inline int cli_resolve_scale_only(cli_args &a);
static inline int cli_resolve_scale(cli_args &a);
static inline int cli_resolve_gamut(cli_args &a, int src_matrix_arg);
static inline int cli_resolve_gamut_compress(cli_args &a);
static inline int cli_resolve_tone_map(cli_args &a, int src_matrix_arg);
static inline int cli_resolve_hlg(cli_args &a, int src_matrix_arg);
static inline int cli_resolve_lut3d(cli_args &a, int src_matrix_arg);
/* is m the matrix --src_ictcp 1 gave the source? (--src_matrix_coeffs 14 without the flag stays what it was: refused) */
static inline bool cli_src_is_ictcp(const cli_args &a, int m) { return a.src_ictcp == 1 && m == H2Y_MATRIX_ICTCP; }
static inline int cli_resolve_ictcp(cli_args &a, int src_matrix_arg);
static inline int cli_resolve_src_ictcp(cli_args &a);
static inline int cli_resolve_siting(cli_args &a);
static inline int cli_resolve_src_siting(cli_args &a);
static inline int cli_resolve_light_only(cli_args &a);
static inline int cli_resolve_gamut_check(cli_args &a);
static inline int cli_resolve_scenes(cli_args &a);
static inline int cli_resolve_linearize(cli_args &a);
static inline int cli_resolve_src_hlg(cli_args &a);
static inline int cli_resolve_src_sdr(cli_args &a);
static inline int cli_resolve_src_signal(cli_args &a);
static inline int cli_resolve_delta_e(cli_args &a);
static inline int cli_resolve_dither(cli_args &a);
static inline int cli_resolve_dither_only(cli_args &a);
static inline int cli_resolve_all(cli_args &a);
static inline int cli_resolve_flows(cli_args &a);
static inline int cli_resolve_pack(cli_args &a);
static inline int cli_resolve(cli_args &a)
{
    /* (before the comparison's own resolver, which refuses the depth it was not given in words of its own) */
    if (a.compare_only && a.src_pack_name && !strcasecmp(a.src_pack_name, "p010") && !a.src_depth_given) {
        printf("WARNING: --compare_only 1 --src_pack p010 needs --src_bit_depth: the samples lie in the words' high bits\n");
        return 1;
    }
    int arg_errors = cli_resolve_flows(a);
    /* (after every flow's resolver: whichever flow runs, the flags are refused where it compares nothing) */
    if (a.regions_given || a.regions_flat_var_given || a.regions_radius_given) arg_errors += cli_resolve_regions(a);
    /* last: the packings are those of the files the resolved run reads and writes */
    return arg_errors || !(a.dst_pack_name || a.src_pack_name) ? arg_errors : cli_resolve_pack(a);
}

/* the ffmpeg -pix_fmt of a .yuv of this chroma format and depth packed so; "" where ffmpeg has no name for it */
static inline std::string cli_pix_fmt(int chroma, int bit_depth, int packing)
{
    const std::string planar = chroma == H2Y_CHROMA_420 ? "yuv420p" : chroma == H2Y_CHROMA_444 ? "yuv444p" : "";
    if (packing == H2Y_PACK_PLANAR8) return planar;
    if (packing == H2Y_PACK_NV12) return "nv12";
    if (packing == H2Y_PACK_P010) return bit_depth == 10 ? "p010le" : bit_depth == 12 ? "p012le" : bit_depth == 16 ? "p016le" : "";
    return planar.empty() || bit_depth < 8 || bit_depth > 16 ? "" : bit_depth == 8 ? planar : planar + std::to_string(bit_depth) + "le";
}

/* --dst_pack / --src_pack: the names, the refusals and the banner's lines; returns the number of argument errors */
static inline int cli_resolve_pack(cli_args &a)
{
    static const char *const kNames[4] = {"planar16", "planar8", "nv12", "p010"};
    auto packing_of = [](const char *name) {
        for (int p = 0; p < 4; p++)
            if (!strcasecmp(name, kNames[p])) return p;
        return -1;
    };
    /* is the packing one this depth and chroma format take?  The warning where not. */
    auto legal = [](const char *flag, int packing, int depth, int chroma) { /* (4:2:2 never gets here: every flow's resolver refuses it) */
        if ((packing == H2Y_PACK_NV12 || packing == H2Y_PACK_P010) && chroma != H2Y_CHROMA_420) {
            printf("WARNING: %s %s is 4:2:0: not with chroma_format_idc %d\n", flag, kNames[packing], chroma);
            return false;
        }
        if ((packing == H2Y_PACK_PLANAR8 || packing == H2Y_PACK_NV12) && depth != 8) {
            printf("WARNING: %s %s holds one byte a sample: it needs a bit depth of 8, not %d\n", flag, kNames[packing], depth);
            return false;
        }
        if (packing == H2Y_PACK_P010 && (depth < 10 || depth > 16)) {
            printf("WARNING: %s p010 holds 16-bit words: it needs a bit depth of 10..16, not %d (8 bits: planar8 or nv12)\n", flag, depth);
            return false;
        }
        return true;
    };
    auto line = [](const char *key, int packing, int depth, int chroma) {
        const std::string fmt = cli_pix_fmt(chroma, depth, packing);
        if (fmt.empty()) printf("%s: %s (no ffmpeg -pix_fmt at %d bits)\n", key, kNames[packing], depth);
        else printf("%s: %s (ffmpeg -pix_fmt %s)\n", key, kNames[packing], fmt.c_str());
    };
    if (a.src_pack_name) {
        const int p = packing_of(a.src_pack_name);
        if (p < 0) { printf("WARNING: --src_pack %s: not one of planar16, planar8, nv12, p010\n", a.src_pack_name); return 1; }
        const cli_pic &pic = a.linearize == 1 ? a.lin : a.in;
        const int type = a.linearize == 1 ? a.lin_type : a.in_type;
        const int depth = a.dither_only == 1 ? a.dither_from : pic.bit_depth;
        if (type != CLI_IN_YUV || strcasecmp(cli_ext_of(a.src), "yuv")) {
            printf("WARNING: --src_pack is how a .yuv packs its samples: source file (%s) is a .%s\n", a.src ? a.src : "(none)", cli_ext_of(a.src));
            return 1;
        }
        if (p != H2Y_PACK_PLANAR16) {
            const bool reads_codes = a.inverse || a.compare_only || a.hist_only || a.light_only == 1 || a.scale_only || a.dither_only == 1 || a.linearize == 1;
            if (!reads_codes) {
                printf("WARNING: --src_pack: the integer .yuv -> .yuv flow reads the reference's 16-bit planar frames; a packed source goes "
                       "through --linearize 1\n");
                return 1;
            }
            if (!legal("--src_pack", p, depth, pic.chroma_format_idc)) return 1;
        }
        a.src_pack = p;
        line("src_pack", p, depth, pic.chroma_format_idc);
    }
    if (a.dst_pack_name) {
        const int p = packing_of(a.dst_pack_name);
        if (p < 0) { printf("WARNING: --dst_pack %s: not one of planar16, planar8, nv12, p010\n", a.dst_pack_name); return 1; }
        if (!a.dst) { printf("WARNING: --dst_pack needs --dst_filename\n"); return 1; }
        if (a.out_type != CLI_OUT_YUV || strcasecmp(cli_ext_of(a.dst), "yuv")) {
            printf("WARNING: --dst_pack is how a .yuv packs its samples: destination file (%s) is a .%s\n", a.dst, cli_ext_of(a.dst));
            return 1;
        }
        const int depth = a.dithers() ? a.dither_to : a.out.bit_depth;
        if (p != H2Y_PACK_PLANAR16) {
            if (a.ref || a.hist || a.ssim || a.delta_e) {
                printf("WARNING: --dst_pack is not combined with --ref_filename, --histogram, --ssim or --delta_e: compare or count the written "
                       "file (--compare_only 1, --histogram_only 1, with --src_pack)\n");
                return 1;
            }
            if (a.out.matrix_coeffs == H2Y_MATRIX_YUVPRIME2) {
                printf("WARNING: --dst_pack: dst_matrix_coeffs %d (Y'u'v') is not packed\n", H2Y_MATRIX_YUVPRIME2);
                return 1;
            }
            if (!legal("--dst_pack", p, depth, a.out.chroma_format_idc)) return 1;
        }
        a.dst_pack = p;
        line("dst_pack", p, depth, a.out.chroma_format_idc);
    }
    return 0;
}

static inline int cli_resolve_flows(cli_args &a)
{
    const bool dither_flags = a.dither_given || a.dither_temporal_given || a.dither_seed_given || a.dither_only_given;
    /* first, and without a line of its own yet: every later resolver sees a conversion at the working depth */
    if (dither_flags && cli_resolve_dither(a)) return 1;
    if ((a.hlg_given || a.hlg_peak_given) && a.dither_only == 1) {
        printf("hlg: %d\nWARNING: --hlg writes a conversion's rung: not with --dither_only 1\n", a.hlg);
        return 1;
    }
    if ((a.src_hlg_given || a.src_hlg_peak_given) && a.dither_only == 1) {
        printf("src_hlg: %d\nWARNING: --src_hlg goes with --linearize 1: not with --dither_only 1\n", a.src_hlg);
        return 1;
    }
    if ((a.src_sdr_given || a.src_sdr_white_given) && a.dither_only == 1) {
        printf("src_sdr: %d\nWARNING: --src_sdr goes with --linearize 1: not with --dither_only 1\n", a.src_sdr);
        return 1;
    }
    if (a.src_signal_given && a.dither_only == 1) {
        printf("src_signal: %d\nWARNING: --src_signal goes with --linearize 1: not with --dither_only 1\n", a.src_signal);
        return 1;
    }
    if ((a.lut3d || a.lut3d_interp_given || a.lut3d_signal_given) && a.dither_only == 1) {
        printf("lut3d: %s\nWARNING: --lut3d applies to a conversion's source: not with --dither_only 1\n", a.lut3d ? a.lut3d : "(none)");
        return 1;
    }
    if ((a.ictcp_given || a.src_ictcp_given) && a.dither_only == 1) {
        printf("%s: %d\nWARNING: --%s goes with a conversion or a measurement: not with --dither_only 1\n", a.ictcp_given ? "ictcp" : "src_ictcp",
               a.ictcp_given ? a.ictcp : a.src_ictcp, a.ictcp_given ? "ictcp" : "src_ictcp");
        return 1;
    }
    if (a.gamut_check_any() && a.light_only != 1) { /* whatever the flow and the value: its one refusal, in the resolver's words */
        cli_resolve_gamut_check(a);
        return 1;
    }
    const int arg_errors = a.dither_only == 1 ? cli_resolve_dither_only(a) : cli_resolve_all(a);
    if (arg_errors || !a.dithers()) return arg_errors;
    printf("dither: %d (%s)\ndither_depth: %d -> %d\ndither_temporal: %d\ndither_seed: %u\n", a.dither, a.dither == 1 ? "ordered" : "noise",
           a.dither_from, a.dither_to, a.dither_temporal, a.dither_seed);
    return 0;
}

static inline int cli_resolve_all(cli_args &a)
{
    if (a.hlg == 1) { /* before anything resolves the destination: the flag is its transfer, and the run's becomes the source's 8 */
        a.hlg_dst_transfer = a.out.transfer_characteristics;
        a.out.transfer_characteristics = H2Y_TRANSFER_LINEAR;
    }
    if (a.ictcp == 1 && a.hlg != 1) { /* likewise: the flag is the destination's matrix and transfer; the run's is the passthrough's */
        a.ictcp_dst_transfer = a.out.transfer_characteristics;
        a.ictcp_dst_matrix = a.out.matrix_coeffs;
        a.out.transfer_characteristics = H2Y_TRANSFER_LINEAR;
        a.out.matrix_coeffs = H2Y_MATRIX_GBR;
    }
    if (a.linearize_given) { /* first: what follows resolves the linearised source */
        printf("linearize: %d\n", a.linearize);
        if (a.linearize != 0 && a.linearize != 1) {
            printf("WARNING: linearize(%d) not 0 or 1\n", a.linearize);
            return 1;
        }
    }
    if ((a.src_hlg_given || a.src_hlg_peak_given) && cli_resolve_src_hlg(a)) return 1; /* the transfer of --linearize 1's source */
    if ((a.src_sdr_given || a.src_sdr_white_given) && cli_resolve_src_sdr(a)) return 1; /* likewise: BT.1886 codes at a reference white */
    if (a.src_signal_given && cli_resolve_src_signal(a)) return 1; /* likewise: no transfer at all, the codes stay signal for the LUT */
    if (a.src_ictcp_given && cli_resolve_src_ictcp(a)) return 1; /* the matrix of the codes the three flows below read */
    if (a.linearize == 1 && cli_resolve_linearize(a)) return 1;
    const bool lut3d_flags = a.lut3d || a.lut3d_interp_given || a.lut3d_signal_given;
    if (a.lut3d && a.lut3d_signal == 1 && a.hlg != 1 && a.ictcp != 1) { /* the LUT is the destination's transfer: the run's becomes the source's */
        a.lut3d_dst_transfer = a.out.transfer_characteristics;
        a.out.transfer_characteristics = a.in.transfer_characteristics;
    }
    if (a.light_only_given) { /* its own flow: it resolves everything it takes and refuses the rest */
        printf("light_only: %d\n", a.light_only);
        if (a.light_only != 0 && a.light_only != 1) {
            printf("WARNING: light_only(%d) not 0 or 1\n", a.light_only);
            return 1;
        }
        if (a.light_only && lut3d_flags) {
            printf("lut3d: %s\nWARNING: --lut3d applies to a conversion's source: not with --light_only 1\n", a.lut3d ? a.lut3d : "(none)");
            return 1;
        }
        if (a.light_only && (a.hlg_given || a.hlg_peak_given)) {
            printf("hlg: %d\nWARNING: --hlg writes a conversion's rung: not with --light_only 1\n", a.hlg);
            return 1;
        }
        if (a.light_only && a.ictcp_given) {
            printf("ictcp: %d\nWARNING: --ictcp writes a conversion's rung: not with --light_only 1 (the light of an ICtCp file: --src_ictcp 1)\n", a.ictcp);
            return 1;
        }
        if (a.light_only) {
            int arg_errors = cli_resolve_light_only(a);
            if (a.scene_detect_given || a.scene_threshold_given || a.scene_cuts || a.scene_qpfile) arg_errors += cli_resolve_scenes(a);
            if (a.gamut_check_any()) arg_errors += cli_resolve_gamut_check(a);
            return arg_errors + (a.delta_e_given || a.delta_e_threshold_given || a.delta_e_limit_given ? cli_resolve_delta_e(a) : 0);
        }
    }
    const int src_matrix_arg = a.in.matrix_coeffs; /* as given: the float readers force G,B,R on the input picture below */
    int arg_errors = a.hist_only    ? cli_resolve_histogram_only(a)
                     : a.compare_only ? cli_resolve_compare(a)
                     : a.scale_only   ? cli_resolve_scale_only(a)
                                      : cli_resolve_convert(a);
    if (a.hist || a.hist_bits_given || a.hist_only || a.check_range) arg_errors += cli_resolve_histogram(a);
    if (a.ssim_given) arg_errors += cli_resolve_ssim(a);
    if (a.light_given) arg_errors += cli_resolve_light(a);
    if (a.dynmeta) arg_errors += cli_resolve_dynmeta(a);
    if (a.scene_detect_given || a.scene_threshold_given || a.scene_cuts || a.scene_qpfile) arg_errors += cli_resolve_scenes(a);
    if (a.scale_given || a.scale_only || a.scale_taps_given) arg_errors += cli_resolve_scale(a);
    if (a.gamut_given || a.gamut_clip_given || a.gamut_compress_any()) arg_errors += cli_resolve_gamut(a, src_matrix_arg);
    if (a.tone_map_given || a.tone_src_peak_given || a.tone_dst_peak_given) arg_errors += cli_resolve_tone_map(a, src_matrix_arg);
    if (lut3d_flags) arg_errors += cli_resolve_lut3d(a, src_matrix_arg);
    if (a.hlg_given || a.hlg_peak_given) arg_errors += cli_resolve_hlg(a, src_matrix_arg);
    if (a.ictcp_given) arg_errors += cli_resolve_ictcp(a, src_matrix_arg);
    if (a.siting_given) arg_errors += cli_resolve_siting(a);
    const bool de_flags = a.delta_e_given || a.delta_e_threshold_given || a.delta_e_limit_given;
    /* (--linearize 1 resolved its own; under --compare_only 1 --delta_e 1 the flag chooses Delta E's upsampler, checked there) */
    if (a.src_siting_given && !a.linearize && !(a.compare_only && a.delta_e == 1)) arg_errors += cli_resolve_src_siting(a);
    if (de_flags) arg_errors += cli_resolve_delta_e(a);
    return arg_errors;
}

/* --dither / --dither_temporal / --dither_seed / --dither_only: the refusals, W (dither_from) and D (dither_to); on the forward
 * flow the run's destination depth becomes W.  Prints warnings only; returns the number of argument errors */
static inline int cli_resolve_dither(cli_args &a)
{
    int arg_errors = 0;
    if (a.dither < 0 || a.dither > 2) { printf("WARNING: dither(%d) outside range [0,2]\n", a.dither); arg_errors++; }
    if (a.dither_only != 0 && a.dither_only != 1) { printf("WARNING: dither_only(%d) not 0 or 1\n", a.dither_only); arg_errors++; }
    if (a.dither_temporal != 0 && a.dither_temporal != 1) { printf("WARNING: dither_temporal(%d) not 0 or 1\n", a.dither_temporal); arg_errors++; }
    if (arg_errors) return arg_errors;
    if ((a.dither_temporal_given || a.dither_seed_given) && !a.dithers()) {
        printf("WARNING: --dither_temporal and --dither_seed need --dither 1 or 2\n");
        arg_errors++;
    }
    if (a.dither_only && !a.dithers()) { printf("WARNING: --dither_only 1 needs --dither 1 or 2\n"); arg_errors++; }
    if (arg_errors || !a.dithers()) return arg_errors;
    const char *flag = a.dither_only ? "--dither_only 1" : "--dither";
    const char *other = a.compare_only ? "compare_only" : a.hist_only ? "histogram_only" : a.scale_only ? "scale_only" : a.light_only ? "light_only" : nullptr;
    if (other) { printf("WARNING: %s: not with --%s 1\n", flag, other); return 1; }
    if (a.dither_only && a.linearize) { printf("WARNING: --linearize 1 is the source of a conversion: not with --dither_only 1\n"); return 1; }
    if (a.ref || a.hist || a.ssim || a.delta_e) {
        printf("WARNING: %s is not combined with --ref_filename, --histogram, --ssim or --delta_e: compare or count the written file "
               "(--compare_only 1, --histogram_only 1)\n", flag);
        return 1;
    }
    if (!a.dst) { printf("WARNING: %s needs --dst_filename\n", flag); return 1; }
    const char *sext = cli_ext_of(a.src), *dext = cli_ext_of(a.dst);
    int W, chroma;
    if (a.dither_only) {
        if (strcasecmp(sext, "yuv") && strcasecmp(sext, "rgb")) {
            printf("WARNING: --dither_only reads .yuv or .rgb; source file (%s) is a .%s\n", a.src ? a.src : "(none)", sext);
            return 1;
        }
        if (strcasecmp(dext, sext)) {
            printf("WARNING: --dither_only writes what it reads: destination file (%s) must be a .%s like the source\n", a.dst, sext);
            return 1;
        }
        W = a.in.bit_depth;
        chroma = a.in.chroma_format_idc;
    } else {
        if (strcasecmp(dext, "yuv")) {
            printf("WARNING: --dither dithers the forward flow's .yuv frames: destination file (%s) is a .%s\n", a.dst, dext);
            return 1;
        }
        if ((a.out.matrix_coeffs == -1 ? a.in.matrix_coeffs : a.out.matrix_coeffs) == H2Y_MATRIX_YUVPRIME2) {
            printf("WARNING: --dither: dst_matrix_coeffs %d (Y'u'v') is not dithered\n", H2Y_MATRIX_YUVPRIME2);
            return 1;
        }
        /* the working depth: a U16 source's own (the reference converts there and shifts), 16 bits for float and half planes */
        const bool u16 = a.linearize != 1 && a.synthetic < 0 && (!strcasecmp(sext, "yuv") || !strcasecmp(sext, "rgb") || !strcasecmp(sext, "tiff"));
        W = !u16 ? 16 : !strcasecmp(sext, "tiff") ? 16 : a.in.bit_depth;
        chroma = a.out.chroma_format_idc == -1 ? (u16 && strcasecmp(sext, "tiff") ? a.in.chroma_format_idc : H2Y_CHROMA_444) : a.out.chroma_format_idc;
    }
    if (chroma == 2) { printf("WARNING: %s: chroma_format_idc 2 (4:2:2) is not dithered\n", flag); return 1; }
    const int D = a.out.bit_depth ? a.out.bit_depth : a.in.bit_depth;
    if (W < 9 || W > 16 || D < 8 || D >= W || W - D > 8) {
        printf("WARNING: %s reduces the working depth (%d) to dst_bit_depth (%d): it needs 8 <= dst_bit_depth < %d <= 16, at most 8 bits apart\n",
               flag, W, D, W);
        return 1;
    }
    a.dither_from = W, a.dither_to = D;
    if (!a.dither_only) a.out.bit_depth = W;
    return 0;
}

/* --dither_only 1: one file reduced into another of the same layout, no conversion (cli_resolve_dither made the checks); returns
 * the number of argument errors */
static inline int cli_resolve_dither_only(cli_args &a)
{
    int arg_errors = 0;
    a.in_type = !strcasecmp(cli_ext_of(a.src), "rgb") ? CLI_IN_RGB : CLI_IN_YUV;
    printf("dither_only: 1\nsrc_filename: %s\ndst_filename: %s\n", a.src, a.dst);
    printf("src_pic_width: %d\nsrc_pic_height: %d\nsrc_chroma_format_idc: %d\nsrc_bit_depth: %d\nsrc_video_full_range_flag: %d\n"
           "dst_bit_depth: %d\nsrc_start_frame: %d\nn_frames: %d\n", a.in.width, a.in.height, a.in.chroma_format_idc, a.in.bit_depth,
           a.in.video_full_range_flag, a.dither_to, a.start_frame, a.n_frames);
    if (a.in.width < 1 || a.in.width > 10000) { printf("WARNING: pic_width(%d) outside range [1,10000]\n", a.in.width); arg_errors++; }
    if (a.in.height < 1 || a.in.height > 10000) { printf("WARNING: pic_height(%d) outside range [1,10000]\n", a.in.height); arg_errors++; }
    if (a.in.video_full_range_flag != 0 && a.in.video_full_range_flag != 1) {
        printf("WARNING: video_full_range_flag(%d) not 0 or 1\n", a.in.video_full_range_flag);
        arg_errors++;
    }
    if (a.in_type == CLI_IN_RGB && a.in.chroma_format_idc != H2Y_CHROMA_444) { /* three full planes R, G, B */
        printf("WARNING: a .rgb holds three planes of width x height: --dither_only of a .rgb takes chroma_format_idc %d, not %d\n",
               H2Y_CHROMA_444, a.in.chroma_format_idc);
        arg_errors++;
    } else if (a.in.chroma_format_idc != H2Y_CHROMA_420 && a.in.chroma_format_idc != H2Y_CHROMA_444) {
        printf("WARNING: chroma_format_idc(%d) not %d or %d\n", a.in.chroma_format_idc, H2Y_CHROMA_420, H2Y_CHROMA_444);
        arg_errors++;
    } else if (a.in.chroma_format_idc == H2Y_CHROMA_420 && ((a.in.width | a.in.height) & 1)) {
        printf("WARNING: --dither_only 1: 4:2:0 needs an even width and height, not %dx%d\n", a.in.width, a.in.height);
        arg_errors++;
    }
    if ((a.out.width && a.out.width != a.in.width) || (a.out.height && a.out.height != a.in.height)) {
        printf("WARNING: --dither_only 1 keeps the picture's size: leave out --dst_pic_width and --dst_pic_height\n");
        arg_errors++;
    }
    a.out = a.in;
    a.out.bit_depth = a.dither_to;
    a.out_type = a.in_type == CLI_IN_RGB ? CLI_OUT_RGB : CLI_OUT_YUV;
    return arg_errors;
}

/* --scale_only 1: one file resampled into another of the same layout, no conversion; returns the number of argument errors */
static inline int cli_resolve_scale_only(cli_args &a)
{
    int arg_errors = 0;
    const char *ext = cli_ext_of(a.src);
    if (!strcasecmp(ext, "yuv")) a.in_type = CLI_IN_YUV;
    else if (!strcasecmp(ext, "rgb")) a.in_type = CLI_IN_RGB;
    else {
        printf("WARNING: --scale_only reads .yuv or .rgb; source file (%s) is a .%s\n", a.src ? a.src : "(none)", ext);
        arg_errors++;
    }
    if (!a.dst) { printf("WARNING: --scale_only needs --dst_filename\n"); arg_errors++; }
    else if (a.in_type != CLI_IN_NONE && strcasecmp(cli_ext_of(a.dst), ext)) {
        printf("WARNING: --scale_only writes what it reads: destination file (%s) must be a .%s like the source\n", a.dst, ext);
        arg_errors++;
    }
    if (a.ref || a.hist) { printf("WARNING: --scale_only reads one file and writes one: leave out --ref_filename and --histogram\n"); arg_errors++; }
    printf("scale_only: 1\nsrc_filename: %s\ndst_filename: %s\n", a.src ? a.src : "(none)", a.dst ? a.dst : "(none)");
    printf("src_pic_width: %d\nsrc_pic_height: %d\nsrc_chroma_format_idc: %d\nsrc_bit_depth: %d\nsrc_video_full_range_flag: %d\n"
           "src_start_frame: %d\nn_frames: %d\n", a.in.width, a.in.height, a.in.chroma_format_idc, a.in.bit_depth,
           a.in.video_full_range_flag, a.start_frame, a.n_frames);
    if (a.in.bit_depth < 8 || a.in.bit_depth > 16) { printf("WARNING: src bit_depth(%d) outside range [8,16]\n", a.in.bit_depth); arg_errors++; }
    if (a.in.video_full_range_flag != 0 && a.in.video_full_range_flag != 1) {
        printf("WARNING: video_full_range_flag(%d) not 0 or 1\n", a.in.video_full_range_flag);
        arg_errors++;
    }
    if (a.in_type == CLI_IN_RGB && a.in.chroma_format_idc != H2Y_CHROMA_444 && a.in.chroma_format_idc != 2) { /* three full planes R, G, B */
        printf("WARNING: a .rgb holds three planes of width x height: --scale_only of a .rgb takes chroma_format_idc %d, not %d\n",
               H2Y_CHROMA_444, a.in.chroma_format_idc);
        arg_errors++;
    }
    const int dw = a.out.width ? a.out.width : a.in.width, dh = a.out.height ? a.out.height : a.in.height;
    a.out = a.in;
    a.out.width = dw, a.out.height = dh;
    a.out_type = a.in_type == CLI_IN_RGB ? CLI_OUT_RGB : CLI_OUT_YUV;
    printf("dst_pic_width: %d\ndst_pic_height: %d\n", dw, dh);
    return arg_errors;
}

/* --scale / --scale_only / --scale_taps: what is resampled, printed; returns the number of argument errors */
static inline int cli_resolve_scale(cli_args &a)
{
    int arg_errors = 0;
    if (a.scale != 0 && a.scale != 1) { printf("WARNING: scale(%d) not 0 or 1\n", a.scale); arg_errors++; }
    if (a.scale_only != 0 && a.scale_only != 1) { printf("WARNING: scale_only(%d) not 0 or 1\n", a.scale_only); arg_errors++; }
    if (a.scale_taps_given && !a.scale && !a.scale_only) { printf("WARNING: --scale_taps needs --scale 1 or --scale_only 1\n"); arg_errors++; }
    if (a.scale_taps < 2 || a.scale_taps > 4) { printf("WARNING: scale_taps(%d) outside range [2,4]\n", a.scale_taps); arg_errors++; }
    if (a.scale && a.scale_only) { printf("WARNING: --scale 1 scales a conversion, --scale_only 1 a file: give one of them\n"); arg_errors++; }
    if (a.scale_only && (a.compare_only || a.hist_only)) {
        printf("WARNING: --scale_only 1: not with --%s 1\n", a.compare_only ? "compare_only" : "histogram_only");
        arg_errors++;
    }
    if (arg_errors || (!a.scale && !a.scale_only)) return arg_errors;
    if (a.scale) {
        if (a.compare_only || a.hist_only) {
            printf("WARNING: --scale 1 scales a conversion: not with --%s 1\n", a.compare_only ? "compare_only" : "histogram_only");
            return 1;
        }
        if (a.ref || a.hist || a.ssim) {
            printf("WARNING: --scale 1 is not combined with --ref_filename, --histogram or --ssim: compare or count the written file "
                   "(--compare_only 1, --histogram_only 1)\n");
            return 1;
        }
        if (a.inverse) {
            printf("WARNING: --scale 1 scales the forward flow (to .yuv), not the .yuv -> RGB flow\n");
            return 1;
        }
        if (a.out_type != CLI_OUT_YUV) return 0; /* refused above with its own message */
    }
    const int chroma = a.out.chroma_format_idc, depth = a.out.bit_depth, full = a.out.video_full_range_flag;
    const bool gbr = a.scale_only && a.in_type == CLI_IN_RGB;
    if (chroma == 2) { printf("WARNING: --scale%s 1: chroma_format_idc 2 (4:2:2) is not scaled\n", a.scale_only ? "_only" : ""); return 1; }
    if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) {
        printf("WARNING: chroma_format_idc(%d) not %d or %d\n", chroma, H2Y_CHROMA_420, H2Y_CHROMA_444);
        return 1;
    }
    const int sw = a.in.width, sh = a.in.height, dw = a.out.width, dh = a.out.height;
    if (sw < 2 || sh < 2 || dw < 2 || dh < 2 || sw > 10000 || sh > 10000 || dw > 10000 || dh > 10000) {
        printf("WARNING: scaling %dx%d -> %dx%d: widths and heights outside range [2,10000]\n", sw, sh, dw, dh);
        return 1;
    }
    if (sw > 4 * dw || dw > 4 * sw || sh > 4 * dh || dh > 4 * sh) {
        printf("WARNING: scaling %dx%d -> %dx%d: each axis ratio must lie within [1/4, 4]\n", sw, sh, dw, dh);
        return 1;
    }
    if (chroma == H2Y_CHROMA_420 && ((sw | sh | dw | dh) & 1)) {
        printf("WARNING: scaling %dx%d -> %dx%d: 4:2:0 needs even widths and heights\n", sw, sh, dw, dh);
        return 1;
    }
    if (depth < 8 || depth > 16) { printf("WARNING: scaling takes frames of bit_depth 8..16, not %d\n", depth); return 1; }
    std::vector<int32_t> first((size_t)std::max(dw, dh)), count(first.size());
    std::vector<int16_t> coef(first.size() * H2Y_SCALE_TAPS);
    int th = 0, tv = 0;
    if (h2y_scale_taps(sw, dw, a.scale_taps, first.data(), count.data(), coef.data(), &th) ||
        h2y_scale_taps(sh, dh, a.scale_taps, first.data(), count.data(), coef.data(), &tv)) {
        printf("WARNING: scaling %dx%d -> %dx%d: %s\n", sw, sh, dw, dh, h2y_last_error(nullptr));
        return 1;
    }
    printf("scale: %dx%d -> %dx%d lanczos%d chroma_format_idc %d bit_depth %d %s range, planes %s, taps h %d v %d\n", sw, sh, dw, dh,
           a.scale_taps, chroma, depth, full ? "full" : "video", gbr ? "G,B,R" : "Y,Cb,Cr", th, tv);
    return 0;
}

/* what measures light (`flag`: --content_light 1, --dynamic_metadata FILE) takes: the forward flow of a conversion to PQ from another
 * transfer, of a G,B,R source; returns the number of argument errors */
static inline int cli_light_scope(const cli_args &a, const char *flag)
{
    if (a.compare_only || a.hist_only) {
        printf("WARNING: %s measures a conversion: not with --%s 1\n", flag, a.compare_only ? "compare_only" : "histogram_only");
        return 1;
    }
    if (a.inverse) {
        printf("WARNING: %s measures the forward flow (to .yuv), not the .yuv -> RGB flow\n", flag);
        return 1;
    }
    if (a.out.transfer_characteristics != 16) {
        printf("WARNING: %s needs a PQ destination: dst_transfer_characteristics(%d) is not 16\n", flag, a.out.transfer_characteristics);
        return 1;
    }
    if (a.in.transfer_characteristics == 16) {
        printf("WARNING: %s: a PQ source (src_transfer_characteristics 16) goes to PQ without linear light\n", flag);
        return 1;
    }
    if (a.in.matrix_coeffs != H2Y_MATRIX_GBR) {
        printf("WARNING: %s needs a G,B,R source: src_matrix_coeffs(%d) is not %d\n", flag, a.in.matrix_coeffs, H2Y_MATRIX_GBR);
        return 1;
    }
    return 0;
}

/* --content_light; returns the number of argument errors */
static inline int cli_resolve_light(cli_args &a)
{
    printf("content_light: %d\n", a.light);
    if (a.light != 0 && a.light != 1) {
        printf("WARNING: content_light(%d) not 0 or 1\n", a.light);
        return 1;
    }
    if (!a.light) return 0;
    if (cli_light_scope(a, "--content_light 1")) return 1;
    printf("content_light_from: src_transfer_characteristics %d -> PQ, G,B,R, floor and ceiling %s\n", a.in.transfer_characteristics,
           a.linearize == 1 ? "0 and 1 (--linearize 1)" : a.tone_map == 1 ? "0 and 1 (--tone_map 1)" : a.lut3d ? "0 and 1 (--lut3d)" : "of each frame's pic_stats");
    return 0;
}

/* can `path` be created: an existing regular file that can be written, or a name in a directory that can be written to */
static inline bool cli_can_create(const char *path)
{
    struct stat st;
    if (!stat(path, &st)) return S_ISREG(st.st_mode) && !access(path, W_OK);
    const char *slash = strrchr(path, '/');
    const std::string dir = !slash ? "." : slash == path ? "/" : std::string(path, slash);
    return *path && !stat(dir.c_str(), &st) && S_ISDIR(st.st_mode) && !access(dir.c_str(), W_OK | X_OK);
}

/* --light_only 1: the light of a PQ .yuv or .rgb from its codes, one file read, no conversion; with --dynamic_metadata FILE the
 * light distribution too.  Sets a.light (and keeps a.dynmeta) so that the run keeps and reports those figures; returns the number
 * of argument errors */
static inline int cli_resolve_light_only(cli_args &a)
{
    int arg_errors = 0;
    const char *ext = cli_ext_of(a.src);
    if (!strcasecmp(ext, "yuv")) a.in_type = CLI_IN_YUV;
    else if (!strcasecmp(ext, "rgb")) a.in_type = CLI_IN_RGB;
    else {
        printf("WARNING: --light_only reads .yuv or .rgb; source file (%s) is a .%s\n", a.src ? a.src : "(none)", ext);
        arg_errors++;
    }
    if (a.dst) { printf("WARNING: --light_only writes no frames: leave out --dst_filename\n"); arg_errors++; }
    if (a.ref || a.hist || a.hist_bits_given || a.check_range || a.ssim_given || a.scale_given || a.scale_taps_given || a.gamut_given ||
        a.gamut_clip_given || a.gamut_compress_any() || a.light_given || a.siting_given) {
        printf("WARNING: --light_only measures one file's light: leave out --ref_filename, --histogram, --ssim, --scale, --gamut_convert, "
               "--content_light and --dst_chroma_sample_loc_type\n");
        arg_errors++;
    }
    if (a.compare_only || a.hist_only || a.scale_only) {
        printf("WARNING: --light_only 1: not with --%s 1\n", a.compare_only ? "compare_only" : a.hist_only ? "histogram_only" : "scale_only");
        arg_errors++;
    }
    if (a.tone_map_given || a.tone_src_peak_given || a.tone_dst_peak_given) {
        printf("WARNING: --tone_map maps a conversion's source: not with --light_only 1\n");
        arg_errors++;
    }
    printf("src_filename: %s\n", a.src ? a.src : "(none)");
    printf("src_pic_width: %d\nsrc_pic_height: %d\nsrc_chroma_format_idc: %d\nsrc_bit_depth: %d\nsrc_video_full_range_flag: %d\n"
           "src_matrix_coeffs: %d\nsrc_transfer_characteristics: %d\nsrc_start_frame: %d\nn_frames: %d\n", a.in.width, a.in.height,
           a.in.chroma_format_idc, a.in.bit_depth, a.in.video_full_range_flag, a.in.matrix_coeffs, a.in.transfer_characteristics,
           a.start_frame, a.n_frames);
    if (a.src_siting_given) printf("src_chroma_sample_loc_type: %d\n", a.src_siting);
    if (a.dynmeta) printf("dynamic_metadata_file: %s\n", a.dynmeta);
    if (a.in.width < 1 || a.in.width > 10000) { printf("WARNING: pic_width(%d) outside range [1,10000]\n", a.in.width); arg_errors++; }
    if (a.in.height < 1 || a.in.height > 10000) { printf("WARNING: pic_height(%d) outside range [1,10000]\n", a.in.height); arg_errors++; }
    if (a.in.bit_depth < 8 || a.in.bit_depth > 16) { printf("WARNING: src bit_depth(%d) outside range [8,16]\n", a.in.bit_depth); arg_errors++; }
    if (a.in.video_full_range_flag != 0 && a.in.video_full_range_flag != 1) {
        printf("WARNING: video_full_range_flag(%d) not 0 or 1\n", a.in.video_full_range_flag);
        arg_errors++;
    }
    if (a.in.transfer_characteristics != 16) {
        printf("WARNING: --light_only 1 measures PQ codes: src_transfer_characteristics(%d) is not 16\n", a.in.transfer_characteristics);
        arg_errors++;
    }
    const int m = a.in.matrix_coeffs, chroma = a.in.chroma_format_idc;
    if (m != H2Y_MATRIX_GBR && m != H2Y_MATRIX_BT709 && m != H2Y_MATRIX_BT2020NC && !cli_src_is_ictcp(a, m)) {
        printf("WARNING: --light_only 1: src_matrix_coeffs(%d) not %d (G,B,R), %d (BT.709) or %d (BT.2020nc)\n", m, H2Y_MATRIX_GBR,
               H2Y_MATRIX_BT709, H2Y_MATRIX_BT2020NC);
        arg_errors++;
    } else if (a.in_type == CLI_IN_RGB && m != H2Y_MATRIX_GBR) {
        printf("WARNING: a .rgb holds planes R, G, B: --light_only of a .rgb takes src_matrix_coeffs %d, not %d\n", H2Y_MATRIX_GBR, m);
        arg_errors++;
    }
    if (chroma == 2) { printf("WARNING: --light_only 1: chroma_format_idc 2 (4:2:2) is not measured\n"); arg_errors++; }
    else if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) {
        printf("WARNING: chroma_format_idc(%d) not %d or %d\n", chroma, H2Y_CHROMA_420, H2Y_CHROMA_444);
        arg_errors++;
    } else if (a.in_type == CLI_IN_RGB && chroma != H2Y_CHROMA_444) { /* three full planes R, G, B */
        printf("WARNING: a .rgb holds three planes of width x height: --light_only of a .rgb takes chroma_format_idc %d, not %d\n",
               H2Y_CHROMA_444, chroma);
        arg_errors++;
    } else if (chroma == H2Y_CHROMA_420 && m == H2Y_MATRIX_GBR) {
        printf("WARNING: --light_only 1: G,B,R planes (src_matrix_coeffs %d) are 4:4:4, not chroma_format_idc %d\n", H2Y_MATRIX_GBR, chroma);
        arg_errors++;
    } else if (chroma == H2Y_CHROMA_420 && ((a.in.width | a.in.height) & 1)) {
        printf("WARNING: --light_only 1: 4:2:0 needs an even width and height, not %dx%d\n", a.in.width, a.in.height);
        arg_errors++;
    }
    if (a.src_siting == 1) {
        printf("WARNING: src_chroma_sample_loc_type(1) is replication's siting, --chroma_resampler_type 0: not selected by this flag\n");
        arg_errors++;
    } else if (a.src_siting != 0 && a.src_siting != 2) {
        printf("WARNING: src_chroma_sample_loc_type(%d) not 0 or 2\n", a.src_siting);
        arg_errors++;
    } else if (a.src_siting == 2 && chroma != H2Y_CHROMA_420) {
        printf("WARNING: --src_chroma_sample_loc_type 2 sites 4:2:0 chroma: src_chroma_format_idc(%d) has none to site\n", chroma);
        arg_errors++;
    } else if (a.src_siting == 2 && a.resampler == 0) {
        printf("WARNING: --src_chroma_sample_loc_type 2 needs the FIR resampler: replication (--chroma_resampler_type 0) is centre sited by "
               "construction\n");
        arg_errors++;
    }
    if (a.dynmeta && !cli_can_create(a.dynmeta)) {
        printf("WARNING: --dynamic_metadata: file (%s) cannot be created\n", a.dynmeta);
        arg_errors++;
    }
    a.out = a.in;
    if (arg_errors) return arg_errors;
    a.light = 1; /* the run keeps and reports content light's figures */
    static const char *const kMatrix[15] = {"G,B,R", "BT.709", "", "", "", "", "", "", "", "BT.2020nc", "", "", "", "", "ICtCp"};
    printf("light_only_from: PQ codes, bit_depth %d %s range, matrix_coeffs %d (%s), chroma_format_idc %d, upsampler %s\n", a.in.bit_depth,
           a.in.video_full_range_flag ? "full" : "video", m, kMatrix[m], chroma,
           chroma == H2Y_CHROMA_444 ? "none" : !a.resampler ? "replicate" : a.src_siting == 2 ? "fir_top_left" : "fir");
    if (a.dynmeta)
        printf("dynamic_metadata_from: PQ codes; HDR10+ profile A, one scene, percentiles of max(R,G,B) in %d bins\n", H2Y_LIGHTDIST_BINS);
    return 0;
}

static inline const char *cli_primaries_name(int p)
{
    return p == 1 ? "BT.709" : p == 8 || p == 9 ? "BT.2020" : p == 12 ? "P3-D65" : "unknown";
}

/* --gamut_check 1 and its sub-flags, beside --light_only 1: the checked sets from --src_colour_primaries, the widest first, T, A, the
 * set the limit judges; returns the number of argument errors */
static inline int cli_resolve_gamut_check(cli_args &a)
{
    int arg_errors = 0;
    printf("gamut_check: %d\n", a.gamut_check);
    if (a.gamut_check != 0 && a.gamut_check != 1) {
        printf("WARNING: gamut_check(%d) not 0 or 1\n", a.gamut_check);
        return 1;
    }
    if (a.light_only != 1) {
        printf("WARNING: --gamut_check and its sub-flags check a finished PQ master: they need --light_only 1 (a conversion's output: check the "
               "written file)\n");
        return 1;
    }
    if (a.gamut_check != 1) {
        if (a.gamut_check_ratio_given || a.gamut_check_floor_given || a.gamut_check_against_given || a.gamut_check_limit_given) {
            printf("WARNING: --gamut_check_ratio, --gamut_check_floor, --gamut_check_against and --gamut_check_limit need --gamut_check 1\n");
            arg_errors++;
        }
        return arg_errors;
    }
    const int f = a.in.colour_primaries;
    if (f == 8 || f == 9) a.gamut_check_n_sets = 2, a.gamut_check_sets[0] = 12, a.gamut_check_sets[1] = 1;
    else if (f == 12) a.gamut_check_n_sets = 1, a.gamut_check_sets[0] = 1;
    else {
        printf("WARNING: --gamut_check 1: src_colour_primaries(%d) must be 8 or 9 (BT.2020: checked against P3-D65 and BT.709) or 12 (P3-D65: "
               "against BT.709)%s\n", f, f == 1 ? "; nothing narrower than BT.709 is known" : "");
        arg_errors++;
    }
    if (!(a.gamut_check_ratio >= 0.0 && a.gamut_check_ratio <= 1.0)) {
        printf("WARNING: gamut_check_ratio(%g) outside range [0,1]\n", a.gamut_check_ratio);
        arg_errors++;
    }
    if (!(a.gamut_check_floor >= 0.0 && a.gamut_check_floor <= 1.7e308)) { /* negative, a NaN or an infinity */
        printf("WARNING: gamut_check_floor(%g) is not a finite number of cd/m2, 0 or more\n", a.gamut_check_floor);
        arg_errors++;
    }
    if (a.gamut_check_limit_given && !(a.gamut_check_limit >= 0.0 && a.gamut_check_limit <= 1.0)) {
        printf("WARNING: gamut_check_limit(%g) outside range [0,1]\n", a.gamut_check_limit);
        arg_errors++;
    }
    if (a.gamut_check_n_sets) {
        if (!a.gamut_check_against_given) a.gamut_check_against = a.gamut_check_sets[0];
        bool found = false;
        for (int s = 0; s < a.gamut_check_n_sets; s++) found = found || a.gamut_check_sets[s] == a.gamut_check_against;
        if (!found) {
            printf("WARNING: gamut_check_against(%d) is not among the checked sets (%d%s)\n", a.gamut_check_against, a.gamut_check_sets[0],
                   a.gamut_check_n_sets == 2 ? ", 1" : "");
            arg_errors++;
        }
    }
    if (arg_errors) return arg_errors;
    printf("gamut_check_from: primaries %d (%s) against", f, cli_primaries_name(f));
    for (int s = 0; s < a.gamut_check_n_sets; s++)
        printf("%s %d (%s)", s ? "," : "", a.gamut_check_sets[s], cli_primaries_name(a.gamut_check_sets[s]));
    printf("; ratio %g%s, floor %g cd/m2%s", a.gamut_check_ratio, a.gamut_check_ratio_given ? "" : " (default)", a.gamut_check_floor,
           a.gamut_check_floor_given ? "" : " (default)");
    if (a.gamut_check_limit_given)
        printf("; limit %g of the pixels beyond %d%s", a.gamut_check_limit, a.gamut_check_against, a.gamut_check_against_given ? "" : " (default)");
    printf("\n");
    return 0;
}

/* --src_ictcp: the codes --linearize 1, --light_only 1 or --compare_only 1 --delta_e 1 read are PQ I, Ct, Cp (include/hdr2yuv_hip.h,
 * "light of ICtCp code planes").  Runs before those flows' resolvers and gives the source matrix_coeffs 14, which they then accept;
 * returns the number of argument errors */
static inline int cli_resolve_src_ictcp(cli_args &a)
{
    printf("src_ictcp: %d\n", a.src_ictcp);
    if (a.src_ictcp != 0 && a.src_ictcp != 1) {
        printf("WARNING: src_ictcp(%d) not 0 or 1\n", a.src_ictcp);
        return 1;
    }
    if (!a.src_ictcp) return 0;
    int arg_errors = 0;
    if (a.linearize != 1 && a.light_only != 1 && !(a.compare_only && a.delta_e == 1)) {
        printf("WARNING: --src_ictcp 1 is the matrix of the codes a flow reads: it needs --linearize 1, --light_only 1 or --compare_only 1 --delta_e 1\n");
        arg_errors++;
    }
    if (a.src_hlg == 1) {
        printf("WARNING: --src_ictcp 1 reads PQ I, Ct, Cp: not with --src_hlg 1 (BT.2100's HLG form of ICtCp has other coefficients and is not built)\n");
        arg_errors++;
    }
    if (a.src_matrix_given) {
        printf("WARNING: --src_ictcp 1 is the source's matrix: leave out --src_matrix_coeffs (%d); 14 is YUVPrime1 in this program's list, "
               "H.273's 14 (ICtCp) is --src_ictcp 1\n", a.in.matrix_coeffs);
        arg_errors++;
    }
    if (!strcasecmp(cli_ext_of(a.src), "rgb")) {
        printf("WARNING: --src_ictcp 1: a .rgb holds planes R, G, B, not I, Ct, Cp: the source must be a .yuv\n");
        arg_errors++;
    }
    if (a.src_hlg != 1 && a.in.transfer_characteristics != 16) {
        printf("WARNING: --src_ictcp 1 reads PQ I, Ct, Cp: src_transfer_characteristics(%d) is not 16\n", a.in.transfer_characteristics);
        arg_errors++;
    }
    if (a.in.colour_primaries != 8 && a.in.colour_primaries != 9) {
        printf("WARNING: --src_ictcp 1: ICtCp is defined on BT.2020 primaries: src_colour_primaries(%d) is not 8 or 9\n", a.in.colour_primaries);
        arg_errors++;
    }
    if (a.linearize == 1 && a.ictcp != 1 && a.out.matrix_coeffs == -1) {
        printf("WARNING: --src_ictcp 1: the source has no matrix code for the destination to take: give --dst_matrix_coeffs (or --ictcp 1)\n");
        arg_errors++;
    }
    if (arg_errors) return arg_errors;
    a.in.matrix_coeffs = H2Y_MATRIX_ICTCP;
    return 0;
}

/* --src_hlg / --src_hlg_peak: the codes --linearize 1 reads are HLG's (include/hdr2yuv_hip.h, "light of HLG code planes"), turned into
 * display light at a peak of src_hlg_peak cd/m2.  Runs before cli_resolve_linearize, which then skips its transfer check; prints the
 * src_hlg lines; returns the number of argument errors */
static inline int cli_resolve_src_hlg(cli_args &a)
{
    printf("src_hlg: %d\n", a.src_hlg);
    if (a.src_hlg != 0 && a.src_hlg != 1) {
        printf("WARNING: src_hlg(%d) not 0 or 1\n", a.src_hlg);
        return 1;
    }
    if (!a.src_hlg) {
        if (a.src_hlg_peak_given) {
            printf("WARNING: --src_hlg_peak needs --src_hlg 1\n");
            return 1;
        }
        return 0;
    }
    int arg_errors = 0;
    if (a.linearize != 1) {
        printf("WARNING: --src_hlg 1 is the transfer of the source --linearize 1 reads: it needs --linearize 1\n");
        arg_errors++;
    }
    if (a.light_only || a.compare_only || a.delta_e) {
        printf("WARNING: --src_hlg 1: --%s reads PQ codes, not an HLG master's (MaxCLL and HDR10+ of one: --linearize 1 --src_hlg 1 --content_light 1 "
               "--dynamic_metadata FILE to a PQ destination)\n", a.light_only ? "light_only" : a.compare_only ? "compare_only" : "delta_e");
        arg_errors++;
    }
    if (a.src_transfer_given) {
        printf("WARNING: --src_hlg 1 is the source's transfer: leave out --src_transfer_characteristics (%d); 18 is RHO_GAMMA in this program, "
               "H.273's 18 (HLG) is --src_hlg 1\n", a.in.transfer_characteristics);
        arg_errors++;
    }
    if (a.out.transfer_characteristics == -1) {
        printf("WARNING: --src_hlg 1: the source has no transfer code for the destination to take: give --dst_transfer_characteristics (or --hlg 1)\n");
        arg_errors++;
    }
    std::vector<float> ootf(H2Y_LIGHTDIST_BINS), inv(H2Y_LIGHTDIST_BINS);
    float kappa;
    double gamma = 0;
    const char *why;
    if (h2y_hlg_inverse_tables(a.src_hlg_peak, ootf.data(), inv.data(), &kappa, &gamma, &why)) {
        printf("WARNING: --src_hlg 1: src_hlg_peak(%d): %s\n", a.src_hlg_peak, why);
        arg_errors++;
    }
    if (arg_errors) return arg_errors;
    printf("src_hlg_peak: %d%s\nsrc_hlg_gamma: %.4f\n", a.src_hlg_peak, a.src_hlg_peak_given ? "" : " (default)", gamma);
    printf("src_hlg_note: src_transfer_characteristics 18 is RHO_GAMMA in this program; H.273's 18 (HLG) is --src_hlg 1\n");
    return 0;
}

/* --src_sdr / --src_sdr_white: the codes --linearize 1 reads are an SDR master's (include/hdr2yuv_hip.h, "light of SDR code planes"),
 * placed in absolute light with the reference white at src_sdr_white cd/m2.  Runs before cli_resolve_linearize, which then skips its
 * transfer check; prints the src_sdr lines; returns the number of argument errors */
static inline int cli_resolve_src_sdr(cli_args &a)
{
    printf("src_sdr: %d\n", a.src_sdr);
    if (a.src_sdr != 0 && a.src_sdr != 1) {
        printf("WARNING: src_sdr(%d) not 0 or 1\n", a.src_sdr);
        return 1;
    }
    if (!a.src_sdr) {
        if (a.src_sdr_white_given) {
            printf("WARNING: --src_sdr_white needs --src_sdr 1\n");
            return 1;
        }
        return 0;
    }
    int arg_errors = 0;
    if (a.linearize != 1) {
        printf("WARNING: --src_sdr 1 is the transfer of the source --linearize 1 reads: it needs --linearize 1\n");
        arg_errors++;
    }
    if (a.src_hlg == 1 || a.src_ictcp == 1) {
        printf("WARNING: --src_sdr 1: the file's codes are BT.1886's: not with --%s 1\n", a.src_hlg == 1 ? "src_hlg" : "src_ictcp");
        arg_errors++;
    }
    if (a.light_only || a.compare_only || a.hist_only || a.scale_only) {
        printf("WARNING: --src_sdr 1 is the source of a conversion: not with --%s 1\n",
               a.light_only ? "light_only" : a.compare_only ? "compare_only" : a.hist_only ? "histogram_only" : "scale_only");
        arg_errors++;
    }
    const int t = a.in.transfer_characteristics;
    if (a.src_transfer_given && t != 1 && t != 6 && t != 14 && t != 15) {
        printf("WARNING: --src_sdr 1 reads BT.1886 codes: src_transfer_characteristics(%d) is not 1, 6, 14 or 15 (or leave it out)\n", t);
        arg_errors++;
    }
    if (a.out.transfer_characteristics == -1) {
        printf("WARNING: --src_sdr 1: the destination must not inherit BT.1886 from a source that becomes absolute light: give "
               "--dst_transfer_characteristics (or --hlg 1 / --ictcp 1)\n");
        arg_errors++;
    }
    if (a.src_sdr_white < H2Y_SDR_WHITE_MIN || a.src_sdr_white > H2Y_SDR_WHITE_MAX) {
        printf("WARNING: --src_sdr 1: src_sdr_white(%d) outside %d <= white <= %d cd/m2\n", a.src_sdr_white, H2Y_SDR_WHITE_MIN, H2Y_SDR_WHITE_MAX);
        arg_errors++;
    }
    if (arg_errors) return arg_errors;
    printf("src_sdr_white: %d%s\nsrc_sdr_gamma: 2.4\n", a.src_sdr_white, a.src_sdr_white_given ? "" : " (default)");
    return 0;
}

/* --src_signal: the codes --linearize 1 reads reach the signal-mode LUT as the signal they are (include/hdr2yuv_hip.h, "signal of code
 * planes").  Runs before cli_resolve_linearize, which then skips its transfer check; prints the src_signal line; returns the number
 * of argument errors */
static inline int cli_resolve_src_signal(cli_args &a)
{
    printf("src_signal: %d\n", a.src_signal);
    if (a.src_signal != 0 && a.src_signal != 1) {
        printf("WARNING: src_signal(%d) not 0 or 1\n", a.src_signal);
        return 1;
    }
    if (!a.src_signal) return 0;
    int arg_errors = 0;
    if (a.linearize != 1) {
        printf("WARNING: --src_signal 1 is what becomes of the source --linearize 1 reads: it needs --linearize 1\n");
        arg_errors++;
    }
    if (!a.lut3d || a.lut3d_signal != 1) {
        printf("WARNING: --src_signal 1 needs --lut3d FILE.cube --lut3d_signal 1: unscaled signal cannot reach a passthrough conversion, the "
               "table's scale step must stand between them\n");
        arg_errors++;
    }
    if (a.src_hlg == 1 || a.src_sdr == 1 || a.src_ictcp == 1) {
        printf("WARNING: --src_signal 1 applies no transfer and reads R'G'B' signal: not with --%s 1\n",
               a.src_hlg == 1 ? "src_hlg" : a.src_sdr == 1 ? "src_sdr" : "src_ictcp");
        arg_errors++;
    }
    if (a.tone_map == 1 || a.gamut == 1) {
        printf("WARNING: --src_signal 1: the planes hold signal, and --%s 1 acts on light: not together\n", a.tone_map == 1 ? "tone_map" : "gamut_convert");
        arg_errors++;
    }
    if (a.light_only || a.compare_only || a.hist_only || a.scale_only) {
        printf("WARNING: --src_signal 1 is the source of a conversion: not with --%s 1\n",
               a.light_only ? "light_only" : a.compare_only ? "compare_only" : a.hist_only ? "histogram_only" : "scale_only");
        arg_errors++;
    }
    return arg_errors;
}

/* --linearize 1: a PQ .yuv or .rgb as the forward flow's source.  Checks the file's attributes as --light_only checks them, gives the
 * destination what it leaves unset from the source as parsed (hdr2yuv.cpp:265-318), keeps the file's attributes in a.lin and
 * rewrites a.in to the planes the ring decodes -- F32, LINEAR, G,B,R, 4:4:4 -- so that every resolver after this one sees a .f32
 * source; returns the number of argument errors */
static inline int cli_resolve_linearize(cli_args &a)
{
    int arg_errors = 0;
    const char *ext = cli_ext_of(a.src);
    if (a.synthetic < 0 && !strcasecmp(ext, "yuv")) a.lin_type = CLI_IN_YUV;
    else if (a.synthetic < 0 && !strcasecmp(ext, "rgb")) a.lin_type = CLI_IN_RGB;
    else {
        printf("WARNING: --linearize 1 reads .yuv or .rgb; source file (%s) is a .%s\n", a.src ? a.src : "(none)", ext);
        arg_errors++;
    }
    if (a.light_only || a.compare_only || a.hist_only || a.scale_only) {
        printf("WARNING: --linearize 1 is the source of a conversion: not with --%s 1\n",
               a.light_only ? "light_only" : a.compare_only ? "compare_only" : a.hist_only ? "histogram_only" : "scale_only");
        arg_errors++;
    }
    const char *dext = cli_ext_of(a.dst ? a.dst : a.ref);
    if (!strcasecmp(dext, "rgb") || !strcasecmp(dext, "tiff")) {
        printf("WARNING: --linearize 1 is the forward flow's source (to .yuv): a .%s %s is the .yuv -> RGB flow's\n", dext,
               a.dst ? "destination" : "reference");
        arg_errors++;
    }
    if (a.in.width < 1 || a.in.width > 10000) { printf("WARNING: pic_width(%d) outside range [1,10000]\n", a.in.width); arg_errors++; }
    if (a.in.height < 1 || a.in.height > 10000) { printf("WARNING: pic_height(%d) outside range [1,10000]\n", a.in.height); arg_errors++; }
    if (a.in.bit_depth < 8 || a.in.bit_depth > 16) { printf("WARNING: src bit_depth(%d) outside range [8,16]\n", a.in.bit_depth); arg_errors++; }
    if (a.in.video_full_range_flag != 0 && a.in.video_full_range_flag != 1) {
        printf("WARNING: video_full_range_flag(%d) not 0 or 1\n", a.in.video_full_range_flag);
        arg_errors++;
    }
    if (a.src_hlg != 1 && a.src_sdr != 1 && a.src_signal != 1 && a.in.transfer_characteristics != 16) { /* (--src_hlg 1 and --src_sdr 1 are the source's transfer: their resolvers; --src_signal 1 applies none) */
        printf("WARNING: --linearize 1 linearises PQ codes: src_transfer_characteristics(%d) is not 16\n", a.in.transfer_characteristics);
        arg_errors++;
    }
    const int m = a.in.matrix_coeffs, chroma = a.in.chroma_format_idc;
    if (m != H2Y_MATRIX_GBR && m != H2Y_MATRIX_BT709 && m != H2Y_MATRIX_BT2020NC && !cli_src_is_ictcp(a, m)) {
        printf("WARNING: --linearize 1: src_matrix_coeffs(%d) not %d (G,B,R), %d (BT.709) or %d (BT.2020nc)\n", m, H2Y_MATRIX_GBR,
               H2Y_MATRIX_BT709, H2Y_MATRIX_BT2020NC);
        arg_errors++;
    } else if (a.lin_type == CLI_IN_RGB && m != H2Y_MATRIX_GBR) {
        printf("WARNING: a .rgb holds planes R, G, B: --linearize of a .rgb takes src_matrix_coeffs %d, not %d\n", H2Y_MATRIX_GBR, m);
        arg_errors++;
    } else if (a.lin_type == CLI_IN_YUV && m == H2Y_MATRIX_GBR) {
        printf("WARNING: a .yuv holds planes Y, Cb, Cr: --linearize of a .yuv takes src_matrix_coeffs %d or %d, not %d\n", H2Y_MATRIX_BT709,
               H2Y_MATRIX_BT2020NC, m);
        arg_errors++;
    }
    if (chroma == 2) { printf("WARNING: --linearize 1: chroma_format_idc 2 (4:2:2) is not linearised\n"); arg_errors++; }
    else if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) {
        printf("WARNING: chroma_format_idc(%d) not %d or %d\n", chroma, H2Y_CHROMA_420, H2Y_CHROMA_444);
        arg_errors++;
    } else if (chroma == H2Y_CHROMA_420 && (a.lin_type == CLI_IN_RGB || m == H2Y_MATRIX_GBR)) {
        printf("WARNING: --linearize 1: G,B,R planes (a .rgb, src_matrix_coeffs %d) are 4:4:4, not chroma_format_idc %d\n", H2Y_MATRIX_GBR, chroma);
        arg_errors++;
    } else if (chroma == H2Y_CHROMA_420 && ((a.in.width | a.in.height) & 1)) {
        printf("WARNING: --linearize 1: 4:2:0 needs an even width and height, not %dx%d\n", a.in.width, a.in.height);
        arg_errors++;
    }
    if (a.src_siting_given) printf("src_chroma_sample_loc_type: %d\n", a.src_siting);
    if (a.src_siting == 1) {
        printf("WARNING: src_chroma_sample_loc_type(1) is replication's siting, --chroma_resampler_type 0: not selected by this flag\n");
        arg_errors++;
    } else if (a.src_siting != 0 && a.src_siting != 2) {
        printf("WARNING: src_chroma_sample_loc_type(%d) not 0 or 2\n", a.src_siting);
        arg_errors++;
    } else if (a.src_siting == 2 && chroma != H2Y_CHROMA_420) {
        printf("WARNING: --src_chroma_sample_loc_type 2 sites 4:2:0 chroma: src_chroma_format_idc(%d) has none to site\n", chroma);
        arg_errors++;
    } else if (a.src_siting == 2 && a.resampler == 0) {
        printf("WARNING: --src_chroma_sample_loc_type 2 needs the FIR resampler: replication (--chroma_resampler_type 0) is centre sited by "
               "construction\n");
        arg_errors++;
    }
    if (arg_errors) return arg_errors;
    static const char *const kMatrix[15] = {"G,B,R", "BT.709", "", "", "", "", "", "", "", "BT.2020nc", "", "", "", "", "ICtCp"};
    printf("linearize_from: %s, bit_depth %d %s range, matrix_coeffs %d (%s), chroma_format_idc %d, upsampler %s\n",
           a.src_hlg == 1 ? "HLG codes" : a.src_sdr == 1 ? "SDR (BT.1886) codes" : a.src_signal == 1 ? "signal (no transfer applied)" : "PQ codes", a.in.bit_depth,
           a.in.video_full_range_flag ? "full" : "video", m, kMatrix[m], chroma,
           chroma == H2Y_CHROMA_444 ? "none" : !a.resampler ? "replicate" : a.src_siting == 2 ? "fir_top_left" : "fir");
    /* hdr2yuv.cpp:265-318: unset destination attributes <- the source's, as parsed */
    if (a.out.bit_depth == 0) a.out.bit_depth = a.in.bit_depth;
    if (a.out.chroma_format_idc == -1) a.out.chroma_format_idc = a.in.chroma_format_idc;
    if (a.out.video_full_range_flag == -1) a.out.video_full_range_flag = a.in.video_full_range_flag;
    if (a.out.colour_primaries == -1) a.out.colour_primaries = a.in.colour_primaries;
    if (a.out.transfer_characteristics == -1) a.out.transfer_characteristics = a.in.transfer_characteristics;
    if (a.out.matrix_coeffs == -1) a.out.matrix_coeffs = a.in.matrix_coeffs;
    /* the planes the ring decodes: what a .f32 of the same picture would be given as */
    a.lin = a.in;
    a.in.bit_depth = 32;
    a.in.half_float_flag = 0;
    a.in.chroma_format_idc = H2Y_CHROMA_444;
    a.in.transfer_characteristics = H2Y_TRANSFER_LINEAR;
    a.in.matrix_coeffs = H2Y_MATRIX_GBR;
    return 0;
}

/* --dynamic_metadata FILE: content light's scope, and a FILE that can be created (an existing regular file that can be written, or
 * a name in a directory that can be written to; nothing is created here); returns the number of argument errors */
static inline int cli_resolve_dynmeta(cli_args &a)
{
    printf("dynamic_metadata_file: %s\n", a.dynmeta);
    if (cli_light_scope(a, "--dynamic_metadata FILE")) return 1;
    if (!cli_can_create(a.dynmeta)) {
        printf("WARNING: --dynamic_metadata: file (%s) cannot be created\n", a.dynmeta);
        return 1;
    }
    printf("dynamic_metadata_from: src_transfer_characteristics %d -> PQ, G,B,R, floor and ceiling %s; HDR10+ profile A, one scene, "
           "percentiles of max(R,G,B) in %d bins\n", a.in.transfer_characteristics,
           a.linearize == 1 ? "0 and 1 (--linearize 1)" : a.tone_map == 1 ? "0 and 1 (--tone_map 1)" : a.lut3d ? "0 and 1 (--lut3d)" : "of each frame's pic_stats",
           H2Y_LIGHTDIST_BINS);
    return 0;
}

/* The first frames a --scene_cuts FILE names into `firsts`, 0 put in front where the file leaves it out: decimal indices one a line,
 * strictly ascending, below n_frames; '#' comments and blank lines ignored.  Returns "" or what is wrong with the file. */
static inline std::string cli_read_scene_cuts(const char *path, long n_frames, std::vector<long> &firsts)
{
    FILE *f = fopen(path, "r");
    if (!f) return "cannot be read";
    firsts.assign(1, 0);
    std::string err;
    char line[256];
    long prev = -1;
    for (long no = 1; err.empty() && fgets(line, sizeof line, f); no++) {
        char *p = line;
        while (*p == ' ' || *p == '\t') p++;
        if (*p == '#' || *p == '\n' || *p == '\r' || !*p) continue;
        char *end = nullptr;
        const long v = (*p >= '0' && *p <= '9') ? strtol(p, &end, 10) : -1;
        while (end && (*end == ' ' || *end == '\t' || *end == '\r' || *end == '\n')) end++;
        if (v < 0 || !end || *end) err = "line " + std::to_string(no) + " is not a decimal frame index";
        else if (v <= prev) err = "line " + std::to_string(no) + " is not above the line before it";
        else if (v >= n_frames) err = "line " + std::to_string(no) + " names frame " + std::to_string(v) + ", the run has --n_frames " + std::to_string(n_frames);
        else if (v > 0) firsts.push_back(v);
        prev = v;
    }
    fclose(f);
    return err;
}

/* --scene_detect / --scene_threshold / --scene_cuts / --scene_qpfile: beside a --dynamic_metadata FILE that resolved; returns the
 * number of argument errors */
static inline int cli_resolve_scenes(cli_args &a)
{
    int arg_errors = 0;
    if (a.scene_detect_given) printf("scene_detect: %d\n", a.scene_detect);
    if (a.scene_detect != 0 && a.scene_detect != 1) {
        printf("WARNING: scene_detect(%d) not 0 or 1\n", a.scene_detect);
        return 1;
    }
    if (a.scene_detect == 1 && a.scene_cuts) {
        printf("WARNING: --scene_detect 1 finds the cuts, --scene_cuts FILE gives them: not both\n");
        return 1;
    }
    if (a.scenes() && !a.dynmeta) {
        printf("WARNING: %s makes the scenes of --dynamic_metadata FILE: it needs that flag\n", a.scene_cuts ? "--scene_cuts FILE" : "--scene_detect 1");
        return 1;
    }
    if (a.scene_threshold_given && a.scene_detect != 1) {
        printf("WARNING: --scene_threshold needs --scene_detect 1\n");
        arg_errors++;
    } else if (a.scene_detect == 1) {
        printf("scene_threshold: %.4f%s\nscene_grid: %dx%d\n", a.scene_threshold, a.scene_threshold_given ? "" : " (default)",
               H2Y_SCENESIG_COLS, H2Y_SCENESIG_ROWS);
        if (!(a.scene_threshold >= 0.0) || !std::isfinite(a.scene_threshold)) {
            printf("WARNING: scene_threshold(%g) is negative or not finite\n", a.scene_threshold);
            arg_errors++;
        }
    }
    if (a.scene_cuts) {
        const std::string err = cli_read_scene_cuts(a.scene_cuts, a.n_frames > 0 ? a.n_frames : 1, a.scene_firsts);
        if (!err.empty()) {
            printf("WARNING: --scene_cuts: file (%s) %s\n", a.scene_cuts, err.c_str());
            arg_errors++;
        } else printf("scene_cuts: %s %zu scenes\n", a.scene_cuts, a.scene_firsts.size());
    }
    if (a.scene_qpfile) {
        printf("scene_qpfile: %s\n", a.scene_qpfile);
        if (!a.scenes()) {
            printf("WARNING: --scene_qpfile OUT lists the scene starts: it needs --scene_detect 1 or --scene_cuts FILE\n");
            arg_errors++;
        } else if (!cli_can_create(a.scene_qpfile)) {
            printf("WARNING: --scene_qpfile: file (%s) cannot be created\n", a.scene_qpfile);
            arg_errors++;
        }
    }
    return arg_errors;
}

/* --gamut_convert / --gamut_clip: the forward flow's float or half G,B,R planes in linear light, between two sets of primaries the
 * library converts (src_matrix_arg: --src_matrix_coeffs as given); prints the matrix; returns the number of argument errors */
static inline int cli_resolve_gamut(cli_args &a, int src_matrix_arg)
{
    printf("gamut_convert: %d\ngamut_clip: %d%s\n", a.gamut, a.gamut_clip, a.gamut_clip_given ? "" : " (default)");
    if (a.gamut != 0 && a.gamut != 1) {
        printf("WARNING: gamut_convert(%d) not 0 or 1\n", a.gamut);
        return 1;
    }
    if (a.gamut_clip != 0 && a.gamut_clip != 1) {
        printf("WARNING: gamut_clip(%d) not 0 or 1\n", a.gamut_clip);
        return 1;
    }
    if (a.gamut_compress_given && a.gamut_compress != 0 && a.gamut_compress != 1) {
        printf("WARNING: gamut_compress(%d) not 0 or 1\n", a.gamut_compress);
        return 1;
    }
    if (a.gamut_compress_threshold_bad || a.gamut_compress_power_bad) {
        printf("WARNING: --gamut_compress_%s is not a number\n", a.gamut_compress_threshold_bad ? "threshold" : "power");
        return 1;
    }
    if (!a.gamut_compress && (a.gamut_compress_threshold_given || a.gamut_compress_power_given)) {
        printf("WARNING: --gamut_compress_%s needs --gamut_compress 1\n", a.gamut_compress_threshold_given ? "threshold" : "power");
        return 1;
    }
    if (!a.gamut) {
        if (a.gamut_clip_given) { printf("WARNING: --gamut_clip needs --gamut_convert 1\n"); return 1; }
        if (a.gamut_compress) { printf("WARNING: --gamut_compress 1 needs --gamut_convert 1\n"); return 1; }
        return 0;
    }
    if (a.compare_only || a.hist_only || a.scale_only) {
        printf("WARNING: --gamut_convert 1 converts a conversion's source: not with --%s 1\n",
               a.compare_only ? "compare_only" : a.hist_only ? "histogram_only" : "scale_only");
        return 1;
    }
    if (a.inverse) {
        printf("WARNING: --gamut_convert 1 converts the forward flow's source (to .yuv), not the .yuv -> RGB flow\n");
        return 1;
    }
    if (a.in_type != CLI_IN_F32 && a.in_type != CLI_IN_F16 && a.in_type != CLI_IN_EXR && a.in_type != CLI_IN_DPX) {
        printf("WARNING: --gamut_convert 1 converts float or half planes (.f32, .f16, .exr, .dpx input), not .%s input\n",
               a.in_type == CLI_IN_SYNTH ? "(synthetic)" : cli_ext_of(a.src));
        return 1;
    }
    if (a.in.transfer_characteristics != H2Y_TRANSFER_LINEAR) {
        printf("WARNING: --gamut_convert 1 converts linear light: src_transfer_characteristics(%d) is not %d\n",
               a.in.transfer_characteristics, H2Y_TRANSFER_LINEAR);
        return 1;
    }
    if (src_matrix_arg != H2Y_MATRIX_GBR) { /* the readers would override it: a source called Y'CbCr is not one to convert as R, G, B */
        printf("WARNING: --gamut_convert 1 needs a G,B,R source: src_matrix_coeffs(%d) is not %d\n", src_matrix_arg, H2Y_MATRIX_GBR);
        return 1;
    }
    float m[9];
    const char *why = nullptr;
    if (h2y_gamut_matrix(a.in.colour_primaries, a.out.colour_primaries, m, &why)) {
        printf("WARNING: --gamut_convert 1: src_colour_primaries(%d) -> dst_colour_primaries(%d): %s\n", a.in.colour_primaries,
               a.out.colour_primaries, why);
        return 1;
    }
    printf("gamut_matrix:");
    for (int i = 0; i < 9; i++) printf(" %.9g", m[i]);
    printf("\n");
    return a.gamut_compress ? cli_resolve_gamut_compress(a) : 0;
}

/* --gamut_compress 1 and its two parameters beside a --gamut_convert 1 that resolved: prints the setting and the limits; returns the
 * number of argument errors */
static inline int cli_resolve_gamut_compress(cli_args &a)
{
    printf("gamut_compress: 1\ngamut_compress_threshold: %.9g%s\ngamut_compress_power: %.9g%s\n", a.gamut_compress_threshold,
           a.gamut_compress_threshold_given ? "" : " (default)", a.gamut_compress_power, a.gamut_compress_power_given ? "" : " (default)");
    if (a.gamut_clip_given) {
        printf("WARNING: --gamut_compress 1 has its own rule at 0: leave out --gamut_clip\n");
        return 1;
    }
    std::unique_ptr<h2y_gamut_compress_tables> c(new h2y_gamut_compress_tables);
    const char *why = nullptr;
    if (h2y_gamut_compress_curve(a.in.colour_primaries, a.out.colour_primaries, a.gamut_compress_threshold, a.gamut_compress_power, c.get(),
                                 &why)) {
        printf("WARNING: --gamut_compress 1: src_colour_primaries(%d) -> dst_colour_primaries(%d), threshold %g, power %g: %s\n",
               a.in.colour_primaries, a.out.colour_primaries, a.gamut_compress_threshold, a.gamut_compress_power, why);
        return 1;
    }
    printf("gamut_compress_limits:");
    for (int i = 0; i < 3; i++) {
        if (c->limit[i] > 1.0f) printf(" %.9g", c->limit[i]);
        else printf(" none");
    }
    printf("\n");
    return 0;
}

/* ST 2084's inverse EOTF and its inverse in binary64, as include/hdr2yuv_hip.h states them: for the knee the banner prints */
static inline double cli_pq_n(double l)
{
    const double p = pow(l, 2610.0 / 16384.0);
    return pow((3424.0 / 4096.0 + 2413.0 / 4096.0 * 32.0 * p) / (1.0 + 2392.0 / 4096.0 * 32.0 * p), 2523.0 / 4096.0 * 128.0);
}
static inline double cli_pq_n_inv(double v)
{
    const double p = pow(v, 1.0 / (2523.0 / 4096.0 * 128.0)), num = p - 3424.0 / 4096.0;
    return pow((num > 0.0 ? num : 0.0) / (2413.0 / 4096.0 * 32.0 - 2392.0 / 4096.0 * 32.0 * p), 1.0 / (2610.0 / 16384.0));
}

/* --tone_map / --tone_map_src_peak / --tone_map_dst_peak: the forward flow's float or half G,B,R planes in linear light, between
 * two peaks the library's curve takes (src_matrix_arg: --src_matrix_coeffs as given); prints the peaks, the output's reference and
 * the knee; returns the number of argument errors */
static inline int cli_resolve_tone_map(cli_args &a, int src_matrix_arg)
{
    printf("tone_map: %d\n", a.tone_map);
    if (a.tone_map != 0 && a.tone_map != 1) {
        printf("WARNING: tone_map(%d) not 0 or 1\n", a.tone_map);
        return 1;
    }
    if (!a.tone_map) {
        if (a.tone_src_peak_given || a.tone_dst_peak_given) {
            printf("WARNING: --tone_map_src_peak and --tone_map_dst_peak need --tone_map 1\n");
            return 1;
        }
        return 0;
    }
    printf("tone_map_src_peak: %d%s\ntone_map_dst_peak: %d%s\n", a.tone_src_peak, a.tone_src_peak_given ? "" : " (default)",
           a.tone_dst_peak, a.tone_dst_peak_given ? "" : " (default)");
    if (a.compare_only || a.hist_only || a.scale_only) {
        printf("WARNING: --tone_map 1 maps a conversion's source: not with --%s 1\n",
               a.compare_only ? "compare_only" : a.hist_only ? "histogram_only" : "scale_only");
        return 1;
    }
    if (a.inverse) {
        printf("WARNING: --tone_map 1 maps the forward flow's source (to .yuv), not the .yuv -> RGB flow\n");
        return 1;
    }
    if (a.in_type != CLI_IN_F32 && a.in_type != CLI_IN_F16 && a.in_type != CLI_IN_EXR && a.in_type != CLI_IN_DPX) {
        printf("WARNING: --tone_map 1 maps float or half planes (.f32, .f16, .exr, .dpx input), not .%s input\n",
               a.in_type == CLI_IN_SYNTH ? "(synthetic)" : cli_ext_of(a.src));
        return 1;
    }
    if (a.in.transfer_characteristics != H2Y_TRANSFER_LINEAR) {
        printf("WARNING: --tone_map 1 maps linear light: src_transfer_characteristics(%d) is not %d\n", a.in.transfer_characteristics,
               H2Y_TRANSFER_LINEAR);
        return 1;
    }
    if (src_matrix_arg != H2Y_MATRIX_GBR) { /* the readers would override it: a source called Y'CbCr is not one to map as R, G, B */
        printf("WARNING: --tone_map 1 needs a G,B,R source: src_matrix_coeffs(%d) is not %d\n", src_matrix_arg, H2Y_MATRIX_GBR);
        return 1;
    }
    const bool lut_signal = a.lut3d && a.lut3d_signal == 1; /* (--hlg 1, --ictcp 1 and a signal-mode LUT are the display's transfer) */
    if (a.out.transfer_characteristics == H2Y_TRANSFER_LINEAR && a.hlg != 1 && a.ictcp != 1 && !lut_signal) {
        printf("WARNING: --tone_map 1 maps light for a display: dst_transfer_characteristics(%d) keeps linear light\n",
               a.out.transfer_characteristics);
        return 1;
    }
    a.tone_relative = a.out.transfer_characteristics != 16 && a.ictcp != 1; /* (an ICtCp rung is PQ) */
    std::vector<float> gain(H2Y_LIGHTDIST_BINS);
    float cap = 0.0f;
    const char *why = nullptr;
    if (h2y_tonemap_curve(a.tone_src_peak, a.tone_dst_peak, a.tone_relative, gain.data(), &cap, &why)) {
        printf("WARNING: --tone_map 1: tone_map_src_peak(%d) -> tone_map_dst_peak(%d): %s\n", a.tone_src_peak, a.tone_dst_peak, why);
        return 1;
    }
    const double W = cli_pq_n(a.tone_src_peak / 10000.0), ks = 1.5 * (cli_pq_n(a.tone_dst_peak / 10000.0) / W) - 0.5;
    printf("tone_map_output: %s\ntone_map_knee: %.9g\n", a.tone_relative ? "relative" : "absolute", 10000.0 * cli_pq_n_inv(ks * W));
    return 0;
}

/* --lut3d / --lut3d_interp / --lut3d_signal: the forward flow's float or half G,B,R planes through a .cube table the library's
 * parser reads (src_matrix_arg: --src_matrix_coeffs as given; in signal mode cli_resolve_all replaced the destination's transfer
 * with the source's and kept what was given; cli_resolve_tone_map ran before); prints the file, the table's title, size and domain
 * and the two modes; returns the number of argument errors */
static inline int cli_resolve_lut3d(cli_args &a, int src_matrix_arg)
{
    printf("lut3d: %s\n", a.lut3d ? a.lut3d : "(none)");
    if (!a.lut3d) {
        printf("WARNING: --lut3d_interp and --lut3d_signal need --lut3d FILE.cube\n");
        return 1;
    }
    int arg_errors = 0;
    if (a.lut3d_interp != 0 && a.lut3d_interp != 1) { printf("WARNING: lut3d_interp(%d) not 0 or 1\n", a.lut3d_interp); arg_errors++; }
    if (a.lut3d_signal != 0 && a.lut3d_signal != 1) { printf("WARNING: lut3d_signal(%d) not 0 or 1\n", a.lut3d_signal); arg_errors++; }
    if (arg_errors) return arg_errors;
    if (a.compare_only || a.hist_only || a.scale_only) {
        printf("WARNING: --lut3d applies to a conversion's source: not with --%s 1\n",
               a.compare_only ? "compare_only" : a.hist_only ? "histogram_only" : "scale_only");
        return 1;
    }
    if (a.inverse) {
        printf("WARNING: --lut3d applies to the forward flow's source (to .yuv), not the .yuv -> RGB flow\n");
        return 1;
    }
    if (a.in_type != CLI_IN_F32 && a.in_type != CLI_IN_F16 && a.in_type != CLI_IN_EXR && a.in_type != CLI_IN_DPX) {
        printf("WARNING: --lut3d applies to float or half planes (.f32, .f16, .exr, .dpx input, or --linearize 1 from a .yuv / .rgb), not "
               ".%s input\n", a.in_type == CLI_IN_SYNTH ? "(synthetic)" : cli_ext_of(a.src));
        return 1;
    }
    if (src_matrix_arg != H2Y_MATRIX_GBR) { /* the readers would override it: a source called Y'CbCr is not one to look up as R, G, B */
        printf("WARNING: --lut3d needs a G,B,R source: src_matrix_coeffs(%d) is not %d\n", src_matrix_arg, H2Y_MATRIX_GBR);
        return 1;
    }
    if (a.lut3d_signal == 1) {
        if (a.hlg == 1 || a.ictcp == 1) {
            printf("WARNING: --lut3d_signal 1 leaves the destination's signal: not with --%s 1, which writes its own\n", a.hlg == 1 ? "hlg" : "ictcp");
            arg_errors++;
        }
        if (a.light || a.dynmeta) {
            printf("WARNING: --lut3d_signal 1: --content_light and --dynamic_metadata measure light, not a LUT's signal\n");
            arg_errors++;
        }
        if (a.in_type != CLI_IN_F32 && a.in_type != CLI_IN_DPX) {
            printf("WARNING: --lut3d_signal 1 leaves code-valued samples in float planes (.f32 or .dpx input, or --linearize 1), not in the "
                   "half planes of .%s input\n", cli_ext_of(a.src));
            arg_errors++;
        }
        if (a.out_type != CLI_OUT_YUV) {
            printf("WARNING: --lut3d_signal 1 writes .yuv frames: not a .%s destination\n", cli_ext_of(a.dst ? a.dst : a.ref));
            arg_errors++;
        }
        const int m = a.out.matrix_coeffs;
        if (m != H2Y_MATRIX_GBR && m != H2Y_MATRIX_BT2020NC) {
            printf("WARNING: --lut3d_signal 1: dst_matrix_coeffs(%d) not %d (G,B,R) or %d (BT.2020nc)\n", m, H2Y_MATRIX_GBR, H2Y_MATRIX_BT2020NC);
            arg_errors++;
        }
        if (arg_errors) return arg_errors;
    }
    /* the file, whole */
    std::string text;
    FILE *f = fopen(a.lut3d, "rb");
    if (!f) {
        printf("WARNING: --lut3d: unable to open file %s\n", a.lut3d);
        return 1;
    }
    char buf[65536];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    const char *why = "";
    if (bad || h2y_lut3d_parse(text.data(), text.size(), &a.lut3d_table, &why)) {
        printf("WARNING: --lut3d: file %s: %s\n", a.lut3d, bad ? "read error" : why);
        return 1;
    }
    int n = 0;
    float dom[6];
    const char *title = "";
    h2y_lut3d_info(a.lut3d_table, &n, dom, &title);
    printf("lut3d_title: %s\nlut3d_size: %d\nlut3d_domain: %.9g %.9g %.9g .. %.9g %.9g %.9g\n", title, n, dom[0], dom[1], dom[2], dom[3], dom[4],
           dom[5]);
    printf("lut3d_interp: %d (%s)\nlut3d_signal: %d (%s)\n", a.lut3d_interp, a.lut3d_interp ? "tetrahedral" : "trilinear", a.lut3d_signal,
           a.lut3d_signal ? "signal" : "planes");
    if (a.lut3d_signal == 1 && a.lut3d_dst_transfer != -1) printf("lut3d_dst_transfer: %d\n", a.lut3d_dst_transfer);
    return 0;
}

/* --hlg / --hlg_peak: the forward flow's float G,B,R planes of display light in BT.2020 primaries, written as an HLG signal at a
 * nominal peak the library's tables take (src_matrix_arg: --src_matrix_coeffs as given; cli_resolve_all replaced the destination
 * transfer and kept what was given, cli_resolve_tone_map ran before); prints the peak, the system gamma, how the planes are
 * referred, the note on code 18 and the encoder flags; returns the number of argument errors */
static inline int cli_resolve_hlg(cli_args &a, int src_matrix_arg)
{
    printf("hlg: %d\n", a.hlg);
    if (a.hlg != 0 && a.hlg != 1) {
        printf("WARNING: hlg(%d) not 0 or 1\n", a.hlg);
        return 1;
    }
    if (!a.hlg) {
        if (a.hlg_peak_given) {
            printf("WARNING: --hlg_peak needs --hlg 1\n");
            return 1;
        }
        return 0;
    }
    if (a.tone_map == 1) {
        if (a.hlg_peak_given && a.hlg_peak != a.tone_dst_peak) {
            printf("WARNING: --hlg 1 beside --tone_map 1 writes the tone mapper's target: hlg_peak(%d) is not tone_map_dst_peak(%d)\n",
                   a.hlg_peak, a.tone_dst_peak);
            return 1;
        }
        if (!a.hlg_peak_given) a.hlg_peak = a.tone_dst_peak;
    }
    a.hlg_relative = a.tone_map == 1;
    printf("hlg_peak: %d%s\n", a.hlg_peak, a.hlg_peak_given ? "" : " (default)");
    int arg_errors = 0;
    if (a.hlg_dst_transfer != -1) {
        printf("WARNING: --hlg 1 is the destination's transfer: leave out --dst_transfer_characteristics (%d); 18 is RHO_GAMMA in this "
               "program, H.273's 18 (HLG) is --hlg 1\n", a.hlg_dst_transfer);
        arg_errors++;
    }
    if (a.compare_only || a.hist_only || a.scale_only) {
        printf("WARNING: --hlg 1 writes a conversion's rung: not with --%s 1\n",
               a.compare_only ? "compare_only" : a.hist_only ? "histogram_only" : "scale_only");
        return arg_errors + 1;
    }
    if (a.inverse) {
        printf("WARNING: --hlg 1 is the forward flow's (to .yuv), not the .yuv -> RGB flow's\n");
        return arg_errors + 1;
    }
    if (a.out_type != CLI_OUT_YUV) {
        printf("WARNING: --hlg 1 writes .yuv frames: not a .%s destination\n", cli_ext_of(a.dst ? a.dst : a.ref));
        return arg_errors + 1;
    }
    if (a.in_type != CLI_IN_F32 && a.in_type != CLI_IN_DPX) {
        printf("WARNING: --hlg 1 leaves code-valued samples in float planes (.f32 or .dpx input, or --linearize 1 from a PQ .yuv / .rgb), not "
               ".%s input\n", a.in_type == CLI_IN_SYNTH ? "(synthetic)" : cli_ext_of(a.src));
        return arg_errors + 1;
    }
    if (a.in.transfer_characteristics != H2Y_TRANSFER_LINEAR) {
        printf("WARNING: --hlg 1 takes linear light: src_transfer_characteristics(%d) is not %d\n", a.in.transfer_characteristics,
               H2Y_TRANSFER_LINEAR);
        arg_errors++;
    }
    if (src_matrix_arg != H2Y_MATRIX_GBR) {
        printf("WARNING: --hlg 1 needs a G,B,R source: src_matrix_coeffs(%d) is not %d\n", src_matrix_arg, H2Y_MATRIX_GBR);
        arg_errors++;
    }
    const int sp = a.in.colour_primaries, dp = a.out.colour_primaries;
    if ((dp != 8 && dp != 9) || (a.gamut != 1 && sp != dp)) {
        printf("WARNING: --hlg 1 takes BT.2020 primaries: %s_colour_primaries(%d) is not 8 or 9%s\n", (dp != 8 && dp != 9) ? "dst" : "src",
               (dp != 8 && dp != 9) ? dp : sp, a.gamut == 1 ? "" : " and the destination's (other primaries need --gamut_convert 1)");
        arg_errors++;
    }
    const int m = a.out.matrix_coeffs;
    if (m != H2Y_MATRIX_GBR && m != H2Y_MATRIX_BT2020NC) {
        printf("WARNING: --hlg 1: dst_matrix_coeffs(%d) not %d (G,B,R) or %d (BT.2020nc)\n", m, H2Y_MATRIX_GBR, H2Y_MATRIX_BT2020NC);
        arg_errors++;
    } else if (m == H2Y_MATRIX_GBR && sp != dp) { /* convert.cpp:1159, :1195: no ring opens on such a descriptor; said here, before any device */
        printf("WARNING: --hlg 1: dst_matrix_coeffs %d keeps G,B,R only where src_colour_primaries(%d) equals dst_colour_primaries(%d)\n", m,
               sp, dp);
        arg_errors++;
    }
    if (a.light || a.dynmeta || a.scene_detect_given || a.scene_threshold_given || a.scene_cuts || a.scene_qpfile) {
        printf("WARNING: --hlg 1: --content_light, --dynamic_metadata and the scene flags measure PQ's light, not an HLG rung's\n");
        arg_errors++;
    }
    if (a.delta_e_given || a.delta_e_threshold_given || a.delta_e_limit_given) {
        printf("WARNING: --hlg 1: --delta_e judges PQ codes, not an HLG rung's\n");
        arg_errors++;
    }
    std::vector<float> gain(H2Y_LIGHTDIST_BINS), oetf(H2Y_LIGHTDIST_BINS);
    float k = 0.0f;
    double gamma = 0.0;
    const char *why = nullptr;
    if (h2y_hlg_tables(a.hlg_peak, a.hlg_relative, gain.data(), oetf.data(), &k, &gamma, &why)) {
        printf("WARNING: --hlg 1: hlg_peak(%d): %s\n", a.hlg_peak, why);
        arg_errors++;
    }
    if (arg_errors) return arg_errors;
    printf("hlg_gamma: %.9g\nhlg_input: %s\n", gamma, a.hlg_relative ? "relative" : "absolute");
    printf("hlg_note: dst_transfer_characteristics 18 is RHO_GAMMA in this program; H.273's 18 (HLG) is --hlg 1\n");
    printf("hlg_encoder: x265 --transfer arib-std-b67 --colorprim bt2020 --colormatrix %s; SvtAv1EncApp --transfer-characteristics 18 "
           "--color-primaries 9 --matrix-coefficients %d\n", m == H2Y_MATRIX_GBR ? "gbr" : "bt2020nc", m);
    return 0;
}

/* --ictcp: the forward flow's float G,B,R planes of display light in BT.2020 primaries (1.0 = 10000 cd/m2), written as PQ I, Ct, Cp
 * (include/hdr2yuv_hip.h, "ICtCp").  src_matrix_arg: --src_matrix_coeffs as given; cli_resolve_all replaced the destination's transfer
 * and matrix with the passthrough descriptor's and kept what was given; prints the scale, the note on code 14 and the encoder flags;
 * returns the number of argument errors */
static inline int cli_resolve_ictcp(cli_args &a, int src_matrix_arg)
{
    printf("ictcp: %d\n", a.ictcp);
    if (a.ictcp != 0 && a.ictcp != 1) {
        printf("WARNING: ictcp(%d) not 0 or 1\n", a.ictcp);
        return 1;
    }
    if (!a.ictcp) return 0;
    if (a.hlg == 1) {
        printf("WARNING: --ictcp 1 writes PQ I, Ct, Cp: not with --hlg 1 (BT.2100's HLG form of ICtCp has other coefficients and is not built)\n");
        return 1;
    }
    int arg_errors = 0;
    if (a.ictcp_dst_matrix != -1) {
        printf("WARNING: --ictcp 1 is the destination's matrix: leave out --dst_matrix_coeffs (%d); 14 is YUVPrime1 in this program's list, "
               "H.273's 14 (ICtCp) is --ictcp 1\n", a.ictcp_dst_matrix);
        arg_errors++;
    }
    if (a.ictcp_dst_transfer != -1 && a.ictcp_dst_transfer != 16) {
        printf("WARNING: --ictcp 1 writes PQ I, Ct, Cp: dst_transfer_characteristics(%d) is not 16\n", a.ictcp_dst_transfer);
        arg_errors++;
    }
    if (a.compare_only || a.hist_only || a.scale_only) {
        printf("WARNING: --ictcp 1 writes a conversion's rung: not with --%s 1\n",
               a.compare_only ? "compare_only" : a.hist_only ? "histogram_only" : "scale_only");
        return arg_errors + 1;
    }
    if (a.inverse) {
        printf("WARNING: --ictcp 1 is the forward flow's (to .yuv), not the .yuv -> RGB flow's\n");
        return arg_errors + 1;
    }
    if (a.out_type != CLI_OUT_YUV) {
        printf("WARNING: --ictcp 1 writes .yuv frames: not a .%s destination\n", cli_ext_of(a.dst ? a.dst : a.ref));
        return arg_errors + 1;
    }
    if (a.in_type != CLI_IN_F32 && a.in_type != CLI_IN_DPX) {
        printf("WARNING: --ictcp 1 leaves code-valued samples in float planes (.f32 or .dpx input, or --linearize 1 from a .yuv / .rgb), not "
               ".%s input\n", a.in_type == CLI_IN_SYNTH ? "(synthetic)" : cli_ext_of(a.src));
        return arg_errors + 1;
    }
    if (a.in.transfer_characteristics != H2Y_TRANSFER_LINEAR) {
        printf("WARNING: --ictcp 1 takes linear light: src_transfer_characteristics(%d) is not %d\n", a.in.transfer_characteristics,
               H2Y_TRANSFER_LINEAR);
        arg_errors++;
    }
    if (src_matrix_arg != H2Y_MATRIX_GBR) {
        printf("WARNING: --ictcp 1 needs a G,B,R source: src_matrix_coeffs(%d) is not %d\n", src_matrix_arg, H2Y_MATRIX_GBR);
        arg_errors++;
    }
    const int sp = a.in.colour_primaries, dp = a.out.colour_primaries;
    if ((dp != 8 && dp != 9) || (a.gamut != 1 && sp != dp)) {
        printf("WARNING: --ictcp 1 takes BT.2020 primaries: %s_colour_primaries(%d) is not 8 or 9%s\n", (dp != 8 && dp != 9) ? "dst" : "src",
               (dp != 8 && dp != 9) ? dp : sp, a.gamut == 1 ? "" : " and the destination's (other primaries need --gamut_convert 1)");
        arg_errors++;
    }
    if (a.light || a.dynmeta || a.scene_detect_given || a.scene_threshold_given || a.scene_cuts || a.scene_qpfile) {
        printf("WARNING: --ictcp 1: --content_light, --dynamic_metadata and the scene flags read a ring whose dst_transfer is 16: measure the "
               "written file with --light_only 1 --src_ictcp 1\n");
        arg_errors++;
    }
    if (a.delta_e_given || a.delta_e_threshold_given || a.delta_e_limit_given) {
        printf("WARNING: --ictcp 1: --delta_e on the same run is not built: judge the written file with --compare_only 1 --src_ictcp 1 --delta_e 1\n");
        arg_errors++;
    }
    const int n = a.out.bit_depth, full = a.out.video_full_range_flag == 1;
    if (arg_errors || n < 8 || n > 16) return arg_errors; /* (a depth out of range has been refused already) */
    const long s = 1L << (n - 8), top = (1L << n) - 1;
    printf("ictcp_scale: oY %ld aY %ld oC %ld aC %ld\n", full ? top : 219 * s, full ? 0L : 16 * s, full ? top : 224 * s, full ? 1L << (n - 1) : 128 * s);
    printf("ictcp_note: dst_matrix_coeffs 14 is YUVPrime1, an unbuilt Y'u'v' variant, in this program's list; H.273's 14 (ICtCp) is --ictcp 1\n");
    printf("ictcp_encoder: x265 --colormatrix ictcp --transfer smpte2084 --colorprim bt2020 (no encoder has checked this output)\n");
    return 0;
}

/* --dst_chroma_sample_loc_type: the siting of the forward flow's 4:2:0 chroma, 0 (the FIR resampler's own) or 2 (top-left); returns
 * the number of argument errors */
static inline int cli_resolve_siting(cli_args &a)
{
    printf("dst_chroma_sample_loc_type: %d\n", a.siting);
    if (a.siting == 1) {
        printf("WARNING: dst_chroma_sample_loc_type(1) is the box resampler's siting, --chroma_resampler_type 0: not selected by this flag\n");
        return 1;
    }
    if (a.siting != 0 && a.siting != 2) {
        printf("WARNING: dst_chroma_sample_loc_type(%d) not 0 or 2\n", a.siting);
        return 1;
    }
    if (a.compare_only || a.hist_only) {
        printf("WARNING: --dst_chroma_sample_loc_type sites a conversion's chroma: not with --%s 1\n",
               a.compare_only ? "compare_only" : "histogram_only");
        return 1;
    }
    if (a.inverse) {
        printf("WARNING: --dst_chroma_sample_loc_type sites the forward flow's chroma (to .yuv): the .yuv -> RGB flow does not honour it\n");
        return 1;
    }
    if (!a.siting) return 0;
    if (a.scale_only) {
        printf("WARNING: --dst_chroma_sample_loc_type 2 sites a conversion's chroma: not with --scale_only 1\n");
        return 1;
    }
    if (a.out.chroma_format_idc != H2Y_CHROMA_420) {
        printf("WARNING: --dst_chroma_sample_loc_type 2 sites 4:2:0 chroma: dst_chroma_format_idc(%d) has none to site\n", a.out.chroma_format_idc);
        return 1;
    }
    if (a.resampler == 0) {
        printf("WARNING: --dst_chroma_sample_loc_type 2 needs the FIR resampler: the box (--chroma_resampler_type 0) is centre sited by construction\n");
        return 1;
    }
    if (a.out.matrix_coeffs == H2Y_MATRIX_YUVPRIME2) {
        printf("WARNING: --dst_chroma_sample_loc_type 2 is not defined for dst_matrix_coeffs(%d)\n", a.out.matrix_coeffs);
        return 1;
    }
    if (a.scale) {
        printf("WARNING: --dst_chroma_sample_loc_type 2 is not combined with --scale 1: the scaler aligns sample centres and would move the siting\n");
        return 1;
    }
    return 0;
}

/* --src_chroma_sample_loc_type: how the .yuv -> RGB flow takes its 4:2:0 chroma, 0 (as the reference's upsampler) or 2 (top-left);
 * returns the number of argument errors */
static inline int cli_resolve_src_siting(cli_args &a)
{
    printf("src_chroma_sample_loc_type: %d\n", a.src_siting);
    if (a.src_siting == 1) {
        printf("WARNING: src_chroma_sample_loc_type(1) is replication's siting, --chroma_resampler_type 0: not selected by this flag\n");
        return 1;
    }
    if (a.src_siting != 0 && a.src_siting != 2) {
        printf("WARNING: src_chroma_sample_loc_type(%d) not 0 or 2\n", a.src_siting);
        return 1;
    }
    if (a.compare_only || a.hist_only || a.scale_only) {
        printf("WARNING: --src_chroma_sample_loc_type sites the chroma a conversion reads: not with --%s 1\n",
               a.compare_only ? "compare_only" : a.hist_only ? "histogram_only" : "scale_only");
        return 1;
    }
    if (!a.inverse) {
        printf("WARNING: --src_chroma_sample_loc_type sites the chroma of the .yuv -> RGB flow (.yuv to .rgb or .tiff): the forward flow "
               "reads no subsampled chroma\n");
        return 1;
    }
    if (!a.src_siting) return 0;
    if (a.in.chroma_format_idc != H2Y_CHROMA_420) {
        printf("WARNING: --src_chroma_sample_loc_type 2 sites 4:2:0 chroma: src_chroma_format_idc(%d) has none to site\n", a.in.chroma_format_idc);
        return 1;
    }
    if (a.resampler == 0) {
        printf("WARNING: --src_chroma_sample_loc_type 2 needs the FIR resampler: replication (--chroma_resampler_type 0) is centre sited by "
               "construction\n");
        return 1;
    }
    return 0;
}

/* --ssim: valid wherever a comparison runs, on frames of 4:2:0 or 4:4:4 whose every plane holds an 8x8 window; returns the number
 * of argument errors */
static inline int cli_resolve_ssim(cli_args &a)
{
    printf("ssim: %d\n", a.ssim);
    if (a.ssim != 0 && a.ssim != 1) {
        printf("WARNING: ssim(%d) not 0 or 1\n", a.ssim);
        return 1;
    }
    if (!a.ssim) return 0;
    if (!a.ref) {
        printf("WARNING: --ssim 1 needs a comparison: --ref_filename R (with or without --dst_filename, or with --compare_only 1)\n");
        return 1;
    }
    const bool yuv = a.compare_only ? a.in_type == CLI_IN_YUV : a.out_type == CLI_OUT_YUV;
    const int chroma = yuv ? a.out.chroma_format_idc : H2Y_CHROMA_444, sub = chroma == H2Y_CHROMA_420;
    if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) {
        printf("WARNING: --ssim 1 compares 4:2:0 or 4:4:4 frames, not chroma_format_idc %d\n", chroma);
        return 1;
    }
    if ((a.out.width >> sub) < 8 || (a.out.height >> sub) < 8) {
        printf("WARNING: --ssim 1 needs every plane at least 8x8 (one window): %dx%d chroma_format_idc %d is smaller\n", a.out.width,
               a.out.height, chroma);
        return 1;
    }
    return 0;
}

/* --regions: valid wherever a comparison runs, on frames of 4:2:0 or 4:4:4; resolves V's default; returns the number of argument
 * errors */
static inline int cli_resolve_regions(cli_args &a)
{
    printf("regions: %d\n", a.regions);
    if (a.regions != 0 && a.regions != 1) {
        printf("WARNING: regions(%d) not 0 or 1\n", a.regions);
        a.regions = 0;
        return 1;
    }
    if (!a.regions) {
        if (a.regions_flat_var_given || a.regions_radius_given) {
            printf("WARNING: --regions_flat_var and --regions_radius need --regions 1\n");
            return 1;
        }
        return 0;
    }
    int arg_errors = 0;
    if (a.regions_radius < 1 || a.regions_radius > 4) { printf("WARNING: regions_radius(%d) outside range [1,4]\n", a.regions_radius); arg_errors++; }
    if (a.regions_flat_var_given && (a.regions_flat_var_arg < 0 || a.regions_flat_var_arg > 4294967295ll)) {
        printf("WARNING: regions_flat_var(%lld) outside range [0,4294967295]\n", a.regions_flat_var_arg);
        arg_errors++;
    }
    const bool compares = a.ref && !a.hist_only && !a.scale_only && !a.light_only && !a.dither_only;
    if (!compares) {
        printf("WARNING: --regions 1 needs a comparison: --ref_filename R (with or without --dst_filename, or with --compare_only 1)\n");
        return arg_errors + 1;
    }
    const bool yuv = a.compare_only ? a.in_type == CLI_IN_YUV : a.out_type == CLI_OUT_YUV;
    const int chroma = yuv ? a.out.chroma_format_idc : H2Y_CHROMA_444;
    if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) {
        printf("WARNING: --regions 1 compares 4:2:0 or 4:4:4 frames, not chroma_format_idc %d\n", chroma);
        return arg_errors + 1;
    }
    if (arg_errors) return arg_errors;
    const int d = a.out.bit_depth < 8 ? 8 : a.out.bit_depth > 16 ? 16 : a.out.bit_depth; /* (a depth outside 8..16 is refused by its flow) */
    a.regions_flat_var = a.regions_flat_var_given ? (uint32_t)a.regions_flat_var_arg : 4u << (2 * (d - 8));
    printf("regions_flat_var: %u%s\nregions_radius: %d\n", a.regions_flat_var, a.regions_flat_var_given ? "" : " (default)", a.regions_radius);
    return 0;
}

/* --delta_e: valid wherever a comparison runs on PQ code frames of BT.2020 primaries -- the source and R of --compare_only, or the
 * .yuv a forward run produces -- with the attribute checks of --light_only on those frames; fills a.de and a.de_siting; returns the
 * number of argument errors */
static inline int cli_resolve_delta_e(cli_args &a)
{
    printf("delta_e: %d\n", a.delta_e);
    if (a.delta_e != 0 && a.delta_e != 1) {
        printf("WARNING: delta_e(%d) not 0 or 1\n", a.delta_e);
        return 1;
    }
    if (!a.delta_e) {
        if (a.delta_e_threshold_given || a.delta_e_limit_given) {
            printf("WARNING: --delta_e_threshold and --delta_e_limit need --delta_e 1\n");
            return 1;
        }
        return 0;
    }
    int arg_errors = 0;
    if (!(a.delta_e_threshold >= 0.0f)) { printf("WARNING: delta_e_threshold(%g) is not a number >= 0\n", a.delta_e_threshold); arg_errors++; }
    if (!(a.delta_e_limit >= 0.0)) { printf("WARNING: delta_e_limit(%g) is not a number >= 0\n", a.delta_e_limit); arg_errors++; }
    if (a.hist_only || a.scale_only || a.light_only) {
        printf("WARNING: --delta_e 1 judges a comparison: not with --%s 1\n", a.hist_only ? "histogram_only" : a.scale_only ? "scale_only" : "light_only");
        return arg_errors + 1;
    }
    if (!a.ref) {
        printf("WARNING: --delta_e 1 needs a comparison: --ref_filename R (with or without --dst_filename, or with --compare_only 1)\n");
        return arg_errors + 1;
    }
    if (a.inverse) {
        printf("WARNING: --delta_e 1 judges PQ code frames: the .yuv -> RGB flow's output is compared by --compare_only 1 on the written .rgb\n");
        return arg_errors + 1;
    }
    if (!a.compare_only && a.out_type != CLI_OUT_YUV) return arg_errors; /* refused elsewhere with its own message */
    const bool src = a.compare_only != 0, rgb = src && a.in_type == CLI_IN_RGB;
    const cli_pic &p = src ? a.in : a.out;
    const char *side = src ? "src" : "dst";
    const int m = p.matrix_coeffs, chroma = p.chroma_format_idc, siting = src ? a.src_siting : a.siting;
    if (src && a.src_siting_given) printf("src_chroma_sample_loc_type: %d\n", a.src_siting);
    if (p.bit_depth < 8 || p.bit_depth > 16) { printf("WARNING: --delta_e 1 takes frames of bit_depth 8..16, not %d\n", p.bit_depth); arg_errors++; }
    if (p.video_full_range_flag != 0 && p.video_full_range_flag != 1) {
        printf("WARNING: video_full_range_flag(%d) not 0 or 1\n", p.video_full_range_flag);
        arg_errors++;
    }
    if (p.transfer_characteristics != 16) {
        printf("WARNING: --delta_e 1 judges PQ codes: %s_transfer_characteristics(%d) is not 16\n", side, p.transfer_characteristics);
        arg_errors++;
    }
    if (p.colour_primaries != 8 && p.colour_primaries != 9) {
        printf("WARNING: --delta_e 1 takes BT.2020 primaries: %s_colour_primaries(%d) is not 8 or 9 (other primaries need --gamut_convert's pass "
               "first)\n", side, p.colour_primaries);
        arg_errors++;
    }
    if (m != H2Y_MATRIX_GBR && m != H2Y_MATRIX_BT709 && m != H2Y_MATRIX_BT2020NC && !(src && cli_src_is_ictcp(a, m))) {
        printf("WARNING: --delta_e 1: %s_matrix_coeffs(%d) not %d (G,B,R), %d (BT.709) or %d (BT.2020nc)\n", side, m, H2Y_MATRIX_GBR, H2Y_MATRIX_BT709,
               H2Y_MATRIX_BT2020NC);
        arg_errors++;
    } else if (rgb && m != H2Y_MATRIX_GBR) {
        printf("WARNING: a .rgb holds planes R, G, B: --delta_e of .rgb files takes src_matrix_coeffs %d, not %d\n", H2Y_MATRIX_GBR, m);
        arg_errors++;
    } else if (src && !rgb && a.in_type == CLI_IN_YUV && m == H2Y_MATRIX_GBR) {
        printf("WARNING: --delta_e of .yuv files takes src_matrix_coeffs %d or %d, not %d: G,B,R planes come as .rgb\n", H2Y_MATRIX_BT709,
               H2Y_MATRIX_BT2020NC, m);
        arg_errors++;
    }
    if (chroma == 2) { printf("WARNING: --delta_e 1: chroma_format_idc 2 (4:2:2) is not judged\n"); arg_errors++; }
    else if (chroma != H2Y_CHROMA_420 && chroma != H2Y_CHROMA_444) { /* (--compare_only has said so already) */
        if (!src) { printf("WARNING: chroma_format_idc(%d) not %d or %d\n", chroma, H2Y_CHROMA_420, H2Y_CHROMA_444); arg_errors++; }
    } else if (chroma == H2Y_CHROMA_420 && m == H2Y_MATRIX_GBR) {
        printf("WARNING: --delta_e 1: G,B,R planes (%s_matrix_coeffs %d) are 4:4:4, not chroma_format_idc %d\n", side, H2Y_MATRIX_GBR, chroma);
        arg_errors++;
    } else if (chroma == H2Y_CHROMA_420 && ((p.width | p.height) & 1)) {
        printf("WARNING: --delta_e 1: 4:2:0 needs an even width and height, not %dx%d\n", p.width, p.height);
        arg_errors++;
    }
    if (src) { /* the forward flow's --dst_chroma_sample_loc_type has its own checks (cli_resolve_siting) */
        if (siting == 1) {
            printf("WARNING: src_chroma_sample_loc_type(1) is replication's siting, --chroma_resampler_type 0: not selected by this flag\n");
            arg_errors++;
        } else if (siting != 0 && siting != 2) {
            printf("WARNING: src_chroma_sample_loc_type(%d) not 0 or 2\n", siting);
            arg_errors++;
        } else if (siting == 2 && chroma != H2Y_CHROMA_420) {
            printf("WARNING: --src_chroma_sample_loc_type 2 sites 4:2:0 chroma: src_chroma_format_idc(%d) has none to site\n", chroma);
            arg_errors++;
        } else if (siting == 2 && a.resampler == 0) {
            printf("WARNING: --src_chroma_sample_loc_type 2 needs the FIR resampler: replication (--chroma_resampler_type 0) is centre sited by "
                   "construction\n");
            arg_errors++;
        }
    } else if (a.linearize && a.lin.chroma_format_idc == H2Y_CHROMA_420 && chroma == H2Y_CHROMA_420 && a.src_siting != a.siting) {
        printf("WARNING: --delta_e 1 with --linearize 1: --src_chroma_sample_loc_type (%d) and --dst_chroma_sample_loc_type (%d) must agree, one "
               "inverse chroma siting serves both upsamplers\n", a.src_siting, a.siting);
        arg_errors++;
    }
    if (arg_errors) return arg_errors;
    a.de = h2y_codelight_desc{p.width, p.height, chroma, p.bit_depth, p.video_full_range_flag, m, a.resampler};
    a.de_siting = siting == 2 ? 2 : 0;
    static const char *const kMatrix[15] = {"G,B,R", "BT.709", "", "", "", "", "", "", "", "BT.2020nc", "", "", "", "", "ICtCp"};
    printf("delta_e_from: %s PQ codes, bit_depth %d %s range, matrix_coeffs %d (%s), chroma_format_idc %d, upsampler %s, threshold %g%s\n",
           src ? "source" : "output", p.bit_depth, p.video_full_range_flag ? "full" : "video", m, kMatrix[m], chroma,
           chroma == H2Y_CHROMA_444 ? "none" : !a.resampler ? "replicate" : siting == 2 ? "fir_top_left" : "fir", (double)a.delta_e_threshold,
           a.delta_e_threshold_given ? "" : " (default)");
    if (a.delta_e_limit_given) printf("delta_e_limit: %g\n", a.delta_e_limit);
    return 0;
}

static inline int cli_resolve_convert(cli_args &a)
{
    int arg_errors = 0;
    /* :265-318: unset destination attributes <- the source's, as parsed */
    if (a.out.bit_depth == 0) a.out.bit_depth = a.in.bit_depth;
    if (a.out.width == 0) a.out.width = a.in.width;
    if (a.out.height == 0) a.out.height = a.in.height;
    if (a.out.chroma_format_idc == -1) a.out.chroma_format_idc = a.in.chroma_format_idc;
    if (a.out.video_full_range_flag == -1) a.out.video_full_range_flag = a.in.video_full_range_flag;
    if (a.out.colour_primaries == -1) a.out.colour_primaries = a.in.colour_primaries;
    if (a.out.transfer_characteristics == -1) a.out.transfer_characteristics = a.in.transfer_characteristics;
    if (a.out.matrix_coeffs == -1) a.out.matrix_coeffs = a.in.matrix_coeffs;

    /* :321-372 input type */
    const char *ext = cli_ext_of(a.src);
    if (a.linearize == 1) a.in_type = CLI_IN_F32; /* cli_resolve_linearize: the F32 planes the ring decodes from the file's codes */
    else if (a.synthetic >= 0) a.in_type = CLI_IN_SYNTH;
    else if (!strcasecmp(ext, "yuv")) a.in_type = CLI_IN_YUV;
    else if (!strcasecmp(ext, "rgb")) a.in_type = CLI_IN_RGB;
    else if (!strcasecmp(ext, "f32")) a.in_type = CLI_IN_F32;
    else if (!strcasecmp(ext, "f16")) a.in_type = CLI_IN_F16;
    else if (!strcasecmp(ext, "dpx")) a.in_type = CLI_IN_DPX;
    else if (!strcasecmp(ext, "tiff")) a.in_type = CLI_IN_TIFF; /* not .tif: the reference's input_file_types name .tiff only */
    else if (!strcasecmp(ext, "exr")) a.in_type = CLI_IN_EXR;
    if (a.in_type == CLI_IN_NONE) {
        printf("WARNING: input file (%s) type extension (%s) is either not recongized or not supported\n", a.src ? a.src : "(none)", ext);
        arg_errors++;
    }
    const bool int_in = a.in_type == CLI_IN_YUV || a.in_type == CLI_IN_RGB || a.in_type == CLI_IN_TIFF; /* :336 */
    if (int_in) {
        if (a.in.bit_depth < 10 || a.in.bit_depth > 16)
            printf("WARNING: src bit_depth(%d) outside range [10,16] for integer input file type(%s)\n", a.in.bit_depth, ext);
    } else if (a.in.chroma_format_idc != H2Y_CHROMA_444) {
        printf("file-type is 4:4:4.  Settig chroma_format_idc(%d) to  %d.\n", a.in.chroma_format_idc, H2Y_CHROMA_444);
        a.in.chroma_format_idc = H2Y_CHROMA_444; /* :351-355: after the destination took its copy */
    }

    /* :386-440 output type (without a destination: the reference file's) */
    ext = cli_ext_of(a.dst ? a.dst : a.ref ? a.ref : a.hist || a.light || a.dynmeta ? "(none).yuv" : nullptr); /* only a histogram or the light: the .yuv flow */
    if (!strcasecmp(ext, "yuv")) a.out_type = CLI_OUT_YUV;
    else if (!strcasecmp(ext, "rgb")) a.out_type = CLI_OUT_RGB;
    else if (!strcasecmp(ext, "tiff")) a.out_type = CLI_OUT_TIFF;
    else if (!strcasecmp(ext, "exr") || !strcasecmp(ext, "dpx")) a.out_type = CLI_OUT_CODEC;
    if (a.out_type == CLI_OUT_NONE) {
        printf("WARNING: output file (%s) type extension (%s) is either not recongized or not supported\n", a.dst ? a.dst : "(none)", ext);
        arg_errors++;
    } else if (!a.dst && (a.out_type == CLI_OUT_TIFF || a.out_type == CLI_OUT_CODEC)) { /* the reference names the output type */
        arg_errors += cli_ref_check(a);
    } else if (a.out_type == CLI_OUT_CODEC) {
        printf("WARNING: output file (%s): the .%s writers stay with the reference's host I/O; this program writes .yuv, and\n"
               "         from .yuv input .tiff (or its samples as planar .rgb)\n", a.dst, ext);
        arg_errors++;
    } else if (a.out.bit_depth < 10 || a.out.bit_depth > 16)
        printf("WARNING: dst bit_depth(%d) outside range [10,16] for integer input file type(%s)\n", a.out.bit_depth, ext);
    /* hdr2yuv.cpp:818: a .yuv read for a .tiff goes through matrix_inverse(); planar .rgb holds the same samples */
    a.inverse = a.in_type == CLI_IN_YUV && (a.out_type == CLI_OUT_RGB || a.out_type == CLI_OUT_TIFF);
    if (a.out_type == CLI_OUT_RGB && !a.inverse) {
        printf("WARNING: .rgb output is the .yuv -> RGB flow's (matrix_inverse); the reference writes no .rgb either\n");
        arg_errors++;
    }
    if (a.out_type == CLI_OUT_TIFF && !a.inverse) { /* the reference would hand write_tiff() the converted 4:2:0 / YCbCr planes */
        printf("WARNING: .tiff output is the .yuv -> RGB flow's (matrix_inverse): it takes .yuv input only\n");
        arg_errors++;
    }
    if (a.ref && a.dst && a.out_type != CLI_OUT_NONE && a.out_type != CLI_OUT_CODEC) arg_errors += cli_ref_check(a);
    if (a.sigma < 0) { printf("WARNING: sigma_compare(%d) is negative\n", a.sigma); arg_errors++; }

    const bool numbered = (a.in_type == CLI_IN_DPX || a.in_type == CLI_IN_TIFF || a.in_type == CLI_IN_EXR) && cli_frame_pattern(a.src) == 1;
    if (a.start_frame != 0 && (!int_in || a.in_type == CLI_IN_TIFF) && a.in_type != CLI_IN_F32 && a.in_type != CLI_IN_F16 &&
        a.in_type != CLI_IN_SYNTH && !numbered)
        printf("WARNING: start_frame(%d) only makes sense when file type is .yuv, .rgb, or .y4m\n", a.start_frame);

    /* :472-507: what was resolved */
    printf("src_filename: %s\n", a.src ? a.src : "(synthetic)");
    printf("src_pic_width: %d\nsrc_pic_height: %d\nsrc_chroma_format_idc: %d\nsrc_bit_depth: %d\nsrc_half_float_flag: %d\n",
           a.in.width, a.in.height, a.in.chroma_format_idc, a.in.bit_depth, a.in.half_float_flag);
    printf("src_full_range_video_flag: %d\nsrc_colour_primaries: %d\nsrc_transfer_characteristics: %d\nsrc_matrix_coeffs: %d\n",
           a.in.video_full_range_flag, a.in.colour_primaries, a.in.transfer_characteristics, a.in.matrix_coeffs);
    printf("dst_filename: %s\n", a.dst ? a.dst : "(none)");
    if (a.ref) printf("ref_filename: %s\nsigma_compare: %d%s\n", a.ref, a.sigma, a.sigma_given ? "" : " (default)");
    printf("dst_pic_width: %d\ndst_pic_height: %d\ndst_chroma_format_idc: %d\ndst_bit_depth: %d\ndst_half_float_flag: %d\n",
           a.out.width, a.out.height, a.out.chroma_format_idc, a.out.bit_depth, a.out.half_float_flag);
    printf("dst_video_full_range_flag: %d\ndst_colour_primaries: %d\ndst_transfer_characteristics: %d\ndst_matrix_coeffs: %d\n",
           a.out.video_full_range_flag, a.out.colour_primaries, a.out.transfer_characteristics, a.out.matrix_coeffs);
    printf("verbose_level: %d\nsrc_start_frame: %d\nn_frames: %d\nchroma_resampler_type: %d\n", a.verbose, a.start_frame, a.n_frames, a.resampler);

    /* :519-572 sanity checks */
    if (a.in.width < 2 || a.in.width > 10000) { printf("WARNING: pic_width(%d) outside range [0,10000]\n", a.in.width); arg_errors++; }
    if (a.in.height < 2 || a.in.height > 10000) { printf("WARNING: pic_height(%d) outside range [0,10000]\n", a.in.height); arg_errors++; }
    if (a.in.bit_depth < 8 || a.in.bit_depth > 32) { printf("WARNING: src bit_depth(%d) outside range [8,32]\n", a.in.bit_depth); arg_errors++; }
    if (a.in.chroma_format_idc != H2Y_CHROMA_444 && !(a.inverse && a.in.chroma_format_idc == H2Y_CHROMA_420)) {
        /* (4:2:0 input is taken on the inverse flow only, the yuv2tiff.cpp:341-342 order: upsample, then matrix_inverse) */
        printf("WARNING: chroma_format_idc(%d) not %d, Only 4:4:4 input supported at this moment..\n", a.in.chroma_format_idc, H2Y_CHROMA_444);
        arg_errors++;
    }
    if (a.out.width < 2 || a.out.width > 10000) { printf("WARNING: pic_width(%d) outside range [0,10000]\n", a.out.width); arg_errors++; }
    if (a.out.height < 2 || a.out.height > 10000) { printf("WARNING: pic_height(%d) outside range [0,10000]\n", a.out.height); arg_errors++; }
    if (a.out.bit_depth < 8 || a.out.bit_depth > 32) { printf("WARNING: dst bit_depth(%d) outside range [32]\n", a.out.bit_depth); arg_errors++; }
    if ((a.in_type == CLI_IN_DPX || a.in_type == CLI_IN_TIFF || a.in_type == CLI_IN_EXR) && cli_frame_pattern(a.src) < 0) {
        printf("WARNING: input file name (%s): '%%' other than one integer conversion (%%d, %%0Nd) numbering the frames\n", a.src);
        arg_errors++;
    }
    if (a.out_type == CLI_OUT_TIFF && cli_frame_pattern(a.dst) < 0) {
        printf("WARNING: output file name (%s): '%%' other than one integer conversion (%%d, %%0Nd) numbering the frames\n", a.dst);
        arg_errors++;
    }
    if (arg_errors) return arg_errors;
    if (a.in_type == CLI_IN_DPX && a.in.half_float_flag == 1) { /* dpx.cpp:232-236 */
        printf(" %s half-float reading not supported for dpx files in this version, aborting\n", a.src);
        return 1;
    }

    /* read_file(): what the readers force on the INPUT picture (the destination's copies were taken above) */
    if (a.in_type == CLI_IN_RGB && a.in.matrix_coeffs != H2Y_MATRIX_GBR) {
        printf("WARNING: RGB src matrix_coefs(%d) being overriden to MATRIX_GBR (%d)\n", a.in.matrix_coeffs, H2Y_MATRIX_GBR); /* :677-680 */
        a.in.matrix_coeffs = H2Y_MATRIX_GBR;
    }
    if (a.in_type == CLI_IN_TIFF) { /* read_tiff, tiff.cpp:214-225; the range flag stays the command line's */
        if (a.in.bit_depth != 16) {
            printf("WARNING, read_tiff(): bit_depth(%d) != 16-bit precision assumed for tiff input samples\n", a.in.bit_depth);
            a.in.bit_depth = 16;
        }
        if (a.in.chroma_format_idc != H2Y_CHROMA_444) {
            printf("WARNING, read_tiff(): chroma_format_idc(%d) != CHROMA_444 assumed for tiff input\n", a.in.chroma_format_idc);
            a.in.chroma_format_idc = H2Y_CHROMA_444;
        }
        if (a.in.matrix_coeffs != H2Y_MATRIX_GBR) {
            printf("WARNING, read_tiff(): matrix_coefs(%d) != MATRIX_GBR assumed for tiff input\n", a.in.matrix_coeffs);
            a.in.matrix_coeffs = H2Y_MATRIX_GBR;
        }
    }
    if (!int_in) { /* .dpx :729-734, .exr exr.cpp:172-183 */
        if (a.in.matrix_coeffs != H2Y_MATRIX_GBR) printf("overriding matrix_coeffs(%d) to MATRIX_GBR(%d)\n", a.in.matrix_coeffs, H2Y_MATRIX_GBR);
        a.in.matrix_coeffs = H2Y_MATRIX_GBR;
        a.in.chroma_format_idc = H2Y_CHROMA_444;
        a.in.bit_depth = 32;
        if (a.in_type != CLI_IN_F32 && a.in_type != CLI_IN_DPX) a.in.video_full_range_flag = 1; /* read_exr() only; dpx keeps the flag (:712-713 prints, does not set) */
    }
    if (int_in && (a.in.bit_depth < 10 || a.in.bit_depth > 16)) { /* :592-610 */
        printf("read_planar_integer_file(), WARNING: bit_depth(%d) outside supported range [10,16]\n", a.in.bit_depth);
        return 1;
    }
    return 0;
}

/* the picture pair as the C-ABI takes it */
static inline void cli_make_desc(const cli_args &a, h2y_desc *d)
{
    memset(d, 0, sizeof *d);
    d->width = a.in.width;
    d->height = a.in.height;
    switch (a.in_type) {
    case CLI_IN_F32:
    case CLI_IN_DPX: d->in_sample_type = H2Y_SAMPLE_F32; break;
    case CLI_IN_F16:
    case CLI_IN_EXR: d->in_sample_type = H2Y_SAMPLE_F16; break;
    case CLI_IN_SYNTH: d->in_sample_type = a.in.half_float_flag ? H2Y_SAMPLE_F16 : H2Y_SAMPLE_F32; break;
    default: d->in_sample_type = H2Y_SAMPLE_U16; break;
    }
    d->src_bit_depth = a.in.bit_depth;
    d->dst_bit_depth = a.out.bit_depth;
    d->src_transfer = a.in.transfer_characteristics;
    d->dst_transfer = a.out.transfer_characteristics;
    d->src_matrix = a.in.matrix_coeffs;
    d->dst_matrix = a.out.matrix_coeffs;
    const bool lut_signal = a.lut3d && a.lut3d_signal == 1; /* the LUT leaves the destination's signal, in its primaries */
    d->src_primaries = a.ictcp == 1 || lut_signal ? a.out.colour_primaries : a.in.colour_primaries; /* the passthrough descriptor's are equal: --gamut_convert
                                                                                          * has the source's (h2y_stream_gamut) */
    d->dst_primaries = a.out.colour_primaries;
    d->dst_full_range = a.out.video_full_range_flag;
    d->dst_chroma_format_idc = a.out.chroma_format_idc;
    d->chroma_resampler_type = a.resampler;
    if (a.tone_map || a.linearize == 1 || a.hlg == 1 || a.ictcp == 1 || a.lut3d) { /* (a LUT's planes are referred to its own range;) mapped planes are referred to their target, linearised ones lie in [0, 1] by
                                                         * definition, HLG's are code-valued: floor 0 and ceiling 1, not each frame's
                                                         * pic_stats */
        d->stats_override = 1;
        for (int c = 0; c < 3; c++) d->floor[c] = 0, d->ceiling[c] = 1;
    }
}

#endif /* H2Y_CLI_ARGS_H */
