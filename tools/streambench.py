#!/usr/bin/env python3
"""tools/streambench.py -- end-to-end frames/s from HOST memory, GPU box.
One 4K C2 frame = 99.5 MB up, 24.9 MB down: PCIe-bound.  Compares the synchronous entry
(h2y_convert_frame: upload, convert, download one after the other, pageable numpy buffers) with the
pinned ring of h2y_stream_* (the three overlapped).

`streambench.py inverse`: the .yuv -> G,B,R flow on 4K frames instead.
  1. kernel us per frame (HIP events, h2y_last_kernel_ms) and wall time per frame (host clock, every call synchronous) of
     h2y_inverse_batch at 64 frames per call, next to the single-frame entries (h2y_inverse_420 / h2y_matrix_inverse) called
     64 times, in the same process: 4:2:0 FIR, 4:2:0 replication, 4:4:4;
  2. the top-left sited form beside the FIR form (h2y_ctx_set_inverse_chroma_siting 2 and 0): k_inverse420_batch<FIR_TL> and
     k_inverse420_batch<FIR> on the same 64 frames, five calls each, taken in turn: the median kernel us per frame and the
     lowest and highest call of each;
  3. frames/s from host memory, 4:2:0 FIR: h2y_inverse_frame (pageable, serial) against the inverse stream (depth 3).
Prints one line per figure, then one JSON line with all of them.

`streambench.py dpx`: DPX input on 4K pictures, for each of 10-bit, 16-bit and float DPX:
  1. ms/frame and frames/s from host memory of the DPX ring (h2y_dpx_stream_open: the payload goes up, k_dpx_decode, the
     forward conversion) against the .f32 ring (h2y_stream_open) on the same decoded pictures, both at depth 3, each frame
     copied into its pinned slot by the host (a memcpy standing in for the file read);
  2. the kernel time of h2y_dpx_decode_batch over 64 frames (HIP events, median of reps), the bytes it moves -- the payload
     plus 12 B/pixel of float planes -- over that time, and their share of the 8 TB/s HBM peak.
Prints one line per figure, then one JSON line with all of them.

`streambench.py tiff`: 16-bit RGB TIFF on 4K pictures:
  1. ms/frame and frames/s from host memory of the TIFF ring (h2y_tiff_stream_open: the rows go up, k_tiff_decode, the forward
     conversion) against the .rgb ring (h2y_stream_open, U16 planes) on the same samples, both at depth 3: the same PCIe bytes;
  2. the TIFF inverse ring (h2y_tiff_inverse_stream_open: the inverse kernel, then k_rgb_interleave) against the inverse ring;
  3. the kernel time of h2y_tiff_decode_batch and h2y_rgb_interleave_batch over 64 frames (HIP events, median of reps), and the
     12 B/pixel each moves over that time as a share of the 8 TB/s HBM peak.
Prints one line per figure, then one JSON line with all of them.

`streambench.py exr`: scanline OpenEXR on 4K half R,G,B pictures, NONE and ZIP:
  1. ms/frame and frames/s from host memory of the EXR ring (h2y_exr_stream_open: the unpacked payload goes up, k_exr_decode,
     the forward conversion), each frame unpacked into its pinned slot by UNPACK_THREADS (16) host threads, against the .f16
     ring (h2y_stream_open) on the same half planes, both at depth 3;
  2. the kernel time of h2y_exr_decode_batch over 64 frames (HIP events, median of reps), raw (NONE) and encoded (ZIP) chunks,
     and the algorithmic bytes over that time as a share of the 8 TB/s HBM peak: 6 B/pixel read and 6 written raw, 9 read
     (the first half of each chunk twice) and 6 written encoded;
  3. host unpack ms per frame (h2y_exr_unpack, the file already in memory) with that many threads.
Prints one line per figure, then one JSON line with all of them.

`streambench.py compare`: the comparison with a reference on 4K 4:2:0 10-bit frames:
  1. the kernel time of h2y_compare_batch (k_compare and k_compare_sum) over 64 frame pairs (HIP events, median of reps), the
     49.8 MB per frame it reads over that time, and their share of the 8 TB/s HBM peak;
  2. frames/s from host memory of the forward ring (16-bit G,B,R planes in, BT.2020nc 10-bit 4:2:0 box out, depth 3) unarmed,
     armed with keep_output 1 (the reference goes up, the frame comes down) and armed with keep_output 0 (only the stats come
     down), on the same pictures;
  3. frames/s of the compare-only ring (both frames go up, the stats come down).
Prints one line per figure, then one JSON line with all of them.

`streambench.py histogram`: code-value histograms on 4K frames:
  1. the kernel time of h2y_histogram_batch (the zeroing, k_histogram and k_histogram_finish) over 64 distinct frames per call
     (HIP events, median of five), the bytes per frame it reads over that time and their share of the 8 TB/s HBM peak, for
     10-bit 4:2:0 (24.9 MB) and 16-bit 4:4:4 (49.8 MB) frames at full resolution, on uniform random, constant and
     one-code-per-row content;
  2. frames/s from host memory of the forward ring (as `compare`) unarmed and armed with h2y_stream_histogram;
  3. frames/s of the histogram-only ring on the 10-bit 4:2:0 frames (the frame goes up, the counts come down).
Prints one line per figure, then one JSON line with all of them.

`streambench.py ssim`: SSIM beside the comparison on 4K frames:
  1. the kernel time of h2y_ssim_batch (k_ssim and k_ssim_sum) over 64 distinct frame pairs per call (HIP events, median of
     five), the bytes per pair it reads over that time and their share of the 8 TB/s HBM peak, for 10-bit 4:2:0 (49.8 MB) and
     16-bit 4:4:4 (99.5 MB) pairs;
  2. frames/s from host memory of the forward ring (as `compare`) armed with h2y_stream_compare alone and with h2y_stream_ssim
     too, keep_output 1;
  3. frames/s of the compare-only ring on the 10-bit 4:2:0 frames, without and with SSIM.
Prints one line per figure, then one JSON line with all of them.

`streambench.py regions`: flat and busy areas, over- and undershoot beside the comparison on 4K frames:
  1. the kernel times of h2y_regions_batch (k_regions and k_regions_sum), h2y_compare_batch and h2y_ssim_batch over the same 64
     distinct frame pairs per call, five calls each taken in turn after a warm-up (HIP events, the median per frame, the smallest and
     largest beside it), the bytes per pair each reads once over that time and their share of the 8 TB/s HBM peak: 10-bit 4:2:0
     pairs (49.8 MB) at radius 1 and 4, 16-bit 4:4:4 pairs (99.5 MB) at radius 1; and k_regions' time over k_ssim's;
  2. frames/s of the compare-only ring on the 10-bit 4:2:0 frames from host memory, unarmed and armed with h2y_stream_regions.
Prints one line per figure, then one JSON line with all of them.

`streambench.py light`: the content light level on 4K frames:
  1. the kernel time of h2y_light_batch (k_light) over 64 distinct frames per call (HIP events, median of five; floor and
     ceiling given, so no k_stats runs), the bytes per frame it reads over that time and their share of the 8 TB/s HBM peak, for
     F32 (99.5 MB), F16 and U16 (49.8 MB) LINEAR sources and an F32 BT.1886 source (the transfer's table tier);
  2. frames/s from host memory of every forward ring -- .f32, float DPX, 16-bit TIFF, half EXR (NONE) -- to PQ BT.2020nc 10-bit
     4:2:0, unarmed and armed with h2y_stream_light.
Prints one line per figure, then one JSON line with all of them.

`streambench.py lightdist`: the light distribution (HDR10+ dynamic metadata) on 4K frames, in one job:
  1. h2y_lightdist_batch (k_lightdist) beside h2y_light_batch (k_light, the yardstick: it reads the same bytes) over the same 64
     distinct device frames per call, five calls each taken in turn after a warm-up (HIP events round the launch; floor and ceiling
     given, so no k_stats runs; the one memset that zeroes a call's accumulators -- 2.2 MB of bins for k_lightdist, 1 KB for k_light
     -- lies before the first event): the median and spread in us per frame, the ratio to k_light, and the bytes per frame over
     that time as a share of the 8 TB/s HBM peak, for F32, F16 and U16 LINEAR sources and an F32 BT.1886 source, on noise;
  2. the same on a constant and on a letterboxed F32 picture (the flat-run path: whole waves in one bin);
  3. frames/s from host memory of the .f32 ring to PQ BT.2020nc 10-bit 4:2:0, unarmed and armed with h2y_stream_lightdist.
Prints one line per figure, then one JSON line with all of them.

`streambench.py scenes`: the scene signature (k_scenesig, k_codescenesig) on 4K frames, in one job:
  1. h2y_scenesig_batch beside h2y_lightdist_batch (k_lightdist) and h2y_light_batch (k_light, the yardstick: the same bytes and the
     same transfer arithmetic) over the same 64 distinct device frames per call, five calls each taken in turn after a warm-up (HIP
     events round the launch; floor and ceiling given, so no k_stats runs; the memset that zeroes a call's accumulators lies before
     the first event): the median and spread in us per frame, the ratios to k_light and k_lightdist, and the bytes per frame over
     that time as a share of the 8 TB/s HBM peak at 12 (F32) and 6 (F16, U16) B/pixel, on noise, and for F32 on a constant and on a
     letterboxed picture;
  2. h2y_codescenesig_batch beside h2y_codelight_batch with DIST on 10-bit 4:2:0 BT.2020nc noise, timed the same way (launches of
     up to 8 frames, k_up444 included in both; 11 B/pixel as `codelight` counts them);
  3. frames/s from host memory of the .f32 ring to PQ BT.2020nc 10-bit 4:2:0, armed with h2y_stream_lightdist alone and with
     h2y_stream_scenesig as well (the bins taken with every output), three runs of each in turn after a warm-up.
Prints one line per figure, then one JSON line with all of them.

`streambench.py deltae`: Delta E ITP of PQ code planes (k_deltae) on 4K frames, in one job:
  1. h2y_deltae_batch over 64 distinct device frame pairs per call, 10-bit 4:2:0 and 4:4:4, beside h2y_codelight_batch (on A),
     h2y_compare_batch and h2y_ssim_batch on the same pairs, five calls each taken in turn after a warm-up, the median per frame; the
     k_up444 share of the 4:2:0 time from the 4:4:4 figure.
  2. the compare-only ring from host memory, unarmed and armed with h2y_stream_deltae, three runs of each in turn.

`streambench.py codelight`: the light of PQ code planes (k_codelight) on 4K frames, in one job:
  1. h2y_codelight_batch over 64 distinct device frames per call, DIST off and on, five calls each taken in turn after a warm-up (HIP
     events round each launch of up to 8 frames, k_up444 included; the memset of the accumulators lies before the first event): the
     median and spread in us per frame for 10-bit 4:2:0 BT.2020nc frames (noise, constant, letterboxed), the same noise as 10-bit
     4:4:4 (no upsampling: the k_up444 share of the 4:2:0 time is what is left), and 16-bit 4:4:4 noise; the algorithmic bytes per
     frame -- 4:2:0: 3 B/pixel read by k_up444 and k_codelight, 4 B/pixel of scratch written and 4 read back, 11 in all; 4:4:4:
     6 B/pixel -- over that time as a share of the 8 TB/s HBM peak;
  2. the yardsticks, in the same job, on the 16-bit 4:4:4 frames' planes read as a U16 LINEAR source: h2y_light_batch (k_light) and
     h2y_lightdist_batch (k_lightdist), timed the same way: the same 6 B/pixel, no matrix and no transfer;
  3. frames/s of the light-only ring from host memory, 10-bit 4:2:0, without and with want_dist.
Prints one line per figure, then one JSON line with all of them.

`streambench.py gamutcheck`: the gamut containment check of PQ code planes (k_gamutcheck) on 4K frames, in one job:
  1. h2y_gamutcheck_batch of a BT.2020 file against one set (P3-D65) and against two (P3-D65, BT.709), and h2y_codelight_batch without
     the distribution on the same 64 distinct device frames, five calls of each taken in turn after a warm-up (HIP events round each
     launch of up to 8 frames, k_up444 included): the median and spread in us per frame for 10-bit 4:2:0 and 4:4:4 BT.2020nc noise and
     16-bit G,B,R noise, the bytes per frame as `codelight` counts them, the ratios to k_codelight, and the k_up444 share of the
     4:2:0 time from the 4:4:4 figure;
  2. frames/s of the light-only ring from host memory, 10-bit 4:2:0, unarmed and armed with h2y_stream_gamutcheck (two sets), three
     runs of each in turn.
Prints one line per figure, then one JSON line with all of them.

`streambench.py scale`: the Lanczos resampler:
  1. the kernel time of h2y_scale_batch (k_scale) over 64 distinct device frames per call (HIP events, median of five after a
     warm-up call), the bytes per frame -- the source read once plus the output written -- over that time and their share of the
     8 TB/s HBM peak, for 4K -> 1080p, 4K -> 720p and 1080p -> 4K (10-bit 4:2:0, 3 lobes) and 4K -> 1080p 16-bit 4:4:4 with 4 lobes;
  2. frames/s from host memory of the forward ring (as `compare`) unarmed and armed with h2y_stream_scale to 1080p;
  3. frames/s of the scale-only ring, 4K 10-bit 4:2:0 -> 1080p (the frame goes up, the scaled frame comes down).
Prints one line per figure, then one JSON line with all of them.

`streambench.py gamut`: the conversion between colour primaries on 4K frames:
  1. the kernel time of h2y_gamut_batch (k_gamut, BT.709 -> BT.2020, clip on) over 64 distinct device frames per call (HIP events,
     median of five after a warm-up call), F32 and F16, out of place and in place, the algorithmic bytes per frame -- every plane
     read once and written once: 24 and 12 B/pixel -- over that time and their share of the 8 TB/s HBM peak;
  2. the yardstick, in the same job: h2y_tiff_decode_batch (12 B/pixel) and h2y_dpx_decode_batch (10-bit: 16 B/pixel, float:
     24 B/pixel) timed the same way -- streaming kernels of the same shape that this change does not touch;
  3. frames/s from host memory of the .f32 ring and the half EXR ring (NONE) to PQ BT.2020nc 10-bit 4:2:0, unarmed and armed with
     h2y_stream_gamut.
Prints one line per figure, then one JSON line with all of them.

`streambench.py gamut_compress`: gamut compression on 4K frames, beside k_gamut and k_tonemap in the same job: the kernel time of
h2y_gamut_compress_batch (k_gamut_compress, BT.2020 -> BT.709, the default threshold and power), of h2y_gamut_batch (clip on) and of
h2y_tonemap_batch (1000 -> 100 cd/m2, relative) over the same 64 distinct device frames per call (HIP events, median of five after a
warm-up call), F32 and F16, out of place and in place (the frames put back before every in-place call), on uniformly random BT.2020
pixels and on a smooth, mostly in-gamut picture; each picture's share of pixels with a channel past the threshold; the algorithmic
bytes per frame over the time, their share of the 8 TB/s HBM peak, and k_gamut_compress' time over k_gamut's and k_tonemap's.
Prints one line per figure, then one JSON line with all of them.

`streambench.py tonemap`: the tone curve on 4K frames, beside k_gamut in the same job:
  1. the kernel time of h2y_tonemap_batch (k_tonemap, 1000 -> 100 cd/m2, relative) and of h2y_gamut_batch (k_gamut, BT.2020 ->
     BT.709, clip on) on the same 64 distinct device frames per call (HIP events, median of five after a warm-up call), F32 and
     F16, out of place and in place, the algorithmic bytes per frame -- every plane read once and written once: 24 and 12 B/pixel
     -- over that time and their share of the 8 TB/s HBM peak.  The frames hold light up to 5000 cd/m2, most of it dark;
  2. frames/s from host memory of the .f32 ring to BT.709 10-bit 4:2:0 with the 0 / 1 statistics override, unarmed and armed with
     h2y_stream_tonemap, three times in turn.
Prints one line per figure, then one JSON line with all of them.

`streambench.py hlg`: the HLG pass on 4K frames, beside k_tonemap and k_gamut in the same job:
  1. the kernel time of h2y_hlg_batch (k_hlg, 1000 cd/m2, display-referred planes, 10-bit video-range BT.2020nc scale) on 64 distinct
     device frames per call (HIP events, median of five after a warm-up call): F32 out of place, F32 in place (the light is put back
     before every call: what the pass leaves is codes, not light) and F16 -> F32; beside them h2y_tonemap_batch (1000 -> 100 cd/m2)
     and h2y_gamut_batch (BT.2020 -> BT.709) on the same F32 frames, out of place and in place; the algorithmic bytes per frame --
     24 B/pixel for F32, 18 for F16 -> F32 -- over that time, their share of the 8 TB/s HBM peak, and k_hlg's time over
     k_tonemap's.  The frames hold light up to the peak, most of it dark;
  2. frames/s from host memory of the .f32 ring with equal transfers (the passthrough flow) to BT.2020nc 10-bit 4:2:0 with the 0 / 1
     statistics override, unarmed and armed with h2y_stream_hlg, three times in turn.
Prints one line per figure, then one JSON line with all of them.

`streambench.py ictcp`: the ICtCp pass on 4K frames, beside k_hlg and k_gamut in the same job:
  1. the kernel time of h2y_ictcp_batch (k_ictcp, 10-bit video-range scale) on 64 distinct device frames per call (HIP events, median
     of five after a warm-up call): F32 out of place, F32 in place (the light is put back before every call) and F16 -> F32; beside
     them h2y_hlg_batch (1000 cd/m2, absolute) and h2y_gamut_batch (BT.2020 -> BT.709) on the same F32 frames, out of place and in
     place; the algorithmic bytes per frame -- 24 B/pixel for F32, 18 for F16 -> F32 -- over that time, their share of the 8 TB/s HBM
     peak, and k_ictcp's time over k_hlg's and k_gamut's;
  2. the way back: h2y_linearize_batch and h2y_codelight_batch (DIST) with matrix_coeffs 14 beside matrix_coeffs 9 on the same 64
     10-bit 4:2:0 code frames (k_up444 included), taken in turn five times after a warm-up, and the ratios;
  3. frames/s from host memory of the .f32 ring on the passthrough descriptor (equal transfers, matrix 0 -> 0) to 10-bit 4:2:0 with the
     0 / 1 statistics override, unarmed and armed with h2y_stream_ictcp, three times in turn.
Prints one line per figure, then one JSON line with all of them.

`streambench.py siting`: top-left co-sited 4:2:0 chroma (chroma siting 2) on 4K frames, in one job:
  1. k_fir420 and k_fir420_tl through h2y_subsample_420_sited (loc 0 / loc 2) over the 128 distinct chroma planes of 64 frames, one
     launch per plane (HIP events; the two planes of a frame added up), five passes: median and spread in us per frame, and the
     5 B/pixel a frame's second pass moves (two 4:4:4 planes read, two 4:2:0 planes written) over that time as a share of the
     8 TB/s HBM peak.  k_fir420 is the yardstick;
  2. h2y_convert_batch of 64 C2 frames (fp32 -> PQ -> 12-bit BT.2020nc 4:2:0) with "fir" "twopass", siting 0 against siting 2:
     wall time of a call (two kernels on two streams: there is no single kernel time), median and spread of five calls after a
     warm-up, us per frame, and the two-pass form's 23 B/pixel over that time as a share of the peak;
  3. the two sitings alternating, five calls each (ABAB...: drift of the card shows in both alike), the same figures; and the
     default one-pass form (k_fir_fused, siting 0, "fir" "auto") in the same job: what a user gives up by choosing siting 2.
Prints one line per figure, then one JSON line with all of them.

`streambench.py linearize`: the linearisation of PQ code planes (k_linearize) on 4K frames, beside its yardsticks in the same job:
  1. h2y_linearize_batch over 64 distinct device frames per call (HIP events round each launch of up to 8 frames, k_up444 included),
     h2y_codelight_batch (LIGHT) on the same frames and h2y_gamut_batch (k_gamut, F32, in place, BT.2020 -> BT.709, clip on) on the
     planes just written, the three taken in turn five times after a warm-up: median and spread in us per frame for 10-bit 4:2:0
     BT.2020nc FIR noise, the same as 10-bit 4:4:4, and 16-bit 4:4:4 matrix 0; the algorithmic bytes per frame -- the 18 B/pixel
     of k_linearize itself (6 read, 12 written), and for 4:2:0 k_up444's 3 read, 4 written and 4 read back less the 4 of chroma
     k_linearize no longer reads from the frame: 23 -- over that time as a share of the 8 TB/s HBM peak.  The yardstick printed
     beside each: with no overlap at all the kernel would cost k_codelight's time plus a plain 18 B/pixel streaming pass at
     k_gamut's rate (18 / 24 of k_gamut's time);
  2. frames/s from host memory to PQ BT.2020nc 10-bit 4:2:0 of the PQ code ring (h2y_pqcode_stream_open, 10-bit 4:2:0 frames of
     24.9 MB) beside the .f32 ring fed the linearised planes (99.5 MB a frame), both with the 0 / 1 override, three times in turn.
Prints one line per figure, then one JSON line with all of them.

`streambench.py hlgsrc`: the light of HLG code planes (k_hlg_linearize) on 4K frames, beside its yardsticks in the same job:
  1. h2y_hlg_linearize_batch (1000 cd/m2) and h2y_linearize_batch over the same 64 distinct device frames per call (HIP events round
     each launch of up to 8 frames, k_up444 included) and h2y_hlg_batch (k_hlg, F32, absolute, in place) on the planes just written,
     the three taken in turn five times after a warm-up: median and spread in us per frame for 10-bit 4:2:0 BT.2020nc FIR noise, the
     same as 10-bit 4:4:4, and 16-bit 4:4:4 matrix 0; the algorithmic bytes per frame as `linearize` counts them (18 B/pixel, 23 for
     4:2:0) over that time as a share of the 8 TB/s HBM peak; and k_hlg_linearize's time over k_linearize's;
  2. frames/s from host memory to PQ BT.2020nc 10-bit 4:2:0 of the HLG code ring (h2y_hlgcode_stream_open) beside the PQ code ring
     (h2y_pqcode_stream_open) on the same 10-bit 4:2:0 frames of 24.9 MB, both with the 0 / 1 override, five times in turn.
Prints one line per figure, then one JSON line with all of them.

`streambench.py sdrsrc`: the light of SDR code planes (k_sdr_linearize) on 4K frames, beside its yardsticks in the same job:
  1. h2y_sdr_linearize_batch (203 cd/m2), h2y_linearize_batch and h2y_hlg_linearize_batch (1000 cd/m2) over the same 64 distinct device
     frames per call (HIP events round each launch of up to 8 frames, k_up444 included), the three taken in turn five times after a
     warm-up: median and spread in us per frame for 10-bit 4:2:0 BT.709 FIR noise, the same as 10-bit 4:4:4, and 16-bit 4:4:4 matrix 0;
     the algorithmic bytes per frame as `linearize` counts them (18 B/pixel, 23 for 4:2:0) over that time as a share of the 8 TB/s HBM
     peak; and k_sdr_linearize's time over k_linearize's;
  2. frames/s from host memory to PQ BT.2020nc 10-bit 4:2:0 of the SDR code ring (h2y_sdrcode_stream_open) beside the PQ code ring
     (h2y_pqcode_stream_open) on the same 10-bit 4:2:0 frames of 24.9 MB, both with the 0 / 1 override, five times in turn.
Prints one line per figure, then one JSON line with all of them.

`streambench.py sigsrc`: the signal of code planes (k_code_signal) on 4K frames, beside its yardsticks in the same job:
  1. h2y_code_signal_batch over 64 distinct device frames per call (HIP events round each launch of up to 8 frames, k_up444 included)
     for 10-bit 4:2:0 BT.2020nc FIR noise, the same as 10-bit 4:4:4, and 16-bit 4:4:4 matrix 0; h2y_linearize_batch on the 10-bit
     4:4:4 frames; h2y_tiff_decode_batch (k_tiff_decode, 6 B in and 6 B out per pixel) on 64 payloads; h2y_lut3d_batch (k_lut3d, F32,
     tetrahedral, signal mode, a 17-node table, in place) on the planes just written; each taken in turn five times after a warm-up:
     median and spread in us per frame, the algorithmic bytes per frame over that time as a share of the 8 TB/s HBM peak, and
     k_code_signal's 4:4:4 time over k_tiff_decode's;
  2. frames/s from host memory to BT.2020nc 10-bit 4:2:0 of the signal code ring (h2y_sigcode_stream_open) beside the PQ code ring
     (h2y_pqcode_stream_open) armed with the same table in signal mode, on the same 10-bit 4:2:0 frames of 24.9 MB, five times in turn.
Prints one line per figure, then one JSON line with all of them.

`streambench.py dither`: the reduction to the output bit depth (k_dither) on 4K frames, beside its yardsticks in the same job:
  1. the kernel time of h2y_dither_batch over 64 distinct device frames per call (HIP events, median of five after a warm-up call,
     out of place): 16 -> 10 4:2:0 ordered, 16 -> 10 4:2:0 noise, 16 -> 8 4:2:0 ordered and 16 -> 10 4:4:4 ordered; the 4 bytes a
     sample it moves over that time and their share of the 8 TB/s HBM peak;
  2. the yardsticks, timed the same way: h2y_compare_batch (k_compare, two 4:2:0 frames read: the same 4 bytes a sample) and
     h2y_tiff_decode_batch (k_tiff_decode, 12 B/pixel) -- plain u16 streaming passes that this change does not touch;
  3. h2y_convert_batch of 64 device-resident C2 frames (fp32 -> PQ -> BT.2020nc 4:2:0, FIR) at 10 bits against the same at 16 bits
     followed by h2y_dither_batch to 10 in place: wall time of the calls, five of each taken in turn after a warm-up, and the
     kernel variant each conversion ran;
  4. frames/s from host memory of the .f32 ring (16-bit destination), unarmed and armed with h2y_stream_dither to 10 bits, and the
     unarmed ring with a 10-bit destination, three runs of each in turn.
Prints one line per figure, then one JSON line with all of them.

`streambench.py pack`: the sample packings (k_pack, k_unpack) on 4K frames, beside their yardsticks in the same job:
  1. the kernel time of h2y_pack_batch and h2y_unpack_batch over 64 distinct device frames per call (HIP events, median of five after
     a warm-up call) per packing: PLANAR8, NV12 and P010 (10 bits) in 4:2:0, PLANAR8 also in 4:4:4; the 3 bytes a sample (P010: 4) they
     move over that time and their share of the 8 TB/s HBM peak; and NV12 and P010 at 3838 x 2158, where w h is no multiple of 16 and the
     chroma block takes the kernels' narrow path (one element an access);
  2. the yardsticks, timed the same way: h2y_dither_batch 16 -> 8 4:2:0 ordered (k_dither, 4 bytes a sample) and
     h2y_tiff_decode_batch (k_tiff_decode, 12 B/pixel) -- same-shaped streaming passes that this change does not touch;
  3. frames/s from host memory of the .f32 ring (16-bit destination) armed with h2y_stream_dither to 8 bits, without and with
     h2y_stream_pack(PLANAR8) behind it, three runs of each in turn;
  4. frames/s of the compare-only ring on 8-bit 4:2:0 frames, fed planar16 frames and, armed with h2y_stream_unpack(PLANAR8), the same
     frames as bytes, three runs of each in turn.
Prints one line per figure, then one JSON line with all of them."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import hdr2yuv_amd as h
from hdr2yuv_amd.synth import synth_frame


def inverse_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 7
    n = w * hh
    rng = np.random.default_rng(4096)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "stat": "median over reps"}
    for name, chroma, alg in (("420_fir", 1, 1), ("420_replicate", 1, 0), ("444", 3, 0)):
        nc = n // 4 if chroma == 1 else n
        srcs = [[torch.from_numpy(rng.integers(0, 4096, m).astype(np.uint16).view(np.int16)).cuda() for m in (n, nc, nc)] for _ in range(8)]
        frames_in = [srcs[k % 8] for k in range(nb)]  # eight distinct inputs, 64 distinct outputs
        frames_out = [[torch.empty(n, dtype=torch.int16, device="cuda") for _ in range(3)] for _ in range(nb)]
        torch.cuda.synchronize()
        single_k, single_w, batch_k, batch_w = [], [], [], []
        for rep in range(reps + 1):  # rep 0 warms up
            ks = 0.0
            t0 = time.perf_counter()
            for f in range(nb):
                if chroma == 1:
                    ctx.inverse_420(w, hh, 12, 0, 1, 16, alg, frames_in[f], frames_out[f])
                else:
                    ctx.matrix_inverse(w, hh, 12, 0, 1, 16, frames_in[f], frames_out[f])
                ks += ctx.last_kernel_ms()[0]
            tw = time.perf_counter() - t0
            t0 = time.perf_counter()
            ctx.inverse_batch(w, hh, chroma, 12, 0, 1, 16, alg, frames_in, frames_out)
            bw = time.perf_counter() - t0
            if rep:
                single_k.append(ks / nb * 1e3)
                single_w.append(tw / nb * 1e6)
                batch_k.append(ctx.last_kernel_ms()[0] / nb * 1e3)
                batch_w.append(bw / nb * 1e6)
        r = {k: round(float(np.median(v)), 1) for k, v in (("single_kernel_us", single_k), ("single_wall_us", single_w),
                                                            ("batch_kernel_us", batch_k), ("batch_wall_us", batch_w))}
        res[name] = r
        print(f"{name:14s} us/frame  single: kernel {r['single_kernel_us']:7.1f} wall {r['single_wall_us']:7.1f}   "
              f"batch of {nb}: kernel {r['batch_kernel_us']:7.1f} wall {r['batch_wall_us']:7.1f}", flush=True)
        if name == "420_fir":  # the sited form beside it, on the same buffers: one warm-up call each, then five each in turn
            calls = {0: [], 2: []}
            variant = {}
            for rep in range(6):
                for loc in (0, 2):
                    ctx.set_inverse_chroma_siting(loc)
                    ctx.inverse_batch(w, hh, 1, 12, 0, 1, 16, 1, frames_in, frames_out)
                    variant[loc] = ctx.last_kernel_variant()
                    if rep:
                        calls[loc].append(ctx.last_kernel_ms()[0] / nb * 1e3)
            ctx.set_inverse_chroma_siting(0)
            for loc, key in ((0, "sited_0"), (2, "sited_2")):
                v = calls[loc]
                res[key] = {"variant": variant[loc], "calls": len(v), "median_us": round(float(np.median(v)), 1),
                            "min_us": round(min(v), 1), "max_us": round(max(v), 1)}
                print(f"{variant[loc]:28s} us/frame over {len(v)} calls of {nb}: median {np.median(v):7.1f}  min {min(v):7.1f}  max {max(v):7.1f}",
                      flush=True)
        del srcs, frames_in, frames_out
        torch.cuda.empty_cache()

    # host memory, 4:2:0 FIR, BT.709 12 -> 16 bits
    nf = int(os.environ.get("N", "120"))
    depth = int(os.environ.get("DEPTH", "3"))
    planes = [rng.integers(0, 4096, m).astype(np.uint16) for m in (n, n // 4, n // 4)]
    ctx.inverse_frame(w, hh, 1, 12, 0, 1, 16, 1, planes)
    t0 = time.perf_counter()
    for _ in range(nf // 4):
        ctx.inverse_frame(w, hh, 1, 12, 0, 1, 16, 1, planes)
    dt = (time.perf_counter() - t0) / (nf // 4)
    res["host_inverse_frame_ms"] = round(dt * 1e3, 2)
    print(f"h2y_inverse_frame (pageable host buffers, serial): {dt*1e3:7.2f} ms/frame  {1/dt:7.1f} frames/s", flush=True)
    ctx.inverse_stream_open(w, hh, 1, 12, 0, 1, 16, 1, depth)
    inflight = 0
    t0 = time.perf_counter()
    for _ in range(nf):
        dst = ctx.stream_input()
        for c in range(3):
            dst[c][:] = planes[c]  # a memcpy standing in for the file read
        ctx.stream_submit()
        inflight += 1
        if inflight == depth - 1:
            ctx.stream_output()
            inflight -= 1
    while inflight:
        ctx.stream_output()
        inflight -= 1
    dt = (time.perf_counter() - t0) / nf
    ctx.stream_close()
    gb = (n * 3 + n * 6) / 1e9  # 1.5 samples up, 3 down, 2 bytes each
    res["host_inverse_stream_ms"] = round(dt * 1e3, 2)
    res["host_inverse_stream_depth"] = depth
    print(f"inverse stream depth {depth} + host copy into the slot:   {dt*1e3:7.2f} ms/frame  {1/dt:7.1f} frames/s  ({gb/dt:5.1f} GB/s over PCIe)", flush=True)
    ctx.close()
    print(json.dumps({"streambench_inverse": res}), flush=True)


def dpx_main():
    import json

    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from dpx_files import pack_pixels, read_dpx, write_dpx

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(10)
    ctx = h.Context(0)
    d = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth,
           "desc": "F32 GBR linear -> PQ BT.2020nc 10-bit 4:2:0 box", "hbm_peak_tbs": 8.0}
    for bits in (10, 16, 32):
        if bits == 32:
            rgb = [rng.random(n, dtype=np.float32).view(np.uint32) for _ in range(3)]
        else:
            rgb = [rng.integers(0, 1 << bits if bits == 16 else 1024, n, dtype=np.uint64) for _ in range(3)]
        data = write_dpx(w, hh, bits, pack_pixels(*rgb, bits), big_endian=True)
        info = h.parse_dpx(data[:2048], len(data))
        payload = np.frombuffer(data, np.uint8, count=info.payload_bytes, offset=info.data_offset)
        planes = read_dpx(data)[1]
        r = {"payload_mb": round(info.payload_bytes / 1e6, 1)}

        # 1. host memory: the DPX ring against the .f32 ring on the same pictures
        def ring(open_fn, fill):
            open_fn()
            inflight = 0
            t0 = time.perf_counter()
            for _ in range(nf):
                fill(ctx.stream_input())
                ctx.stream_submit()
                inflight += 1
                if inflight == depth - 1:
                    ctx.stream_output()
                    inflight -= 1
            while inflight:
                ctx.stream_output()
                inflight -= 1
            dt = (time.perf_counter() - t0) / nf
            ctx.stream_close()
            return dt

        def fill_dpx(slot):
            slot[0][:] = payload

        def fill_f32(slot):
            for c in range(3):
                slot[c][:] = planes[c]

        ring(lambda: ctx.dpx_stream_open(d, info, depth), fill_dpx)  # warm-up
        t_dpx = ring(lambda: ctx.dpx_stream_open(d, info, depth), fill_dpx)
        ring(lambda: ctx.stream_open(d, depth), fill_f32)
        t_f32 = ring(lambda: ctx.stream_open(d, depth), fill_f32)
        r.update(dpx_ring_ms=round(t_dpx * 1e3, 2), dpx_ring_fps=round(1 / t_dpx, 1), f32_ring_ms=round(t_f32 * 1e3, 2),
                 f32_ring_fps=round(1 / t_f32, 1), ring_speedup=round(t_f32 / t_dpx, 2))
        print(f"{bits:2d}-bit DPX  ring from host memory: dpx {t_dpx*1e3:6.2f} ms/frame {1/t_dpx:6.1f} frames/s   "
              f".f32 {t_f32*1e3:6.2f} ms/frame {1/t_f32:6.1f} frames/s   ({t_f32/t_dpx:4.2f}x)", flush=True)

        # 2. the decode kernel over 64 frames on the device: 64 distinct payloads and 64 distinct sets of planes
        pays = [torch.randint(-(1 << 31), (1 << 31) - 1, (info.payload_bytes // 4,), dtype=torch.int32, device="cuda") for _ in range(nb)]
        outs = [[torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in range(nb)]
        torch.cuda.synchronize()
        ks = []
        for rep in range(reps + 1):  # rep 0 warms up
            ctx.dpx_decode_batch(info, pays, outs)
            if rep:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        moved = info.payload_bytes + 12 * n
        tbs = moved / (k_ms * 1e-3) / 1e12
        r.update(kernel_us_per_frame=round(k_ms * 1e3, 1), bytes_per_frame=moved, kernel_tbs=round(tbs, 2),
                 hbm_peak_fraction=round(tbs / 8.0, 3))
        print(f"{bits:2d}-bit DPX  k_dpx_decode, {nb} frames per call: {k_ms*1e3:6.1f} us/frame  {moved/1e6:6.1f} MB/frame  "
              f"{tbs:5.2f} TB/s = {tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)
        res[f"dpx{bits}"] = r
        del pays, outs
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps({"streambench_dpx": res}), flush=True)


def tiff_main():
    import json

    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from tiff_files import read_tiff, write_tiff

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(16)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def ring(open_fn, fill):
        open_fn()
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            fill(ctx.stream_input())
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    # 1. forward: GBR 16-bit video range -> BT.2020nc 10-bit 4:2:0 FIR, the samples of one picture
    rgb = rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16)
    info, _ = h.parse_tiff(write_tiff(rgb))
    payload = np.ascontiguousarray(rgb).view(np.uint8).reshape(-1)
    planes = read_tiff(rgb)[0]  # the .rgb ring gets the clamped planes: the same .yuv
    d = h.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=10, src_transfer=1, dst_transfer=1, src_primaries=1,
                    dst_primaries=1, dst_matrix=h.MATRIX_BT2020NC, resampler=1)

    def fill_tiff(slot):
        slot[0][:] = payload

    def fill_rgb(slot):
        for c in range(3):
            slot[c][:] = planes[c]

    ring(lambda: ctx.tiff_stream_open(d, info, 1, depth), fill_tiff)  # warm-up
    t_tiff = ring(lambda: ctx.tiff_stream_open(d, info, 1, depth), fill_tiff)
    ring(lambda: ctx.stream_open(d, depth), fill_rgb)
    t_rgb = ring(lambda: ctx.stream_open(d, depth), fill_rgb)
    res["forward"] = dict(tiff_ring_ms=round(t_tiff * 1e3, 2), tiff_ring_fps=round(1 / t_tiff, 1), rgb_ring_ms=round(t_rgb * 1e3, 2),
                          rgb_ring_fps=round(1 / t_rgb, 1), ratio=round(t_rgb / t_tiff, 2))
    print(f"forward ring from host memory: tiff {t_tiff*1e3:6.2f} ms/frame {1/t_tiff:6.1f} frames/s   "
          f".rgb {t_rgb*1e3:6.2f} ms/frame {1/t_rgb:6.1f} frames/s   ({t_rgb/t_tiff:4.2f}x)", flush=True)

    # 2. inverse: 12-bit BT.709 4:2:0 FIR -> 16-bit R,G,B
    yuv = [rng.integers(0, 4096, m).astype(np.uint16) for m in (n, n // 4, n // 4)]

    def fill_yuv(slot):
        for c in range(3):
            slot[c][:] = yuv[c]

    args = (w, hh, 1, 12, 0, 1, 16, 1, depth)
    ring(lambda: ctx.tiff_inverse_stream_open(*args), fill_yuv)
    t_ti = ring(lambda: ctx.tiff_inverse_stream_open(*args), fill_yuv)
    ring(lambda: ctx.inverse_stream_open(*args), fill_yuv)
    t_inv = ring(lambda: ctx.inverse_stream_open(*args), fill_yuv)
    res["inverse"] = dict(tiff_inverse_ring_ms=round(t_ti * 1e3, 2), tiff_inverse_ring_fps=round(1 / t_ti, 1),
                          inverse_ring_ms=round(t_inv * 1e3, 2), inverse_ring_fps=round(1 / t_inv, 1), ratio=round(t_inv / t_ti, 2))
    print(f"inverse ring from host memory: tiff {t_ti*1e3:6.2f} ms/frame {1/t_ti:6.1f} frames/s   "
          f"planar {t_inv*1e3:6.2f} ms/frame {1/t_inv:6.1f} frames/s   ({t_inv/t_ti:4.2f}x)", flush=True)

    # 3. the kernels over 64 frames on the device: 64 distinct inputs and outputs
    pays = [torch.randint(-(1 << 15), (1 << 15) - 1, (info.payload_bytes // 2,), dtype=torch.int16, device="cuda") for _ in range(nb)]
    outs = [[torch.empty(n, dtype=torch.int16, device="cuda") for _ in range(3)] for _ in range(nb)]
    rgbs = [torch.empty(3 * n, dtype=torch.int16, device="cuda") for _ in range(nb)]
    torch.cuda.synchronize()
    for name, call in (("k_tiff_decode", lambda: ctx.tiff_decode_batch(info, 1, pays, outs)),
                       ("k_rgb_interleave", lambda: ctx.rgb_interleave_batch(w, hh, outs, rgbs))):
        ks = []
        for rep in range(reps + 1):  # rep 0 warms up
            call()
            if rep:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        tbs = 12 * n / (k_ms * 1e-3) / 1e12
        res[name] = dict(kernel_us_per_frame=round(k_ms * 1e3, 1), bytes_per_frame=12 * n, kernel_tbs=round(tbs, 2),
                         hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"{name:16s} {nb} frames per call: {k_ms*1e3:6.1f} us/frame  {12*n/1e6:6.1f} MB/frame  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)
    ctx.close()
    print(json.dumps({"streambench_tiff": res}), flush=True)


def main():
    n = int(os.environ.get("N", "200"))  # long enough for the start-up (three slots filled by host copies) not to weigh
    depth = int(os.environ.get("DEPTH", "3"))
    w, hh = 3840, 2160
    d = h.make_desc(w, hh, dst_depth=12, dst_matrix=9, resampler=0)
    planes = synth_frame(w, hh, 0)
    ctx = h.Context(0)
    ctx.convert_frame(d, planes)
    t0 = time.perf_counter()
    for _ in range(n // 4):
        ctx.convert_frame(d, planes)
    dt = (time.perf_counter() - t0) / (n // 4)
    print(f"h2y_convert_frame (pageable host buffers, serial):   {dt*1e3:7.2f} ms/frame  {1/dt:7.1f} frames/s", flush=True)

    ctx.stream_open(d, depth)
    for fill in (False, True):
        # fill=True also pays for writing the input into the pinned slot (a memcpy standing in for the file read)
        inflight = 0
        done = 0
        t0 = time.perf_counter()
        for _ in range(n):
            dst = ctx.stream_input()
            if fill or done + inflight < depth:
                for c in range(3):
                    dst[c][:] = planes[c]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
                done += 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
            done += 1
        dt = (time.perf_counter() - t0) / n
        gb = (3 * w * hh * 4 + h.frame_bytes(d)) / 1e9
        print(f"h2y_stream_* depth {depth}{' + host copy into the slot' if fill else '':28s}: {dt*1e3:7.2f} ms/frame  {1/dt:7.1f} frames/s  ({gb/dt:5.1f} GB/s over PCIe)", flush=True)
    ctx.stream_close()
    ctx.close()


def exr_main():
    import json
    from concurrent.futures import ThreadPoolExecutor

    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from exr_files import HALF, NONE, ZIP, read_exr, smooth_half, write_exr

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    threads = int(os.environ.get("UNPACK_THREADS", "16"))
    depth = 3
    ctx = h.Context(0)
    pool = ThreadPoolExecutor(threads)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth,
           "unpack_threads": threads, "hbm_peak_tbs": 8.0}

    def ring(open_fn, fill):
        open_fn()
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            fill(ctx.stream_input())
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    def unpack(info, chunks, data, payload):
        step = max(1, info.n_chunks // (4 * threads))
        list(pool.map(lambda c0: h.exr_unpack(info, chunks, data, payload, c0, min(step, info.n_chunks - c0)),
                      range(0, info.n_chunks, step)))

    ch = {name: (HALF, smooth_half(hh, w, 101 * k)) for k, name in enumerate("RGB")}
    d = h.make_desc(w, hh, sample=h.SAMPLE_F16, dst_depth=10, src_transfer=8, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, resampler=1)
    for comp, cname in ((NONE, "none"), (ZIP, "zip")):
        data, _ = write_exr(ch, comp)
        buf = np.frombuffer(data, np.uint8)
        info, chunks = h.parse_exr(buf)
        planes = [p.reshape(-1) for p in read_exr(data)]

        def fill_exr(slot):
            unpack(info, chunks, buf, slot[0])

        def fill_f16(slot):
            for c in range(3):
                slot[c][:] = planes[c]

        ring(lambda: ctx.exr_stream_open(d, info, depth), fill_exr)  # warm-up
        t_exr = ring(lambda: ctx.exr_stream_open(d, info, depth), fill_exr)
        ring(lambda: ctx.stream_open(d, depth), fill_f16)
        t_f16 = ring(lambda: ctx.stream_open(d, depth), fill_f16)
        payload = np.zeros(info.payload_bytes, np.uint8)
        unpack(info, chunks, buf, payload)
        t0 = time.perf_counter()
        for _ in range(10):
            unpack(info, chunks, buf, payload)
        t_un = (time.perf_counter() - t0) / 10
        res[cname] = dict(file_mb=round(len(data) / 1e6, 1), exr_ring_ms=round(t_exr * 1e3, 2), exr_ring_fps=round(1 / t_exr, 1),
                          f16_ring_ms=round(t_f16 * 1e3, 2), f16_ring_fps=round(1 / t_f16, 1), ratio=round(t_f16 / t_exr, 2),
                          unpack_ms=round(t_un * 1e3, 2))
        print(f"{cname:4s} ({len(data)/1e6:5.1f} MB file): exr ring {t_exr*1e3:6.2f} ms/frame {1/t_exr:6.1f} frames/s   "
              f".f16 ring {t_f16*1e3:6.2f} ms/frame {1/t_f16:6.1f} frames/s   ({t_f16/t_exr:4.2f}x)   "
              f"host unpack {t_un*1e3:6.2f} ms/frame with {threads} threads", flush=True)

        # the kernel over 64 frames on the device: 64 distinct payloads and outputs
        dev = torch.from_numpy(payload).cuda()
        pays = [dev.clone() for _ in range(nb)]
        outs = [[torch.empty(n, dtype=torch.int16, device="cuda") for _ in range(3)] for _ in range(nb)]
        torch.cuda.synchronize()
        ks = []
        for rep in range(reps + 1):  # rep 0 warms up
            ctx.exr_decode_batch(info, pays, outs)
            if rep:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        nbytes = (12 if comp == NONE else 15) * n
        tbs = nbytes / (k_ms * 1e-3) / 1e12
        got = [o.cpu().numpy().view(np.uint16) for o in outs[nb - 1]]
        assert all(np.array_equal(g, p) for g, p in zip(got, planes)), "k_exr_decode differs from read_exr"
        res[cname].update(kernel_us_per_frame=round(k_ms * 1e3, 1), bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2),
                          hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"k_exr_decode {cname:4s} {nb} frames per call: {k_ms*1e3:6.1f} us/frame  {nbytes/1e6:6.1f} MB/frame  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)
        del pays, outs, dev
    pool.shutdown()
    ctx.close()
    print(json.dumps({"streambench_exr": res}), flush=True)


def compare_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n, nc = w * hh, (w // 2) * (hh // 2)
    total = n + 2 * nc
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(17)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    # 1. the kernels over 64 distinct frame pairs on the device
    a = [torch.randint(0, 1024, (total,), dtype=torch.int16, device="cuda") for _ in range(nb)]
    b = [x + torch.randint(-2, 3, (total,), dtype=torch.int16, device="cuda") for x in a]
    torch.cuda.synchronize()
    ks = []
    for rep in range(reps + 1):  # rep 0 warms up
        ctx.compare_batch(w, hh, h.CHROMA_420, 0, a, b)
        if rep:
            ks.append(ctx.last_kernel_ms()[0] / nb)
    k_ms = float(np.median(ks))
    nbytes = 2 * 2 * total
    tbs = nbytes / (k_ms * 1e-3) / 1e12
    res["k_compare"] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2),
                            hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
    print(f"k_compare        {nb} frames per call: {k_ms*1e3:6.2f} us/frame  {nbytes/1e6:6.1f} MB/frame  {tbs:5.2f} TB/s = "
          f"{tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)
    del a, b
    torch.cuda.empty_cache()

    def ring(open_fn, fill, ref=None, keep=1):
        open_fn()
        if ref is not None and open_fn is not open_cmp:
            ctx.stream_compare(0, keep)
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            fill(ctx.stream_input())
            if ref is not None:
                ctx.stream_reference()[:] = ref
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                if ref is not None:
                    ctx.stream_compare_result()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            if ref is not None:
                ctx.stream_compare_result()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    # 2. the forward ring: 16-bit G,B,R -> BT.2020nc 10-bit 4:2:0 box, unarmed and armed
    planes = [rng.integers(0, 65536, n, dtype=np.uint16) for _ in range(3)]
    d = h.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=10, src_transfer=1, dst_transfer=1, src_primaries=1,
                    dst_primaries=1, dst_matrix=h.MATRIX_BT2020NC, resampler=0)
    yuv_ref = ctx.convert_frame(d, planes)

    def fill_planes(slot):
        for c in range(3):
            slot[c][:] = planes[c]

    def open_fwd():
        ctx.stream_open(d, depth)

    def open_cmp():
        ctx.compare_stream_open(w, hh, h.CHROMA_420, 0, depth)

    ring(open_fwd, fill_planes)  # warm-up
    t_plain = ring(open_fwd, fill_planes)
    t_keep = ring(open_fwd, fill_planes, yuv_ref, 1)
    t_none = ring(open_fwd, fill_planes, yuv_ref, 0)
    res["forward_ring"] = dict(unarmed_fps=round(1 / t_plain, 1), armed_keep1_fps=round(1 / t_keep, 1), armed_keep0_fps=round(1 / t_none, 1),
                               unarmed_ms=round(t_plain * 1e3, 2), armed_keep1_ms=round(t_keep * 1e3, 2), armed_keep0_ms=round(t_none * 1e3, 2))
    print(f"forward ring from host memory: unarmed {1/t_plain:6.1f} frames/s   armed keep_output 1 {1/t_keep:6.1f} frames/s   "
          f"keep_output 0 {1/t_none:6.1f} frames/s", flush=True)

    # 3. the compare-only ring
    yuv_a = [yuv_ref[:n], yuv_ref[n:n + nc], yuv_ref[n + nc:]]

    def fill_a(slot):
        for c in range(3):
            slot[c][:] = yuv_a[c]

    ring(open_cmp, fill_a, yuv_ref)
    t_cmp = ring(open_cmp, fill_a, yuv_ref)
    res["compare_only_ring"] = dict(fps=round(1 / t_cmp, 1), ms=round(t_cmp * 1e3, 2))
    print(f"compare-only ring from host memory: {1/t_cmp:6.1f} frames/s ({t_cmp*1e3:6.2f} ms/frame)", flush=True)
    ctx.close()
    print(json.dumps({"streambench_compare": res}), flush=True)


def histogram_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n, nc = w * hh, (w // 2) * (hh // 2)
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(19)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    # 1. the kernels over 64 distinct frames on the device
    for chroma, bd in ((h.CHROMA_420, 10), (h.CHROMA_444, 16)):
        total = n + 2 * (nc if chroma == h.CHROMA_420 else n)
        for content in ("uniform", "constant", "row"):
            if content == "uniform":
                frames = [torch.randint(0, 1 << bd, (total,), dtype=torch.int32, device="cuda").to(torch.int16) for _ in range(nb)]
            elif content == "constant":
                frames = [torch.full((total,), (37 * k + 100) % (1 << bd), dtype=torch.int32, device="cuda").to(torch.int16)
                          for k in range(nb)]
            else:
                rows = total // w
                frames = [(((torch.arange(rows, device="cuda") * 37 + k) % (1 << bd)).to(torch.int16)).repeat_interleave(w)
                          for k in range(nb)]
            frames = [f.contiguous() for f in frames]
            torch.cuda.synchronize()
            ks = []
            for rep in range(reps + 1):  # rep 0 warms up
                ctx.histogram_batch(w, hh, chroma, bd, 0, 0, bd, frames, want_bins=False)
                if rep:
                    ks.append(ctx.last_kernel_ms()[0] / nb)
            k_ms = float(np.median(ks))
            nbytes = 2 * total
            tbs = nbytes / (k_ms * 1e-3) / 1e12
            key = f"k_histogram_{'420' if chroma == h.CHROMA_420 else '444'}_{bd}bit_{content}"
            res[key] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2),
                            hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
            print(f"{key:34s} {nb} frames per call: {k_ms*1e3:6.2f} us/frame  {nbytes/1e6:6.1f} MB/frame  {tbs:5.2f} TB/s = "
                  f"{tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)
            del frames
            torch.cuda.empty_cache()

    def ring(open_fn, fill, arm=False):
        open_fn()
        if arm:
            ctx.stream_histogram()
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            fill(ctx.stream_input())
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                if arm:
                    ctx.stream_histogram_result()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            if arm:
                ctx.stream_histogram_result()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    # 2. the forward ring: 16-bit G,B,R -> BT.2020nc 10-bit 4:2:0 box, unarmed and armed
    planes = [rng.integers(0, 65536, n, dtype=np.uint16) for _ in range(3)]
    d = h.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=10, src_transfer=1, dst_transfer=1, src_primaries=1,
                    dst_primaries=1, dst_matrix=h.MATRIX_BT2020NC, resampler=0)
    yuv = ctx.convert_frame(d, planes)

    def fill_planes(slot):
        for c in range(3):
            slot[c][:] = planes[c]

    def open_fwd():
        ctx.stream_open(d, depth)

    ring(open_fwd, fill_planes)  # warm-up
    t_plain = ring(open_fwd, fill_planes)
    t_armed = ring(open_fwd, fill_planes, True)
    res["forward_ring"] = dict(unarmed_fps=round(1 / t_plain, 1), armed_fps=round(1 / t_armed, 1), armed_share=round(t_plain / t_armed, 3),
                               unarmed_ms=round(t_plain * 1e3, 2), armed_ms=round(t_armed * 1e3, 2))
    print(f"forward ring from host memory: unarmed {1/t_plain:6.1f} frames/s   armed {1/t_armed:6.1f} frames/s "
          f"({t_plain/t_armed*100:5.1f} %)", flush=True)

    # 3. the histogram-only ring
    yuv_planes = [yuv[:n], yuv[n:n + nc], yuv[n + nc:]]

    def fill_yuv(slot):
        for c in range(3):
            slot[c][:] = yuv_planes[c]

    def open_hist():
        ctx.histogram_stream_open(w, hh, h.CHROMA_420, 10, 0, 0, 10, depth)

    ring(open_hist, fill_yuv)
    t_hist = ring(open_hist, fill_yuv)
    res["histogram_only_ring"] = dict(fps=round(1 / t_hist, 1), ms=round(t_hist * 1e3, 2))
    print(f"histogram-only ring from host memory: {1/t_hist:6.1f} frames/s ({t_hist*1e3:6.2f} ms/frame)", flush=True)
    ctx.close()
    print(json.dumps({"streambench_histogram": res}), flush=True)


def ssim_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(19)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    # 1. the kernels over 64 distinct frame pairs on the device
    for name, chroma, bits in (("10bit_420", h.CHROMA_420, 10), ("16bit_444", h.CHROMA_444, 16)):
        total = w * hh + 2 * ((w // 2) * (hh // 2) if chroma == h.CHROMA_420 else w * hh)
        hi = 1 << bits
        a = [torch.randint(0, hi, (total,), dtype=torch.int32, device="cuda").to(torch.int16) for _ in range(nb)]
        b = [x + torch.randint(-2, 3, (total,), dtype=torch.int16, device="cuda") for x in a]
        torch.cuda.synchronize()
        ks = []
        for rep in range(reps + 1):  # rep 0 warms up
            ctx.ssim_batch(w, hh, chroma, bits, a, b)
            if rep:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        nbytes = 2 * 2 * total
        tbs = nbytes / (k_ms * 1e-3) / 1e12
        res["k_ssim_" + name] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2),
                                     hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"k_ssim {name} {nb} pairs per call: {k_ms*1e3:6.2f} us/pair  {nbytes/1e6:6.1f} MB/pair  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)
        del a, b
        torch.cuda.empty_cache()

    n, nc = w * hh, (w // 2) * (hh // 2)

    def ring(open_fn, fill, ref, ssim, arm=True):
        open_fn()
        if arm:
            ctx.stream_compare(0, 1)
        if ssim is not None:
            ctx.stream_ssim(ssim)
        inflight = 0

        def take():
            ctx.stream_output()
            ctx.stream_compare_result()
            if ssim is not None:
                ctx.stream_ssim_result()

        t0 = time.perf_counter()
        for _ in range(nf):
            fill(ctx.stream_input())
            ctx.stream_reference()[:] = ref
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                take()
                inflight -= 1
        while inflight:
            take()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    # 2. the forward ring: 16-bit G,B,R -> BT.2020nc 10-bit 4:2:0 box, compare alone and compare + SSIM
    planes = [rng.integers(0, 65536, n, dtype=np.uint16) for _ in range(3)]
    d = h.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=10, src_transfer=1, dst_transfer=1, src_primaries=1,
                    dst_primaries=1, dst_matrix=h.MATRIX_BT2020NC, resampler=0)
    yuv_ref = ctx.convert_frame(d, planes)

    def fill_planes(slot):
        for c in range(3):
            slot[c][:] = planes[c]

    def open_fwd():
        ctx.stream_open(d, depth)

    ring(open_fwd, fill_planes, yuv_ref, None)  # warm-up
    t_cmp = ring(open_fwd, fill_planes, yuv_ref, None)
    t_ssim = ring(open_fwd, fill_planes, yuv_ref, -1)
    res["forward_ring"] = dict(compare_fps=round(1 / t_cmp, 1), compare_ssim_fps=round(1 / t_ssim, 1), compare_ms=round(t_cmp * 1e3, 2),
                               compare_ssim_ms=round(t_ssim * 1e3, 2))
    print(f"forward ring from host memory: compare {1/t_cmp:6.1f} frames/s   compare + ssim {1/t_ssim:6.1f} frames/s", flush=True)

    # 3. the compare-only ring, without and with SSIM
    yuv_a = [yuv_ref[:n], yuv_ref[n:n + nc], yuv_ref[n + nc:]]

    def fill_a(slot):
        for c in range(3):
            slot[c][:] = yuv_a[c]

    def open_cmp():
        ctx.compare_stream_open(w, hh, h.CHROMA_420, 0, depth)

    ring(open_cmp, fill_a, yuv_ref, None, arm=False)
    t_c = ring(open_cmp, fill_a, yuv_ref, None, arm=False)
    t_s = ring(open_cmp, fill_a, yuv_ref, 10, arm=False)
    res["compare_only_ring"] = dict(fps=round(1 / t_c, 1), ssim_fps=round(1 / t_s, 1), ms=round(t_c * 1e3, 2), ssim_ms=round(t_s * 1e3, 2))
    print(f"compare-only ring from host memory: {1/t_c:6.1f} frames/s, with ssim {1/t_s:6.1f} frames/s", flush=True)
    ctx.close()
    print(json.dumps({"streambench_ssim": res}), flush=True)


def regions_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    nf = int(os.environ.get("N", "60"))
    depth = 3
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def timed(calls):
        """every call of calls in turn, reps times after a warm-up: per call its kernel times in ms per frame"""
        out = [[] for _ in calls]
        for rep in range(reps + 1):
            for k, call in enumerate(calls):
                call()
                if rep:
                    out[k].append(ctx.last_kernel_ms()[0] / nb)
        return out

    def report(key, label, t, nbytes, variant):
        med = float(np.median(t))
        tbs = nbytes / (med * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(med * 1e3, 2), min_us=round(min(t) * 1e3, 2), max_us=round(max(t) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=variant)
        print(f"{label:30s} {nb} pairs per call: {med*1e3:7.2f} us/frame ({min(t)*1e3:.2f}..{max(t)*1e3:.2f})  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s  {variant}", flush=True)
        return med

    # 1. the kernels over 64 distinct frame pairs on the device, in turn; each reads both sides once: 4 bytes a sample pair
    for name, chroma, bits, radii in (("10bit_420", h.CHROMA_420, 10, (1, 4)), ("16bit_444", h.CHROMA_444, 16, (1,))):
        total = w * hh + 2 * ((w // 2) * (hh // 2) if chroma == h.CHROMA_420 else w * hh)
        hi, v = 1 << bits, 4 * 4 ** (bits - 8)
        b = [torch.randint(0, hi, (total,), dtype=torch.int32, device="cuda").to(torch.int16) for _ in range(nb)]
        a = [x + torch.randint(-2, 3, (total,), dtype=torch.int16, device="cuda") for x in b]
        torch.cuda.synchronize()
        variants = {}
        note = lambda key: variants.setdefault(key, ctx.last_kernel_variant())  # noqa: E731
        calls = [(lambda r: lambda: (ctx.regions_batch(w, hh, chroma, v, r, a, b), note(f"r{r}")))(r) for r in radii]
        calls += [lambda: (ctx.compare_batch(w, hh, chroma, 0, a, b), note("cmp")), lambda: (ctx.ssim_batch(w, hh, chroma, bits, a, b), note("ssim"))]
        t = timed(calls)
        nbytes = 2 * 2 * total
        m_reg = [report(f"k_regions_{name}_r{r}", f"k_regions {name} r={r}", t[k], nbytes, variants[f"r{r}"]) for k, r in enumerate(radii)]
        report(f"k_compare_{name}", f"k_compare {name}", t[len(radii)], nbytes, variants["cmp"])
        m_ssim = report(f"k_ssim_{name}", f"k_ssim {name}", t[len(radii) + 1], nbytes, variants["ssim"])
        for r, m in zip(radii, m_reg):
            res[f"ratio_to_k_ssim_{name}_r{r}"] = round(m / m_ssim, 3)
            print(f"k_regions / k_ssim {name} r={r}: {m/m_ssim:5.3f}", flush=True)
        del a, b
        torch.cuda.empty_cache()

    # 2. the compare-only ring on 10-bit 4:2:0 frames from host memory, unarmed and armed
    n, nc = w * hh, (w // 2) * (hh // 2)
    rng = np.random.default_rng(23)
    ref = rng.integers(0, 1024, n + 2 * nc, dtype=np.uint16)
    pic = np.clip(ref.astype(np.int32) + rng.integers(-2, 3, ref.size), 0, 1023).astype(np.uint16)
    planes = [pic[:n], pic[n:n + nc], pic[n + nc:]]

    def ring(regions):
        ctx.compare_stream_open(w, hh, h.CHROMA_420, 0, depth)
        if regions:
            ctx.stream_regions(64, regions)
        inflight = 0

        def take():
            ctx.stream_output()
            ctx.stream_compare_result()
            if regions:
                ctx.stream_regions_result()

        t0 = time.perf_counter()
        for _ in range(nf):
            slot = ctx.stream_input()
            for c in range(3):
                slot[c][:] = planes[c]
            ctx.stream_reference()[:] = ref
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                take()
                inflight -= 1
        while inflight:
            take()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    ring(0)  # warm-up
    t_c = float(np.median([ring(0) for _ in range(3)]))
    t_r = {r: float(np.median([ring(r) for _ in range(3)])) for r in (1, 4)}
    res["compare_only_ring"] = dict(fps=round(1 / t_c, 1), ms=round(t_c * 1e3, 2), regions_r1_fps=round(1 / t_r[1], 1), regions_r1_ms=round(t_r[1] * 1e3, 2),
                                    regions_r4_fps=round(1 / t_r[4], 1), regions_r4_ms=round(t_r[4] * 1e3, 2))
    print(f"compare-only ring from host memory: {1/t_c:6.1f} frames/s, with regions r=1 {1/t_r[1]:6.1f}, r=4 {1/t_r[4]:6.1f} frames/s", flush=True)
    ctx.close()
    print(json.dumps({"streambench_regions": res}), flush=True)


def light_main():
    import json

    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from dpx_files import pack_pixels, write_dpx
    from exr_files import HALF, NONE, smooth_half, write_exr
    from tiff_files import write_tiff

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(23)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    # 1. k_light over 64 distinct frames on the device (floor and ceiling given: the kernel alone is timed)
    for name, sample, src_transfer, depth_in in (("f32", h.SAMPLE_F32, 8, 32), ("f16", h.SAMPLE_F16, 8, 32), ("u16", h.SAMPLE_U16, 8, 16),
                                                 ("f32_bt1886", h.SAMPLE_F32, 1, 32)):
        d = h.make_desc(w, hh, sample=sample, src_depth=depth_in, dst_depth=10, src_transfer=src_transfer, dst_transfer=16,
                        dst_matrix=h.MATRIX_BT2020NC, resampler=0, stats=[(0, 1 if sample != h.SAMPLE_U16 else 65535)] * 3)
        if sample == h.SAMPLE_U16:
            frames = [[torch.randint(0, 65536, (n,), dtype=torch.int32, device="cuda").to(torch.int16) for _ in range(3)] for _ in range(nb)]
        else:
            dt = torch.float32 if sample == h.SAMPLE_F32 else torch.float16
            frames = [[torch.rand(n, device="cuda").to(dt) for _ in range(3)] for _ in range(nb)]
        torch.cuda.synchronize()
        ks = []
        for rep in range(reps + 1):  # rep 0 warms up
            ctx.light_batch(d, frames)
            if rep:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        nbytes = 3 * n * (4 if sample == h.SAMPLE_F32 else 2)
        tbs = nbytes / (k_ms * 1e-3) / 1e12
        res[f"k_light_{name}"] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2),
                                      hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"k_light {name:11s} {nb} frames per call: {k_ms*1e3:6.2f} us/frame  {nbytes/1e6:6.1f} MB/frame  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)
        del frames
        torch.cuda.empty_cache()

    def ring(open_fn, fill, arm):
        open_fn()
        if arm:
            ctx.stream_light()
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            fill(ctx.stream_input())
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                if arm:
                    ctx.stream_light_result()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            if arm:
                ctx.stream_light_result()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    def both(key, open_fn, fill):
        ring(open_fn, fill, False)  # warm-up
        t_plain, t_armed = ring(open_fn, fill, False), ring(open_fn, fill, True)
        res[key] = dict(unarmed_fps=round(1 / t_plain, 1), armed_fps=round(1 / t_armed, 1), armed_share=round(t_plain / t_armed, 3))
        print(f"{key:12s} ring from host memory: unarmed {1/t_plain:6.1f} frames/s   armed {1/t_armed:6.1f} frames/s "
              f"({t_plain/t_armed*100:5.1f} %)", flush=True)

    # 2. every forward ring, unarmed and armed, linear light -> PQ BT.2020nc 10-bit 4:2:0
    d32 = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=1)
    rgb = [rng.random(n, dtype=np.float32) for _ in range(3)]
    planes = [rgb[1], rgb[2], rgb[0]]

    def fill_planes(slot):
        for c in range(3):
            slot[c][:] = planes[c]

    both("f32", lambda: ctx.stream_open(d32, depth), fill_planes)
    data = write_dpx(w, hh, 32, pack_pixels(*(c.view(np.uint32) for c in rgb), 32))
    info = h.parse_dpx(data[:2048], len(data))
    payload = np.frombuffer(data, np.uint8, count=info.payload_bytes, offset=info.data_offset)

    def fill_payload(slot, p=payload):
        slot[0][:] = p

    both("dpx_float", lambda: ctx.dpx_stream_open(d32, info, depth), fill_payload)
    pic = rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16)
    tdata = write_tiff(pic)
    tinfo, rows = h.parse_tiff(tdata)
    tpay = np.frombuffer(b"".join(tdata[int(o):int(o) + int(tinfo.row_bytes)] for o in rows), np.uint8)
    d16 = h.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=1)
    both("tiff", lambda: ctx.tiff_stream_open(d16, tinfo, 0, depth), lambda slot: fill_payload(slot, tpay))
    edata, _ = write_exr({name: (HALF, smooth_half(hh, w, 101 * k)) for k, name in enumerate("RGB")}, NONE)
    ebuf = np.frombuffer(edata, np.uint8)
    einfo, echunks = h.parse_exr(ebuf)
    dh = h.make_desc(w, hh, sample=h.SAMPLE_F16, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=1)
    both("exr", lambda: ctx.exr_stream_open(dh, einfo, depth), lambda slot: h.exr_unpack(einfo, echunks, ebuf, slot[0]))
    ctx.close()
    print(json.dumps({"streambench_light": res}), flush=True)


def lightdist_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(29)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def noise(dt):
        return lambda: [torch.rand(n, device="cuda").to(dt) for _ in range(3)]

    def codes():
        return [torch.randint(0, 65536, (n,), dtype=torch.int32, device="cuda").to(torch.int16) for _ in range(3)]

    def constant():
        return [torch.full((n,), 0.25, dtype=torch.float32, device="cuda") for _ in range(3)]

    def letterbox():  # a 2.39:1 picture in a 16:9 frame: black bars above and below
        bar = (hh - int(w / 2.39)) // 2 * w
        planes = noise(torch.float32)()
        for p in planes:
            p[:bar] = 0.0
            p[n - bar:] = 0.0
        return planes

    # 1. and 2.: k_lightdist beside k_light on the same 64 device frames, the calls taken in turn
    F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
    for name, sample, src_transfer, depth_in, make in (("f32", F32, 8, 32, noise(torch.float32)), ("f16", F16, 8, 32, noise(torch.float16)),
                                                       ("u16", U16, 8, 16, codes), ("f32_bt1886", F32, 1, 32, noise(torch.float32)),
                                                       ("f32_constant", F32, 8, 32, constant), ("f32_letterbox", F32, 8, 32, letterbox)):
        d = h.make_desc(w, hh, sample=sample, src_depth=depth_in, dst_depth=10, src_transfer=src_transfer, dst_transfer=16,
                        dst_matrix=h.MATRIX_BT2020NC, resampler=0, stats=[(0, 1 if sample != U16 else 65535)] * 3)
        frames = [make() for _ in range(nb)]
        torch.cuda.synchronize()
        light, dist = [], []
        for rep in range(reps + 1):  # rep 0 warms up
            ctx.light_batch(d, frames)
            if rep:
                light.append(ctx.last_kernel_ms()[0] / nb)
            ctx.lightdist_batch(d, frames)
            if rep:
                dist.append(ctx.last_kernel_ms()[0] / nb)
        variant = ctx.last_kernel_variant()
        l_ms, d_ms = float(np.median(light)), float(np.median(dist))
        nbytes = 3 * n * (4 if sample == F32 else 2)
        tbs = nbytes / (d_ms * 1e-3) / 1e12
        res[f"k_lightdist_{name}"] = dict(kernel_us_per_frame=round(d_ms * 1e3, 2), min_us=round(min(dist) * 1e3, 2), max_us=round(max(dist) * 1e3, 2),
                                          k_light_us_per_frame=round(l_ms * 1e3, 2), k_light_min_us=round(min(light) * 1e3, 2),
                                          k_light_max_us=round(max(light) * 1e3, 2), ratio_to_k_light=round(d_ms / l_ms, 3),
                                          bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=variant)
        print(f"k_lightdist {name:13s} {nb} frames per call: {d_ms*1e3:6.2f} us/frame ({min(dist)*1e3:.2f}..{max(dist)*1e3:.2f})  k_light "
              f"{l_ms*1e3:6.2f} us/frame ({min(light)*1e3:.2f}..{max(light)*1e3:.2f})  ratio {d_ms/l_ms:5.3f}  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)
        del frames
        torch.cuda.empty_cache()

    # 3. the .f32 ring, unarmed and armed
    def ring(arm):
        ctx.stream_open(d32, depth)
        if arm:
            ctx.stream_lightdist()
        inflight = 0
        t0 = time.perf_counter()

        def take():
            ctx.stream_output()
            if arm:
                ctx.stream_lightdist_result()

        for _ in range(nf):
            slot = ctx.stream_input()
            for c in range(3):
                slot[c][:] = planes[c]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                take()
                inflight -= 1
        while inflight:
            take()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    d32 = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=1)
    planes = [rng.random(n, dtype=np.float32) for _ in range(3)]
    ring(False)  # warm-up
    t_plain, t_armed = ring(False), ring(True)
    res["f32_ring"] = dict(unarmed_fps=round(1 / t_plain, 1), armed_fps=round(1 / t_armed, 1), armed_share=round(t_plain / t_armed, 3))
    print(f"f32 ring from host memory: unarmed {1/t_plain:6.1f} frames/s   armed {1/t_armed:6.1f} frames/s ({t_plain/t_armed*100:5.1f} %)", flush=True)
    ctx.close()
    print(json.dumps({"streambench_lightdist": res}), flush=True)


def scenes_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(31)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def noise(dt):
        return lambda: [torch.rand(n, device="cuda").to(dt) for _ in range(3)]

    def codes16():
        return [torch.randint(0, 65536, (n,), dtype=torch.int32, device="cuda").to(torch.int16) for _ in range(3)]

    def constant():
        return [torch.full((n,), 0.25, dtype=torch.float32, device="cuda") for _ in range(3)]

    def letterbox():  # a 2.39:1 picture in a 16:9 frame: black bars above and below
        bar = (hh - int(w / 2.39)) // 2 * w
        planes = noise(torch.float32)()
        for p in planes:
            p[:bar] = 0.0
            p[n - bar:] = 0.0
        return planes

    def timed(calls):
        """every call of calls in turn, reps times after a warm-up: per call its kernel times in ms per frame, and its variant"""
        out, variants = [[] for _ in calls], [None] * len(calls)
        for rep in range(reps + 1):
            for k, call in enumerate(calls):
                call()
                variants[k] = ctx.last_kernel_variant()
                if rep:
                    out[k].append(ctx.last_kernel_ms()[0] / nb)
        return out, variants

    def figures(t, nbytes, variant):
        med = float(np.median(t))
        tbs = nbytes / (med * 1e-3) / 1e12
        return dict(kernel_us_per_frame=round(med * 1e3, 2), min_us=round(min(t) * 1e3, 2), max_us=round(max(t) * 1e3, 2), bytes_per_frame=nbytes,
                    kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=variant)

    def line(label, f):
        print(f"{label:34s} {nb} frames per call: {f['kernel_us_per_frame']:7.2f} us/frame ({f['min_us']:.2f}..{f['max_us']:.2f})  "
              f"{f['kernel_tbs']:5.2f} TB/s = {f['hbm_peak_fraction']*100:4.1f} % of 8 TB/s  {f['variant']}", flush=True)

    # 1. k_scenesig beside k_lightdist and k_light on the same 64 device frames
    F32, F16, U16 = h.SAMPLE_F32, h.SAMPLE_F16, h.SAMPLE_U16
    for name, sample, depth_in, make in (("f32", F32, 32, noise(torch.float32)), ("f16", F16, 32, noise(torch.float16)), ("u16", U16, 16, codes16),
                                         ("f32_constant", F32, 32, constant), ("f32_letterbox", F32, 32, letterbox)):
        d = h.make_desc(w, hh, sample=sample, src_depth=depth_in, dst_depth=10, src_transfer=8, dst_transfer=16,
                        dst_matrix=h.MATRIX_BT2020NC, resampler=0, stats=[(0, 1 if sample != U16 else 65535)] * 3)
        frames = [make() for _ in range(nb)]
        torch.cuda.synchronize()
        (light, dist, sig), variants = timed([lambda: ctx.light_batch(d, frames), lambda: ctx.lightdist_batch(d, frames),
                                              lambda: ctx.scenesig_batch(d, frames)])
        nbytes = 3 * n * (4 if sample == F32 else 2)
        fl, fd, fs = figures(light, nbytes, variants[0]), figures(dist, nbytes, variants[1]), figures(sig, nbytes, variants[2])
        fs["ratio_to_k_light"] = round(fs["kernel_us_per_frame"] / fl["kernel_us_per_frame"], 3)
        fs["ratio_to_k_lightdist"] = round(fs["kernel_us_per_frame"] / fd["kernel_us_per_frame"], 3)
        res[f"k_scenesig_{name}"], res[f"k_lightdist_{name}"], res[f"k_light_{name}"] = fs, fd, fl
        line(f"k_scenesig {name}", fs)
        line(f"k_lightdist {name}", fd)
        line(f"k_light {name} (yardstick)", fl)
        print(f"k_scenesig / k_light {fs['ratio_to_k_light']:5.3f}   k_scenesig / k_lightdist {fs['ratio_to_k_lightdist']:5.3f}", flush=True)
        del frames
        torch.cuda.empty_cache()

    # 2. k_codescenesig beside k_codelight DIST on 10-bit 4:2:0
    def code_frame():
        part = lambda count, lo, hi: torch.randint(lo, hi + 1, (count,), dtype=torch.int32, device="cuda").to(torch.int16)
        return torch.cat([part(n, 64, 940), part(n // 4, 64, 960), part(n // 4, 64, 960)])

    dc = h.make_codelight_desc(w, hh, 1, 10, 0, h.MATRIX_BT2020NC, 1)
    frames = [code_frame() for _ in range(nb)]
    torch.cuda.synchronize()
    (cl, cs), variants = timed([lambda: ctx.codelight_batch(dc, frames, dist=True), lambda: ctx.codescenesig_batch(dc, frames)])
    fcl, fcs = figures(cl, 11 * n, variants[0]), figures(cs, 11 * n, variants[1])
    fcs["ratio_to_k_codelight_dist"] = round(fcs["kernel_us_per_frame"] / fcl["kernel_us_per_frame"], 3)
    res["k_codescenesig_420_10_noise"], res["k_codelight_420_10_noise_dist"] = fcs, fcl
    line("k_codescenesig 420_10_noise", fcs)
    line("k_codelight 420_10_noise DIST", fcl)
    print(f"k_codescenesig / k_codelight DIST {fcs['ratio_to_k_codelight_dist']:5.3f}", flush=True)
    del frames
    torch.cuda.empty_cache()

    # 3. the .f32 ring from host memory: the distribution alone, and the signature as well
    def ring(sig):
        ctx.stream_open(d32, depth)
        ctx.stream_lightdist()
        if sig:
            ctx.stream_scenesig()
        inflight = 0
        t0 = time.perf_counter()

        def take():
            ctx.stream_output()
            ctx.stream_lightdist_result()
            if sig:
                ctx.stream_scenesig_result()
                ctx.stream_lightdist_bins()

        for _ in range(nf):
            slot = ctx.stream_input()
            for c in range(3):
                slot[c][:] = planes[c]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                take()
                inflight -= 1
        while inflight:
            take()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    d32 = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=1)
    planes = [rng.random(n, dtype=np.float32) for _ in range(3)]
    ring(False)  # warm-up
    runs = [(ring(False), ring(True)) for _ in range(3)]
    t_dist, t_sig = float(np.median([r[0] for r in runs])), float(np.median([r[1] for r in runs]))
    res["f32_ring"] = dict(lightdist_fps=round(1 / t_dist, 1), lightdist_scenesig_fps=round(1 / t_sig, 1), share=round(t_dist / t_sig, 3),
                           runs_fps=[[round(1 / a, 1), round(1 / b, 1)] for a, b in runs])
    print(f"f32 ring from host memory: h2y_stream_lightdist {1/t_dist:6.1f} frames/s   with h2y_stream_scenesig {1/t_sig:6.1f} frames/s "
          f"({t_dist/t_sig*100:5.1f} %)", flush=True)
    ctx.close()
    print(json.dumps({"streambench_scenes": res}), flush=True)


def codelight_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "frames_per_launch": h.CODELIGHT_FRAMES_PER_LAUNCH, "reps": reps,
           "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def codes(count, lo, hi):
        return torch.randint(lo, hi + 1, (count,), dtype=torch.int32, device="cuda").to(torch.int16)

    def noise(chroma, bits):
        s = 1 << (bits - 8)
        nc = n // 4 if chroma == 1 else n
        return lambda: torch.cat([codes(n, 16 * s, 235 * s), codes(nc, 16 * s, 240 * s), codes(nc, 16 * s, 240 * s)])

    def constant():
        return torch.cat([torch.full((n,), 600, dtype=torch.int16, device="cuda"), torch.full((n // 2,), 512, dtype=torch.int16, device="cuda")])

    def letterbox():  # a 2.39:1 picture in a 16:9 frame: black bars above and below
        bar = (hh - int(w / 2.39)) // 2 // 2 * 2
        f = noise(1, 10)()
        f[:bar * w] = 64
        f[n - bar * w:n] = 64
        for c in range(2):
            plane = f[n + c * (n // 4):n + (c + 1) * (n // 4)]
            plane[:bar // 2 * (w // 2)] = 512
            plane[n // 4 - bar // 2 * (w // 2):] = 512
        return f

    def timed(calls):
        """every call of calls in turn, reps times after a warm-up: per call its kernel times in ms per frame"""
        out = [[] for _ in calls]
        for rep in range(reps + 1):
            for k, call in enumerate(calls):
                call()
                if rep:
                    out[k].append(ctx.last_kernel_ms()[0] / nb)
        return out

    def report(key, label, t, nbytes, variant, **more):
        med = float(np.median(t))
        tbs = nbytes / (med * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(med * 1e3, 2), min_us=round(min(t) * 1e3, 2), max_us=round(max(t) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=variant, **more)
        print(f"{label:34s} {nb} frames per call: {med*1e3:7.2f} us/frame ({min(t)*1e3:.2f}..{max(t)*1e3:.2f})  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s  {variant}", flush=True)
        return med

    # 1. k_codelight, DIST off and on
    med = {}
    for name, chroma, bits, make in (("420_10_noise", 1, 10, noise(1, 10)), ("420_10_constant", 1, 10, constant),
                                     ("420_10_letterbox", 1, 10, letterbox), ("444_10_noise", 3, 10, noise(3, 10))):
        d = h.make_codelight_desc(w, hh, chroma, bits, 0, h.MATRIX_BT2020NC, 1)
        frames = [make() for _ in range(nb)]
        torch.cuda.synchronize()
        variants = []
        off, on = timed([lambda: (ctx.codelight_batch(d, frames), variants.append(ctx.last_kernel_variant())),
                         lambda: (ctx.codelight_batch(d, frames, dist=True), variants.append(ctx.last_kernel_variant()))])
        nbytes = n * (11 if chroma == 1 else 6)
        med[name, 0] = report(f"k_codelight_{name}", f"k_codelight {name}", off, nbytes, variants[0])
        med[name, 1] = report(f"k_codelight_{name}_dist", f"k_codelight {name} DIST", on, nbytes, variants[1])
        del frames
        torch.cuda.empty_cache()
    for dist in (0, 1):
        share = 1.0 - med["444_10_noise", dist] / med["420_10_noise", dist]
        res[f"k_up444_share{'_dist' if dist else ''}"] = round(share, 3)
        print(f"k_up444 share of the 4:2:0 time ({'DIST' if dist else 'LIGHT'}): {share*100:4.1f} %", flush=True)

    # 16-bit 4:4:4, and 2. the yardsticks on the same planes
    d = h.make_codelight_desc(w, hh, 3, 16, 0, h.MATRIX_BT2020NC, 1)
    dl = h.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=10, src_transfer=8, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC,
                     resampler=0, stats=[(0, 65535)] * 3)
    frames = [noise(3, 16)() for _ in range(nb)]
    planes = [[f[c * n:(c + 1) * n] for c in range(3)] for f in frames]
    torch.cuda.synchronize()
    variants = []
    note = lambda: variants.append(ctx.last_kernel_variant())
    off, on, light, ldist = timed([lambda: (ctx.codelight_batch(d, frames), note()), lambda: (ctx.codelight_batch(d, frames, dist=True), note()),
                                   lambda: (ctx.light_batch(dl, planes), note()), lambda: (ctx.lightdist_batch(dl, planes), note())])
    m_off = report("k_codelight_444_16_noise", "k_codelight 444_16_noise", off, 6 * n, variants[0])
    m_on = report("k_codelight_444_16_noise_dist", "k_codelight 444_16_noise DIST", on, 6 * n, variants[1])
    m_l = report("k_light_u16", "k_light U16 LINEAR (yardstick)", light, 6 * n, variants[2])
    m_ld = report("k_lightdist_u16", "k_lightdist U16 LINEAR (yardstick)", ldist, 6 * n, variants[3])
    res["ratio_to_k_light"] = round(m_off / m_l, 3)
    res["ratio_to_k_lightdist"] = round(m_on / m_ld, 3)
    print(f"k_codelight / k_light {m_off/m_l:5.3f}   k_codelight DIST / k_lightdist {m_on/m_ld:5.3f}", flush=True)
    del frames, planes
    torch.cuda.empty_cache()

    # 3. the light-only ring from host memory
    d = h.make_codelight_desc(w, hh, 1, 10, 0, h.MATRIX_BT2020NC, 1)
    host = noise(1, 10)().cpu().numpy().view(np.uint16)
    parts = [host[:n], host[n:n + n // 4], host[n + n // 4:]]

    def ring(want_dist):
        ctx.codelight_stream_open(d, want_dist, depth)
        inflight = 0
        t0 = time.perf_counter()

        def take():
            ctx.stream_output()
            ctx.stream_light_result()
            if want_dist:
                ctx.stream_lightdist_result()

        for _ in range(nf):
            slot = ctx.stream_input()
            for c in range(3):
                slot[c][:] = parts[c]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                take()
                inflight -= 1
        while inflight:
            take()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    ring(0)  # warm-up
    t_light, t_dist = ring(0), ring(1)
    res["light_only_ring"] = dict(light_fps=round(1 / t_light, 1), dist_fps=round(1 / t_dist, 1), bytes_per_frame=3 * n)
    print(f"light-only ring from host memory, 10-bit 4:2:0: {1/t_light:6.1f} frames/s   with want_dist {1/t_dist:6.1f} frames/s", flush=True)
    ctx.close()
    print(json.dumps({"streambench_codelight": res}), flush=True)


def gamutcheck_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "frames_per_launch": h.CODELIGHT_FRAMES_PER_LAUNCH, "reps": reps,
           "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def codes(count, lo, hi):
        return torch.randint(lo, hi + 1, (count,), dtype=torch.int32, device="cuda").to(torch.int16)

    def noise(chroma, bits):
        s = 1 << (bits - 8)
        nc = n // 4 if chroma == 1 else n
        return lambda: torch.cat([codes(n, 16 * s, 235 * s), codes(nc, 16 * s, 240 * s), codes(nc, 16 * s, 240 * s)])

    def timed(calls):
        """every call of calls in turn, reps times after a warm-up: per call its kernel times in ms per frame"""
        out = [[] for _ in calls]
        for rep in range(reps + 1):
            for k, call in enumerate(calls):
                call()
                if rep:
                    out[k].append(ctx.last_kernel_ms()[0] / nb)
        return out

    def report(key, label, t, nbytes, variant, **more):
        med = float(np.median(t))
        tbs = nbytes / (med * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(med * 1e3, 2), min_us=round(min(t) * 1e3, 2), max_us=round(max(t) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=variant, **more)
        print(f"{label:34s} {nb} frames per call: {med*1e3:7.2f} us/frame ({min(t)*1e3:.2f}..{max(t)*1e3:.2f})  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s  {variant}", flush=True)
        return med

    # 1. k_gamutcheck with one and with two sets beside k_codelight (LIGHT) on the same frames, in turn
    med = {}
    for name, chroma, bits, matrix in (("420_10_noise", 1, 10, h.MATRIX_BT2020NC), ("444_10_noise", 3, 10, h.MATRIX_BT2020NC),
                                       ("444_16_gbr_noise", 3, 16, h.MATRIX_GBR)):
        d = h.make_codelight_desc(w, hh, chroma, bits, 0, matrix, 1)
        frames = [noise(chroma, bits)() for _ in range(nb)]
        torch.cuda.synchronize()
        variants = {}
        note = lambda key: variants.setdefault(key, ctx.last_kernel_variant())
        one, two, light = timed([lambda: (ctx.gamutcheck_batch(d, frames, 9, [12]), note(1)), lambda: (ctx.gamutcheck_batch(d, frames, 9, [12, 1]), note(2)),
                                 lambda: (ctx.codelight_batch(d, frames), note(0))])
        nbytes = n * (11 if chroma == 1 else 6)
        med[name, 1] = report(f"k_gamutcheck_{name}_1set", f"k_gamutcheck {name} 1 set", one, nbytes, variants[1])
        med[name, 2] = report(f"k_gamutcheck_{name}_2sets", f"k_gamutcheck {name} 2 sets", two, nbytes, variants[2])
        med[name, 0] = report(f"k_codelight_{name}", f"k_codelight {name} (yardstick)", light, nbytes, variants[0])
        for sets in (1, 2):
            res[f"ratio_to_k_codelight_{name}_{sets}"] = round(med[name, sets] / med[name, 0], 3)
        res[f"ratio_2sets_to_1set_{name}"] = round(med[name, 2] / med[name, 1], 3)
        print(f"k_gamutcheck / k_codelight {name}: 1 set {med[name, 1]/med[name, 0]:5.3f}   2 sets {med[name, 2]/med[name, 0]:5.3f}   "
              f"2 sets / 1 set {med[name, 2]/med[name, 1]:5.3f}", flush=True)
        del frames
        torch.cuda.empty_cache()
    for sets in (1, 2):
        share = 1.0 - med["444_10_noise", sets] / med["420_10_noise", sets]
        res[f"k_up444_share_{sets}"] = round(share, 3)
        print(f"k_up444 share of the 4:2:0 time ({sets} set{'s' if sets > 1 else ''}): {share*100:4.1f} %", flush=True)

    # 2. the light-only ring from host memory, unarmed and armed
    d = h.make_codelight_desc(w, hh, 1, 10, 0, h.MATRIX_BT2020NC, 1)
    host = noise(1, 10)().cpu().numpy().view(np.uint16)
    parts = [host[:n], host[n:n + n // 4], host[n + n // 4:]]

    def ring(armed):
        ctx.codelight_stream_open(d, 0, depth)
        if armed:
            ctx.stream_gamutcheck(9, [12, 1])
        inflight = 0
        t0 = time.perf_counter()

        def take():
            ctx.stream_output()
            ctx.stream_light_result()
            if armed:
                ctx.stream_gamutcheck_result()

        for _ in range(nf):
            slot = ctx.stream_input()
            for c in range(3):
                slot[c][:] = parts[c]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                take()
                inflight -= 1
        while inflight:
            take()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    ring(0)  # warm-up
    ring(1)
    t = {0: [], 1: []}
    for _ in range(3):
        for armed in (0, 1):
            t[armed].append(ring(armed))
    plain, armed = float(np.median(t[0])), float(np.median(t[1]))
    res["light_only_ring"] = dict(unarmed_fps=round(1 / plain, 1), armed_fps=round(1 / armed, 1), bytes_per_frame=3 * n)
    print(f"light-only ring from host memory, 10-bit 4:2:0: {1/plain:6.1f} frames/s   armed with h2y_stream_gamutcheck (2 sets) {1/armed:6.1f} frames/s",
          flush=True)
    ctx.close()
    print(json.dumps({"streambench_gamutcheck": res}), flush=True)


def deltae_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "frames_per_launch": h.DELTAE_FRAMES_PER_LAUNCH, "reps": reps, "ring_frames": nf,
           "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def codes(count, lo, hi):
        return torch.randint(lo, hi + 1, (count,), dtype=torch.int32, device="cuda").to(torch.int16)

    def noise(chroma):
        nc = n // 4 if chroma == 1 else n
        return torch.cat([codes(n, 64, 940), codes(nc, 64, 960), codes(nc, 64, 960)])

    def timed(calls):
        """every call of calls in turn, reps times after a warm-up: per call its kernel times in ms per frame"""
        out = [[] for _ in calls]
        for rep in range(reps + 1):
            for k, call in enumerate(calls):
                call()
                if rep:
                    out[k].append(ctx.last_kernel_ms()[0] / nb)
        return out

    def report(key, label, t, nbytes, variant):
        med = float(np.median(t))
        tbs = nbytes / (med * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(med * 1e3, 2), min_us=round(min(t) * 1e3, 2), max_us=round(max(t) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=variant)
        print(f"{label:30s} {nb} pairs per call: {med*1e3:7.2f} us/frame ({min(t)*1e3:.2f}..{max(t)*1e3:.2f})  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s  {variant}", flush=True)
        return med

    # 1. k_deltae beside k_codelight (on A), k_compare and k_ssim on the same 64 pairs, in turn.  Bytes: 4:2:0 -- 6 B/pixel read by
    # k_up444 and k_deltae's lumas, 8 B/pixel of scratch written and 8 read back, 22 in all; 4:4:4 -- 12 read.
    med = {}
    for name, chroma in (("420_10", 1), ("444_10", 3)):
        d = h.make_codelight_desc(w, hh, chroma, 10, 0, h.MATRIX_BT2020NC, 1)
        a = [noise(chroma) for _ in range(nb)]
        b = [torch.clamp(x + torch.randint(-2, 3, x.shape, dtype=torch.int16, device="cuda"), 0, 1023) for x in a]
        torch.cuda.synchronize()
        variants = {}
        note = lambda key: variants.setdefault(key, ctx.last_kernel_variant())
        t = timed([lambda: (ctx.deltae_batch(d, a, b), note("de")), lambda: (ctx.codelight_batch(d, a), note("cl")),
                   lambda: (ctx.compare_batch(w, hh, chroma, 0, a, b), note("cmp")), lambda: (ctx.ssim_batch(w, hh, chroma, 10, a, b), note("ssim"))])
        frame = n * (3 if chroma == 1 else 6)
        med[name] = report(f"k_deltae_{name}", f"k_deltae {name}", t[0], n * (22 if chroma == 1 else 12), variants["de"])
        m_cl = report(f"k_codelight_{name}", f"k_codelight {name} (A alone)", t[1], n * (11 if chroma == 1 else 6), variants["cl"])
        report(f"k_compare_{name}", f"k_compare {name}", t[2], 2 * frame, variants["cmp"])
        report(f"k_ssim_{name}", f"k_ssim {name}", t[3], 2 * frame, variants["ssim"])
        res[f"ratio_to_k_codelight_{name}"] = round(med[name] / m_cl, 3)
        print(f"k_deltae / k_codelight {name}: {med[name]/m_cl:5.3f} (four times the table transfers, twice the bytes)", flush=True)
        del a, b
        torch.cuda.empty_cache()
    share = 1.0 - med["444_10"] / med["420_10"]
    res["k_up444_share"] = round(share, 3)
    print(f"k_up444 share of the 4:2:0 time: {share*100:4.1f} %", flush=True)

    # 2. the compare-only ring from host memory, 10-bit 4:2:0, unarmed and armed for Delta E
    d = h.make_codelight_desc(w, hh, 1, 10, 0, h.MATRIX_BT2020NC, 1)
    host = noise(1).cpu().numpy().view(np.uint16)
    parts = [host[:n], host[n:n + n // 4], host[n + n // 4:]]
    ref = np.clip(host.astype(np.int32) + 1, 0, 1023).astype(np.uint16)

    def ring(armed):
        ctx.compare_stream_open(w, hh, h.CHROMA_420, 0, depth)
        if armed:
            ctx.stream_deltae(d, 1.0)
        inflight = 0
        t0 = time.perf_counter()

        def take():
            ctx.stream_output()
            ctx.stream_compare_result()
            if armed:
                ctx.stream_deltae_result()

        for _ in range(nf):
            slot = ctx.stream_input()
            for c in range(3):
                slot[c][:] = parts[c]
            ctx.stream_reference()[:] = ref
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                take()
                inflight -= 1
        while inflight:
            take()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    ring(False)  # warm-up
    ts = [(ring(False), ring(True)) for _ in range(3)]
    t_plain, t_armed = float(np.median([x[0] for x in ts])), float(np.median([x[1] for x in ts]))
    res["compare_only_ring"] = dict(unarmed_fps=round(1 / t_plain, 1), armed_fps=round(1 / t_armed, 1), unarmed_ms=round(t_plain * 1e3, 2),
                                    armed_ms=round(t_armed * 1e3, 2))
    print(f"compare-only ring from host memory, 10-bit 4:2:0: unarmed {1/t_plain:6.1f} frames/s   armed for Delta E {1/t_armed:6.1f} frames/s",
          flush=True)
    ctx.close()
    print(json.dumps({"streambench_deltae": res}), flush=True)


def linearize_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "frames_per_launch": h.api.LINEARIZE_FRAMES_PER_LAUNCH, "reps": reps,
           "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def codes(count, lo, hi):
        return torch.randint(lo, hi + 1, (count,), dtype=torch.int32, device="cuda").to(torch.int16)

    def noise(chroma, bits):
        s = 1 << (bits - 8)
        nc = n // 4 if chroma == 1 else n
        return torch.cat([codes(n, 16 * s, 235 * s), codes(nc, 16 * s, 240 * s), codes(nc, 16 * s, 240 * s)])

    def report(key, label, t, nbytes, variant):
        med = float(np.median(t))
        tbs = nbytes / (med * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(med * 1e3, 2), min_us=round(min(t) * 1e3, 2), max_us=round(max(t) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=variant)
        print(f"{label:34s} {nb} frames per call: {med*1e3:7.2f} us/frame ({min(t)*1e3:.2f}..{max(t)*1e3:.2f})  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s  {variant}", flush=True)
        return med

    # 1. k_linearize, k_codelight on the same frames, k_gamut on the planes just written, in turn
    outs = [[torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in range(nb)]
    for name, chroma, bits, matrix in (("420_10_noise", 1, 10, h.MATRIX_BT2020NC), ("444_10_noise", 3, 10, h.MATRIX_BT2020NC),
                                       ("444_16_gbr_noise", 3, 16, h.MATRIX_GBR)):
        d = h.make_codelight_desc(w, hh, chroma, bits, 0, matrix, 1)
        frames = [noise(chroma, bits) for _ in range(nb)]
        torch.cuda.synchronize()
        t = {"lin": [], "light": [], "gamut": []}
        variants = {}
        for rep in range(reps + 1):  # the first round warms up
            for key, call in (("lin", lambda: ctx.linearize_batch(d, frames, outs)), ("light", lambda: ctx.codelight_batch(d, frames)),
                              ("gamut", lambda: ctx.gamut_batch(w, hh, h.SAMPLE_F32, 9, 1, 1, outs))):
                call()
                variants[key] = ctx.last_kernel_variant()
                if rep:
                    t[key].append(ctx.last_kernel_ms()[0] / nb)
        m_lin = report(f"k_linearize_{name}", f"k_linearize {name}", t["lin"], n * (23 if chroma == 1 else 18), variants["lin"])
        m_light = report(f"k_codelight_{name}", f"k_codelight {name} (yardstick)", t["light"], n * (11 if chroma == 1 else 6), variants["light"])
        m_gamut = report(f"k_gamut_f32_{name}", f"k_gamut F32 in place (yardstick)", t["gamut"], 24 * n, variants["gamut"])
        yard = m_light + m_gamut * 18.0 / 24.0
        res[f"yardstick_{name}"] = dict(no_overlap_us_per_frame=round(yard * 1e3, 2), measured_over_yardstick=round(m_lin / yard, 3))
        print(f"k_linearize {name}: {m_lin*1e3:7.2f} us/frame against k_codelight + 18 B/pixel at k_gamut's rate = {yard*1e3:7.2f} us/frame "
              f"({m_lin/yard:5.3f} of it)", flush=True)
        del frames
        torch.cuda.empty_cache()

    # 2. the PQ code ring beside the .f32 ring fed the linearised planes
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, h.MATRIX_BT2020NC, 1)
    code = noise(1, 10)
    ctx.linearize_batch(cd, [code], outs[:1])
    planes = [t.cpu().numpy() for t in outs[0]]
    payload = code.cpu().numpy().view(np.uint8)
    del outs, code
    torch.cuda.empty_cache()
    d32 = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=1, stats=[(0, 1)] * 3)

    def ring(open_fn, fill):
        open_fn()
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            fill(ctx.stream_input())
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    def fill_code(slot):
        slot[0][:] = payload

    def fill_planes(slot):
        for c in range(3):
            slot[c][:] = planes[c]

    rings = (("pqcode", lambda: ctx.pqcode_stream_open(d32, cd, depth), fill_code), ("f32", lambda: ctx.stream_open(d32, depth), fill_planes))
    fps = {key: [] for key, _, _ in rings}
    for rep in range(4):  # the first round warms up
        for key, open_fn, fill in rings:
            dt = ring(open_fn, fill)
            if rep:
                fps[key].append(1 / dt)
    for key, bytes_up in (("pqcode", 3 * n), ("f32", 12 * n)):
        res[f"{key}_ring"] = dict(fps=round(float(np.median(fps[key])), 1), min_fps=round(min(fps[key]), 1), max_fps=round(max(fps[key]), 1),
                                  upload_bytes_per_frame=bytes_up)
        print(f"{key:7s} ring from host memory to PQ BT.2020nc 10-bit 4:2:0: {np.median(fps[key]):6.1f} frames/s "
              f"({min(fps[key]):.1f}..{max(fps[key]):.1f}), {bytes_up/1e6:5.1f} MB up per frame", flush=True)
    ctx.close()
    print(json.dumps({"streambench_linearize": res}), flush=True)


def hlgsrc_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    peak = 1000
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "frames_per_launch": h.api.LINEARIZE_FRAMES_PER_LAUNCH, "reps": reps,
           "ring_frames": nf, "ring_depth": depth, "peak": peak, "hbm_peak_tbs": 8.0}

    def codes(count, lo, hi):
        return torch.randint(lo, hi + 1, (count,), dtype=torch.int32, device="cuda").to(torch.int16)

    def noise(chroma, bits):
        s = 1 << (bits - 8)
        nc = n // 4 if chroma == 1 else n
        return torch.cat([codes(n, 16 * s, 235 * s), codes(nc, 16 * s, 240 * s), codes(nc, 16 * s, 240 * s)])

    def report(key, label, t, nbytes, variant):
        med = float(np.median(t))
        tbs = nbytes / (med * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(med * 1e3, 2), min_us=round(min(t) * 1e3, 2), max_us=round(max(t) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=variant)
        print(f"{label:34s} {nb} frames per call: {med*1e3:7.2f} us/frame ({min(t)*1e3:.2f}..{max(t)*1e3:.2f})  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s  {variant}", flush=True)
        return med

    # 1. k_hlg_linearize and k_linearize on the same frames, k_hlg in place on the planes just written, in turn
    outs = [[torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in range(nb)]
    for name, chroma, bits, matrix in (("420_10_noise", 1, 10, h.MATRIX_BT2020NC), ("444_10_noise", 3, 10, h.MATRIX_BT2020NC),
                                       ("444_16_gbr_noise", 3, 16, h.MATRIX_GBR)):
        d = h.make_codelight_desc(w, hh, chroma, bits, 0, matrix, 1)
        frames = [noise(chroma, bits) for _ in range(nb)]
        torch.cuda.synchronize()
        t = {"hlgsrc": [], "lin": [], "hlg": []}
        variants = {}
        for rep in range(reps + 1):  # the first round warms up
            for key, call in (("hlgsrc", lambda: ctx.hlg_linearize_batch(d, peak, frames, outs)), ("lin", lambda: ctx.linearize_batch(d, frames, outs)),
                              ("hlg", lambda: ctx.hlg_batch(w, hh, h.SAMPLE_F32, peak, 0, 10, 0, h.MATRIX_BT2020NC, outs))):
                call()
                variants[key] = ctx.last_kernel_variant()
                if rep:
                    t[key].append(ctx.last_kernel_ms()[0] / nb)
        nbytes = n * (23 if chroma == 1 else 18)
        m_src = report(f"k_hlg_linearize_{name}", f"k_hlg_linearize {name}", t["hlgsrc"], nbytes, variants["hlgsrc"])
        m_lin = report(f"k_linearize_{name}", f"k_linearize {name} (yardstick)", t["lin"], nbytes, variants["lin"])
        report(f"k_hlg_f32_{name}", "k_hlg F32 in place (yardstick)", t["hlg"], 24 * n, variants["hlg"])
        res[f"k_hlg_linearize_over_k_linearize_{name}"] = round(m_src / m_lin, 3)
        print(f"k_hlg_linearize / k_linearize {name}: {m_src/m_lin:5.3f}", flush=True)
        del frames
        torch.cuda.empty_cache()

    # 2. the HLG code ring beside the PQ code ring on the same code frames
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, h.MATRIX_BT2020NC, 1)
    payload = noise(1, 10).cpu().numpy().view(np.uint8)
    del outs
    torch.cuda.empty_cache()
    d32 = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=1, stats=[(0, 1)] * 3)

    def ring(open_fn):
        open_fn()
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            ctx.stream_input()[0][:] = payload
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    rings = (("hlgcode", lambda: ctx.hlgcode_stream_open(d32, cd, peak, depth)), ("pqcode", lambda: ctx.pqcode_stream_open(d32, cd, depth)))
    fps = {key: [] for key, _ in rings}
    for rep in range(reps + 1):  # the first round warms up
        for key, open_fn in rings:
            dt = ring(open_fn)
            if rep:
                fps[key].append(1 / dt)
    for key, _ in rings:
        res[f"{key}_ring"] = dict(fps=round(float(np.median(fps[key])), 1), min_fps=round(min(fps[key]), 1), max_fps=round(max(fps[key]), 1),
                                  upload_bytes_per_frame=3 * n)
        print(f"{key:7s} ring from host memory to PQ BT.2020nc 10-bit 4:2:0: {np.median(fps[key]):6.1f} frames/s "
              f"({min(fps[key]):.1f}..{max(fps[key]):.1f}), {3*n/1e6:5.1f} MB up per frame", flush=True)
    ctx.close()
    print(json.dumps({"streambench_hlgsrc": res}), flush=True)


def sdrsrc_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    white, peak = h.SDR_WHITE_DEFAULT, 1000
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "frames_per_launch": h.api.LINEARIZE_FRAMES_PER_LAUNCH, "reps": reps,
           "ring_frames": nf, "ring_depth": depth, "white": white, "hlg_peak": peak, "hbm_peak_tbs": 8.0}

    def codes(count, lo, hi):
        return torch.randint(lo, hi + 1, (count,), dtype=torch.int32, device="cuda").to(torch.int16)

    def noise(chroma, bits):
        s = 1 << (bits - 8)
        nc = n // 4 if chroma == 1 else n
        return torch.cat([codes(n, 16 * s, 235 * s), codes(nc, 16 * s, 240 * s), codes(nc, 16 * s, 240 * s)])

    def report(key, label, t, nbytes, variant):
        med = float(np.median(t))
        tbs = nbytes / (med * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(med * 1e3, 2), min_us=round(min(t) * 1e3, 2), max_us=round(max(t) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=variant)
        print(f"{label:38s} {nb} frames per call: {med*1e3:7.2f} us/frame ({min(t)*1e3:.2f}..{max(t)*1e3:.2f})  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s  {variant}", flush=True)
        return med

    # 1. k_sdr_linearize, k_linearize and k_hlg_linearize on the same frames, in turn
    outs = [[torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in range(nb)]
    for name, chroma, bits, matrix in (("420_10_noise", 1, 10, h.MATRIX_BT709), ("444_10_noise", 3, 10, h.MATRIX_BT709),
                                       ("444_16_gbr_noise", 3, 16, h.MATRIX_GBR)):
        d = h.make_codelight_desc(w, hh, chroma, bits, 0, matrix, 1)
        frames = [noise(chroma, bits) for _ in range(nb)]
        torch.cuda.synchronize()
        t = {"sdrsrc": [], "lin": [], "hlgsrc": []}
        variants = {}
        for rep in range(reps + 1):  # the first round warms up
            for key, call in (("sdrsrc", lambda: ctx.sdr_linearize_batch(d, white, frames, outs)), ("lin", lambda: ctx.linearize_batch(d, frames, outs)),
                              ("hlgsrc", lambda: ctx.hlg_linearize_batch(d, peak, frames, outs))):
                call()
                variants[key] = ctx.last_kernel_variant()
                if rep:
                    t[key].append(ctx.last_kernel_ms()[0] / nb)
        nbytes = n * (23 if chroma == 1 else 18)
        m_src = report(f"k_sdr_linearize_{name}", f"k_sdr_linearize {name}", t["sdrsrc"], nbytes, variants["sdrsrc"])
        m_lin = report(f"k_linearize_{name}", f"k_linearize {name} (yardstick)", t["lin"], nbytes, variants["lin"])
        report(f"k_hlg_linearize_{name}", f"k_hlg_linearize {name} (yardstick)", t["hlgsrc"], nbytes, variants["hlgsrc"])
        res[f"k_sdr_linearize_over_k_linearize_{name}"] = round(m_src / m_lin, 3)
        print(f"k_sdr_linearize / k_linearize {name}: {m_src/m_lin:5.3f}", flush=True)
        del frames
        torch.cuda.empty_cache()

    # 2. the SDR code ring beside the PQ code ring on the same code frames
    cd = h.make_codelight_desc(w, hh, 1, 10, 0, h.MATRIX_BT709, 1)
    payload = noise(1, 10).cpu().numpy().view(np.uint8)
    del outs
    torch.cuda.empty_cache()
    d32 = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=1, stats=[(0, 1)] * 3)

    def ring(open_fn):
        open_fn()
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            ctx.stream_input()[0][:] = payload
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    rings = (("sdrcode", lambda: ctx.sdrcode_stream_open(d32, cd, white, depth)), ("pqcode", lambda: ctx.pqcode_stream_open(d32, cd, depth)))
    fps = {key: [] for key, _ in rings}
    for rep in range(reps + 1):  # the first round warms up
        for key, open_fn in rings:
            dt = ring(open_fn)
            if rep:
                fps[key].append(1 / dt)
    for key, _ in rings:
        res[f"{key}_ring"] = dict(fps=round(float(np.median(fps[key])), 1), min_fps=round(min(fps[key]), 1), max_fps=round(max(fps[key]), 1),
                                  upload_bytes_per_frame=3 * n)
        print(f"{key:7s} ring from host memory to PQ BT.2020nc 10-bit 4:2:0: {np.median(fps[key]):6.1f} frames/s "
              f"({min(fps[key]):.1f}..{max(fps[key]):.1f}), {3*n/1e6:5.1f} MB up per frame", flush=True)
    ctx.close()
    print(json.dumps({"streambench_sdrsrc": res}), flush=True)


def sigsrc_main():
    import json

    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from cube_files import random_nodes, write_cube
    from tiff_files import write_tiff

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(33)
    ctx = h.Context(0)
    lut = h.Lut3d(write_cube(random_nodes(rng, 17, 0.0, 1.0), (0, 0, 0), (1, 1, 1)))
    res = {"width": w, "height": hh, "frames_per_call": nb, "frames_per_launch": h.api.LINEARIZE_FRAMES_PER_LAUNCH, "reps": reps,
           "ring_frames": nf, "ring_depth": depth, "lut_nodes": 17, "hbm_peak_tbs": 8.0}

    def codes(count, lo, hi):
        return torch.randint(lo, hi + 1, (count,), dtype=torch.int32, device="cuda").to(torch.int16)

    def noise(chroma, bits):
        s = 1 << (bits - 8)
        nc = n // 4 if chroma == 1 else n
        return torch.cat([codes(n, 16 * s, 235 * s), codes(nc, 16 * s, 240 * s), codes(nc, 16 * s, 240 * s)])

    def report(key, label, t, nbytes, variant):
        med = float(np.median(t))
        tbs = nbytes / (med * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(med * 1e3, 2), min_us=round(min(t) * 1e3, 2), max_us=round(max(t) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=variant)
        print(f"{label:38s} {nb} frames per call: {med*1e3:7.2f} us/frame ({min(t)*1e3:.2f}..{max(t)*1e3:.2f})  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s  {variant}", flush=True)
        return med

    # 1. k_code_signal on three kinds of frames, k_linearize, k_tiff_decode and k_lut3d (signal mode), in turn
    outs = [[torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in range(nb)]
    shapes = (("420_10_noise", 1, 10, h.MATRIX_BT2020NC), ("444_10_noise", 3, 10, h.MATRIX_BT2020NC), ("444_16_gbr_noise", 3, 16, h.MATRIX_GBR))
    descs = {name: h.make_codelight_desc(w, hh, chroma, bits, 0, matrix, 1) for name, chroma, bits, matrix in shapes}
    frames = {name: [noise(chroma, bits) for _ in range(nb)] for name, chroma, bits, _ in shapes}
    tdata = write_tiff(rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16))
    tinfo, rows = h.parse_tiff(tdata)
    tpay = np.frombuffer(b"".join(tdata[int(o):int(o) + int(tinfo.row_bytes)] for o in rows), np.uint8)
    pays = [torch.from_numpy(tpay.copy()).cuda() for _ in range(nb)]
    touts = [[torch.empty(n, dtype=torch.int16, device="cuda") for _ in range(3)] for _ in range(nb)]
    torch.cuda.synchronize()
    calls = [(f"sig_{name}", (lambda name=name: ctx.code_signal_batch(descs[name], frames[name], outs))) for name, _, _, _ in shapes]
    calls += [("lut3d", lambda: ctx.lut3d_batch(w, hh, h.SAMPLE_F32, lut, 1, 1, 10, 0, h.MATRIX_BT2020NC, outs)),  # on the signal just written
              ("lin", lambda: ctx.linearize_batch(descs["444_10_noise"], frames["444_10_noise"], outs)),
              ("tiff", lambda: ctx.tiff_decode_batch(tinfo, 0, pays, touts))]
    t = {key: [] for key, _ in calls}
    variants = {}
    for rep in range(reps + 1):  # the first round warms up
        for key, call in calls:
            call()
            variants[key] = ctx.last_kernel_variant()
            if rep:
                t[key].append(ctx.last_kernel_ms()[0] / nb)
    med = {}
    for name, chroma, _, _ in shapes:
        med[name] = report(f"k_code_signal_{name}", f"k_code_signal {name}", t[f"sig_{name}"], n * (23 if chroma == 1 else 18), variants[f"sig_{name}"])
    m_tiff = report("k_tiff_decode", "k_tiff_decode (yardstick)", t["tiff"], 12 * n, variants["tiff"])
    report("k_linearize_444_10_noise", "k_linearize 444_10_noise", t["lin"], 18 * n, variants["lin"])
    report("k_lut3d_f32_signal", "k_lut3d F32 tetrahedral signal", t["lut3d"], 24 * n, variants["lut3d"])
    for name in ("444_10_noise", "444_16_gbr_noise"):
        res[f"k_code_signal_over_k_tiff_decode_{name}"] = round(med[name] / m_tiff, 3)
        print(f"k_code_signal / k_tiff_decode {name}: {med[name]/m_tiff:5.3f}", flush=True)

    # 2. the signal code ring beside the PQ code ring armed with the same table in signal mode, on the same code frames
    cd = descs["420_10_noise"]
    payload = frames["420_10_noise"][0].cpu().numpy().view(np.uint8)
    del outs, frames, pays, touts
    torch.cuda.empty_cache()
    d32 = h.make_desc(w, hh, dst_depth=10, src_transfer=8, dst_transfer=8, dst_matrix=h.MATRIX_BT2020NC, resampler=1, stats=[(0, 1)] * 3)

    def ring(open_fn):
        open_fn()
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            ctx.stream_input()[0][:] = payload
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    def open_pq():
        ctx.pqcode_stream_open(d32, cd, depth)
        ctx.stream_lut3d(lut, 1, 1)

    rings = (("sigcode", lambda: ctx.sigcode_stream_open(d32, cd, lut, 1, depth)), ("pqcode", open_pq))
    fps = {key: [] for key, _ in rings}
    for rep in range(reps + 1):  # the first round warms up
        for key, open_fn in rings:
            dt = ring(open_fn)
            if rep:
                fps[key].append(1 / dt)
    for key, _ in rings:
        res[f"{key}_ring"] = dict(fps=round(float(np.median(fps[key])), 1), min_fps=round(min(fps[key]), 1), max_fps=round(max(fps[key]), 1),
                                  upload_bytes_per_frame=3 * n)
        print(f"{key:7s} ring with a signal-mode LUT, host memory to BT.2020nc 10-bit 4:2:0: {np.median(fps[key]):6.1f} frames/s "
              f"({min(fps[key]):.1f}..{max(fps[key]):.1f}), {3*n/1e6:5.1f} MB up per frame", flush=True)
    ctx.close()
    print(json.dumps({"streambench_sigsrc": res}), flush=True)


def scale_main():
    import json

    import torch

    nb, reps = 64, 5
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(23)
    ctx = h.Context(0)
    res = {"frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    # 1. the kernel over 64 distinct frames on the device
    cases = [("4k_to_1080p", 3840, 2160, 1920, 1080, h.CHROMA_420, 10, 3), ("4k_to_720p", 3840, 2160, 1280, 720, h.CHROMA_420, 10, 3),
             ("1080p_to_4k", 1920, 1080, 3840, 2160, h.CHROMA_420, 10, 3), ("4k_to_1080p_444_16bit_a4", 3840, 2160, 1920, 1080, h.CHROMA_444, 16, 4)]
    for name, sw, sh, dw, dh, chroma, bits, a in cases:
        sb, db = h.scale_frame_bytes(sw, sh, chroma), h.scale_frame_bytes(dw, dh, chroma)
        hi = 1 << min(bits, 15)  # int16 storage: codes below 2^15 (the kernel's time does not depend on the values)
        src = [torch.randint(0, hi, (sb // 2,), dtype=torch.int16, device="cuda") for _ in range(nb)]
        dst = [torch.empty(db // 2, dtype=torch.int16, device="cuda") for _ in range(nb)]
        torch.cuda.synchronize()
        ks = []
        for rep in range(reps + 1):  # rep 0 warms up
            ctx.scale_batch(sw, sh, dw, dh, chroma, bits, 0, 0, a, src, dst)
            if rep:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        tbs = (sb + db) / (k_ms * 1e-3) / 1e12
        res[name] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), min_us=round(min(ks) * 1e3, 2), max_us=round(max(ks) * 1e3, 2),
                         bytes_per_frame=sb + db, kernel_tbs=round(tbs, 3), hbm_peak_fraction=round(tbs / 8.0, 4),
                         variant=ctx.last_kernel_variant())
        print(f"k_scale {name:26s} {nb} frames per call: {k_ms*1e3:7.2f} us/frame ({min(ks)*1e3:.2f}..{max(ks)*1e3:.2f})  "
              f"{(sb+db)/1e6:6.1f} MB/frame  {tbs:5.3f} TB/s = {tbs/8.0*100:5.2f} % of 8 TB/s", flush=True)
        del src, dst
        torch.cuda.empty_cache()

    def ring(open_fn, fill, arm=None):
        open_fn()
        if arm:
            arm()
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            fill(ctx.stream_input())
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    # 2. the forward ring: 16-bit G,B,R -> BT.2020nc 10-bit 4:2:0 box, unarmed and armed to 1080p
    w, hh = 3840, 2160
    n, nc = w * hh, (w // 2) * (hh // 2)
    planes = [rng.integers(0, 65536, n, dtype=np.uint16) for _ in range(3)]
    d = h.make_desc(w, hh, sample=h.SAMPLE_U16, src_depth=16, dst_depth=10, src_transfer=1, dst_transfer=1, src_primaries=1,
                    dst_primaries=1, dst_matrix=h.MATRIX_BT2020NC, resampler=0)
    yuv = ctx.convert_frame(d, planes)

    def fill_planes(slot):
        for c in range(3):
            slot[c][:] = planes[c]

    def open_fwd():
        ctx.stream_open(d, depth)

    ring(open_fwd, fill_planes)  # warm-up
    t_plain = ring(open_fwd, fill_planes)
    t_armed = ring(open_fwd, fill_planes, lambda: ctx.stream_scale(1920, 1080, 3))
    res["forward_ring"] = dict(unarmed_fps=round(1 / t_plain, 1), armed_fps=round(1 / t_armed, 1), unarmed_ms=round(t_plain * 1e3, 2),
                               armed_ms=round(t_armed * 1e3, 2))
    print(f"forward ring from host memory: unarmed {1/t_plain:6.1f} frames/s   armed with h2y_stream_scale to 1080p {1/t_armed:6.1f} frames/s",
          flush=True)

    # 3. the scale-only ring
    yuv_planes = [yuv[:n], yuv[n:n + nc], yuv[n + nc:]]

    def fill_yuv(slot):
        for c in range(3):
            slot[c][:] = yuv_planes[c]

    def open_scale():
        ctx.scale_stream_open(w, hh, h.CHROMA_420, 10, 0, 0, 1920, 1080, 3, depth)

    ring(open_scale, fill_yuv)
    t_only = ring(open_scale, fill_yuv)
    res["scale_only_ring"] = dict(fps=round(1 / t_only, 1), ms=round(t_only * 1e3, 2))
    print(f"scale-only ring from host memory: {1/t_only:6.1f} frames/s ({t_only*1e3:6.2f} ms/frame)", flush=True)
    ctx.close()
    print(json.dumps({"streambench_scale": res}), flush=True)


def dither_main():
    import json

    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from tiff_files import write_tiff

    w, hh, nb, reps = 3840, 2160, 64, 5
    n, nc = w * hh, (w // 2) * (hh // 2)
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(31)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def timed(key, label, nbytes, call):
        ks = []
        for r in range(reps + 1):  # the first call warms up
            call()
            if r:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        tbs = nbytes / (k_ms * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), min_us=round(min(ks) * 1e3, 2), max_us=round(max(ks) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"{label:34s} {nb} frames per call: {k_ms*1e3:7.2f} us/frame ({min(ks)*1e3:.2f}..{max(ks)*1e3:.2f})  {nbytes/1e6:6.1f} MB/frame  "
              f"{tbs:5.2f} TB/s = {tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)

    # 1. k_dither over 64 distinct frames on the device
    for key, chroma, D, mode in (("k_dither_16_10_420_ordered", h.CHROMA_420, 10, 1), ("k_dither_16_10_420_noise", h.CHROMA_420, 10, 2),
                                 ("k_dither_16_8_420_ordered", h.CHROMA_420, 8, 1), ("k_dither_16_10_444_ordered", h.CHROMA_444, 10, 1)):
        words = n + 2 * (nc if chroma == h.CHROMA_420 else n)
        src = [torch.randint(-32768, 32768, (words,), dtype=torch.int16, device="cuda") for _ in range(nb)]
        dst = [torch.empty(words, dtype=torch.int16, device="cuda") for _ in range(nb)]
        torch.cuda.synchronize()
        timed(key, key.replace("_", " ", 1), 4 * words, lambda: ctx.dither_batch(w, hh, chroma, 16, D, 0, 0, mode, 1, 0, 0, src, dst))
        if key == "k_dither_16_10_420_ordered":
            timed(key + "_in_place", "k dither 16_10_420_ordered in place", 4 * words, lambda: ctx.dither_batch(w, hh, chroma, 16, D, 0, 0, mode, 1, 0, 0, src))
        del src, dst
        torch.cuda.empty_cache()

    # 2. the yardsticks
    total = n + 2 * nc
    a = [torch.randint(0, 1024, (total,), dtype=torch.int16, device="cuda") for _ in range(nb)]
    b = [x + torch.randint(-2, 3, (total,), dtype=torch.int16, device="cuda") for x in a]
    torch.cuda.synchronize()
    timed("k_compare", "k_compare 4:2:0", 4 * total, lambda: ctx.compare_batch(w, hh, h.CHROMA_420, 0, a, b))
    del a, b
    torch.cuda.empty_cache()
    tdata = write_tiff(rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16))
    tinfo, rows = h.parse_tiff(tdata)
    tpay = np.frombuffer(b"".join(tdata[int(o):int(o) + int(tinfo.row_bytes)] for o in rows), np.uint8)
    pays = [torch.from_numpy(tpay.copy()).cuda() for _ in range(nb)]
    outs = [[torch.empty(n, dtype=torch.int16, device="cuda") for _ in range(3)] for _ in range(nb)]
    torch.cuda.synchronize()
    timed("k_tiff_decode", "k_tiff_decode", 12 * n, lambda: ctx.tiff_decode_batch(tinfo, 0, pays, outs))
    del pays, outs
    torch.cuda.empty_cache()
    for k in ("k_dither_16_10_420_ordered", "k_dither_16_10_420_noise", "k_dither_16_8_420_ordered", "k_dither_16_10_444_ordered"):
        res[k]["of_k_compare_rate"] = round(res[k]["kernel_tbs"] / res["k_compare"]["kernel_tbs"], 3)

    # 3. the conversion at 10 bits against the conversion at 16 bits and the reduction, on device-resident frames
    d10 = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, resampler=1)
    d16 = h.make_desc(w, hh, dst_depth=16, dst_matrix=h.MATRIX_BT2020NC, resampler=1)
    frames = [[torch.rand(n, device="cuda") for _ in range(3)] for _ in range(nb)]
    for fr in frames:
        for pl in fr:
            pl[0], pl[1] = 0.0, 1.0  # floor 0, ceiling 1
    outs = [torch.empty(total, dtype=torch.int16, device="cuda") for _ in range(nb)]
    torch.cuda.synchronize()
    variants = {}

    def conv10():
        t0 = time.perf_counter()
        ctx.convert_batch(d10, frames, outs)  # synchronous: every frame final on return
        variants["convert_10"] = ctx.last_kernel_variant()
        return (time.perf_counter() - t0) * 1e6 / nb

    def conv16_dither():
        t0 = time.perf_counter()
        ctx.convert_batch(d16, frames, outs)
        variants["convert_16"] = ctx.last_kernel_variant()
        t1 = time.perf_counter()
        ctx.dither_batch(w, hh, h.CHROMA_420, 16, 10, 0, 0, 1, 0, 0, 0, outs)
        return (time.perf_counter() - t0) * 1e6 / nb, (t1 - t0) * 1e6 / nb

    conv10(), conv16_dither()  # warm-up
    t10, t16, t16c = [], [], []
    for _ in range(reps):
        t10.append(conv10())
        both, conv = conv16_dither()
        t16.append(both)
        t16c.append(conv)
    m10, m16, m16c = float(np.median(t10)), float(np.median(t16)), float(np.median(t16c))
    res["convert_batch_c2_fir"] = dict(at_10_us_per_frame=round(m10, 2), at_10_min=round(min(t10), 2), at_10_max=round(max(t10), 2),
                                       at_16_plus_dither_us_per_frame=round(m16, 2), at_16_plus_dither_min=round(min(t16), 2),
                                       at_16_plus_dither_max=round(max(t16), 2), at_16_conversion_alone_us_per_frame=round(m16c, 2),
                                       ratio=round(m16 / m10, 3), **variants)
    print(f"h2y_convert_batch C2 FIR, wall: 10-bit {m10:7.2f} us/frame ({min(t10):.2f}..{max(t10):.2f}) [{variants['convert_10']}]", flush=True)
    print(f"  16-bit + h2y_dither_batch to 10: {m16:7.2f} us/frame ({min(t16):.2f}..{max(t16):.2f}), the conversion alone {m16c:7.2f} "
          f"[{variants['convert_16']}]  ratio {m16/m10:.3f}", flush=True)
    del frames, outs
    torch.cuda.empty_cache()

    # 4. the .f32 ring from host memory
    planes = [rng.random(n, dtype=np.float32) for _ in range(3)]

    def ring(d, arm):
        ctx.stream_open(d, depth)
        if arm:
            ctx.stream_dither(10, 1, 0, 0, 0)
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            slot = ctx.stream_input()
            for c in range(3):
                slot[c][:] = planes[c]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    ring(d16, False)  # warm-up
    runs = {"unarmed_16": [], "armed_16_to_10": [], "unarmed_10": []}
    for _ in range(3):
        runs["unarmed_16"].append(ring(d16, False))
        runs["armed_16_to_10"].append(ring(d16, True))
        runs["unarmed_10"].append(ring(d10, False))
    res["f32_ring"] = {k: dict(fps=round(1 / float(np.median(v)), 1), ms=[round(x * 1e3, 2) for x in v]) for k, v in runs.items()}
    print("f32 ring from host memory: " + "   ".join(f"{k} {1/float(np.median(v)):6.1f} frames/s" for k, v in runs.items()), flush=True)
    ctx.close()
    print(json.dumps({"streambench_dither": res}), flush=True)


def pack_main():
    import json

    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from tiff_files import write_tiff

    w, hh, nb, reps = 3840, 2160, 64, 5
    n, nc = w * hh, (w // 2) * (hh // 2)
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(41)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def timed(key, label, nbytes, call):
        ks = []
        for r in range(reps + 1):  # the first call warms up
            call()
            if r:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        tbs = nbytes / (k_ms * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), min_us=round(min(ks) * 1e3, 2), max_us=round(max(ks) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"{label:34s} {nb} frames per call: {k_ms*1e3:7.2f} us/frame ({min(ks)*1e3:.2f}..{max(ks)*1e3:.2f})  {nbytes/1e6:6.1f} MB/frame  "
              f"{tbs:5.2f} TB/s = {tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)

    # 1. k_pack and k_unpack over 64 distinct frames on the device
    for name, packing, chroma, D in (("planar8_420", h.PACK_PLANAR8, h.CHROMA_420, 8), ("planar8_444", h.PACK_PLANAR8, h.CHROMA_444, 8),
                                     ("nv12", h.PACK_NV12, h.CHROMA_420, 8), ("p010", h.PACK_P010, h.CHROMA_420, 10)):
        words = n + 2 * (nc if chroma == h.CHROMA_420 else n)
        pbytes = h.pack_frame_bytes(w, hh, chroma, packing)
        planar = [torch.randint(0, 1 << D, (words,), dtype=torch.int16, device="cuda") for _ in range(nb)]
        packed = [torch.empty(pbytes, dtype=torch.uint8, device="cuda") for _ in range(nb)]
        torch.cuda.synchronize()
        timed("k_pack_" + name, "k_pack " + name, 2 * words + pbytes, lambda: ctx.pack_batch(w, hh, chroma, D, packing, planar, packed))
        timed("k_unpack_" + name, "k_unpack " + name, 2 * words + pbytes, lambda: ctx.unpack_batch(w, hh, chroma, D, packing, packed, planar))
        del planar, packed
        torch.cuda.empty_cache()
    # the narrow path: 3838 x 2158 has w h = 8282404, no multiple of 16, so the chroma block (a third of the samples) takes one
    # element an access where the luma plane still takes vectors
    w2, h2 = 3838, 2158
    for name, packing, D in (("nv12", h.PACK_NV12, 8), ("p010", h.PACK_P010, 10)):
        words = w2 * h2 + 2 * (w2 // 2) * (h2 // 2)
        pbytes = h.pack_frame_bytes(w2, h2, h.CHROMA_420, packing)
        planar = [torch.randint(0, 1 << D, (words + 8,), dtype=torch.int16, device="cuda") for _ in range(nb)]
        packed = [torch.empty(pbytes + 16, dtype=torch.uint8, device="cuda") for _ in range(nb)]
        torch.cuda.synchronize()
        timed(f"k_pack_{name}_3838x2158", f"k_pack {name} 3838x2158 (narrow chroma)", 2 * words + pbytes,
              lambda: ctx.pack_batch(w2, h2, h.CHROMA_420, D, packing, planar, packed))
        timed(f"k_unpack_{name}_3838x2158", f"k_unpack {name} 3838x2158 (narrow chroma)", 2 * words + pbytes,
              lambda: ctx.unpack_batch(w2, h2, h.CHROMA_420, D, packing, packed, planar))
        del planar, packed
        torch.cuda.empty_cache()

    # 2. the yardsticks
    words = n + 2 * nc
    src = [torch.randint(-32768, 32768, (words,), dtype=torch.int16, device="cuda") for _ in range(nb)]
    dst = [torch.empty(words, dtype=torch.int16, device="cuda") for _ in range(nb)]
    torch.cuda.synchronize()
    timed("k_dither_16_8_420_ordered", "k_dither 16_8_420_ordered", 4 * words, lambda: ctx.dither_batch(w, hh, h.CHROMA_420, 16, 8, 0, 0, 1, 1, 0, 0, src, dst))
    del src, dst
    torch.cuda.empty_cache()
    tdata = write_tiff(rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16))
    tinfo, rows = h.parse_tiff(tdata)
    tpay = np.frombuffer(b"".join(tdata[int(o):int(o) + int(tinfo.row_bytes)] for o in rows), np.uint8)
    pays = [torch.from_numpy(tpay.copy()).cuda() for _ in range(nb)]
    outs = [[torch.empty(n, dtype=torch.int16, device="cuda") for _ in range(3)] for _ in range(nb)]
    torch.cuda.synchronize()
    timed("k_tiff_decode", "k_tiff_decode", 12 * n, lambda: ctx.tiff_decode_batch(tinfo, 0, pays, outs))
    del pays, outs
    torch.cuda.empty_cache()

    def drive(fill):
        """nf frames through the ring ctx has open; seconds a frame"""
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            fill(ctx.stream_input())
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    # 3. the .f32 ring from host memory, dithered to 8 bits
    d16 = h.make_desc(w, hh, dst_depth=16, dst_transfer=1, dst_matrix=h.MATRIX_BT709, resampler=1)
    planes = [rng.random(n, dtype=np.float32) for _ in range(3)]

    def fill_planes(slot):
        for c in range(3):
            slot[c][:] = planes[c]

    def f32_ring(pack):
        ctx.stream_open(d16, depth)
        ctx.stream_dither(8, 1, 0, 0, 0)
        if pack:
            ctx.stream_pack(h.PACK_PLANAR8)
        return drive(fill_planes)

    f32_ring(False)  # warm-up
    runs = {"dither_to_8": [], "dither_to_8_pack_planar8": []}
    for _ in range(3):
        runs["dither_to_8"].append(f32_ring(False))
        runs["dither_to_8_pack_planar8"].append(f32_ring(True))
    res["f32_ring"] = {k: dict(fps=round(1 / float(np.median(v)), 1), ms=[round(x * 1e3, 2) for x in v]) for k, v in runs.items()}
    print("f32 ring from host memory: " + "   ".join(f"{k} {1/float(np.median(v)):6.1f} frames/s" for k, v in runs.items()), flush=True)

    # 4. the compare-only ring at 8 bits
    a16 = rng.integers(16, 236, words, dtype=np.uint16)
    b16 = np.clip(a16.astype(np.int32) + rng.integers(-2, 3, words), 0, 255).astype(np.uint16)
    a8, b8 = a16.astype(np.uint8), b16.astype(np.uint8)

    def cmp_ring(unpack):
        ctx.compare_stream_open(w, hh, h.CHROMA_420, 0, depth)
        if unpack:
            ctx.stream_unpack(h.PACK_PLANAR8)

        def fill(slot):
            if unpack:
                slot[0][:] = a8
                ctx.stream_reference()[:] = b8
            else:
                slot[0][:], slot[1][:], slot[2][:] = a16[:n], a16[n:n + nc], a16[n + nc:]
                ctx.stream_reference()[:] = b16
        return drive(fill)

    cmp_ring(False)  # warm-up
    runs = {"planar16": [], "unpack_planar8": []}
    for _ in range(3):
        runs["planar16"].append(cmp_ring(False))
        runs["unpack_planar8"].append(cmp_ring(True))
    res["compare_only_ring_8bit"] = {k: dict(fps=round(1 / float(np.median(v)), 1), ms=[round(x * 1e3, 2) for x in v]) for k, v in runs.items()}
    print("compare-only ring at 8 bits from host memory: " + "   ".join(f"{k} {1/float(np.median(v)):6.1f} frames/s" for k, v in runs.items()), flush=True)
    ctx.close()
    print(json.dumps({"streambench_pack": res}), flush=True)


def gamut_main():
    import json

    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from dpx_files import pack_pixels, write_dpx
    from exr_files import HALF, NONE, smooth_half, write_exr
    from tiff_files import write_tiff

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    rng = np.random.default_rng(29)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def timed(key, label, nbytes, call):
        ks = []
        for r in range(reps + 1):  # the first call warms up
            call()
            if r:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        tbs = nbytes / (k_ms * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), min_us=round(min(ks) * 1e3, 2), max_us=round(max(ks) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"{label:32s} {nb} frames per call: {k_ms*1e3:7.2f} us/frame ({min(ks)*1e3:.2f}..{max(ks)*1e3:.2f})  {nbytes/1e6:6.1f} MB/frame  "
              f"{tbs:5.2f} TB/s = {tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)

    # 1. k_gamut over 64 distinct frames on the device
    for name, sample, dt in (("f32", h.SAMPLE_F32, torch.float32), ("f16", h.SAMPLE_F16, torch.float16)):
        src = [[torch.rand(n, device="cuda").to(dt) for _ in range(3)] for _ in range(nb)]
        dst = [[torch.empty(n, dtype=dt, device="cuda") for _ in range(3)] for _ in range(nb)]
        torch.cuda.synchronize()
        nbytes = 2 * 3 * n * (4 if sample == h.SAMPLE_F32 else 2)
        timed(f"k_gamut_{name}_out_of_place", f"k_gamut {name} out of place", nbytes, lambda: ctx.gamut_batch(w, hh, sample, 1, 9, 1, src, dst))
        del dst
        timed(f"k_gamut_{name}_in_place", f"k_gamut {name} in place", nbytes, lambda: ctx.gamut_batch(w, hh, sample, 1, 9, 1, src))
        del src
        torch.cuda.empty_cache()

    # 2. the yardstick: the decode kernels of the TIFF and DPX rings, on 64 payloads
    tdata = write_tiff(rng.integers(0, 65536, (hh, w, 3), dtype=np.uint16))
    tinfo, rows = h.parse_tiff(tdata)
    tpay = np.frombuffer(b"".join(tdata[int(o):int(o) + int(tinfo.row_bytes)] for o in rows), np.uint8)
    pays = [torch.from_numpy(tpay.copy()).cuda() for _ in range(nb)]
    outs = [[torch.empty(n, dtype=torch.int16, device="cuda") for _ in range(3)] for _ in range(nb)]
    torch.cuda.synchronize()
    timed("k_tiff_decode", "k_tiff_decode", 12 * n, lambda: ctx.tiff_decode_batch(tinfo, 0, pays, outs))
    del pays, outs
    torch.cuda.empty_cache()
    rgb = [rng.random(n, dtype=np.float32) for _ in range(3)]
    for name, bits in (("10", 10), ("float", 32)):
        vals = [c.view(np.uint32) for c in rgb] if bits == 32 else [rng.integers(0, 1024, n, dtype=np.uint32) for _ in range(3)]
        data = write_dpx(w, hh, bits, pack_pixels(*vals, bits))
        info = h.parse_dpx(data[:2048], len(data))
        pay = np.frombuffer(data, np.uint8, count=info.payload_bytes, offset=info.data_offset)
        pays = [torch.from_numpy(pay.copy()).cuda() for _ in range(nb)]
        outs = [[torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in range(nb)]
        torch.cuda.synchronize()
        timed(f"k_dpx_decode_{name}", f"k_dpx_decode {name}", int(info.payload_bytes) + 12 * n, lambda: ctx.dpx_decode_batch(info, pays, outs))
        del pays, outs
        torch.cuda.empty_cache()

    # 3. the .f32 ring and the EXR ring from host memory, unarmed and armed
    def ring(open_fn, fill, arm):
        open_fn()
        if arm:
            ctx.stream_gamut(1, 9, 1)
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            fill(ctx.stream_input())
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    def both(key, open_fn, fill):
        ring(open_fn, fill, False)  # warm-up
        t_plain, t_armed = ring(open_fn, fill, False), ring(open_fn, fill, True)
        res[key] = dict(unarmed_fps=round(1 / t_plain, 1), armed_fps=round(1 / t_armed, 1), armed_share=round(t_plain / t_armed, 3))
        print(f"{key:12s} ring from host memory: unarmed {1/t_plain:6.1f} frames/s   armed {1/t_armed:6.1f} frames/s "
              f"({t_plain/t_armed*100:5.1f} %)", flush=True)

    d32 = h.make_desc(w, hh, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, src_primaries=1, dst_primaries=9, resampler=1)
    planes = [rgb[1], rgb[2], rgb[0]]

    def fill_planes(slot):
        for c in range(3):
            slot[c][:] = planes[c]

    both("f32", lambda: ctx.stream_open(d32, depth), fill_planes)
    edata, _ = write_exr({name: (HALF, smooth_half(hh, w, 101 * k)) for k, name in enumerate("RGB")}, NONE)
    ebuf = np.frombuffer(edata, np.uint8)
    einfo, echunks = h.parse_exr(ebuf)
    dh = h.make_desc(w, hh, sample=h.SAMPLE_F16, dst_depth=10, dst_matrix=h.MATRIX_BT2020NC, src_primaries=1, dst_primaries=9, resampler=1)
    both("exr", lambda: ctx.exr_stream_open(dh, einfo, depth), lambda slot: h.exr_unpack(einfo, echunks, ebuf, slot[0]))
    ctx.close()
    print(json.dumps({"streambench_gamut": res}), flush=True)


def tonemap_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def timed(key, label, nbytes, call):
        ks = []
        for r in range(reps + 1):  # the first call warms up
            call()
            if r:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        tbs = nbytes / (k_ms * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), min_us=round(min(ks) * 1e3, 2), max_us=round(max(ks) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"{label:32s} {nb} frames per call: {k_ms*1e3:7.2f} us/frame ({min(ks)*1e3:.2f}..{max(ks)*1e3:.2f})  {nbytes/1e6:6.1f} MB/frame  "
              f"{tbs:5.2f} TB/s = {tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)

    # 1. k_tonemap and k_gamut over the same 64 distinct frames on the device; out of place first, so that both kernels read the
    # light as it was made, then in place (k_gamut last: what the curve left is light all the same)
    for name, sample, dt in (("f32", h.SAMPLE_F32, torch.float32), ("f16", h.SAMPLE_F16, torch.float16)):
        src = [[(torch.rand(n, device="cuda") ** 3 * 0.5).to(dt) for _ in range(3)] for _ in range(nb)]
        dst = [[torch.empty(n, dtype=dt, device="cuda") for _ in range(3)] for _ in range(nb)]
        torch.cuda.synchronize()
        nbytes = 2 * 3 * n * (4 if sample == h.SAMPLE_F32 else 2)
        timed(f"k_tonemap_{name}_out_of_place", f"k_tonemap {name} out of place", nbytes, lambda: ctx.tonemap_batch(w, hh, sample, 1000, 100, 1, src, dst))
        timed(f"k_gamut_{name}_out_of_place", f"k_gamut {name} out of place", nbytes, lambda: ctx.gamut_batch(w, hh, sample, 9, 1, 1, src, dst))
        del dst
        timed(f"k_tonemap_{name}_in_place", f"k_tonemap {name} in place", nbytes, lambda: ctx.tonemap_batch(w, hh, sample, 1000, 100, 1, src))
        timed(f"k_gamut_{name}_in_place", f"k_gamut {name} in place", nbytes, lambda: ctx.gamut_batch(w, hh, sample, 9, 1, 1, src))
        del src
        torch.cuda.empty_cache()

    # 2. the .f32 ring from host memory, unarmed and armed
    planes = [(np.random.default_rng(31 + c).random(n, dtype=np.float32) ** 3 * np.float32(0.5)) for c in range(3)]
    d32 = h.make_desc(w, hh, dst_depth=10, dst_transfer=1, dst_matrix=h.MATRIX_BT709, src_primaries=9, dst_primaries=1, resampler=1,
                      stats=[(0, 1)] * 3)

    def ring(arm):
        ctx.stream_open(d32, depth)
        if arm:
            ctx.stream_tonemap(1000, 100, 1)
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            slot = ctx.stream_input()
            for c in range(3):
                slot[c][:] = planes[c]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    ring(False)  # warm-up
    res["f32"] = []
    for _ in range(3):  # unarmed and armed in turn: what the card drifts by shows in both alike
        t_plain, t_armed = ring(False), ring(True)
        res["f32"].append(dict(unarmed_fps=round(1 / t_plain, 1), armed_fps=round(1 / t_armed, 1), armed_share=round(t_plain / t_armed, 3)))
        print(f"f32          ring from host memory: unarmed {1/t_plain:6.1f} frames/s   armed {1/t_armed:6.1f} frames/s "
              f"({t_plain/t_armed*100:5.1f} %)", flush=True)
    ctx.close()
    print(json.dumps({"streambench_tonemap": res}), flush=True)


def gamut_compress_main():
    """k_gamut_compress (BT.2020 -> BT.709, the default parameters) F32 and F16, out of place and in place, beside k_gamut and
    k_tonemap on the same 64 distinct 4K device frames in the same job, on two pictures: uniformly random BT.2020 pixels (the worst
    case: more than half of them have a channel in a curve) and a smooth, mostly in-gamut picture.  An in-place pass changes what the
    next repetition would read, so the frames are put back from a copy before every in-place call (untimed: the times are the
    kernels' HIP events)."""
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "hbm_peak_tbs": 8.0}
    m = torch.tensor(h.gamut_matrix(9, 1), device="cuda")
    t = float(np.float32(h.GAMUT_COMPRESS_THRESHOLD))

    def timed(key, label, nbytes, call, before=None):
        ks = []
        for r in range(reps + 1):  # the first call warms up
            if before:
                before()
            call()
            if r:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        tbs = nbytes / (k_ms * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), min_us=round(min(ks) * 1e3, 2), max_us=round(max(ks) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"{label:44s} {nb} frames per call: {k_ms*1e3:7.2f} us/frame ({min(ks)*1e3:.2f}..{max(ks)*1e3:.2f})  {nbytes/1e6:6.1f} MB/frame  "
              f"{tbs:5.2f} TB/s = {tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)
        return k_ms

    def random_frame():
        return [torch.rand(n, device="cuda") for _ in range(3)]  # G, B, R

    def smooth_frame():
        # a luminance ramp with slow waves, and a chroma of a few percent of it: every pixel far inside the threshold
        x = torch.linspace(0, 1, n, device="cuda")
        y = 0.05 + 0.6 * x + 0.1 * torch.sin(x * (37.0 + 3.0 * torch.rand(1, device="cuda")))
        return [y * (1.0 + 0.04 * torch.sin(x * f)) for f in (11.0, 17.0, 23.0)]

    def curve_share(f):
        """the share of a frame's pixels with a channel past the threshold (in a curve or beyond its limit), in torch's binary32"""
        v = torch.stack([f[2].float(), f[0].float(), f[1].float()])
        o = m @ v
        a = o.max(dim=0).values
        return float((((a - o) / a > t).any(dim=0) & (a > 0)).float().mean())

    for pic, make in (("random", random_frame), ("smooth", smooth_frame)):
        for name, sample, dt in (("f32", h.SAMPLE_F32, torch.float32), ("f16", h.SAMPLE_F16, torch.float16)):
            keep = [[x.to(dt) for x in make()] for _ in range(nb)]
            src = [[x.clone() for x in f] for f in keep]
            dst = [[torch.empty(n, dtype=dt, device="cuda") for _ in range(3)] for _ in range(nb)]
            torch.cuda.synchronize()
            res[f"{pic}_{name}_share_past_threshold"] = round(curve_share(keep[0]), 4)
            print(f"{pic} {name}: {res[f'{pic}_{name}_share_past_threshold']*100:.1f} % of the pixels have a channel past the threshold", flush=True)
            nbytes = 2 * 3 * n * (4 if sample == h.SAMPLE_F32 else 2)

            def restore():
                for fs, fk in zip(src, keep):
                    for a, b in zip(fs, fk):
                        a.copy_(b)
                torch.cuda.synchronize()

            tag = f"{pic}_{name}"
            c_out = timed(f"k_gamut_compress_{tag}_out_of_place", f"k_gamut_compress {pic} {name} out of place", nbytes,
                          lambda: ctx.gamut_compress_batch(w, hh, sample, 9, 1, src, dst))
            g_out = timed(f"k_gamut_{tag}_out_of_place", f"k_gamut {pic} {name} out of place", nbytes,
                          lambda: ctx.gamut_batch(w, hh, sample, 9, 1, 1, src, dst))
            t_out = timed(f"k_tonemap_{tag}_out_of_place", f"k_tonemap {pic} {name} out of place", nbytes,
                          lambda: ctx.tonemap_batch(w, hh, sample, 1000, 100, 1, src, dst))
            del dst
            c_in = timed(f"k_gamut_compress_{tag}_in_place", f"k_gamut_compress {pic} {name} in place", nbytes,
                         lambda: ctx.gamut_compress_batch(w, hh, sample, 9, 1, src), restore)
            g_in = timed(f"k_gamut_{tag}_in_place", f"k_gamut {pic} {name} in place", nbytes,
                         lambda: ctx.gamut_batch(w, hh, sample, 9, 1, 1, src), restore)
            t_in = timed(f"k_tonemap_{tag}_in_place", f"k_tonemap {pic} {name} in place", nbytes,
                         lambda: ctx.tonemap_batch(w, hh, sample, 1000, 100, 1, src), restore)
            res[f"{tag}_compress_over_gamut"] = dict(out_of_place=round(c_out / g_out, 3), in_place=round(c_in / g_in, 3))
            res[f"{tag}_compress_over_tonemap"] = dict(out_of_place=round(c_out / t_out, 3), in_place=round(c_in / t_in, 3))
            print(f"{tag}: k_gamut_compress / k_gamut out of place {c_out/g_out:.3f}, in place {c_in/g_in:.3f}; / k_tonemap out of place "
                  f"{c_out/t_out:.3f}, in place {c_in/t_in:.3f}", flush=True)
            del src, keep
            torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps({"streambench_gamut_compress": res}), flush=True)


def lut3d_main():
    """k_lut3d at N = 17, 33 and 65, F32 and F16, tetrahedral and trilinear, out of place and in place, beside k_tonemap and k_gamut
    in the same job; then the .f32 ring from host memory armed against unarmed.  The bytes counted are the six plane streams only."""
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}

    def timed(key, label, nbytes, call):
        ks = []
        for r in range(reps + 1):  # the first call warms up
            call()
            if r:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        tbs = nbytes / (k_ms * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), min_us=round(min(ks) * 1e3, 2), max_us=round(max(ks) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"{label:40s} {nb} frames per call: {k_ms*1e3:7.2f} us/frame ({min(ks)*1e3:.2f}..{max(ks)*1e3:.2f})  {nbytes/1e6:6.1f} MB/frame  "
              f"{tbs:5.2f} TB/s = {tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)

    def table(size):
        """a look: the identity on the unit domain, every node moved a little"""
        ax = np.linspace(0, 1, size)
        b, g, r = np.meshgrid(ax, ax, ax, indexing="ij")
        nodes = np.stack([r, g, b], -1).reshape(-1, 3) + np.random.default_rng(size).uniform(-0.02, 0.02, (size ** 3, 3))
        return h.Lut3d(f"LUT_3D_SIZE {size}\n" + "\n".join("%.9g %.9g %.9g" % tuple(v) for v in nodes.astype(np.float32)) + "\n")

    luts = {size: table(size) for size in (17, 33, 65)}
    sc = (10, 0, h.MATRIX_BT2020NC)
    # 1. the same 64 distinct frames for every kernel: uniformly random samples, so neighbouring pixels gather from unrelated cells of
    # the table (a picture's neighbours mostly share a cell: the last line of the block times one such frame set)
    for name, sample, dt in (("f32", h.SAMPLE_F32, torch.float32), ("f16", h.SAMPLE_F16, torch.float16)):
        src = [[torch.rand(n, device="cuda").to(dt) for _ in range(3)] for _ in range(nb)]
        dst = [[torch.empty(n, dtype=dt, device="cuda") for _ in range(3)] for _ in range(nb)]
        torch.cuda.synchronize()
        nbytes = 2 * 3 * n * (4 if sample == h.SAMPLE_F32 else 2)
        timed(f"k_tonemap_{name}_out_of_place", f"k_tonemap {name} out of place", nbytes, lambda: ctx.tonemap_batch(w, hh, sample, 1000, 100, 1, src, dst))
        timed(f"k_gamut_{name}_out_of_place", f"k_gamut {name} out of place", nbytes, lambda: ctx.gamut_batch(w, hh, sample, 9, 1, 1, src, dst))
        for size, lut in luts.items():
            for interp, iname in ((1, "tetra"), (0, "trilinear")):
                timed(f"k_lut3d_{size}_{name}_{iname}_out_of_place", f"k_lut3d N={size} {name} {iname} out of place", nbytes,
                      lambda: ctx.lut3d_batch(w, hh, sample, lut, interp, 0, *sc, src, dst))
                if size == 17:  # the same table through L2, as the larger ones are read
                    ctx.set_option("lut3d_lds", 0)
                    timed(f"k_lut3d_{size}_{name}_{iname}_out_of_place_l2", f"k_lut3d N={size} {name} {iname} out of place, no LDS", nbytes,
                          lambda: ctx.lut3d_batch(w, hh, sample, lut, interp, 0, *sc, src, dst))
                    ctx.set_option("lut3d_lds", 1)
        if sample == h.SAMPLE_F32:
            timed("k_lut3d_33_f32_tetra_signal_out_of_place", "k_lut3d N=33 f32 tetra signal out of place", nbytes,
                  lambda: ctx.lut3d_batch(w, hh, sample, luts[33], 1, 1, *sc, src, dst))
        del dst
        # in place: the look keeps the samples in the domain, call after call
        for size, lut in luts.items():
            for interp, iname in ((1, "tetra"), (0, "trilinear")):
                timed(f"k_lut3d_{size}_{name}_{iname}_in_place", f"k_lut3d N={size} {name} {iname} in place", nbytes,
                      lambda: ctx.lut3d_batch(w, hh, sample, lut, interp, 0, *sc, src))
        timed(f"k_tonemap_{name}_in_place", f"k_tonemap {name} in place", nbytes, lambda: ctx.tonemap_batch(w, hh, sample, 1000, 100, 1, src))
        if sample == h.SAMPLE_F32:  # a smooth picture: ramps with a little noise, neighbours in one cell
            x = torch.arange(n, device="cuda") % w / w
            y = torch.arange(n, device="cuda") // w / hh
            for f in src:
                f[0].copy_((x + 0.01 * torch.rand(n, device="cuda")).clamp(0, 1))
                f[1].copy_((y + 0.01 * torch.rand(n, device="cuda")).clamp(0, 1))
                f[2].copy_(((x + y) / 2 + 0.01 * torch.rand(n, device="cuda")).clamp(0, 1))
            torch.cuda.synchronize()
            for size, lut in luts.items():
                timed(f"k_lut3d_{size}_f32_tetra_in_place_smooth", f"k_lut3d N={size} f32 tetra in place, smooth", nbytes,
                      lambda: ctx.lut3d_batch(w, hh, sample, lut, 1, 0, *sc, src))
            ctx.set_option("lut3d_lds", 0)
            timed("k_lut3d_17_f32_tetra_in_place_smooth_l2", "k_lut3d N=17 f32 tetra in place, smooth, no LDS", nbytes,
                  lambda: ctx.lut3d_batch(w, hh, sample, luts[17], 1, 0, *sc, src))
            ctx.set_option("lut3d_lds", 1)
        del src
        torch.cuda.empty_cache()
    t, l33, l65 = (res[k]["kernel_us_per_frame"] for k in ("k_tonemap_f32_out_of_place", "k_lut3d_33_f32_tetra_out_of_place",
                                                          "k_lut3d_65_f32_tetra_out_of_place"))
    res["lut3d_33_over_tonemap"] = round(l33 / t, 3)
    res["lut3d_65_over_33"] = round(l65 / l33, 3)
    print(f"k_lut3d N=33 tetra f32 / k_tonemap f32: {l33 / t:.3f};  N=65 / N=33: {l65 / l33:.3f}", flush=True)

    # 2. the .f32 ring from host memory, unarmed and armed
    planes = [np.random.default_rng(31 + c).random(n, dtype=np.float32) for c in range(3)]
    d32 = h.make_desc(w, hh, dst_depth=10, src_transfer=16, dst_transfer=16, dst_matrix=h.MATRIX_BT2020NC, src_primaries=9, dst_primaries=9,
                      resampler=1, stats=[(0, 1)] * 3)

    def ring(arm):
        ctx.stream_open(d32, depth)
        if arm:
            ctx.stream_lut3d(luts[33], 1, 0)
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            slot = ctx.stream_input()
            for c in range(3):
                slot[c][:] = planes[c]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    ring(False)  # warm-up
    res["f32"] = []
    for _ in range(3):  # unarmed and armed in turn: what the card drifts by shows in both alike
        t_plain, t_armed = ring(False), ring(True)
        res["f32"].append(dict(unarmed_fps=round(1 / t_plain, 1), armed_fps=round(1 / t_armed, 1), armed_share=round(t_plain / t_armed, 3)))
        print(f"f32          ring from host memory: unarmed {1/t_plain:6.1f} frames/s   armed {1/t_armed:6.1f} frames/s "
              f"({t_plain/t_armed*100:5.1f} %)", flush=True)
    ctx.close()
    print(json.dumps({"streambench_lut3d": res}), flush=True)


def hlg_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}
    hlg = (1000, 1, 10, 0, h.MATRIX_BT2020NC)

    def timed(key, label, nbytes, call, before=None):
        ks = []
        for r in range(reps + 1):  # the first call warms up
            if before:
                before()
            call()
            if r:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        tbs = nbytes / (k_ms * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), min_us=round(min(ks) * 1e3, 2), max_us=round(max(ks) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"{label:32s} {nb} frames per call: {k_ms*1e3:7.2f} us/frame ({min(ks)*1e3:.2f}..{max(ks)*1e3:.2f})  {nbytes/1e6:6.1f} MB/frame  "
              f"{tbs:5.2f} TB/s = {tbs/8.0*100:4.1f} % of 8 TB/s", flush=True)
        return k_ms

    # 1. the three kernels over the same 64 distinct F32 frames on the device, out of place, then in place
    src = [[torch.rand(n, device="cuda") ** 3 for _ in range(3)] for _ in range(nb)]
    dst = [[torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in range(nb)]
    torch.cuda.synchronize()
    b32 = 2 * 3 * n * 4
    h_out = timed("k_hlg_f32_out_of_place", "k_hlg f32 out of place", b32, lambda: ctx.hlg_batch(w, hh, h.SAMPLE_F32, *hlg, src, dst))
    t_out = timed("k_tonemap_f32_out_of_place", "k_tonemap f32 out of place", b32, lambda: ctx.tonemap_batch(w, hh, h.SAMPLE_F32, 1000, 100, 1, src, dst))
    timed("k_gamut_f32_out_of_place", "k_gamut f32 out of place", b32, lambda: ctx.gamut_batch(w, hh, h.SAMPLE_F32, 9, 1, 1, src, dst))

    def put_back():  # dst keeps the light for the in-place calls of k_hlg
        for f, g in zip(src, dst):
            for a, b in zip(f, g):
                a.copy_(b)
        torch.cuda.synchronize()

    for f, g in zip(dst, src):
        for a, b in zip(f, g):
            a.copy_(b)
    h_in = timed("k_hlg_f32_in_place", "k_hlg f32 in place", b32, lambda: ctx.hlg_batch(w, hh, h.SAMPLE_F32, *hlg, src), before=put_back)
    put_back()
    t_in = timed("k_tonemap_f32_in_place", "k_tonemap f32 in place", b32, lambda: ctx.tonemap_batch(w, hh, h.SAMPLE_F32, 1000, 100, 1, src))
    timed("k_gamut_f32_in_place", "k_gamut f32 in place", b32, lambda: ctx.gamut_batch(w, hh, h.SAMPLE_F32, 9, 1, 1, src))
    del src
    torch.cuda.empty_cache()
    half = [[(torch.rand(n, device="cuda") ** 3).to(torch.float16) for _ in range(3)] for _ in range(nb)]
    torch.cuda.synchronize()
    timed("k_hlg_f16_to_f32", "k_hlg f16 -> f32", 3 * n * (2 + 4), lambda: ctx.hlg_batch(w, hh, h.SAMPLE_F16, *hlg, half, dst))
    res["k_hlg_over_k_tonemap_out_of_place"] = round(h_out / t_out, 3)
    res["k_hlg_over_k_tonemap_in_place"] = round(h_in / t_in, 3)
    print(f"k_hlg / k_tonemap: out of place {h_out/t_out:.3f}, in place {h_in/t_in:.3f}", flush=True)
    del half, dst
    torch.cuda.empty_cache()

    # 2. the .f32 ring from host memory with equal transfers, unarmed and armed
    planes = [(np.random.default_rng(31 + c).random(n, dtype=np.float32) ** 3) for c in range(3)]
    d32 = h.make_desc(w, hh, dst_depth=10, src_transfer=8, dst_transfer=8, dst_matrix=h.MATRIX_BT2020NC, resampler=1, stats=[(0, 1)] * 3)

    def ring(arm):
        ctx.stream_open(d32, depth)
        if arm:
            ctx.stream_hlg(1000, 1)
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            slot = ctx.stream_input()
            for c in range(3):
                slot[c][:] = planes[c]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    ring(False)  # warm-up
    res["f32"] = []
    for _ in range(3):  # unarmed and armed in turn: what the card drifts by shows in both alike
        t_plain, t_armed = ring(False), ring(True)
        res["f32"].append(dict(unarmed_fps=round(1 / t_plain, 1), armed_fps=round(1 / t_armed, 1), armed_share=round(t_plain / t_armed, 3)))
        print(f"f32          ring from host memory: unarmed {1/t_plain:6.1f} frames/s   armed {1/t_armed:6.1f} frames/s "
              f"({t_plain/t_armed*100:5.1f} %)", flush=True)
    ctx.close()
    print(json.dumps({"streambench_hlg": res}), flush=True)


def ictcp_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    nf = int(os.environ.get("N", "60"))
    depth = 3
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "ring_frames": nf, "ring_depth": depth, "hbm_peak_tbs": 8.0}
    hlg = (1000, 0, 10, 0, h.MATRIX_BT2020NC)

    def timed(key, label, nbytes, call, before=None):
        ks = []
        for r in range(reps + 1):  # the first call warms up
            if before:
                before()
            call()
            if r:
                ks.append(ctx.last_kernel_ms()[0] / nb)
        k_ms = float(np.median(ks))
        tbs = nbytes / (k_ms * 1e-3) / 1e12
        res[key] = dict(kernel_us_per_frame=round(k_ms * 1e3, 2), min_us=round(min(ks) * 1e3, 2), max_us=round(max(ks) * 1e3, 2),
                        bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3), variant=ctx.last_kernel_variant())
        print(f"{label:34s} {nb} frames per call: {k_ms*1e3:7.2f} us/frame ({min(ks)*1e3:.2f}..{max(ks)*1e3:.2f})  {nbytes/1e6:6.1f} MB/frame  "
              f"{tbs:5.2f} TB/s = {tbs/8.0*100:4.1f} % of 8 TB/s  {ctx.last_kernel_variant()}", flush=True)
        return k_ms

    # 1. k_ictcp beside k_hlg and k_gamut over the same 64 distinct F32 frames on the device, out of place, then in place; then F16
    src = [[torch.rand(n, device="cuda") ** 3 for _ in range(3)] for _ in range(nb)]
    dst = [[torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(3)] for _ in range(nb)]
    torch.cuda.synchronize()
    b32 = 2 * 3 * n * 4  # 24 algorithmic bytes a pixel
    i_out = timed("k_ictcp_f32_out_of_place", "k_ictcp f32 out of place", b32, lambda: ctx.ictcp_batch(w, hh, h.SAMPLE_F32, 10, 0, src, dst))
    h_out = timed("k_hlg_f32_out_of_place", "k_hlg f32 out of place", b32, lambda: ctx.hlg_batch(w, hh, h.SAMPLE_F32, *hlg, src, dst))
    g_out = timed("k_gamut_f32_out_of_place", "k_gamut f32 out of place", b32, lambda: ctx.gamut_batch(w, hh, h.SAMPLE_F32, 9, 1, 1, src, dst))
    keep = [[p.clone() for p in f] for f in src]

    def put_back():  # the in-place passes leave code values: the light comes back before each call
        for f, g in zip(src, keep):
            for a, b in zip(f, g):
                a.copy_(b)
        torch.cuda.synchronize()

    i_in = timed("k_ictcp_f32_in_place", "k_ictcp f32 in place", b32, lambda: ctx.ictcp_batch(w, hh, h.SAMPLE_F32, 10, 0, src), before=put_back)
    h_in = timed("k_hlg_f32_in_place", "k_hlg f32 in place", b32, lambda: ctx.hlg_batch(w, hh, h.SAMPLE_F32, *hlg, src), before=put_back)
    put_back()
    timed("k_gamut_f32_in_place", "k_gamut f32 in place", b32, lambda: ctx.gamut_batch(w, hh, h.SAMPLE_F32, 9, 1, 1, src))
    del src, keep
    torch.cuda.empty_cache()
    half = [[(torch.rand(n, device="cuda") ** 3).to(torch.float16) for _ in range(3)] for _ in range(nb)]
    torch.cuda.synchronize()
    timed("k_ictcp_f16_to_f32", "k_ictcp f16 -> f32", 3 * n * (2 + 4), lambda: ctx.ictcp_batch(w, hh, h.SAMPLE_F16, 10, 0, half, dst))
    res["k_ictcp_over_k_hlg"] = dict(out_of_place=round(i_out / h_out, 3), in_place=round(i_in / h_in, 3))
    res["k_ictcp_over_k_gamut_out_of_place"] = round(i_out / g_out, 3)
    print(f"k_ictcp / k_hlg: out of place {i_out/h_out:.3f}, in place {i_in/h_in:.3f}; k_ictcp / k_gamut out of place {i_out/g_out:.3f}", flush=True)
    del half
    torch.cuda.empty_cache()

    # 2. the way back: k_linearize and k_codelight on ICtCp codes beside their BT.2020nc forms, the same code frames, in turn
    def codes(count, lo, hi):
        return torch.randint(lo, hi + 1, (count,), dtype=torch.int32, device="cuda").to(torch.int16)

    frames = [torch.cat([codes(n, 64, 940), codes(n // 4, 384, 640), codes(n // 4, 384, 640)]) for _ in range(nb)]
    torch.cuda.synchronize()
    t, variants = {}, {}
    descs = {"ICTCP": h.make_codelight_desc(w, hh, 1, 10, 0, h.MATRIX_ICTCP, 1), "BT2020NC": h.make_codelight_desc(w, hh, 1, 10, 0, h.MATRIX_BT2020NC, 1)}
    for rep in range(reps + 1):  # the first round warms up
        for name, d in descs.items():
            for kernel, call in (("k_linearize", lambda: ctx.linearize_batch(d, frames, dst)), ("k_codelight", lambda: ctx.codelight_batch(d, frames, dist=True))):
                call()
                variants[kernel, name] = ctx.last_kernel_variant()
                if rep:
                    t.setdefault((kernel, name), []).append(ctx.last_kernel_ms()[0] / nb)
    for kernel, nbytes in (("k_linearize", 23 * n), ("k_codelight", 11 * n)):
        med = {}
        for name in descs:
            ks = t[kernel, name]
            med[name] = float(np.median(ks))
            tbs = nbytes / (med[name] * 1e-3) / 1e12
            res[f"{kernel}_{name}_420_10"] = dict(kernel_us_per_frame=round(med[name] * 1e3, 2), min_us=round(min(ks) * 1e3, 2), max_us=round(max(ks) * 1e3, 2),
                                                 bytes_per_frame=nbytes, kernel_tbs=round(tbs, 2), variant=variants[kernel, name])
            print(f"{kernel} {name:9s} 4:2:0 10 bit, upsampling included: {med[name]*1e3:7.2f} us/frame ({min(ks)*1e3:.2f}..{max(ks)*1e3:.2f})  "
                  f"{variants[kernel, name]}", flush=True)
        res[f"{kernel}_ictcp_over_bt2020nc"] = round(med["ICTCP"] / med["BT2020NC"], 3)
        print(f"{kernel}<ICTCP> / {kernel}<BT2020NC>: {med['ICTCP']/med['BT2020NC']:.3f}", flush=True)
    del frames, dst
    torch.cuda.empty_cache()

    # 3. the .f32 ring from host memory on the passthrough descriptor, unarmed and armed
    planes = [(np.random.default_rng(31 + c).random(n, dtype=np.float32) ** 3) for c in range(3)]
    d32 = h.make_desc(w, hh, dst_depth=10, src_transfer=8, dst_transfer=8, dst_matrix=h.MATRIX_GBR, resampler=1, stats=[(0, 1)] * 3)

    def ring(arm):
        ctx.stream_open(d32, depth)
        if arm:
            ctx.stream_ictcp()
        inflight = 0
        t0 = time.perf_counter()
        for _ in range(nf):
            slot = ctx.stream_input()
            for c in range(3):
                slot[c][:] = planes[c]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
        dt = (time.perf_counter() - t0) / nf
        ctx.stream_close()
        return dt

    ring(False)  # warm-up
    res["f32"] = []
    for _ in range(3):  # unarmed and armed in turn: what the card drifts by shows in both alike
        t_plain, t_armed = ring(False), ring(True)
        res["f32"].append(dict(unarmed_fps=round(1 / t_plain, 1), armed_fps=round(1 / t_armed, 1), armed_share=round(t_plain / t_armed, 3)))
        print(f"f32          ring from host memory: unarmed {1/t_plain:6.1f} frames/s   armed {1/t_armed:6.1f} frames/s "
              f"({t_plain/t_armed*100:5.1f} %)", flush=True)
    ctx.close()
    print(json.dumps({"streambench_ictcp": res}), flush=True)


def siting_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 5
    n = w * hh
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "hbm_peak_tbs": 8.0}

    def figures(key, label, us, nbytes, extra=""):
        """us: per-frame times of the passes"""
        med = float(np.median(us))
        tbs = nbytes / (med * 1e-6) / 1e12
        res[key] = dict(us_per_frame=round(med, 2), min_us=round(min(us), 2), max_us=round(max(us), 2), bytes_per_frame=nbytes,
                        tbs=round(tbs, 2), hbm_peak_fraction=round(tbs / 8.0, 3))
        print(f"{label:44s} {med:8.2f} us/frame ({min(us):.2f}..{max(us):.2f})  {nbytes/1e6:6.1f} MB/frame  {tbs:5.2f} TB/s = "
              f"{tbs/8.0*100:4.1f} % of 8 TB/s{extra}", flush=True)
        return med

    # 1. the two second-pass kernels alone, plane by plane, on 128 distinct 12-bit planes
    ctx = h.Context(0)
    planes = [torch.randint(0, 4096, (n,), dtype=torch.int16, device="cuda") for _ in range(2 * nb)]
    outs = [torch.empty(n // 4, dtype=torch.int16, device="cuda") for _ in range(2 * nb)]
    torch.cuda.synchronize()
    per = {0: [], 2: []}
    for r in range(reps + 1):  # the first pass warms up; the kernels alternate pass by pass
        for loc in (0, 2):
            ms = 0.0
            for p, o in zip(planes, outs):
                ctx.subsample_420_sited(w, hh, 12, loc, p, o)
                ms += ctx.last_kernel_ms()[0]
            if r:
                per[loc].append(ms * 1e3 / nb)
    ref = figures("k_fir420", "k_fir420 (loc 0), one launch per plane", per[0], 5 * n)
    tl = figures("k_fir420_tl", "k_fir420_tl (loc 2), one launch per plane", per[2], 5 * n)
    res["k_fir420_tl"]["of_k_fir420"] = round(tl / ref, 3)
    res["k_fir420_tl"]["outside_yardstick_spread_on_the_slow_side"] = bool(tl > max(per[0]))
    print(f"k_fir420_tl / k_fir420 = {tl/ref:.3f}; slower than the yardstick's slowest pass: {tl > max(per[0])}", flush=True)
    del planes, outs
    ctx.close()
    torch.cuda.empty_cache()

    # 2. and 3. the batch entry on C2
    d = h.make_desc(w, hh, dst_depth=12, dst_matrix=h.MATRIX_BT2020NC, resampler=1)
    frames = [[torch.rand(n, device="cuda") for _ in range(3)] for _ in range(nb)]
    for fr in frames:
        for p in fr:
            p[0], p[1] = 0.0, 1.0  # floor 0, ceiling 1
    outs = [torch.empty(h.frame_bytes(d) // 2, dtype=torch.int16, device="cuda") for _ in range(nb)]
    torch.cuda.synchronize()
    ctxs = {}
    for key, fir, loc in (("twopass_siting0", "twopass", 0), ("twopass_siting2", "twopass", 2), ("fused_siting0", "auto", 0)):
        c = h.Context(0)
        c.set_option("fir", fir)
        c.set_chroma_siting(loc)
        ctxs[key] = c

    def call(key):
        t0 = time.perf_counter()
        ctxs[key].convert_batch(d, frames, outs)  # synchronous: every frame final on return
        return (time.perf_counter() - t0) * 1e6 / nb

    for key in ctxs:  # warm-up: allocations, the statistics hint, the tier steering
        call(key)
        call(key)
        res[key + "_variant"] = ctxs[key].last_kernel_variant()
    back = {k: [call(k) for _ in range(reps)] for k in ("twopass_siting0", "twopass_siting2")}
    t0 = figures("batch_twopass_siting0", 'h2y_convert_batch C2 "fir" "twopass", siting 0', back["twopass_siting0"], 23 * n)
    t2 = figures("batch_twopass_siting2", 'h2y_convert_batch C2 "fir" "twopass", siting 2', back["twopass_siting2"], 23 * n, f"  ({res['twopass_siting2_variant']})")
    alt = {k: [] for k in ctxs}
    for _ in range(reps):
        for k in ctxs:
            alt[k].append(call(k))
    a0 = figures("alternating_twopass_siting0", "alternating: two-pass, siting 0", alt["twopass_siting0"], 23 * n)
    a2 = figures("alternating_twopass_siting2", "alternating: two-pass, siting 2", alt["twopass_siting2"], 23 * n)
    af = figures("alternating_fused_siting0", 'alternating: "fir" "auto" (one pass), siting 0', alt["fused_siting0"], 15 * n, f"  ({res['fused_siting0_variant']})")
    res["siting2_of_siting0_twopass"] = round(a2 / a0, 3)
    res["siting2_of_default_one_pass"] = round(a2 / af, 3)
    print(f"siting 2 / siting 0, both two-pass: back to back {t2/t0:.3f}, alternating {a2/a0:.3f}; siting 2 / the default one-pass form: {a2/af:.3f}", flush=True)
    for c in ctxs.values():
        c.close()
    print(json.dumps({"streambench_siting": res}), flush=True)


if __name__ == "__main__":
    if sys.argv[1:] == ["siting"]:
        siting_main()
    elif sys.argv[1:] == ["gamut"]:
        gamut_main()
    elif sys.argv[1:] == ["gamut_compress"]:
        gamut_compress_main()
    elif sys.argv[1:] == ["tonemap"]:
        tonemap_main()
    elif sys.argv[1:] == ["lut3d"]:
        lut3d_main()
    elif sys.argv[1:] == ["hlg"]:
        hlg_main()
    elif sys.argv[1:] == ["ictcp"]:
        ictcp_main()
    elif sys.argv[1:] == ["hlgsrc"]:
        hlgsrc_main()
    elif sys.argv[1:] == ["sdrsrc"]:
        sdrsrc_main()
    elif sys.argv[1:] == ["sigsrc"]:
        sigsrc_main()
    elif sys.argv[1:] == ["scale"]:
        scale_main()
    elif sys.argv[1:] == ["dither"]:
        dither_main()
    elif sys.argv[1:] == ["pack"]:
        pack_main()
    elif sys.argv[1:] == ["inverse"]:
        inverse_main()
    elif sys.argv[1:] == ["dpx"]:
        dpx_main()
    elif sys.argv[1:] == ["tiff"]:
        tiff_main()
    elif sys.argv[1:] == ["exr"]:
        exr_main()
    elif sys.argv[1:] == ["compare"]:
        compare_main()
    elif sys.argv[1:] == ["histogram"]:
        histogram_main()
    elif sys.argv[1:] == ["ssim"]:
        ssim_main()
    elif sys.argv[1:] == ["regions"]:
        regions_main()
    elif sys.argv[1:] == ["light"]:
        light_main()
    elif sys.argv[1:] == ["lightdist"]:
        lightdist_main()
    elif sys.argv[1:] == ["codelight"]:
        codelight_main()
    elif sys.argv[1:] == ["gamutcheck"]:
        gamutcheck_main()
    elif sys.argv[1:] == ["scenes"]:
        scenes_main()
    elif sys.argv[1:] == ["linearize"]:
        linearize_main()
    elif sys.argv[1:] == ["deltae"]:
        deltae_main()
    else:
        main()
