"""ctypes mirror of include/hdr2yuv_hip.h (the drop-in C-ABI).

Names follow the reference: a *picture* has three planar planes in the order
0=G/Y, 1=B/Cb(Z/Dz), 2=R/Cr(X/Dx) (hdr.h:359-392); the descriptor carries the
``--src_*`` / ``--dst_*`` attributes of the reference's command line
(hdr2yuv.cpp:73-263).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SAMPLE_U16, SAMPLE_F32, SAMPLE_F16 = 1, 2, 3
CHROMA_420, CHROMA_444 = 1, 3
TRANSFER_LINEAR, TRANSFER_PQ = 8, 16
MATRIX_GBR, MATRIX_BT709, MATRIX_BT2020NC, MATRIX_YDZDX, MATRIX_Y500, MATRIX_Y100 = 0, 1, 9, 11, 12, 13
MATRIX_YUVPRIME2 = 15  # destination only: Y'u'v' (include/hdr2yuv_hip.h)
MATRIX_ICTCP = 14  # H2YCodelightDesc.matrix_coeffs only: PQ ICtCp codes (include/hdr2yuv_hip.h, "light of ICtCp code planes")

H2Y_OK, H2Y_EINVAL, H2Y_EUNSUPPORTED, H2Y_EHIP, H2Y_ENOMEM = 0, 1, 2, 3, 4

EXPORTS = [
    "h2y_abi_version", "h2y_frame_bytes", "h2y_plane_bytes", "h2y_desc_check", "h2y_ctx_create", "h2y_ctx_destroy",
    "h2y_last_error", "h2y_ctx_set_stream", "h2y_convert_frame", "h2y_convert_batch", "h2y_convert_batch_enqueue",
    "h2y_batch_finish", "h2y_pic_stats", "h2y_matrix_convert", "h2y_subsample_420", "h2y_last_kernel_ms", "h2y_last_kernel_name", "h2y_last_kernel_variant",
    "h2y_matrix_inverse", "h2y_upsample_444", "h2y_inverse_420", "h2y_inverse_frame", "h2y_ctx_set_option", "h2y_stream_open", "h2y_stream_input", "h2y_stream_submit", "h2y_stream_output", "h2y_stream_close",
    "h2y_inverse_batch", "h2y_inverse_stream_open", "h2y_dpx_parse", "h2y_dpx_decode_batch", "h2y_dpx_stream_open",
    "h2y_tiff_parse", "h2y_tiff_layout", "h2y_tiff_decode_batch", "h2y_rgb_interleave_batch", "h2y_tiff_stream_open",
    "h2y_tiff_inverse_stream_open", "h2y_exr_parse", "h2y_exr_unpack", "h2y_exr_decode_batch", "h2y_exr_stream_open",
    "h2y_compare_batch", "h2y_stream_compare", "h2y_stream_reference", "h2y_stream_compare_result", "h2y_compare_stream_open",
    "h2y_histogram_batch", "h2y_stream_histogram", "h2y_stream_histogram_ex", "h2y_stream_histogram_result",
    "h2y_histogram_stream_open", "h2y_ssim_batch", "h2y_stream_ssim", "h2y_stream_ssim_result",
    "h2y_regions_host", "h2y_regions_batch", "h2y_stream_regions", "h2y_stream_regions_result",
    "h2y_light_batch", "h2y_stream_light", "h2y_stream_light_result",
    "h2y_lightdist_batch", "h2y_stream_lightdist", "h2y_stream_lightdist_result", "h2y_lightdist_json",
    "h2y_codelight_batch", "h2y_codelight_stream_open",
    "h2y_gamutcheck_planes", "h2y_gamutcheck_batch", "h2y_stream_gamutcheck", "h2y_stream_gamutcheck_result",
    "h2y_scenesig_batch", "h2y_codescenesig_batch", "h2y_stream_scenesig", "h2y_stream_scenesig_result", "h2y_stream_lightdist_bins",
    "h2y_scene_distance", "h2y_scene_cuts", "h2y_scene_merge", "h2y_lightdist_json_scenes",
    "h2y_linearize_batch", "h2y_pqcode_stream_open",
    "h2y_deltae_batch", "h2y_stream_deltae", "h2y_stream_deltae_result",
    "h2y_scale_taps", "h2y_scale_frame_bytes", "h2y_scale_batch", "h2y_stream_scale", "h2y_scale_stream_open",
    "h2y_dither_offsets", "h2y_dither_batch", "h2y_stream_dither", "h2y_dither_stream_open",
    "h2y_pack_frame_bytes", "h2y_pack_frame", "h2y_unpack_frame", "h2y_pack_batch", "h2y_unpack_batch", "h2y_stream_pack", "h2y_stream_unpack", "h2y_stream_unpack_ex",
    "h2y_gamut_matrix", "h2y_gamut_batch", "h2y_stream_gamut",
    "h2y_gamut_compress_curve", "h2y_gamut_compress_planes", "h2y_gamut_compress_batch", "h2y_stream_gamut_compress",
    "h2y_tonemap_curve", "h2y_tonemap_batch", "h2y_stream_tonemap",
    "h2y_lut3d_parse", "h2y_lut3d_free", "h2y_lut3d_info", "h2y_lut3d_nodes", "h2y_lut3d_planes", "h2y_lut3d_batch", "h2y_stream_lut3d",
    "h2y_hlg_tables", "h2y_hlg_planes", "h2y_hlg_batch", "h2y_stream_hlg",
    "h2y_hlg_inverse_tables", "h2y_hlg_inverse_planes", "h2y_hlg_linearize_batch", "h2y_hlgcode_stream_open",
    "h2y_sdr_inverse_planes", "h2y_sdr_linearize_batch", "h2y_sdrcode_stream_open",
    "h2y_code_signal_planes", "h2y_code_signal_batch", "h2y_sigcode_stream_open",
    "h2y_ictcp_batch", "h2y_stream_ictcp",
    "h2y_ctx_set_chroma_siting", "h2y_subsample_420_sited",
    "h2y_ctx_set_inverse_chroma_siting", "h2y_upsample_444_sited",
]

COMPARE_FRAMES_PER_LAUNCH = 64
HISTOGRAM_FRAMES_PER_LAUNCH = 64
SSIM_FRAMES_PER_LAUNCH = 64
REGIONS_FRAMES_PER_LAUNCH = 64
LIGHT_FRAMES_PER_LAUNCH = 64
LIGHTDIST_FRAMES_PER_LAUNCH = 64
LIGHTDIST_BINS = 8706  # bins of max(L_G, L_B, L_R) by its binary32 bits: below 2^-17, 512 per binade up to 1, and 1 itself
LIGHTDIST_FIRST_BITS = 0x37000000  # 2^-17: the lower edge of bin 1
LIGHTDIST_PCT = (100, 500, 1000, 2500, 5000, 7500, 9000, 9500, 9900, 9998)  # the percentiles, in hundredths of a percent
SCENESIG_COLS, SCENESIG_ROWS = 16, 9  # the scene signature's grid of cells
SCENESIG_FRAMES_PER_LAUNCH = 64
CODELIGHT_FRAMES_PER_LAUNCH = 8  # a launch's 4:2:0 scratch stays at 253 MiB for 3840 x 2160
LINEARIZE_FRAMES_PER_LAUNCH = 8  # the same rule, the same scratch
GAMUTCHECK_MAX_SETS = 2  # check sets of one gamut containment check
GAMUTCHECK_RATIO, GAMUTCHECK_FLOOR = 0.02, 0.02  # its defaults: the relative tolerance, and the floor in cd/m2
DELTAE_FRAMES_PER_LAUNCH = 4  # the same scratch again: four upsampled chroma planes a pair
SCALE_FRAMES_PER_LAUNCH = 64
GAMUT_FRAMES_PER_LAUNCH = 64
TONEMAP_FRAMES_PER_LAUNCH = 64
LUT3D_FRAMES_PER_LAUNCH = 64
LUT3D_TRILINEAR, LUT3D_TETRAHEDRAL = 0, 1
LUT3D_PLANES, LUT3D_SIGNAL = 0, 1
HLG_FRAMES_PER_LAUNCH = 64
HLG_PEAK_MIN, HLG_PEAK_MAX = 400, 2000
SDR_WHITE_MIN, SDR_WHITE_MAX, SDR_WHITE_DEFAULT = 80, 1000, 203  # the reference white of an SDR code source, cd/m2
ICTCP_FRAMES_PER_LAUNCH = 64
SCALE_TAPS = 32  # coefficients per row of scale_taps' table
DITHER_FRAMES_PER_LAUNCH = 64
PACK_PLANAR16, PACK_PLANAR8, PACK_NV12, PACK_P010 = 0, 1, 2, 3  # the sample packings (include/hdr2yuv_hip.h)
PACK_FRAMES_PER_LAUNCH = 64
DITHER_CUT, DITHER_ORDERED, DITHER_NOISE = 0, 1, 2


class H2YError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"hdr2yuv_hip error {code}: {msg}")
        self.code = code


class H2YDesc(C.Structure):
    """h2y_desc, include/hdr2yuv_hip.h."""

    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("in_sample_type", C.c_int32),
        ("src_bit_depth", C.c_int32), ("dst_bit_depth", C.c_int32),
        ("src_transfer", C.c_int32), ("dst_transfer", C.c_int32),
        ("src_matrix", C.c_int32), ("dst_matrix", C.c_int32),
        ("src_primaries", C.c_int32), ("dst_primaries", C.c_int32),
        ("dst_full_range", C.c_int32), ("dst_chroma_format_idc", C.c_int32),
        ("chroma_resampler_type", C.c_int32), ("stats_override", C.c_int32),
        ("floor", C.c_int32 * 3), ("ceiling", C.c_int32 * 3),
    ]


class H2YDpxInfo(C.Structure):
    """h2y_dpx_info, include/hdr2yuv_hip.h: what h2y_dpx_parse read from a DPX header."""

    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("bit_size", C.c_int32), ("swap", C.c_int32),
        ("data_offset", C.c_uint64), ("payload_bytes", C.c_uint64),
    ]

    def __repr__(self):
        return (f"H2YDpxInfo(width={self.width}, height={self.height}, bit_size={self.bit_size}, swap={self.swap}, "
                f"data_offset={self.data_offset}, payload_bytes={self.payload_bytes})")


TIFF_CUTOUT_HD = 1
TIFF_CUTOUT_QHD = 2
TIFF_FRAMES_PER_LAUNCH = 64


class H2YTiffInfo(C.Structure):
    """h2y_tiff_info, include/hdr2yuv_hip.h: what h2y_tiff_parse read from a TIFF and the picture read_tiff decodes from it."""

    _fields_ = [
        ("file_width", C.c_int32), ("file_height", C.c_int32), ("rows_per_strip", C.c_int32), ("swap", C.c_int32),
        ("width", C.c_int32), ("height", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32),
        ("row_bytes", C.c_uint64), ("payload_bytes", C.c_uint64), ("data_offset", C.c_uint64),
        ("contiguous", C.c_int32), ("reserved", C.c_int32),
    ]

    def __repr__(self):
        return (f"H2YTiffInfo(file={self.file_width}x{self.file_height} rps={self.rows_per_strip} swap={self.swap}, "
                f"decoded={self.width}x{self.height} at ({self.x0}, {self.y0}), row_bytes={self.row_bytes}, "
                f"payload_bytes={self.payload_bytes}, data_offset={self.data_offset}, contiguous={self.contiguous})")


EXR_NONE, EXR_RLE, EXR_ZIPS, EXR_ZIP = 0, 1, 2, 3
EXR_UINT, EXR_HALF, EXR_FLOAT, EXR_MISSING = 0, 1, 2, -1
EXR_CHUNK_RAW, EXR_CHUNK_ENCODED = 0, 1
EXR_FRAMES_PER_LAUNCH = 64


class H2YExrInfo(C.Structure):
    """h2y_exr_info, include/hdr2yuv_hip.h: what h2y_exr_parse read from a scanline OpenEXR file.  channel_type and
    channel_offset are indexed by plane: 0 = G, 1 = B, 2 = R."""

    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("x_min", C.c_int32), ("y_min", C.c_int32),
        ("compression", C.c_int32), ("line_order", C.c_int32), ("lines_per_chunk", C.c_int32), ("n_chunks", C.c_int32),
        ("n_channels", C.c_int32), ("all_half", C.c_int32), ("channel_type", C.c_int32 * 3), ("channel_offset", C.c_int32 * 3),
        ("line_bytes", C.c_int32), ("reserved", C.c_int32), ("flags_bytes", C.c_uint64), ("payload_bytes", C.c_uint64),
    ]

    def __repr__(self):
        return (f"H2YExrInfo({self.width}x{self.height} at ({self.x_min}, {self.y_min}), compression={self.compression}, "
                f"line_order={self.line_order}, chunks={self.n_chunks}x{self.lines_per_chunk}, channels={self.n_channels}, "
                f"all_half={self.all_half}, types={list(self.channel_type)}, offsets={list(self.channel_offset)}, "
                f"line_bytes={self.line_bytes}, payload_bytes={self.payload_bytes})")


class H2YExrChunk(C.Structure):
    """h2y_exr_chunk: one checked entry of the offset table."""

    _fields_ = [("offset", C.c_uint64), ("packed_bytes", C.c_uint32), ("row", C.c_int32)]


class H2YCompareStats(C.Structure):
    """h2y_compare_stats: per plane (0, 1, 2 = Y, Cb, Cr or G, B, R) the samples compared, the sums of squared and absolute
    differences, the count of |a - b| > sigma and the plane index of the first of them (-1: none), max |a - b|, and a and b
    at that first sample."""

    _fields_ = [
        ("samples", C.c_uint64 * 3), ("sse", C.c_uint64 * 3), ("sad", C.c_uint64 * 3), ("over", C.c_uint64 * 3),
        ("first_over", C.c_int64 * 3), ("max_abs", C.c_uint32 * 3), ("first_a", C.c_uint32 * 3), ("first_b", C.c_uint32 * 3),
        ("reserved", C.c_uint32),
    ]

    def as_dict(self):
        return {k: list(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}

    def __repr__(self):
        return f"H2YCompareStats({self.as_dict()})"


class H2YHistogramStats(C.Structure):
    """h2y_histogram_stats: per plane (0, 1, 2 = Y, Cb, Cr or G, B, R) the samples counted, those below, above and at the limits
    lo and hi of the legal range, the smallest and largest sample; nbins = 2^bits and shift = bit_depth - bits for every plane."""

    _fields_ = [
        ("samples", C.c_uint64 * 3), ("below", C.c_uint64 * 3), ("above", C.c_uint64 * 3), ("at_low", C.c_uint64 * 3),
        ("at_high", C.c_uint64 * 3), ("min", C.c_uint32 * 3), ("max", C.c_uint32 * 3), ("lo", C.c_uint32 * 3),
        ("hi", C.c_uint32 * 3), ("nbins", C.c_uint32), ("shift", C.c_uint32),
    ]

    def as_dict(self):
        return {k: (list(v) if not isinstance(v := getattr(self, k), int) else v) for k, _ in self._fields_}

    def __repr__(self):
        return f"H2YHistogramStats({self.as_dict()})"


class H2YSsimStats(C.Structure):
    """h2y_ssim_stats: per plane (0, 1, 2 = Y, Cb, Cr or G, B, R) the 8x8 windows, the sum over them of rint(SSIM x 2^32) and
    the plane's SSIM; all weights the planes by their sample counts."""

    _fields_ = [("windows", C.c_uint64 * 3), ("sum_q", C.c_int64 * 3), ("ssim", C.c_double * 3), ("all", C.c_double)]

    def as_dict(self):
        return {k: (list(v) if not isinstance(v := getattr(self, k), (int, float)) else v) for k, _ in self._fields_}

    def __repr__(self):
        return f"H2YSsimStats({self.as_dict()})"


class H2YRegionsStats(C.Structure):
    """h2y_regions_stats: per plane and class (0 flat, 1 busy) the 8x8 tiles, their samples, sum (a - b)^2 and sum |a - b|; per
    plane the samples above (below) the reference's local range, by how much in all and at most; flat_var and radius as given."""

    _fields_ = [("tiles", (C.c_uint64 * 2) * 3), ("samples", (C.c_uint64 * 2) * 3), ("sse", (C.c_uint64 * 2) * 3), ("sad", (C.c_uint64 * 2) * 3),
                ("over", C.c_uint64 * 3), ("over_sum", C.c_uint64 * 3), ("under", C.c_uint64 * 3), ("under_sum", C.c_uint64 * 3),
                ("over_max", C.c_uint32 * 3), ("under_max", C.c_uint32 * 3), ("flat_var", C.c_uint32), ("radius", C.c_uint32)]

    def as_dict(self):
        """Every field as plain ints: [plane][class] lists, [plane] lists, and the two settings."""
        def plain(v):
            return v if isinstance(v, int) else [plain(x) for x in v]
        return {k: plain(getattr(self, k)) for k, _ in self._fields_}

    def __repr__(self):
        return f"H2YRegionsStats({self.as_dict()})"


GAMUT_COMPRESS_FRAMES_PER_LAUNCH = 64  # H2Y_GAMUT_COMPRESS_FRAMES_PER_LAUNCH
GAMUT_COMPRESS_NODES = 1025  # H2Y_GAMUT_COMPRESS_NODES: entries of one channel's table
GAMUT_COMPRESS_THRESHOLD = 0.8  # H2Y_GAMUT_COMPRESS_THRESHOLD (rounded to binary32 on the way in)
GAMUT_COMPRESS_POWER = 1.2  # H2Y_GAMUT_COMPRESS_POWER


class H2YGamutCompressTables(C.Structure):
    """h2y_gamut_compress_tables"""

    _fields_ = [
        ("m", C.c_float * 9),
        ("threshold", C.c_float),
        ("power", C.c_float),
        ("limit", C.c_float * 3),
        ("scale", C.c_float * 3),
        ("table", (C.c_float * GAMUT_COMPRESS_NODES) * 3),
    ]


class H2YLightStats(C.Structure):
    """h2y_light_stats: a frame's content light -- the largest per-pixel max(L_G, L_B, L_R) as binary32 bits and the first pixel
    (x, y) holding it, the sum over the pixels of rint(m x 2^32), the pixel count, and cll / fall in cd/m2."""

    _fields_ = [("max_bits", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("reserved", C.c_uint32), ("sum_q", C.c_uint64),
                ("pixels", C.c_uint64), ("cll", C.c_double), ("fall", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}

    def __repr__(self):
        return f"H2YLightStats({self.as_dict()})"


class H2YLightdistStats(C.Structure):
    """h2y_lightdist_stats: a frame's light distribution -- the largest L of planes G, B, R and the largest m = max(L_G, L_B, L_R)
    as binary32 bits, the sum over the pixels of rint(m x 2^32), the pixel count, the pixels with m <= 0.01f, and the lower bin edges
    of the LIGHTDIST_PCT percentiles of m as binary32 bits."""

    _fields_ = [("maxscl_bits", C.c_uint32 * 3), ("max_bits", C.c_uint32), ("sum_q", C.c_uint64), ("pixels", C.c_uint64),
                ("below_100", C.c_uint64), ("pct_bits", C.c_uint32 * len(LIGHTDIST_PCT))]

    def as_dict(self):
        return dict(maxscl_bits=list(self.maxscl_bits), max_bits=self.max_bits, sum_q=self.sum_q, pixels=self.pixels,
                    below_100=self.below_100, pct_bits=list(self.pct_bits))

    def __repr__(self):
        return f"H2YLightdistStats({self.as_dict()})"


class H2YScenesig(C.Structure):
    """h2y_scenesig: a frame's scene signature -- per cell of the 16 x 9 grid (row-major, cy * 16 + cx) the sum over its pixels of
    the logarithmic bin of m = max(L_G, L_B, L_R), and the pixel count."""

    _fields_ = [("cell", C.c_uint64 * (SCENESIG_COLS * SCENESIG_ROWS)), ("pixels", C.c_uint64)]

    def as_dict(self):
        return dict(cell=list(self.cell), pixels=self.pixels)

    def __repr__(self):
        return f"H2YScenesig({self.as_dict()})"


class H2YGamutcheckSet(C.Structure):
    """h2y_gamutcheck_set: one check set's figures of a frame -- the set's code, the first pixel that holds the largest excursion
    ((-1, -1) when no pixel is outside), that excursion as binary32 bits, the pixels outside and beyond, the sum over the pixels of
    rint(e x 2^32), and the host's doubles."""

    _fields_ = [("primaries", C.c_int32), ("max_x", C.c_int32), ("max_y", C.c_int32), ("max_bits", C.c_uint32),
                ("outside", C.c_uint64), ("beyond", C.c_uint64), ("sum_q", C.c_uint64),
                ("max_cdm2", C.c_double), ("mean_cdm2", C.c_double), ("beyond_share", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def __repr__(self):
        return f"H2YGamutcheckSet({self.as_dict()})"


class H2YGamutcheckStats(C.Structure):
    """h2y_gamutcheck_stats: a frame's gamut containment check -- its pixel count and the figures of its n_sets check sets."""

    _fields_ = [("pixels", C.c_uint64), ("n_sets", C.c_int32), ("reserved", C.c_int32), ("set", H2YGamutcheckSet * GAMUTCHECK_MAX_SETS)]

    def as_dict(self):
        return dict(pixels=self.pixels, n_sets=self.n_sets, sets=[self.set[s].as_dict() for s in range(self.n_sets)])

    def __repr__(self):
        return f"H2YGamutcheckStats({self.as_dict()})"


class H2YSceneStats(C.Structure):
    """h2y_scene_stats: a scene's figures -- its first frame and frame count, the maxima over its frames, the 128-bit sum of their
    sum_q, the sums of their pixels and below_100, and the percentiles of their summed bins."""

    _fields_ = [("first_frame", C.c_int64), ("n_frames", C.c_int64), ("maxscl_bits", C.c_uint32 * 3), ("max_bits", C.c_uint32),
                ("sum_q_hi", C.c_uint64), ("sum_q_lo", C.c_uint64), ("pixels", C.c_uint64), ("below_100", C.c_uint64),
                ("pct_bits", C.c_uint32 * len(LIGHTDIST_PCT))]

    def as_dict(self):
        return dict(first_frame=self.first_frame, n_frames=self.n_frames, maxscl_bits=list(self.maxscl_bits), max_bits=self.max_bits,
                    sum_q=(self.sum_q_hi << 64) | self.sum_q_lo, pixels=self.pixels, below_100=self.below_100,
                    pct_bits=list(self.pct_bits))

    def __repr__(self):
        return f"H2YSceneStats({self.as_dict()})"


class H2YDeltaeStats(C.Structure):
    """h2y_deltae_stats: a frame's Delta E ITP against its reference -- the largest per-pixel d as binary32 bits and the first pixel
    (max_x, max_y) holding it, the caller's threshold, the sum over the pixels of rint(d x 2^20), the pixel count, the pixels with
    d > threshold, and mean / max as doubles."""

    _fields_ = [("max_bits", C.c_uint32), ("max_x", C.c_uint32), ("max_y", C.c_uint32), ("threshold", C.c_float), ("sum_q", C.c_uint64),
                ("pixels", C.c_uint64), ("over", C.c_uint64), ("mean", C.c_double), ("max", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def __repr__(self):
        return f"H2YDeltaeStats({self.as_dict()})"


class H2YCodelightDesc(C.Structure):
    """h2y_codelight_desc: frames of three u16 PQ code planes whose light codelight_batch and codelight_stream_open measure --
    matrix_coeffs 0 (G, B, R), 1 (BT.709) or 9 (BT.2020nc); chroma_format_idc 3, or 1 with even sizes; algorithm: the 4:2:0
    upsampler (0 replication, otherwise the FIR the context's inverse chroma siting selects)."""

    _fields_ = [(n, C.c_int) for n in ("width", "height", "chroma_format_idc", "bit_depth", "full_range", "matrix_coeffs", "algorithm")]


def make_codelight_desc(width, height, chroma=3, bit_depth=10, full_range=0, matrix=9, algorithm=1) -> H2YCodelightDesc:
    return H2YCodelightDesc(width, height, chroma, bit_depth, full_range, matrix, algorithm)


def make_desc(width, height, *, sample=SAMPLE_F32, src_depth=32, dst_depth=10, src_transfer=TRANSFER_LINEAR,
              dst_transfer=TRANSFER_PQ, src_matrix=MATRIX_GBR, dst_matrix=MATRIX_BT2020NC, src_primaries=9,
              dst_primaries=9, full_range=0, chroma=CHROMA_420, resampler=1, stats=None) -> H2YDesc:
    d = H2YDesc()
    d.width, d.height = width, height
    d.in_sample_type = sample
    d.src_bit_depth, d.dst_bit_depth = src_depth, dst_depth
    d.src_transfer, d.dst_transfer = src_transfer, dst_transfer
    d.src_matrix, d.dst_matrix = src_matrix, dst_matrix
    d.src_primaries, d.dst_primaries = src_primaries, dst_primaries
    d.dst_full_range = full_range
    d.dst_chroma_format_idc = chroma
    d.chroma_resampler_type = resampler
    if stats is not None:
        d.stats_override = 1
        for c in range(3):
            d.floor[c], d.ceiling[c] = int(stats[c][0]), int(stats[c][1])
    return d


_LIB_PATH = os.path.join(_HERE, "libhdr2yuv_hip.so")


def library_path() -> str:
    return _LIB_PATH


ABI_VERSION = 1
ABI_EXPERIMENT = 0x40000000  # H2Y_ABI_EXPERIMENT: a -DH2Y_EXPERIMENT build (timing variants, may write wrong bytes)
_ALLOW_EXPERIMENT = False


def set_library_path(path: str, allow_experiment: bool = False) -> None:
    """Load another build of the same library (tuning experiments: bench.py --lib, tools/).  Explicit, never from the
    environment; must be called before the first load_library().  A timing-experiment build (h2y_abi_version() carries
    H2Y_ABI_EXPERIMENT) is refused unless allow_experiment."""
    global _LIB_PATH, _ALLOW_EXPERIMENT
    if _LIB is not None:
        raise RuntimeError("the library is already loaded")
    _LIB_PATH = os.path.abspath(path)
    _ALLOW_EXPERIMENT = allow_experiment


def is_experiment_build() -> bool:
    return bool(load_library().h2y_abi_version() & ABI_EXPERIMENT)


def build_library(force: bool = False) -> str:
    """hipcc --offload-arch=gfx950 build of the kernels + shim, in-tree."""
    args = ["make", "-j4", "-C", os.path.join(_HERE, "csrc"), "--no-print-directory"]
    if force:
        args.append("-B")
    subprocess.run(args, check=True)
    return library_path()


def load_library():
    """Load libhdr2yuv_hip.so. Raises if it has not been built: there is no
    Python or CPU implementation to fall back to."""
    global _LIB
    if _LIB is not None:
        return _LIB
    try:
        # One HIP runtime per process: torch ships its own libamdhip64.so.7; load it
        # first so that our library binds to the same copy (two runtimes in one
        # process cannot both own the device).  Plumbing only -- not required by the
        # library itself (the C++ CLI links the system runtime).
        import torch  # noqa: F401
    except ImportError:
        pass
    path = library_path()
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not built: run hdr2yuv_amd.build_library() (needs hipcc)")
    L = C.CDLL(path)
    L.h2y_abi_version.restype = C.c_int
    ver = L.h2y_abi_version()
    if ver & ABI_EXPERIMENT and not _ALLOW_EXPERIMENT:
        raise RuntimeError(f"{path} is a timing-experiment build (-DH2Y_EXPERIMENT): its kernels may write wrong bytes; refused")
    if ver & ~ABI_EXPERIMENT != ABI_VERSION:
        raise RuntimeError(f"{path}: ABI version {ver & ~ABI_EXPERIMENT}, this binding is for {ABI_VERSION}")
    L.h2y_frame_bytes.restype = C.c_size_t
    L.h2y_frame_bytes.argtypes = [C.POINTER(H2YDesc)]
    L.h2y_plane_bytes.restype = C.c_size_t
    L.h2y_plane_bytes.argtypes = [C.POINTER(H2YDesc)]
    L.h2y_desc_check.restype = C.c_int
    L.h2y_desc_check.argtypes = [C.POINTER(H2YDesc), C.POINTER(C.c_char_p)]
    L.h2y_ctx_create.restype = C.c_int
    L.h2y_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.h2y_ctx_destroy.restype = None
    L.h2y_ctx_destroy.argtypes = [C.c_void_p]
    L.h2y_last_error.restype = C.c_char_p
    L.h2y_last_error.argtypes = [C.c_void_p]
    L.h2y_ctx_set_option.restype = C.c_int
    L.h2y_ctx_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    L.h2y_ctx_set_stream.restype = C.c_int
    L.h2y_ctx_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.h2y_convert_frame.restype = C.c_int
    L.h2y_convert_frame.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.POINTER(C.c_void_p), C.c_void_p]
    for name in ("h2y_convert_batch", "h2y_convert_batch_enqueue"):
        fn = getattr(L, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_batch_finish.restype = C.c_int
    L.h2y_batch_finish.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.h2y_pic_stats.restype = C.c_int
    L.h2y_pic_stats.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_float),
                                C.POINTER(C.c_int32)]
    L.h2y_matrix_convert.restype = C.c_int
    L.h2y_matrix_convert.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_subsample_420.restype = C.c_int
    L.h2y_subsample_420.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.h2y_subsample_420_sited.restype = C.c_int
    L.h2y_subsample_420_sited.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.h2y_ctx_set_chroma_siting.restype = C.c_int
    L.h2y_ctx_set_chroma_siting.argtypes = [C.c_void_p, C.c_int]
    L.h2y_ctx_set_inverse_chroma_siting.restype = C.c_int
    L.h2y_ctx_set_inverse_chroma_siting.argtypes = [C.c_void_p, C.c_int]
    L.h2y_upsample_444_sited.restype = C.c_int
    L.h2y_upsample_444_sited.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
    L.h2y_matrix_inverse.restype = C.c_int
    L.h2y_matrix_inverse.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_upsample_444.restype = C.c_int
    L.h2y_upsample_444.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
    L.h2y_inverse_420.restype = C.c_int
    L.h2y_inverse_420.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_inverse_frame.restype = C.c_int
    L.h2y_inverse_frame.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_inverse_batch.restype = C.c_int
    L.h2y_inverse_batch.argtypes = [C.c_void_p] + [C.c_int] * 9 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_inverse_stream_open.restype = C.c_int
    L.h2y_inverse_stream_open.argtypes = [C.c_void_p] + [C.c_int] * 9
    L.h2y_dpx_parse.restype = C.c_int
    L.h2y_dpx_parse.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.POINTER(H2YDpxInfo), C.POINTER(C.c_char_p)]
    L.h2y_dpx_decode_batch.restype = C.c_int
    L.h2y_dpx_decode_batch.argtypes = [C.c_void_p, C.POINTER(H2YDpxInfo), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_dpx_stream_open.restype = C.c_int
    L.h2y_dpx_stream_open.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.POINTER(H2YDpxInfo), C.c_int]
    L.h2y_tiff_parse.restype = C.c_int
    L.h2y_tiff_parse.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(H2YTiffInfo), C.POINTER(C.c_uint64), C.c_int,
                                 C.POINTER(C.c_char_p)]
    L.h2y_tiff_layout.restype = C.c_int
    L.h2y_tiff_layout.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    L.h2y_tiff_decode_batch.restype = C.c_int
    L.h2y_tiff_decode_batch.argtypes = [C.c_void_p, C.POINTER(H2YTiffInfo), C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_void_p)]
    L.h2y_rgb_interleave_batch.restype = C.c_int
    L.h2y_rgb_interleave_batch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_tiff_stream_open.restype = C.c_int
    L.h2y_tiff_stream_open.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.POINTER(H2YTiffInfo), C.c_int, C.c_int]
    L.h2y_tiff_inverse_stream_open.restype = C.c_int
    L.h2y_tiff_inverse_stream_open.argtypes = [C.c_void_p] + [C.c_int] * 9
    L.h2y_exr_parse.restype = C.c_int
    L.h2y_exr_parse.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(H2YExrInfo), C.POINTER(H2YExrChunk), C.c_int, C.POINTER(C.c_char_p)]
    L.h2y_exr_unpack.restype = C.c_int
    L.h2y_exr_unpack.argtypes = [C.POINTER(H2YExrInfo), C.POINTER(H2YExrChunk), C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                 C.POINTER(C.c_char_p)]
    L.h2y_exr_decode_batch.restype = C.c_int
    L.h2y_exr_decode_batch.argtypes = [C.c_void_p, C.POINTER(H2YExrInfo), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_exr_stream_open.restype = C.c_int
    L.h2y_exr_stream_open.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.POINTER(H2YExrInfo), C.c_int]
    L.h2y_stream_open.restype = C.c_int
    L.h2y_compare_batch.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                                     C.POINTER(H2YCompareStats)]
    L.h2y_compare_batch.restype = C.c_int
    L.h2y_stream_compare.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.h2y_stream_compare.restype = C.c_int
    L.h2y_stream_reference.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.h2y_stream_reference.restype = C.c_int
    L.h2y_stream_compare_result.argtypes = [C.c_void_p, C.POINTER(H2YCompareStats)]
    L.h2y_stream_compare_result.restype = C.c_int
    L.h2y_compare_stream_open.argtypes = [C.c_void_p] + [C.c_int] * 5
    L.h2y_compare_stream_open.restype = C.c_int
    L.h2y_histogram_batch.argtypes = [C.c_void_p] + [C.c_int] * 8 + [C.POINTER(C.c_void_p), C.POINTER(H2YHistogramStats), C.c_void_p]
    L.h2y_histogram_batch.restype = C.c_int
    L.h2y_stream_histogram.argtypes = [C.c_void_p, C.c_int]
    L.h2y_stream_histogram.restype = C.c_int
    L.h2y_stream_histogram_ex.argtypes = [C.c_void_p] + [C.c_int] * 4
    L.h2y_stream_histogram_ex.restype = C.c_int
    L.h2y_stream_histogram_result.argtypes = [C.c_void_p, C.POINTER(H2YHistogramStats), C.c_void_p]
    L.h2y_stream_histogram_result.restype = C.c_int
    L.h2y_histogram_stream_open.argtypes = [C.c_void_p] + [C.c_int] * 8
    L.h2y_histogram_stream_open.restype = C.c_int
    L.h2y_ssim_batch.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(H2YSsimStats)]
    L.h2y_ssim_batch.restype = C.c_int
    L.h2y_stream_ssim.argtypes = [C.c_void_p, C.c_int]
    L.h2y_stream_ssim.restype = C.c_int
    L.h2y_stream_ssim_result.argtypes = [C.c_void_p, C.POINTER(H2YSsimStats)]
    L.h2y_stream_ssim_result.restype = C.c_int
    L.h2y_regions_host.argtypes = [C.c_int] * 3 + [C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(H2YRegionsStats)]
    L.h2y_regions_host.restype = C.c_int
    L.h2y_regions_batch.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                    C.POINTER(H2YRegionsStats)]
    L.h2y_regions_batch.restype = C.c_int
    L.h2y_stream_regions.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    L.h2y_stream_regions.restype = C.c_int
    L.h2y_stream_regions_result.argtypes = [C.c_void_p, C.POINTER(H2YRegionsStats)]
    L.h2y_stream_regions_result.restype = C.c_int
    L.h2y_light_batch.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.c_int, C.POINTER(C.c_void_p), C.POINTER(H2YLightStats)]
    L.h2y_light_batch.restype = C.c_int
    L.h2y_stream_light.argtypes = [C.c_void_p]
    L.h2y_stream_light.restype = C.c_int
    L.h2y_stream_light_result.argtypes = [C.c_void_p, C.POINTER(H2YLightStats)]
    L.h2y_stream_light_result.restype = C.c_int
    L.h2y_lightdist_batch.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.c_int, C.POINTER(C.c_void_p), C.POINTER(H2YLightdistStats), C.c_void_p]
    L.h2y_lightdist_batch.restype = C.c_int
    L.h2y_stream_lightdist.argtypes = [C.c_void_p]
    L.h2y_stream_lightdist.restype = C.c_int
    L.h2y_stream_lightdist_result.argtypes = [C.c_void_p, C.POINTER(H2YLightdistStats)]
    L.h2y_stream_lightdist_result.restype = C.c_int
    L.h2y_codelight_batch.argtypes = [C.c_void_p, C.POINTER(H2YCodelightDesc), C.c_int, C.POINTER(C.c_void_p), C.POINTER(H2YLightStats),
                                      C.POINTER(H2YLightdistStats), C.c_void_p]
    L.h2y_codelight_batch.restype = C.c_int
    L.h2y_codelight_stream_open.argtypes = [C.c_void_p, C.POINTER(H2YCodelightDesc), C.c_int, C.c_int]
    L.h2y_codelight_stream_open.restype = C.c_int
    L.h2y_linearize_batch.argtypes = [C.c_void_p, C.POINTER(H2YCodelightDesc), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_linearize_batch.restype = C.c_int
    L.h2y_pqcode_stream_open.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.POINTER(H2YCodelightDesc), C.c_int]
    L.h2y_pqcode_stream_open.restype = C.c_int
    L.h2y_deltae_batch.argtypes = [C.c_void_p, C.POINTER(H2YCodelightDesc), C.c_float, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                   C.POINTER(H2YDeltaeStats)]
    L.h2y_deltae_batch.restype = C.c_int
    L.h2y_stream_deltae.argtypes = [C.c_void_p, C.POINTER(H2YCodelightDesc), C.c_float]
    L.h2y_stream_deltae.restype = C.c_int
    L.h2y_stream_deltae_result.argtypes = [C.c_void_p, C.POINTER(H2YDeltaeStats)]
    L.h2y_stream_deltae_result.restype = C.c_int
    L.h2y_lightdist_json.argtypes = [C.POINTER(H2YLightdistStats), C.c_int, C.c_long, C.c_char_p, C.c_size_t]
    L.h2y_lightdist_json.restype = C.c_size_t
    L.h2y_scenesig_batch.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.c_int, C.POINTER(C.c_void_p), C.POINTER(H2YScenesig)]
    L.h2y_scenesig_batch.restype = C.c_int
    L.h2y_codescenesig_batch.argtypes = [C.c_void_p, C.POINTER(H2YCodelightDesc), C.c_int, C.POINTER(C.c_void_p), C.POINTER(H2YScenesig)]
    L.h2y_codescenesig_batch.restype = C.c_int
    L.h2y_gamutcheck_planes.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.c_double, C.c_double, C.c_int, C.c_int,
                                        C.POINTER(C.c_void_p), C.POINTER(H2YGamutcheckStats)]
    L.h2y_gamutcheck_planes.restype = C.c_int
    L.h2y_gamutcheck_batch.argtypes = [C.c_void_p, C.POINTER(H2YCodelightDesc), C.c_int, C.c_int, C.POINTER(C.c_int), C.c_double,
                                       C.c_double, C.c_int, C.POINTER(C.c_void_p), C.POINTER(H2YGamutcheckStats)]
    L.h2y_gamutcheck_batch.restype = C.c_int
    L.h2y_stream_gamutcheck.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_double, C.c_double]
    L.h2y_stream_gamutcheck.restype = C.c_int
    L.h2y_stream_gamutcheck_result.argtypes = [C.c_void_p, C.POINTER(H2YGamutcheckStats)]
    L.h2y_stream_gamutcheck_result.restype = C.c_int
    L.h2y_stream_scenesig.argtypes = [C.c_void_p]
    L.h2y_stream_scenesig.restype = C.c_int
    L.h2y_stream_scenesig_result.argtypes = [C.c_void_p, C.POINTER(H2YScenesig)]
    L.h2y_stream_scenesig_result.restype = C.c_int
    L.h2y_stream_lightdist_bins.argtypes = [C.c_void_p, C.c_void_p]
    L.h2y_stream_lightdist_bins.restype = C.c_int
    L.h2y_scene_distance.argtypes = [C.POINTER(H2YScenesig), C.POINTER(H2YScenesig)]
    L.h2y_scene_distance.restype = C.c_double
    L.h2y_scene_cuts.argtypes = [C.POINTER(H2YScenesig), C.c_int, C.c_double, C.POINTER(C.c_int32)]
    L.h2y_scene_cuts.restype = C.c_int
    L.h2y_scene_merge.argtypes = [C.POINTER(H2YLightdistStats), C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(H2YSceneStats), C.c_int]
    L.h2y_scene_merge.restype = C.c_int
    L.h2y_lightdist_json_scenes.argtypes = [C.POINTER(H2YSceneStats), C.c_int, C.c_long, C.c_char_p, C.c_size_t]
    L.h2y_lightdist_json_scenes.restype = C.c_size_t
    L.h2y_scale_taps.argtypes = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.POINTER(C.c_int)]
    L.h2y_scale_taps.restype = C.c_int
    L.h2y_scale_frame_bytes.argtypes = [C.c_int] * 3
    L.h2y_scale_frame_bytes.restype = C.c_size_t
    L.h2y_scale_batch.argtypes = [C.c_void_p] + [C.c_int] * 10 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_scale_batch.restype = C.c_int
    L.h2y_stream_scale.argtypes = [C.c_void_p] + [C.c_int] * 3
    L.h2y_stream_scale.restype = C.c_int
    L.h2y_scale_stream_open.argtypes = [C.c_void_p] + [C.c_int] * 10
    L.h2y_scale_stream_open.restype = C.c_int
    L.h2y_dither_offsets.argtypes = [C.c_int] * 3 + [C.c_uint32] * 2 + [C.c_int] * 3 + [C.c_void_p]
    L.h2y_dither_offsets.restype = C.c_int
    L.h2y_dither_batch.argtypes = ([C.c_void_p] + [C.c_int] * 9 + [C.c_uint32] * 2 + [C.c_int]
                                   + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)])
    L.h2y_dither_batch.restype = C.c_int
    L.h2y_stream_dither.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_uint32] * 2
    L.h2y_stream_dither.restype = C.c_int
    L.h2y_dither_stream_open.argtypes = [C.c_void_p] + [C.c_int] * 9 + [C.c_uint32] * 2 + [C.c_int]
    L.h2y_dither_stream_open.restype = C.c_int
    L.h2y_pack_frame_bytes.argtypes = [C.c_int] * 4
    L.h2y_pack_frame_bytes.restype = C.c_size_t
    L.h2y_pack_frame.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p]
    L.h2y_pack_frame.restype = C.c_int
    L.h2y_unpack_frame.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p]
    L.h2y_unpack_frame.restype = C.c_int
    for fn in (L.h2y_pack_batch, L.h2y_unpack_batch):
        fn.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        fn.restype = C.c_int
    L.h2y_stream_pack.argtypes = [C.c_void_p, C.c_int]
    L.h2y_stream_pack.restype = C.c_int
    L.h2y_stream_unpack.argtypes = [C.c_void_p, C.c_int]
    L.h2y_stream_unpack.restype = C.c_int
    L.h2y_stream_unpack_ex.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.h2y_stream_unpack_ex.restype = C.c_int
    L.h2y_gamut_matrix.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_char_p)]
    L.h2y_gamut_matrix.restype = C.c_int
    L.h2y_gamut_batch.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_gamut_batch.restype = C.c_int
    L.h2y_stream_gamut.argtypes = [C.c_void_p] + [C.c_int] * 3
    L.h2y_stream_gamut.restype = C.c_int
    L.h2y_gamut_compress_curve.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(H2YGamutCompressTables), C.POINTER(C.c_char_p)]
    L.h2y_gamut_compress_curve.restype = C.c_int
    L.h2y_gamut_compress_planes.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_size_t, C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_void_p)]
    L.h2y_gamut_compress_planes.restype = C.c_int
    L.h2y_gamut_compress_batch.argtypes = ([C.c_void_p] + [C.c_int] * 5 + [C.c_float, C.c_float, C.c_int]
                                           + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)])
    L.h2y_gamut_compress_batch.restype = C.c_int
    L.h2y_stream_gamut_compress.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float]
    L.h2y_stream_gamut_compress.restype = C.c_int
    L.h2y_tonemap_curve.argtypes = [C.c_int] * 3 + [C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_char_p)]
    L.h2y_tonemap_curve.restype = C.c_int
    L.h2y_tonemap_batch.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_tonemap_batch.restype = C.c_int
    L.h2y_lut3d_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p)]
    L.h2y_lut3d_parse.restype = C.c_int
    L.h2y_lut3d_free.argtypes = [C.c_void_p]
    L.h2y_lut3d_free.restype = None
    L.h2y_lut3d_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_char_p)]
    L.h2y_lut3d_info.restype = C.c_int
    L.h2y_lut3d_nodes.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.h2y_lut3d_nodes.restype = C.c_int
    L.h2y_lut3d_planes.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_lut3d_planes.restype = C.c_int
    L.h2y_lut3d_batch.argtypes = [C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_lut3d_batch.restype = C.c_int
    L.h2y_stream_lut3d.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.h2y_stream_lut3d.restype = C.c_int
    L.h2y_hlg_tables.argtypes = [C.c_int] * 2 + [C.POINTER(C.c_float)] * 3 + [C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
    L.h2y_hlg_tables.restype = C.c_int
    L.h2y_hlg_planes.argtypes = [C.c_int] * 6 + [C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_hlg_planes.restype = C.c_int
    L.h2y_hlg_inverse_tables.argtypes = [C.c_int] + [C.POINTER(C.c_float)] * 3 + [C.POINTER(C.c_double), C.POINTER(C.c_char_p)]
    L.h2y_hlg_inverse_tables.restype = C.c_int
    L.h2y_hlg_inverse_planes.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_hlg_inverse_planes.restype = C.c_int
    L.h2y_hlg_linearize_batch.argtypes = [C.c_void_p, C.POINTER(H2YCodelightDesc), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_hlg_linearize_batch.restype = C.c_int
    L.h2y_hlgcode_stream_open.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.POINTER(H2YCodelightDesc), C.c_int, C.c_int]
    L.h2y_hlgcode_stream_open.restype = C.c_int
    L.h2y_sdr_inverse_planes.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_sdr_inverse_planes.restype = C.c_int
    L.h2y_sdr_linearize_batch.argtypes = [C.c_void_p, C.POINTER(H2YCodelightDesc), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_sdr_linearize_batch.restype = C.c_int
    L.h2y_sdrcode_stream_open.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.POINTER(H2YCodelightDesc), C.c_int, C.c_int]
    L.h2y_sdrcode_stream_open.restype = C.c_int
    L.h2y_code_signal_planes.argtypes = [C.POINTER(H2YCodelightDesc), C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_code_signal_planes.restype = C.c_int
    L.h2y_code_signal_batch.argtypes = [C.c_void_p, C.POINTER(H2YCodelightDesc), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_code_signal_batch.restype = C.c_int
    L.h2y_sigcode_stream_open.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.POINTER(H2YCodelightDesc), C.c_void_p, C.c_int, C.c_int]
    L.h2y_sigcode_stream_open.restype = C.c_int
    L.h2y_hlg_batch.argtypes = [C.c_void_p] + [C.c_int] * 9 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_hlg_batch.restype = C.c_int
    L.h2y_stream_hlg.argtypes = [C.c_void_p] + [C.c_int] * 2
    L.h2y_stream_hlg.restype = C.c_int
    L.h2y_ictcp_batch.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.h2y_ictcp_batch.restype = C.c_int
    L.h2y_stream_ictcp.argtypes = [C.c_void_p]
    L.h2y_stream_ictcp.restype = C.c_int
    L.h2y_stream_tonemap.argtypes = [C.c_void_p] + [C.c_int] * 3
    L.h2y_stream_tonemap.restype = C.c_int
    L.h2y_stream_open.argtypes = [C.c_void_p, C.POINTER(H2YDesc), C.c_int]
    L.h2y_stream_input.restype = C.c_int
    L.h2y_stream_input.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.h2y_stream_submit.restype = C.c_int
    L.h2y_stream_submit.argtypes = [C.c_void_p]
    L.h2y_stream_output.restype = C.c_int
    L.h2y_stream_output.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint16))]
    L.h2y_stream_close.restype = C.c_int
    L.h2y_stream_close.argtypes = [C.c_void_p]
    L.h2y_last_kernel_name.restype = C.c_char_p
    L.h2y_last_kernel_name.argtypes = [C.c_void_p]
    L.h2y_last_kernel_variant.restype = C.c_char_p
    L.h2y_last_kernel_variant.argtypes = [C.c_void_p]
    L.h2y_last_kernel_ms.restype = C.c_int
    L.h2y_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    _LIB = L
    return L


def frame_bytes(d: H2YDesc) -> int:
    return int(load_library().h2y_frame_bytes(C.byref(d)))


def desc_check(d: H2YDesc):
    why = C.c_char_p()
    rc = load_library().h2y_desc_check(C.byref(d), C.byref(why))
    return rc, (why.value or b"").decode()


def parse_dpx(header_bytes: bytes, file_bytes: int) -> H2YDpxInfo:
    """h2y_dpx_parse on the host (no device needed): header_bytes = the file's first bytes (2048 at least), file_bytes = its
    size.  Raises ValueError with the library's reason where the file is refused."""
    buf = bytes(header_bytes)
    info = H2YDpxInfo()
    why = C.c_char_p()
    rc = load_library().h2y_dpx_parse(buf, len(buf), int(file_bytes), C.byref(info), C.byref(why))
    if rc != H2Y_OK:
        raise ValueError((why.value or b"").decode())
    return info


def parse_tiff(data, cutout=0):
    """h2y_tiff_parse on the host (no device needed): data = the whole file (bytes or a uint8 array), cutout = TIFF_CUTOUT_*
    bits.  Returns (info, row_offsets): the file offset of each decoded row as a uint64 array.  Raises ValueError with the
    library's reason where the file is refused; warns where an "MM" file is decoded byte-swapped (the reference would not)."""
    import numpy as np

    buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    lib = load_library()
    info = H2YTiffInfo()
    why = C.c_char_p()
    ptr = buf.ctypes.data_as(C.c_void_p)
    if lib.h2y_tiff_parse(ptr, buf.size, int(cutout), C.byref(info), None, 0, C.byref(why)) != H2Y_OK:
        raise ValueError((why.value or b"").decode())
    rows = np.zeros(info.height, np.uint64)
    rc = lib.h2y_tiff_parse(ptr, buf.size, int(cutout), C.byref(info), rows.ctypes.data_as(C.POINTER(C.c_uint64)), rows.size, C.byref(why))
    if rc != H2Y_OK:
        raise ValueError((why.value or b"").decode())
    if info.swap:
        import warnings

        warnings.warn("big-endian (MM) TIFF: decoded with the bytes of each sample exchanged; the reference reads them unswapped",
                      stacklevel=2)
    return info, rows


def tiff_layout(width, height):
    """h2y_tiff_layout: (head, tail) -- the bytes before and after the 6 x width x height bytes of interleaved R,G,B u16 samples
    in the file libtiff 4.3 writes for write_tiff()."""
    lib = load_library()
    head = (C.c_uint8 * 8)()
    n = C.c_size_t(0)
    if lib.h2y_tiff_layout(width, height, head, None, C.byref(n)) != H2Y_OK:
        raise ValueError((lib.h2y_last_error(None) or b"").decode())
    tail = (C.c_uint8 * n.value)()
    if lib.h2y_tiff_layout(width, height, head, tail, C.byref(n)) != H2Y_OK:
        raise ValueError((lib.h2y_last_error(None) or b"").decode())
    return bytes(head), bytes(tail)


def parse_exr(data):
    """h2y_exr_parse on the host (no device needed): data = the whole file (bytes or a uint8 array).  Returns (info, chunks):
    chunks is a ctypes array of H2YExrChunk, one per offset-table entry in increasing y.  Raises ValueError with the library's
    reason where the file is refused."""
    import numpy as np

    buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    lib = load_library()
    info = H2YExrInfo()
    why = C.c_char_p()
    ptr = buf.ctypes.data_as(C.c_void_p)
    if lib.h2y_exr_parse(ptr, buf.size, C.byref(info), None, 0, C.byref(why)) != H2Y_OK:
        raise ValueError((why.value or b"").decode())
    chunks = (H2YExrChunk * info.n_chunks)()
    if lib.h2y_exr_parse(ptr, buf.size, C.byref(info), chunks, info.n_chunks, C.byref(why)) != H2Y_OK:
        raise ValueError((why.value or b"").decode())
    return info, chunks


def exr_unpack(info, chunks, data, payload=None, first=0, count=None):
    """h2y_exr_unpack: chunks [first, first + count) of the file `data` into payload (a uint8 array of info.payload_bytes,
    made when None).  Returns the payload.  Raises ValueError with the library's reason."""
    import numpy as np

    buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    if payload is None:
        payload = np.zeros(info.payload_bytes, np.uint8)
    if payload.dtype != np.uint8 or payload.size < info.payload_bytes or not payload.flags.c_contiguous:
        raise ValueError("payload must be a contiguous uint8 array of info.payload_bytes")
    count = info.n_chunks - first if count is None else count
    why = C.c_char_p()
    lib = load_library()
    if lib.h2y_exr_unpack(C.byref(info), chunks, buf.ctypes.data_as(C.c_void_p), first, count,
                          payload.ctypes.data_as(C.c_void_p), C.byref(why)) != H2Y_OK:
        raise ValueError((why.value or b"").decode())
    return payload


def _np_dtype(sample):
    return np.float32 if sample == SAMPLE_F32 else np.uint16


def scale_taps(src: int, dst: int, a: int = 3):
    """h2y_scale_taps: the Lanczos tap table of one axis (host only, no device): (first int32[dst], count int32[dst],
    coef int16[dst, 32], max_taps)."""
    lib = load_library()
    n = max(dst, 1)
    first = np.zeros(n, dtype=np.int32)
    count = np.zeros(n, dtype=np.int32)
    coef = np.zeros((n, SCALE_TAPS), dtype=np.int16)
    most = C.c_int(0)
    rc = lib.h2y_scale_taps(src, dst, a, first.ctypes.data, count.ctypes.data, coef.ctypes.data, C.byref(most))
    if rc != H2Y_OK:
        raise H2YError(rc, (lib.h2y_last_error(None) or b"").decode())
    return first, count, coef, most.value


def dither_offsets(mode: int, shift: int, temporal: int, seed: int, frame: int, plane: int, width: int, height: int):
    """h2y_dither_offsets: t of every sample of one plane (host only, no device): uint16[height, width]."""
    lib = load_library()
    t = np.zeros((max(height, 1), max(width, 1)), dtype=np.uint16)
    rc = lib.h2y_dither_offsets(mode, shift, temporal, seed & 0xFFFFFFFF, frame & 0xFFFFFFFF, plane, width, height, t.ctypes.data)
    if rc != H2Y_OK:
        raise H2YError(rc, (lib.h2y_last_error(None) or b"").decode())
    return t


def regions_host(width: int, height: int, chroma: int, flat_var: int, radius: int, a, b) -> H2YRegionsStats:
    """h2y_regions_host (host only, no device): the figures of frame a against frame b, each three u16 planes one after the other."""
    lib = load_library()
    fa = None if a is None else np.ascontiguousarray(a, dtype=np.uint16).reshape(-1)
    fb = None if b is None else np.ascontiguousarray(b, dtype=np.uint16).reshape(-1)
    if width >= 1 and height >= 1 and chroma in (CHROMA_420, CHROMA_444):
        for f in (fa, fb):
            if f is not None and f.size != _frame_samples(width, height, chroma):
                raise ValueError("a frame does not hold width x height samples and its two chroma planes")
    st = H2YRegionsStats()
    rc = lib.h2y_regions_host(width, height, chroma, flat_var, radius, None if fa is None else fa.ctypes.data,
                              None if fb is None else fb.ctypes.data, C.byref(st))
    if rc != H2Y_OK:
        raise H2YError(rc, (lib.h2y_last_error(None) or b"").decode())
    return st


def pack_frame_bytes(width: int, height: int, chroma: int, packing: int) -> int:
    """h2y_pack_frame_bytes: the bytes of one packed frame; 0 for packing 0 and every combination the packing does not take."""
    return int(load_library().h2y_pack_frame_bytes(width, height, chroma, packing))


def _frame_samples(width, height, chroma):
    return width * height + 2 * ((width >> 1) * (height >> 1) if chroma == CHROMA_420 else width * height)


def pack_frame(width: int, height: int, chroma: int, bit_depth: int, packing: int, frame):
    """h2y_pack_frame (host only, no device): the packed bytes (uint8) of one frame of three u16 planes, one after the other."""
    lib = load_library()
    src = np.ascontiguousarray(frame, dtype=np.uint16).reshape(-1)
    if src.size != _frame_samples(width, height, chroma):
        raise ValueError("the frame does not hold width x height samples and its two chroma planes")
    dst = np.zeros(max(pack_frame_bytes(width, height, chroma, packing), 1), dtype=np.uint8)
    rc = lib.h2y_pack_frame(width, height, chroma, bit_depth, packing, src.ctypes.data, dst.ctypes.data)
    if rc != H2Y_OK:
        raise H2YError(rc, (lib.h2y_last_error(None) or b"").decode())
    return dst[:pack_frame_bytes(width, height, chroma, packing)]


def unpack_frame(width: int, height: int, chroma: int, bit_depth: int, packing: int, packed):
    """h2y_unpack_frame (host only, no device): the three u16 planes, one after the other, of one packed frame (bytes)."""
    lib = load_library()
    src = np.ascontiguousarray(np.frombuffer(packed, dtype=np.uint8) if isinstance(packed, (bytes, bytearray)) else packed).view(np.uint8).reshape(-1)
    need = pack_frame_bytes(width, height, chroma, packing)
    if need and src.size != need:
        raise ValueError("the packed frame does not hold h2y_pack_frame_bytes bytes")
    dst = np.zeros(max(_frame_samples(width, height, chroma), 1), dtype=np.uint16)
    rc = lib.h2y_unpack_frame(width, height, chroma, bit_depth, packing, src.ctypes.data if src.size else None, dst.ctypes.data)
    if rc != H2Y_OK:
        raise H2YError(rc, (lib.h2y_last_error(None) or b"").decode())
    return dst[:_frame_samples(width, height, chroma)]


def lightdist_json(stats, first_frame_index: int = 0) -> str:
    """h2y_lightdist_json (host only, no device): the HDR10+ JSON of the frames of stats (H2YLightdistStats), one scene."""
    lib = load_library()
    n = len(stats)
    arr = (H2YLightdistStats * max(n, 1))(*stats)
    need = lib.h2y_lightdist_json(arr, n, first_frame_index, None, 0)
    if not need:
        raise H2YError(H2Y_EINVAL, "h2y_lightdist_json: no frames, a negative first frame index or a frame without pixels")
    buf = C.create_string_buffer(need + 1)
    lib.h2y_lightdist_json(arr, n, first_frame_index, buf, need + 1)
    return buf.value.decode()


def scene_distance(a: H2YScenesig, b: H2YScenesig) -> float:
    """h2y_scene_distance (host only): the mean absolute change of the cells' mean log light between two signatures, in stops; -1
    for zero or differing pixel counts."""
    return load_library().h2y_scene_distance(C.byref(a), C.byref(b))


def scene_cuts(sigs, threshold: float):
    """h2y_scene_cuts (host only): the scene id of every frame from the frames' signatures -- a list of ints, frame 0 in scene 0."""
    n = len(sigs)
    arr = (H2YScenesig * max(n, 1))(*sigs)
    ids = (C.c_int32 * max(n, 1))()
    scenes = load_library().h2y_scene_cuts(arr, n, threshold, ids)
    if not scenes:
        raise H2YError(H2Y_EINVAL, "h2y_scene_cuts: no frames, or a threshold that is negative or not finite")
    return list(ids[:n])


def scene_merge(stats, bins, scene_id):
    """h2y_scene_merge (host only): a list of H2YSceneStats, the figures of the scenes of the frames of stats (H2YLightdistStats)
    with their bins (uint32, (n, LIGHTDIST_BINS)) and scene ids."""
    lib = load_library()
    n = len(stats)
    arr = (H2YLightdistStats * max(n, 1))(*stats)
    b = np.ascontiguousarray(bins, dtype=np.uint32)
    ids = (C.c_int32 * max(n, 1))(*scene_id)
    if len(scene_id) != n or b.size != n * LIGHTDIST_BINS:
        raise ValueError("stats, bins and scene_id differ in length")
    scenes = lib.h2y_scene_merge(arr, b.ctypes.data, ids, n, None, 0)
    if not scenes:
        raise H2YError(H2Y_EINVAL, "h2y_scene_merge: no frames, a frame without pixels, or scene ids that do not run 0, 0.., 1, ..")
    out = (H2YSceneStats * scenes)()
    lib.h2y_scene_merge(arr, b.ctypes.data, ids, n, out, scenes)
    return list(out)


def lightdist_json_scenes(scenes, first_frame_index: int = 0) -> str:
    """h2y_lightdist_json_scenes (host only): the HDR10+ JSON of the frames of scenes (H2YSceneStats), every frame carrying its
    scene's figures."""
    lib = load_library()
    n = len(scenes)
    arr = (H2YSceneStats * max(n, 1))(*scenes)
    need = lib.h2y_lightdist_json_scenes(arr, n, first_frame_index, None, 0)
    if not need:
        raise H2YError(H2Y_EINVAL, "h2y_lightdist_json_scenes: no scenes, a negative first frame index, a scene without pixels or frames, "
                                   "or scenes that do not tile the frames in order")
    buf = C.create_string_buffer(need + 1)
    lib.h2y_lightdist_json_scenes(arr, n, first_frame_index, buf, need + 1)
    return buf.value.decode()


def gamut_matrix(src_primaries: int, dst_primaries: int) -> np.ndarray:
    """h2y_gamut_matrix (host only, no device): the float32 (3, 3) matrix NPM(dst)^-1 NPM(src) on (R, G, B) columns, every entry
    the exact value rounded to nearest.  Raises H2YError (EUNSUPPORTED: primaries it does not know; EINVAL: equal chromaticities)."""
    m = np.zeros(9, dtype=np.float32)
    why = C.c_char_p()
    rc = load_library().h2y_gamut_matrix(int(src_primaries), int(dst_primaries), m.ctypes.data_as(C.POINTER(C.c_float)), C.byref(why))
    if rc != H2Y_OK:
        raise H2YError(rc, (why.value or b"").decode())
    return m.reshape(3, 3)


def _int_array(values):
    values = [int(v) for v in values]
    return (C.c_int * max(len(values), 1))(*values), len(values)


def gamutcheck_planes(lights, file_primaries: int, sets, ratio: float = GAMUTCHECK_RATIO, floor: float = GAMUTCHECK_FLOOR):
    """h2y_gamutcheck_planes (host only, no device): k_gamutcheck's CPU twin from the matrix on, on three numpy light planes G, B, R
    of float32 and one (height, width) shape (a flat plane counts as one row); returns the frame's H2YGamutcheckStats."""
    src = [np.ascontiguousarray(p, dtype=np.float32) for p in lights]
    if len(src) != 3 or any(p.shape != src[0].shape for p in src):
        raise ValueError("three float32 planes of one shape")
    height, width = src[0].shape if src[0].ndim == 2 else (1, src[0].size)
    ins = (C.c_void_p * 3)(*[p.ctypes.data for p in src])
    arr, n = _int_array(sets)
    out = H2YGamutcheckStats()
    lib = load_library()
    rc = lib.h2y_gamutcheck_planes(int(file_primaries), n, arr, float(ratio), float(floor), width, height, ins, C.byref(out))
    if rc != H2Y_OK:
        raise H2YError(rc, (lib.h2y_last_error(None) or b"").decode())
    return out


def gamut_compress_curve(src_primaries: int, dst_primaries: int, threshold: float = GAMUT_COMPRESS_THRESHOLD,
                         power: float = GAMUT_COMPRESS_POWER):
    """h2y_gamut_compress_curve (host only, no device): a dict of the float32 matrix (3, 3), the limits and scales (R, G, B) and the
    three tables (3, GAMUT_COMPRESS_NODES) of the gamut compression from src_primaries to dst_primaries.  Raises H2YError (EINVAL:
    threshold or power out of range, equal chromaticities; EUNSUPPORTED: XYZ, primaries it does not know)."""
    out = H2YGamutCompressTables()
    why = C.c_char_p()
    rc = load_library().h2y_gamut_compress_curve(int(src_primaries), int(dst_primaries), float(threshold), float(power), C.byref(out),
                                                 C.byref(why))
    if rc != H2Y_OK:
        raise H2YError(rc, (why.value or b"").decode())
    return {
        "matrix": np.array(out.m, np.float32).reshape(3, 3),
        "threshold": np.float32(out.threshold),
        "power": np.float32(out.power),
        "limit": np.array(out.limit, np.float32),
        "scale": np.array(out.scale, np.float32),
        "table": np.ctypeslib.as_array(out.table).astype(np.float32).reshape(3, GAMUT_COMPRESS_NODES),
    }


def gamut_compress_planes(planes, src_primaries: int, dst_primaries: int, threshold: float = GAMUT_COMPRESS_THRESHOLD,
                          power: float = GAMUT_COMPRESS_POWER):
    """h2y_gamut_compress_planes (host only, no device): k_gamut_compress' CPU twin on three numpy planes G, B, R of float32 or
    float16; returns the three planes the kernel writes for them, in the source's type."""
    src = [np.ascontiguousarray(p) for p in planes]
    dt = src[0].dtype
    if len(src) != 3 or dt not in (np.float32, np.float16) or any(p.dtype != dt or p.shape != src[0].shape for p in src):
        raise ValueError("three planes of one shape, float32 or float16")
    out = [np.empty(p.shape, dt) for p in src]
    ins = (C.c_void_p * 3)(*[p.ctypes.data for p in src])
    outs = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
    lib = load_library()
    rc = lib.h2y_gamut_compress_planes(int(src_primaries), int(dst_primaries), float(threshold), float(power),
                                       SAMPLE_F16 if dt == np.float16 else SAMPLE_F32, src[0].size, ins, outs)
    if rc != H2Y_OK:
        raise H2YError(rc, (lib.h2y_last_error(None) or b"").decode())
    return out


def tonemap_curve(src_peak: int, dst_peak: int, relative: int):
    """h2y_tonemap_curve (host only, no device): (the LIGHTDIST_BINS float32 gains of the BT.2390 curve from src_peak to dst_peak
    cd/m2 on the light distribution's nodes, the cap as a float32).  Raises H2YError (EINVAL: peaks or relative out of range)."""
    gain = np.zeros(LIGHTDIST_BINS, dtype=np.float32)
    cap = C.c_float()
    why = C.c_char_p()
    rc = load_library().h2y_tonemap_curve(int(src_peak), int(dst_peak), int(relative), gain.ctypes.data_as(C.POINTER(C.c_float)),
                                          C.byref(cap), C.byref(why))
    if rc != H2Y_OK:
        raise H2YError(rc, (why.value or b"").decode())
    return gain, np.float32(cap.value)


class Lut3d:
    """A parsed .cube table (h2y_lut3d_parse; host only, no device): n, lo and hi (float32 triples r, g, b), title, nodes() and
    planes().  Raises H2YError with the parser's reason (EUNSUPPORTED: a 1D or shaper + 3D file; EINVAL: malformed)."""

    def __init__(self, text):
        data = text.encode() if isinstance(text, str) else bytes(text)
        self.lib = load_library()
        self.h = C.c_void_p()
        why = C.c_char_p()
        rc = self.lib.h2y_lut3d_parse(data, len(data), C.byref(self.h), C.byref(why))
        if rc != H2Y_OK:
            raise H2YError(rc, (why.value or b"").decode(errors="replace"))
        n, dom, title = C.c_int(), (C.c_float * 6)(), C.c_char_p()
        self.lib.h2y_lut3d_info(self.h, C.byref(n), dom, C.byref(title))
        self.n = n.value
        self.lo = np.array(dom[:3], np.float32)
        self.hi = np.array(dom[3:], np.float32)
        self.title = (title.value or b"").decode(errors="replace")

    def close(self):
        if self.h:
            self.lib.h2y_lut3d_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def nodes(self):
        """the float32 (n, n, n, 3) node values as parsed, indexed [b][g][r][channel r, g, b]: the file's order"""
        out = np.zeros(3 * self.n ** 3, np.float32)
        rc = self.lib.h2y_lut3d_nodes(self.h, out.ctypes.data_as(C.POINTER(C.c_float)))
        if rc != H2Y_OK:
            raise H2YError(rc, (self.lib.h2y_last_error(None) or b"").decode())
        return out.reshape(self.n, self.n, self.n, 3)

    def planes(self, planes, interp=1, signal=0, dst_bit_depth=10, dst_full_range=0, dst_matrix=9):
        """h2y_lut3d_planes (host only, no device): the pass on three numpy planes G, B, R of float32 or float16; returns the three
        planes k_lut3d writes for them: the source's type in planes mode, float32 in signal mode."""
        src = [np.ascontiguousarray(p) for p in planes]
        dt = src[0].dtype
        if len(src) != 3 or dt not in (np.float32, np.float16) or any(p.dtype != dt or p.shape != src[0].shape for p in src):
            raise ValueError("three planes of one shape, float32 or float16")
        out = [np.empty(p.shape, np.float32 if signal else dt) for p in src]
        ins = (C.c_void_p * 3)(*[p.ctypes.data for p in src])
        outs = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
        rc = self.lib.h2y_lut3d_planes(self.h, int(interp), int(signal), int(dst_bit_depth), int(dst_full_range), int(dst_matrix),
                                       SAMPLE_F16 if dt == np.float16 else SAMPLE_F32, src[0].size, ins, outs)
        if rc != H2Y_OK:
            raise H2YError(rc, (self.lib.h2y_last_error(None) or b"").decode())
        return out


def hlg_tables(peak: int, relative: int):
    """h2y_hlg_tables (host only, no device): (gain, oetf, k, gamma) -- the two float32 tables of LIGHTDIST_BINS entries of the HLG pass
    at a nominal peak of `peak` cd/m2 (the inverse OOTF's gain, the OETF), the float32 factor k that brings a sample to units of the
    peak, and the system gamma as a float.  Raises H2YError (EINVAL: peak outside 400..2000, relative not 0 / 1)."""
    gain = np.zeros(LIGHTDIST_BINS, dtype=np.float32)
    oetf = np.zeros(LIGHTDIST_BINS, dtype=np.float32)
    k, gamma, why = C.c_float(), C.c_double(), C.c_char_p()
    fp = C.POINTER(C.c_float)
    rc = load_library().h2y_hlg_tables(int(peak), int(relative), gain.ctypes.data_as(fp), oetf.ctypes.data_as(fp), C.byref(k),
                                       C.byref(gamma), C.byref(why))
    if rc != H2Y_OK:
        raise H2YError(rc, (why.value or b"").decode())
    return gain, oetf, np.float32(k.value), float(gamma.value)


def hlg_planes(planes, peak: int, relative: int, dst_bit_depth: int, dst_full_range: int, dst_matrix: int):
    """h2y_hlg_planes (host only, no device): the HLG pass on three numpy planes G, B, R of float32 or float16 display light; returns
    the three float32 planes of code-valued samples k_hlg writes for them.  Raises H2YError as the library refuses."""
    src = [np.ascontiguousarray(p) for p in planes]
    dt = src[0].dtype
    if len(src) != 3 or dt not in (np.float32, np.float16) or any(p.dtype != dt or p.shape != src[0].shape for p in src):
        raise ValueError("three planes of one shape, float32 or float16")
    out = [np.empty(p.shape, np.float32) for p in src]
    ins = (C.c_void_p * 3)(*[p.ctypes.data for p in src])
    outs = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
    lib = load_library()
    rc = lib.h2y_hlg_planes(int(peak), int(relative), int(dst_bit_depth), int(dst_full_range), int(dst_matrix),
                            SAMPLE_F16 if dt == np.float16 else SAMPLE_F32, src[0].size, ins, outs)
    if rc != H2Y_OK:
        raise H2YError(rc, (lib.h2y_last_error(None) or b"").decode())
    return out


def hlg_inverse_tables(peak: int):
    """h2y_hlg_inverse_tables (host only, no device): (ootf, inv, kappa, gamma) -- the two float32 tables of LIGHTDIST_BINS entries of
    the light of HLG code planes at a display peak of `peak` cd/m2 (the OOTF's gain, the OETF's inverse), the float32 factor kappa =
    peak / 10000, and the system gamma as a float.  Raises H2YError (EINVAL: peak outside 400..2000)."""
    ootf = np.zeros(LIGHTDIST_BINS, dtype=np.float32)
    inv = np.zeros(LIGHTDIST_BINS, dtype=np.float32)
    kappa, gamma, why = C.c_float(), C.c_double(), C.c_char_p()
    fp = C.POINTER(C.c_float)
    rc = load_library().h2y_hlg_inverse_tables(int(peak), ootf.ctypes.data_as(fp), inv.ctypes.data_as(fp), C.byref(kappa), C.byref(gamma),
                                               C.byref(why))
    if rc != H2Y_OK:
        raise H2YError(rc, (why.value or b"").decode())
    return ootf, inv, np.float32(kappa.value), float(gamma.value)


def hlg_inverse_planes(planes, peak: int):
    """h2y_hlg_inverse_planes (host only, no device): steps 4h-7h of the light of HLG code planes on three float32 numpy planes G', B',
    R'; returns the three float32 planes of display light (1.0 = 10000 cd/m2) k_hlg_linearize writes for them."""
    src = [np.ascontiguousarray(p) for p in planes]
    if len(src) != 3 or any(p.dtype != np.float32 or p.shape != src[0].shape for p in src):
        raise ValueError("three float32 planes of one shape")
    out = [np.empty(p.shape, np.float32) for p in src]
    ins = (C.c_void_p * 3)(*[p.ctypes.data for p in src])
    outs = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
    lib = load_library()
    rc = lib.h2y_hlg_inverse_planes(int(peak), src[0].size, ins, outs)
    if rc != H2Y_OK:
        raise H2YError(rc, (lib.h2y_last_error(None) or b"").decode())
    return out


def sdr_inverse_planes(planes, white: int = SDR_WHITE_DEFAULT):
    """h2y_sdr_inverse_planes (host only, no device): steps 4s-6s of the light of SDR code planes on three float32 numpy planes G', B',
    R'; returns the three float32 planes of light (1.0 = 10000 cd/m2) k_sdr_linearize writes for them with the reference white at
    `white` cd/m2.  Raises H2YError (EINVAL: white outside 80..1000)."""
    src = [np.ascontiguousarray(p) for p in planes]
    if len(src) != 3 or any(p.dtype != np.float32 or p.shape != src[0].shape for p in src):
        raise ValueError("three float32 planes of one shape")
    out = [np.empty(p.shape, np.float32) for p in src]
    ins = (C.c_void_p * 3)(*[p.ctypes.data for p in src])
    outs = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
    lib = load_library()
    rc = lib.h2y_sdr_inverse_planes(int(white), src[0].size, ins, outs)
    if rc != H2Y_OK:
        raise H2YError(rc, (lib.h2y_last_error(None) or b"").decode())
    return out


def code_signal_planes(d: H2YCodelightDesc, planes):
    """h2y_code_signal_planes (host only, no device): the signal of code planes on three uint16 numpy planes of 4:4:4 codes (Y, Cb, Cr
    or G, B, R as d's matrix_coeffs says); returns the three float32 planes G', B', R' in [+0, 1] k_code_signal writes for them.
    Raises H2YError with the descriptor's refusal (EUNSUPPORTED: matrix_coeffs 14)."""
    src = [np.ascontiguousarray(p) for p in planes]
    if len(src) != 3 or any(p.dtype != np.uint16 or p.shape != src[0].shape for p in src):
        raise ValueError("three uint16 planes of one shape")
    out = [np.empty(p.shape, np.float32) for p in src]
    ins = (C.c_void_p * 3)(*[p.ctypes.data for p in src])
    outs = (C.c_void_p * 3)(*[p.ctypes.data for p in out])
    lib = load_library()
    rc = lib.h2y_code_signal_planes(C.byref(d), src[0].size, ins, outs)
    if rc != H2Y_OK:
        raise H2YError(rc, (lib.h2y_last_error(None) or b"").decode())
    return out


def scale_frame_bytes(width: int, height: int, chroma: int) -> int:
    """h2y_scale_frame_bytes: bytes of a frame of three u16 planes (0 for an unsupported geometry)."""
    return int(load_library().h2y_scale_frame_bytes(width, height, chroma))


class Context:
    """h2y_ctx: one per GPU (one process per GPU in multi-GPU runs)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.h2y_ctx_create(device, C.byref(h))
        if rc != H2Y_OK:
            raise H2YError(rc, (self.lib.h2y_last_error(None) or b"").decode())
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.lib.h2y_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != H2Y_OK:
            raise H2YError(rc, (self.lib.h2y_last_error(self.h) or b"").decode())

    def set_option(self, name: str, value) -> None:
        """h2y_ctx_set_option: "t1", "groups", "cols8", "lut3d_lds", "balance", "fir" (tuning / test knobs; output bytes never change)."""
        self._check(self.lib.h2y_ctx_set_option(self.h, name.encode(), str(value).encode()))

    def set_chroma_siting(self, chroma_sample_loc_type: int) -> None:
        """h2y_ctx_set_chroma_siting: 0 as the resampler sites the 4:2:0 chroma (the default), 2 top-left (HDR10); before a ring is opened."""
        self._check(self.lib.h2y_ctx_set_chroma_siting(self.h, chroma_sample_loc_type))

    def set_inverse_chroma_siting(self, chroma_sample_loc_type: int) -> None:
        """h2y_ctx_set_inverse_chroma_siting: how the .yuv -> RGB entries take 4:2:0 chroma: 0 as the reference's upsampler does (the
        default), 2 top-left (HDR10); before a ring is opened."""
        self._check(self.lib.h2y_ctx_set_inverse_chroma_siting(self.h, chroma_sample_loc_type))

    def set_stream(self, hip_stream_ptr: int | None):
        self._check(self.lib.h2y_ctx_set_stream(self.h, C.c_void_p(hip_stream_ptr or 0)))

    # -- host buffers: the reference's whole pic_stats..write_yuv sequence ----
    def convert_frame(self, d: H2YDesc, planes: Sequence[np.ndarray]) -> np.ndarray:
        dt = _np_dtype(d.in_sample_type)
        keep = [np.ascontiguousarray(p, dtype=dt) for p in planes]
        n = d.width * d.height
        for p in keep:
            if p.size != n:
                raise ValueError("plane size does not match width*height")
        arr = (C.c_void_p * 3)(*[p.ctypes.data for p in keep])
        out = np.empty(frame_bytes(d) // 2, dtype=np.uint16)
        self._check(self.lib.h2y_convert_frame(self.h, C.byref(d), arr, out.ctypes.data))
        return out

    # -- device buffers (torch tensors or raw pointers) -----------------------
    @staticmethod
    def _ptr(x) -> int:
        return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x)

    def _batch_arrays(self, frames_in, frames_out):
        n = len(frames_out)
        ins = (C.c_void_p * (3 * n))()
        outs = (C.c_void_p * n)()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(frames_in[f][c])
            outs[f] = self._ptr(frames_out[f])
        return n, ins, outs

    def convert_batch(self, d: H2YDesc, frames_in, frames_out) -> None:
        """frames_in[f] = three device planes (G,B,R); frames_out[f] = device .yuv frame."""
        n, ins, outs = self._batch_arrays(frames_in, frames_out)
        self._check(self.lib.h2y_convert_batch(self.h, C.byref(d), n, ins, outs))

    def convert_batch_enqueue(self, d: H2YDesc, frames_in, frames_out) -> None:
        n, ins, outs = self._batch_arrays(frames_in, frames_out)
        self._keep = (getattr(self, "_keep", ()) + ((ins, outs),))[-2:]  # up to two batches in flight
        self._check(self.lib.h2y_convert_batch_enqueue(self.h, C.byref(d), n, ins, outs))

    def convert_batch_enqueue_raw(self, d: H2YDesc, n: int, ins, outs) -> None:
        """Pre-built pointer arrays (bench loop: no per-step Python marshalling)."""
        self._check(self.lib.h2y_convert_batch_enqueue(self.h, C.byref(d), n, ins, outs))

    def batch_finish(self) -> int:
        redone = C.c_int(0)
        self._check(self.lib.h2y_batch_finish(self.h, C.byref(redone)))
        return redone.value

    def pic_stats(self, d: H2YDesc, planes):
        arr = (C.c_void_p * 3)(*[self._ptr(p) for p in planes])
        mm = (C.c_float * 6)()
        fc = (C.c_int32 * 6)()
        self._check(self.lib.h2y_pic_stats(self.h, C.byref(d), arr, mm, fc))
        return list(mm), list(fc)

    def matrix_convert(self, d: H2YDesc, planes, out_planes) -> None:
        arr = (C.c_void_p * 3)(*[self._ptr(p) for p in planes])
        outp = (C.c_void_p * 3)(*[self._ptr(p) for p in out_planes])
        self._check(self.lib.h2y_matrix_convert(self.h, C.byref(d), arr, outp))

    def subsample_420(self, width, height, bit_depth, resampler, src, dst) -> None:
        self._check(self.lib.h2y_subsample_420(self.h, width, height, bit_depth, resampler, self._ptr(src), self._ptr(dst)))

    def subsample_420_sited(self, width, height, bit_depth, loc_type, src, dst) -> None:
        """One u16 plane through the FIR, sited as chroma_sample_loc_type says: 0 the reference's, 2 top-left."""
        self._check(self.lib.h2y_subsample_420_sited(self.h, width, height, bit_depth, loc_type, self._ptr(src), self._ptr(dst)))

    def last_kernel_ms(self):
        ms = C.c_float()
        n = C.c_int()
        self.lib.h2y_last_kernel_ms(self.h, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def matrix_inverse(self, width, height, in_depth, in_full_range, in_matrix, out_depth, in_planes, out_planes) -> None:
        """Device U16 4:4:4 planes (Y, Cb/Dz, Cr/Dx) -> device U16 planes (G, B, R)."""
        ip = (C.c_void_p * 3)(*[self._ptr(p) for p in in_planes])
        op = (C.c_void_p * 3)(*[self._ptr(p) for p in out_planes])
        self._check(self.lib.h2y_matrix_inverse(self.h, width, height, in_depth, in_full_range, in_matrix, out_depth, ip, op))

    def upsample_444(self, width, height, algorithm, min_cv, max_cv, src, dst) -> None:
        """Subsample420to444: device U16 (height/2 x width/2) plane -> device U16 (height x width) plane."""
        self._check(self.lib.h2y_upsample_444(self.h, width, height, algorithm, min_cv, max_cv, self._ptr(src), self._ptr(dst)))

    def upsample_444_sited(self, width, height, loc_type, min_cv, max_cv, src, dst) -> None:
        """One u16 chroma plane 4:2:0 -> 4:4:4 by the FIR, its source sited as chroma_sample_loc_type says: 0 the reference's, 2 top-left."""
        self._check(self.lib.h2y_upsample_444_sited(self.h, width, height, loc_type, min_cv, max_cv, self._ptr(src), self._ptr(dst)))

    def inverse_420(self, width, height, in_depth, in_full_range, in_matrix, out_depth, algorithm, in_planes, out_planes) -> None:
        """Device U16 4:2:0 planes (Y, Cb/Dz, Cr/Dx) -> device U16 planes (G, B, R): upsample, then matrix_inverse."""
        ip = (C.c_void_p * 3)(*[self._ptr(p) for p in in_planes])
        op = (C.c_void_p * 3)(*[self._ptr(p) for p in out_planes])
        self._check(self.lib.h2y_inverse_420(self.h, width, height, in_depth, in_full_range, in_matrix, out_depth, algorithm, ip, op))

    def inverse_frame(self, width, height, in_chroma, in_depth, in_full_range, in_matrix, out_depth, algorithm, in_planes):
        """Host U16 planes (Y, Cb/Dz, Cr/Dx; 4:4:4 or 4:2:0) -> host U16 planes (G, B, R): the .yuv -> .tiff flow on one frame."""
        import numpy as np

        ins = [np.ascontiguousarray(p, dtype=np.uint16) for p in in_planes]
        outs = [np.empty(width * height, np.uint16) for _ in range(3)]
        ip = (C.c_void_p * 3)(*[p.ctypes.data for p in ins])
        op = (C.c_void_p * 3)(*[p.ctypes.data for p in outs])
        self._check(self.lib.h2y_inverse_frame(self.h, width, height, in_chroma, in_depth, in_full_range, in_matrix, out_depth, algorithm, ip, op))
        return outs

    def inverse_batch(self, width, height, in_chroma, in_depth, in_full_range, in_matrix, out_depth, algorithm, frames_in, frames_out) -> None:
        """Device U16 planes of many frames: frames_in[f] = (Y, Cb/Dz, Cr/Dx), frames_out[f] = (G, B, R), tensors or pointers."""
        n = len(frames_in)
        if len(frames_out) != n:
            raise ValueError("frames_in and frames_out differ in length")
        ins = (C.c_void_p * (3 * n))()
        outs = (C.c_void_p * (3 * n))()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(frames_in[f][c])
                outs[3 * f + c] = self._ptr(frames_out[f][c])
        self._check(self.lib.h2y_inverse_batch(self.h, width, height, in_chroma, in_depth, in_full_range, in_matrix, out_depth, algorithm,
                                               n, ins, outs))

    def dpx_decode_batch(self, info: H2YDpxInfo, payloads, planes_out) -> None:
        """DPX payloads on the device (payloads[f]: info.payload_bytes each) -> float planes planes_out[f] = (G, B, R), tensors or
        pointers: dpx_read()'s per-pixel loop and the demux, many frames per launch."""
        n = len(payloads)
        if len(planes_out) != n:
            raise ValueError("payloads and planes_out differ in length")
        pay = (C.c_void_p * n)(*[self._ptr(p) for p in payloads])
        outs = (C.c_void_p * (3 * n))()
        for f in range(n):
            for c in range(3):
                outs[3 * f + c] = self._ptr(planes_out[f][c])
        self._check(self.lib.h2y_dpx_decode_batch(self.h, C.byref(info), n, pay, outs))

    def tiff_decode_batch(self, info: H2YTiffInfo, clamp_video_range, payloads, planes_out) -> None:
        """TIFF rows on the device (payloads[f]: info.payload_bytes each, the decoded rows whole, one after the other) -> u16
        planes planes_out[f] = (G, B, R), tensors or pointers: read_tiff()'s per-pixel loop, many frames per launch."""
        n = len(payloads)
        if len(planes_out) != n:
            raise ValueError("payloads and planes_out differ in length")
        pay = (C.c_void_p * n)(*[self._ptr(p) for p in payloads])
        outs = (C.c_void_p * (3 * n))()
        for f in range(n):
            for c in range(3):
                outs[3 * f + c] = self._ptr(planes_out[f][c])
        self._check(self.lib.h2y_tiff_decode_batch(self.h, C.byref(info), int(clamp_video_range), n, pay, outs))

    def rgb_interleave_batch(self, width, height, planes_in, rgb_out) -> None:
        """u16 planes planes_in[f] = (G, B, R) on the device -> rgb_out[f], 3 x width x height u16, R, G, B per pixel."""
        n = len(planes_in)
        if len(rgb_out) != n:
            raise ValueError("planes_in and rgb_out differ in length")
        ins = (C.c_void_p * (3 * n))()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(planes_in[f][c])
        outs = (C.c_void_p * n)(*[self._ptr(p) for p in rgb_out])
        self._check(self.lib.h2y_rgb_interleave_batch(self.h, width, height, n, ins, outs))

    def exr_decode_batch(self, info: H2YExrInfo, payloads, planes_out) -> None:
        """EXR payloads on the device (payloads[f]: info.payload_bytes each, exr_unpack's layout) -> half planes
        planes_out[f] = (G, B, R), tensors or pointers: read_exr()'s scanline decode, many frames per launch."""
        n = len(payloads)
        if len(planes_out) != n:
            raise ValueError("payloads and planes_out differ in length")
        pay = (C.c_void_p * n)(*[self._ptr(p) for p in payloads])
        outs = (C.c_void_p * (3 * n))()
        for f in range(n):
            for c in range(3):
                outs[3 * f + c] = self._ptr(planes_out[f][c])
        self._check(self.lib.h2y_exr_decode_batch(self.h, C.byref(info), n, pay, outs))

    def compare_batch(self, width, height, chroma, sigma, frames_a, frames_b):
        """k_compare on device frame pairs (tensors or pointers, each frame's planes contiguous from a 16-byte aligned base):
        one H2YCompareStats per frame."""
        n = len(frames_a)
        if len(frames_b) != n:
            raise ValueError("frames_a and frames_b differ in length")
        pa = (C.c_void_p * n)(*[self._ptr(x) for x in frames_a])
        pb = (C.c_void_p * n)(*[self._ptr(x) for x in frames_b])
        out = (H2YCompareStats * max(n, 1))()
        self._check(self.lib.h2y_compare_batch(self.h, width, height, chroma, sigma, n, pa, pb, out))
        return list(out[:n])

    def histogram_batch(self, width, height, chroma, bit_depth, full_range, gbr, bits, frames, want_bins=True):
        """k_histogram on device frames (tensors or pointers, each frame's planes contiguous from a 16-byte aligned base):
        a list of H2YHistogramStats and, with want_bins, a uint32 array (n_frames, 3, 2^bits) of the bins (else None)."""
        import numpy as np

        n = len(frames)
        pf = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames])
        out = (H2YHistogramStats * max(n, 1))()
        bins = np.zeros((n, 3, 1 << bits), dtype=np.uint32) if want_bins and 1 <= bits <= 16 else None
        self._check(self.lib.h2y_histogram_batch(self.h, width, height, chroma, bit_depth, full_range, gbr, bits, n, pf, out,
                                                 None if bins is None else bins.ctypes.data))
        return list(out[:n]), bins

    def ssim_batch(self, width, height, chroma, bit_depth, frames_a, frames_b):
        """k_ssim on device frame pairs (tensors or pointers, each frame's planes contiguous from a 16-byte aligned base):
        a list of H2YSsimStats, one per pair."""
        n = len(frames_a)
        if len(frames_b) != n:
            raise ValueError("frames_a and frames_b differ in length")
        pa = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_a])
        pb = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_b])
        out = (H2YSsimStats * max(n, 1))()
        self._check(self.lib.h2y_ssim_batch(self.h, width, height, chroma, bit_depth, n, pa, pb, out))
        return list(out[:n])

    def regions_batch(self, width, height, chroma, flat_var, radius, frames_a, frames_b):
        """k_regions on device frame pairs (tensors or pointers, each frame's planes contiguous from a 16-byte aligned base):
        a list of H2YRegionsStats, one per pair."""
        n = len(frames_a)
        if len(frames_b) != n:
            raise ValueError("frames_a and frames_b differ in length")
        pa = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_a])
        pb = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_b])
        out = (H2YRegionsStats * max(n, 1))()
        self._check(self.lib.h2y_regions_batch(self.h, width, height, chroma, flat_var, radius, n, pa, pb, out))
        return list(out[:n])

    def light_batch(self, d: H2YDesc, frames_in):
        """k_light on device frames (frames_in[f] = three device planes G, B, R, 16-byte aligned): a list of H2YLightStats, one
        per frame, with the floor and ceiling the conversion of d takes for each."""
        n = len(frames_in)
        ins = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(frames_in[f][c])
        out = (H2YLightStats * max(n, 1))()
        self._check(self.lib.h2y_light_batch(self.h, C.byref(d), n, ins, out))
        return list(out[:n])

    def lightdist_batch(self, d: H2YDesc, frames_in, bins: bool = False):
        """k_lightdist on device frames (as light_batch takes them): a list of H2YLightdistStats, one per frame; with bins also the
        uint32 (n, LIGHTDIST_BINS) histograms."""
        n = len(frames_in)
        ins = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(frames_in[f][c])
        out = (H2YLightdistStats * max(n, 1))()
        b = np.zeros((max(n, 1), LIGHTDIST_BINS), dtype=np.uint32) if bins else None
        self._check(self.lib.h2y_lightdist_batch(self.h, C.byref(d), n, ins, out, b.ctypes.data if bins else None))
        return (list(out[:n]), b[:n]) if bins else list(out[:n])

    def codelight_batch(self, d: H2YCodelightDesc, frames, dist: bool = False, bins: bool = False):
        """k_codelight on device frames of PQ codes (tensors or pointers, each frame's planes contiguous from a 16-byte aligned
        base): a list of H2YLightStats; with dist also a list of H2YLightdistStats, with bins also the uint32 (n, LIGHTDIST_BINS)
        histograms -- (light, dist or None, bins or None) when either is asked for."""
        n = len(frames)
        pf = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames])
        out = (H2YLightStats * max(n, 1))()
        dout = (H2YLightdistStats * max(n, 1))() if dist else None
        b = np.zeros((max(n, 1), LIGHTDIST_BINS), dtype=np.uint32) if bins else None
        self._check(self.lib.h2y_codelight_batch(self.h, C.byref(d), n, pf, out, dout, b.ctypes.data if bins else None))
        if not dist and not bins:
            return list(out[:n])
        return list(out[:n]), (list(dout[:n]) if dist else None), (b[:n] if bins else None)

    def scenesig_batch(self, d: H2YDesc, frames_in):
        """k_scenesig on device frames (as lightdist_batch takes them): a list of H2YScenesig, one per frame."""
        n = len(frames_in)
        ins = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(frames_in[f][c])
        out = (H2YScenesig * max(n, 1))()
        self._check(self.lib.h2y_scenesig_batch(self.h, C.byref(d), n, ins, out))
        return list(out[:n])

    def codescenesig_batch(self, d: H2YCodelightDesc, frames):
        """k_codescenesig on device frames of PQ codes (as codelight_batch takes them): a list of H2YScenesig, one per frame."""
        n = len(frames)
        pf = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames])
        out = (H2YScenesig * max(n, 1))()
        self._check(self.lib.h2y_codescenesig_batch(self.h, C.byref(d), n, pf, out))
        return list(out[:n])

    def gamutcheck_batch(self, d: H2YCodelightDesc, frames, file_primaries: int, sets, ratio: float = GAMUTCHECK_RATIO,
                         floor: float = GAMUTCHECK_FLOOR):
        """k_gamutcheck on device frames of PQ codes (as codelight_batch takes them): a list of H2YGamutcheckStats, one per frame --
        how much of each frame lies outside each of the check sets `sets`, the file being coded in `file_primaries`."""
        n = len(frames)
        pf = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames])
        arr, ns = _int_array(sets)
        out = (H2YGamutcheckStats * max(n, 1))()
        self._check(self.lib.h2y_gamutcheck_batch(self.h, C.byref(d), int(file_primaries), ns, arr, float(ratio), float(floor), n, pf, out))
        return list(out[:n])

    def codelight_stream_open(self, d: H2YCodelightDesc, want_dist=0, depth=3) -> None:
        """A ring that only measures light: stream_input lends the frame's three planes, stream_output returns None,
        stream_light_result (and with want_dist stream_lightdist_result) the frame's figures."""
        self._check(self.lib.h2y_codelight_stream_open(self.h, C.byref(d), int(want_dist), depth))
        nc = (d.width >> 1) * (d.height >> 1) if d.chroma_format_idc == CHROMA_420 else d.width * d.height
        self._stream_inverse = None
        self._stream_dpx = None
        self._stream_rgb = False
        self._stream_cmp_planes = (d.width * d.height, nc, nc)
        self._stream_in_geom = (d.width, d.height, d.chroma_format_idc)

    def deltae_batch(self, d: H2YCodelightDesc, frames_a, frames_b, threshold=1.0):
        """k_deltae on device frame pairs of PQ codes (as codelight_batch takes each frame): a list of H2YDeltaeStats, one per
        pair."""
        n = len(frames_a)
        if len(frames_b) != n:
            raise ValueError("frames_a and frames_b differ in length")
        pa = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_a])
        pb = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_b])
        out = (H2YDeltaeStats * max(n, 1))()
        self._check(self.lib.h2y_deltae_batch(self.h, C.byref(d), float(threshold), n, pa, pb, out))
        return list(out[:n])

    def linearize_batch(self, d: H2YCodelightDesc, frames, planes_out) -> None:
        """k_linearize on device frames of PQ codes (as codelight_batch takes them): planes_out[f] = three device planes G, B, R of
        float32, 16-byte aligned, receive the frame's linear light (1.0 = 10000 cd/m2)."""
        n = len(frames)
        if len(planes_out) != n:
            raise ValueError("frames and planes_out differ in length")
        pf = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames])
        outs = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                outs[3 * f + c] = self._ptr(planes_out[f][c])
        self._check(self.lib.h2y_linearize_batch(self.h, C.byref(d), n, pf, outs))

    def hlg_linearize_batch(self, d: H2YCodelightDesc, peak: int, frames, planes_out) -> None:
        """k_hlg_linearize on device frames of HLG codes at a display peak of `peak` cd/m2: linearize_batch's arguments and layout;
        planes_out[f] receive the frame's display light (1.0 = 10000 cd/m2)."""
        n = len(frames)
        if len(planes_out) != n:
            raise ValueError("frames and planes_out differ in length")
        pf = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames])
        outs = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                outs[3 * f + c] = self._ptr(planes_out[f][c])
        self._check(self.lib.h2y_hlg_linearize_batch(self.h, C.byref(d), int(peak), n, pf, outs))

    def sdr_linearize_batch(self, d: H2YCodelightDesc, white: int, frames, planes_out) -> None:
        """k_sdr_linearize on device frames of SDR (BT.1886) codes with the reference white at `white` cd/m2: linearize_batch's
        arguments and layout; planes_out[f] receive the frame's light (1.0 = 10000 cd/m2)."""
        n = len(frames)
        if len(planes_out) != n:
            raise ValueError("frames and planes_out differ in length")
        pf = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames])
        outs = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                outs[3 * f + c] = self._ptr(planes_out[f][c])
        self._check(self.lib.h2y_sdr_linearize_batch(self.h, C.byref(d), int(white), n, pf, outs))

    def code_signal_batch(self, d: H2YCodelightDesc, frames, planes_out) -> None:
        """k_code_signal on device frames of codes, no transfer applied: linearize_batch's arguments and layout; planes_out[f] receive
        the frame's signal G', B', R' in [+0, 1]."""
        n = len(frames)
        if len(planes_out) != n:
            raise ValueError("frames and planes_out differ in length")
        pf = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames])
        outs = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                outs[3 * f + c] = self._ptr(planes_out[f][c])
        self._check(self.lib.h2y_code_signal_batch(self.h, C.byref(d), n, pf, outs))

    def pqcode_stream_open(self, d, src: H2YCodelightDesc, depth=3, hlg_peak=None, sdr_white=None, signal_lut=None) -> None:
        """The forward ring on PQ code frames: stream_input gives one uint8 view of the pinned slot to fill with the frame's three
        u16 planes one after the other; the device linearises them (k_up444, k_linearize) into the F32 G,B,R planes d describes
        (src_transfer 8, src_matrix 0, stats_override 1 with floor 0, ceiling 1); stream_output gives the .yuv frame.  With hlg_peak
        the codes are HLG's at that display peak (h2y_hlgcode_stream_open: k_hlg_linearize), with sdr_white SDR (BT.1886) codes whose
        reference white lies at that many cd/m2 (h2y_sdrcode_stream_open: k_sdr_linearize), with signal_lut = (Lut3d or None, interp)
        the codes stay signal for that table, armed in signal mode in the same call (h2y_sigcode_stream_open: k_code_signal)."""
        if (hlg_peak is not None) + (sdr_white is not None) + (signal_lut is not None) > 1:
            raise ValueError("hlg_peak, sdr_white and signal_lut exclude one another")
        if signal_lut is not None:
            lut, interp = signal_lut
            self._check(self.lib.h2y_sigcode_stream_open(self.h, C.byref(d), C.byref(src), lut.h if lut is not None else None, int(interp), depth))
        elif sdr_white is not None:
            self._check(self.lib.h2y_sdrcode_stream_open(self.h, C.byref(d), C.byref(src), int(sdr_white), depth))
        elif hlg_peak is None:
            self._check(self.lib.h2y_pqcode_stream_open(self.h, C.byref(d), C.byref(src), depth))
        else:
            self._check(self.lib.h2y_hlgcode_stream_open(self.h, C.byref(d), C.byref(src), int(hlg_peak), depth))
        nc = (src.width >> 1) * (src.height >> 1) if src.chroma_format_idc == CHROMA_420 else src.width * src.height
        self._stream_desc = d
        self._stream_out_geom = (d.width, d.height, d.dst_chroma_format_idc)
        self._stream_inverse = None
        self._stream_dpx = 2 * (src.width * src.height + 2 * nc)
        self._stream_in_geom = (src.width, src.height, src.chroma_format_idc)
        self._stream_rgb = False

    def hlgcode_stream_open(self, d, src: H2YCodelightDesc, peak: int, depth=3) -> None:
        """The forward ring on HLG code frames at a display peak of `peak` cd/m2: pqcode_stream_open with k_hlg_linearize as its decode."""
        self.pqcode_stream_open(d, src, depth, hlg_peak=peak)

    def sdrcode_stream_open(self, d, src: H2YCodelightDesc, white: int = SDR_WHITE_DEFAULT, depth=3) -> None:
        """The forward ring on SDR code frames with the reference white at `white` cd/m2: pqcode_stream_open with k_sdr_linearize as its decode."""
        self.pqcode_stream_open(d, src, depth, sdr_white=white)

    def sigcode_stream_open(self, d, src: H2YCodelightDesc, lut, interp=1, depth=3) -> None:
        """The forward ring on code frames that stay signal (no transfer applied), armed with the Lut3d in signal mode in the same
        call: pqcode_stream_open with k_code_signal as its decode; d is the passthrough descriptor stream_lut3d(signal=1) arms on
        (src_transfer 8 = dst_transfer, dst_matrix 0 or 9)."""
        self.pqcode_stream_open(d, src, depth, signal_lut=(lut, interp))

    def scale_batch(self, src_w, src_h, dst_w, dst_h, chroma, bit_depth, full_range, gbr, a, frames_src, frames_dst) -> None:
        """k_scale on device frames (tensors or pointers, each frame's planes contiguous from a 16-byte aligned base):
        frames_dst[f] receives frames_src[f] resampled from src_w x src_h to dst_w x dst_h (Lanczos, a lobes)."""
        n = len(frames_src)
        if len(frames_dst) != n:
            raise ValueError("frames_src and frames_dst differ in length")
        ps = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_src])
        pd = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_dst])
        self._check(self.lib.h2y_scale_batch(self.h, src_w, src_h, dst_w, dst_h, chroma, bit_depth, full_range, gbr, a, n, ps, pd))

    def dither_batch(self, width, height, chroma, src_depth, dst_depth, full_range, gbr, mode, temporal, seed, first_frame,
                     frames_src, frames_dst=None) -> None:
        """k_dither on device frames (tensors or pointers, each frame's planes contiguous from a 16-byte aligned base):
        frames_dst[f] receives frames_src[f] reduced from src_depth to dst_depth as frame number first_frame + f; frames_dst
        None: in place."""
        frames_dst = frames_src if frames_dst is None else frames_dst
        n = len(frames_src)
        if len(frames_dst) != n:
            raise ValueError("frames_src and frames_dst differ in length")
        ps = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_src])
        pd = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_dst])
        self._check(self.lib.h2y_dither_batch(self.h, width, height, chroma, src_depth, dst_depth, full_range, gbr, mode, temporal,
                                              seed & 0xFFFFFFFF, first_frame & 0xFFFFFFFF, n, ps, pd))

    def pack_batch(self, width, height, chroma, bit_depth, packing, frames_src, frames_dst) -> None:
        """k_pack on device frames (tensors or pointers from 16-byte aligned bases): frames_dst[f] receives frames_src[f], three
        u16 planes one after the other, packed (PACK_PLANAR8, PACK_NV12 or PACK_P010).  No overlap of a frame's two sides."""
        n = len(frames_src)
        if len(frames_dst) != n:
            raise ValueError("frames_src and frames_dst differ in length")
        ps = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_src])
        pd = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_dst])
        self._check(self.lib.h2y_pack_batch(self.h, width, height, chroma, bit_depth, packing, n, ps, pd))

    def unpack_batch(self, width, height, chroma, bit_depth, packing, frames_src, frames_dst) -> None:
        """k_unpack on device frames: frames_dst[f] receives the three u16 planes of the packed frame frames_src[f]."""
        n = len(frames_src)
        if len(frames_dst) != n:
            raise ValueError("frames_src and frames_dst differ in length")
        ps = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_src])
        pd = (C.c_void_p * max(n, 1))(*[self._ptr(x) for x in frames_dst])
        self._check(self.lib.h2y_unpack_batch(self.h, width, height, chroma, bit_depth, packing, n, ps, pd))

    def gamut_batch(self, width, height, sample, src_primaries, dst_primaries, clip, frames_src, frames_dst=None) -> None:
        """k_gamut on device frames (frames_src[f] = three device planes G, B, R of float or half samples, 16-byte aligned):
        frames_dst[f] receives them converted from src_primaries to dst_primaries; frames_dst None: in place."""
        frames_dst = frames_src if frames_dst is None else frames_dst
        n = len(frames_src)
        if len(frames_dst) != n:
            raise ValueError("frames_src and frames_dst differ in length")
        ins = (C.c_void_p * max(3 * n, 1))()
        outs = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(frames_src[f][c])
                outs[3 * f + c] = self._ptr(frames_dst[f][c])
        self._check(self.lib.h2y_gamut_batch(self.h, width, height, sample, src_primaries, dst_primaries, clip, n, ins, outs))

    def gamut_compress_batch(self, width, height, sample, src_primaries, dst_primaries, frames_src, frames_dst=None,
                             threshold=GAMUT_COMPRESS_THRESHOLD, power=GAMUT_COMPRESS_POWER) -> None:
        """k_gamut_compress on device frames (frames_src[f] = three device planes G, B, R of float or half samples, 16-byte aligned):
        frames_dst[f] receives them converted from src_primaries to dst_primaries, out-of-gamut colours compressed; frames_dst None:
        in place."""
        frames_dst = frames_src if frames_dst is None else frames_dst
        n = len(frames_src)
        if len(frames_dst) != n:
            raise ValueError("frames_src and frames_dst differ in length")
        ins = (C.c_void_p * max(3 * n, 1))()
        outs = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(frames_src[f][c])
                outs[3 * f + c] = self._ptr(frames_dst[f][c])
        self._check(self.lib.h2y_gamut_compress_batch(self.h, width, height, sample, src_primaries, dst_primaries, threshold, power, n,
                                                      ins, outs))

    def tonemap_batch(self, width, height, sample, src_peak, dst_peak, relative, frames_src, frames_dst=None) -> None:
        """k_tonemap on device frames (frames_src[f] = three device planes G, B, R of float or half samples in linear light, 16-byte
        aligned): frames_dst[f] receives them mapped from src_peak to dst_peak cd/m2; frames_dst None: in place."""
        frames_dst = frames_src if frames_dst is None else frames_dst
        n = len(frames_src)
        if len(frames_dst) != n:
            raise ValueError("frames_src and frames_dst differ in length")
        ins = (C.c_void_p * max(3 * n, 1))()
        outs = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(frames_src[f][c])
                outs[3 * f + c] = self._ptr(frames_dst[f][c])
        self._check(self.lib.h2y_tonemap_batch(self.h, width, height, sample, src_peak, dst_peak, relative, n, ins, outs))

    def lut3d_batch(self, width, height, sample, lut, interp, signal, dst_bit_depth, dst_full_range, dst_matrix, frames_src,
                    frames_dst=None) -> None:
        """k_lut3d on device frames (frames_src[f] = three device planes G, B, R of float or half samples, 16-byte aligned):
        frames_dst[f] receives the Lut3d's value at every pixel, tetrahedral (interp 1) or trilinear (0); in planes mode (signal 0) in
        the source's type, in signal mode as float planes of code values scaled as a conversion to (dst_bit_depth, dst_full_range,
        dst_matrix) scales; frames_dst None: in place (signal mode: float planes only)."""
        frames_dst = frames_src if frames_dst is None else frames_dst
        n = len(frames_src)
        if len(frames_dst) != n:
            raise ValueError("frames_src and frames_dst differ in length")
        ins = (C.c_void_p * max(3 * n, 1))()
        outs = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(frames_src[f][c])
                outs[3 * f + c] = self._ptr(frames_dst[f][c])
        self._check(self.lib.h2y_lut3d_batch(self.h, width, height, sample, lut.h if lut is not None else None, interp, signal,
                                             dst_bit_depth, dst_full_range, dst_matrix, n, ins, outs))

    def hlg_batch(self, width, height, sample, peak, relative, dst_bit_depth, dst_full_range, dst_matrix, frames_src,
                  frames_dst=None) -> None:
        """k_hlg on device frames (frames_src[f] = three device planes G, B, R of float or half display light, 16-byte aligned):
        frames_dst[f] receives the float planes of code-valued HLG samples at a nominal peak of `peak` cd/m2, scaled as a conversion
        to (dst_bit_depth, dst_full_range, dst_matrix) scales; frames_dst None: in place (float planes only)."""
        frames_dst = frames_src if frames_dst is None else frames_dst
        n = len(frames_src)
        if len(frames_dst) != n:
            raise ValueError("frames_src and frames_dst differ in length")
        ins = (C.c_void_p * max(3 * n, 1))()
        outs = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(frames_src[f][c])
                outs[3 * f + c] = self._ptr(frames_dst[f][c])
        self._check(self.lib.h2y_hlg_batch(self.h, width, height, sample, peak, relative, dst_bit_depth, dst_full_range, dst_matrix, n,
                                           ins, outs))

    def ictcp_batch(self, width, height, sample, dst_bit_depth, dst_full_range, frames_src, frames_dst=None) -> None:
        """k_ictcp on device frames (frames_src[f] = three device planes G, B, R of float or half display light, 1.0 = 10000 cd/m2,
        16-byte aligned): frames_dst[f] receives the float planes of code-valued PQ I, Ct, Cp samples on H.273's scale of
        (dst_bit_depth, dst_full_range), the rounding half added; frames_dst None: in place (float planes only)."""
        frames_dst = frames_src if frames_dst is None else frames_dst
        n = len(frames_src)
        if len(frames_dst) != n:
            raise ValueError("frames_src and frames_dst differ in length")
        ins = (C.c_void_p * max(3 * n, 1))()
        outs = (C.c_void_p * max(3 * n, 1))()
        for f in range(n):
            for c in range(3):
                ins[3 * f + c] = self._ptr(frames_src[f][c])
                outs[3 * f + c] = self._ptr(frames_dst[f][c])
        self._check(self.lib.h2y_ictcp_batch(self.h, width, height, sample, dst_bit_depth, dst_full_range, n, ins, outs))

    # ---- host <-> device pipeline -----------------------------------------------------------
    def stream_ictcp(self) -> None:
        """Arm an open forward ring of float planes (plain F32, DPX, PQ or HLG code) that was opened with src_transfer == dst_transfer
        == 8, src_matrix == dst_matrix == 0 and the 0 / 1 statistics override: every slot's decoded planes become code-valued PQ
        I, Ct, Cp samples in place, after stream_gamut's and stream_tonemap's passes, before the conversion (h2y_stream_ictcp)."""
        self._check(self.lib.h2y_stream_ictcp(self.h))

    def stream_lut3d(self, lut, interp=1, signal=0) -> None:
        """Arm an open forward ring of float or half planes (plain, DPX, EXR, PQ or HLG code) that was opened with src_matrix 0 and the
        0 / 1 statistics override: the Lut3d is applied to every slot's decoded planes in place, after stream_gamut's and
        stream_tonemap's passes, before stream_hlg's / stream_ictcp's and the conversion; signal 1 needs float planes and equal
        transfers (h2y_stream_lut3d)."""
        self._check(self.lib.h2y_stream_lut3d(self.h, lut.h if lut is not None else None, interp, signal))

    def stream_hlg(self, peak, relative) -> None:
        """Arm an open forward ring of float planes (plain F32, DPX or PQ code) that was opened with src_transfer == dst_transfer == 8
        and the 0 / 1 statistics override: every slot's decoded planes become code-valued HLG samples in place, after stream_gamut's
        and stream_tonemap's passes, before the conversion (h2y_stream_hlg)."""
        self._check(self.lib.h2y_stream_hlg(self.h, peak, relative))

    def stream_tonemap(self, src_peak, dst_peak, relative) -> None:
        """Arm an open forward ring of float or half planes (plain, DPX or EXR) that was opened with the 0 / 1 statistics override:
        every slot's decoded planes are tone-mapped in place, after stream_gamut's pass, before the conversion (h2y_stream_tonemap)."""
        self._check(self.lib.h2y_stream_tonemap(self.h, src_peak, dst_peak, relative))

    def stream_gamut(self, src_primaries, dst_primaries, clip=1) -> None:
        """Arm an open forward ring of float or half planes (plain, DPX or EXR): every slot's decoded planes are converted in
        place from src_primaries to dst_primaries before pic_stats and the conversion (h2y_stream_gamut)."""
        self._check(self.lib.h2y_stream_gamut(self.h, src_primaries, dst_primaries, clip))

    def stream_gamut_compress(self, src_primaries, dst_primaries, threshold=GAMUT_COMPRESS_THRESHOLD,
                              power=GAMUT_COMPRESS_POWER) -> None:
        """Arm an open forward ring as stream_gamut arms it, with k_gamut_compress in k_gamut's place: out-of-gamut colours are
        compressed, not clipped (h2y_stream_gamut_compress)."""
        self._check(self.lib.h2y_stream_gamut_compress(self.h, src_primaries, dst_primaries, threshold, power))

    def stream_scale(self, dst_w, dst_h, a=3) -> None:
        """Arm an open forward ring (plain, DPX, TIFF or EXR): stream_output then returns the frame scaled to dst_w x dst_h."""
        self._check(self.lib.h2y_stream_scale(self.h, dst_w, dst_h, a))
        self._stream_out_words = scale_frame_bytes(dst_w, dst_h, self._stream_desc.dst_chroma_format_idc) // 2
        self._stream_out_geom = (dst_w, dst_h, self._stream_desc.dst_chroma_format_idc)

    def scale_stream_open(self, src_w, src_h, chroma, bit_depth, full_range, gbr, dst_w, dst_h, a=3, depth=3) -> None:
        """A ring that only scales: stream_input lends the frame's three planes, stream_output returns the scaled frame."""
        self._check(self.lib.h2y_scale_stream_open(self.h, src_w, src_h, chroma, bit_depth, full_range, gbr, dst_w, dst_h, a, depth))
        nc = (src_w >> 1) * (src_h >> 1) if chroma == CHROMA_420 else src_w * src_h
        self._stream_inverse = None
        self._stream_dpx = None
        self._stream_rgb = False
        self._stream_cmp_planes = (src_w * src_h, nc, nc)
        self._stream_out_words = scale_frame_bytes(dst_w, dst_h, chroma) // 2
        self._stream_in_geom, self._stream_out_geom = (src_w, src_h, chroma), (dst_w, dst_h, chroma)

    def stream_dither(self, dst_depth, mode, temporal=0, seed=0, first_frame=0) -> None:
        """Arm an open forward ring (plain, DPX, TIFF, EXR or PQ code), after stream_scale where the ring scales: stream_output
        then returns the frame reduced from the descriptor's dst_bit_depth to dst_depth (h2y_stream_dither)."""
        self._check(self.lib.h2y_stream_dither(self.h, dst_depth, mode, temporal, seed & 0xFFFFFFFF, first_frame & 0xFFFFFFFF))

    def dither_stream_open(self, width, height, chroma, src_depth, dst_depth, full_range, gbr, mode, temporal=0, seed=0,
                           first_frame=0, depth=3) -> None:
        """A ring that only dithers: stream_input lends the frame's three planes, stream_output returns the reduced frame."""
        self._check(self.lib.h2y_dither_stream_open(self.h, width, height, chroma, src_depth, dst_depth, full_range, gbr, mode,
                                                    temporal, seed & 0xFFFFFFFF, first_frame & 0xFFFFFFFF, depth))
        nc = (width >> 1) * (height >> 1) if chroma == CHROMA_420 else width * height
        self._stream_inverse = None
        self._stream_dpx = None
        self._stream_rgb = False
        self._stream_cmp_planes = (width * height, nc, nc)
        self._stream_out_words = width * height + 2 * nc
        self._stream_in_geom = self._stream_out_geom = (width, height, chroma)

    def stream_pack(self, packing) -> None:
        """Arm an open forward, scale-only or dither-only ring, after stream_scale and stream_dither where the ring has them:
        stream_output then returns the frame that would go down packed, as a uint8 view of h2y_pack_frame_bytes bytes
        (h2y_stream_pack)."""
        self._check(self.lib.h2y_stream_pack(self.h, packing))
        self._stream_pack_bytes = pack_frame_bytes(*self._stream_out_geom, packing)  # (the library refused every ring without a .yuv frame)

    def stream_unpack(self, packing, bit_depth=None) -> None:
        """Arm an open inverse, planes or code ring: stream_input (and a compare-only ring's stream_reference) then lends one
        uint8 view of a packed frame (h2y_stream_unpack; with bit_depth given h2y_stream_unpack_ex, which a compare-only ring needs
        for PACK_P010)."""
        if bit_depth is None:
            self._check(self.lib.h2y_stream_unpack(self.h, packing))
        else:
            self._check(self.lib.h2y_stream_unpack_ex(self.h, packing, int(bit_depth)))
        self._stream_unpack_bytes = pack_frame_bytes(*self._stream_in_geom, packing)  # (the library refused every ring without code planes)

    def stream_histogram(self, bits=0, bit_depth=None, full_range=None, gbr=None) -> None:
        """Arm the open ring: every frame is counted on the device (h2y_stream_histogram; with bit_depth, full_range and gbr
        given, h2y_stream_histogram_ex, as a compare-only ring needs)."""
        if bit_depth is None and full_range is None and gbr is None:
            self._check(self.lib.h2y_stream_histogram(self.h, bits))
        else:
            f = (lambda v: -1 if v is None else int(v))
            self._check(self.lib.h2y_stream_histogram_ex(self.h, bits, f(bit_depth), f(full_range), f(gbr)))

    def stream_histogram_result(self):
        """(H2YHistogramStats, uint32 bins of shape (3, nbins)) of the frame stream_output returned last."""
        import numpy as np

        st = H2YHistogramStats()
        self._check(self.lib.h2y_stream_histogram_result(self.h, C.byref(st), None))
        bins = np.zeros((3, st.nbins), dtype=np.uint32)
        self._check(self.lib.h2y_stream_histogram_result(self.h, C.byref(st), bins.ctypes.data))
        return st, bins

    def histogram_stream_open(self, width, height, chroma, bit_depth, full_range, gbr, bits, depth=3) -> None:
        """A ring that only counts: stream_input lends the frame's three planes, stream_output returns None."""
        self._check(self.lib.h2y_histogram_stream_open(self.h, width, height, chroma, bit_depth, full_range, gbr, bits, depth))
        nc = (width >> 1) * (height >> 1) if chroma == CHROMA_420 else width * height
        self._stream_inverse = None
        self._stream_dpx = None
        self._stream_rgb = False
        self._stream_cmp_planes = (width * height, nc, nc)
        self._stream_in_geom = (width, height, chroma)

    def stream_compare(self, sigma, keep_output=1) -> None:
        """Arm the open ring: every frame is compared with the reference stream_reference lends for it."""
        self._check(self.lib.h2y_stream_compare(self.h, sigma, keep_output))
        if getattr(self, "_stream_inverse", None):
            w, h, _ = self._stream_inverse
            self._stream_ref_shape = (3 * w * h,)
        else:
            self._stream_ref_shape = (frame_bytes(self._stream_desc) // 2,)

    def stream_reference(self):
        """The pinned reference slot of the frame about to be submitted, a uint16 view to fill in place (a .yuv frame on the
        forward rings, G | B | R on the inverse rings, the three planes of a compare-only ring)."""
        p = C.c_void_p()
        self._check(self.lib.h2y_stream_reference(self.h, C.byref(p)))
        if getattr(self, "_stream_unpack_bytes", None) and getattr(self, "_stream_cmp_planes", None):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(self._stream_unpack_bytes,))  # a compare-only ring's, packed
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint16)), shape=self._stream_ref_shape)

    def stream_compare_result(self) -> H2YCompareStats:
        st = H2YCompareStats()
        self._check(self.lib.h2y_stream_compare_result(self.h, C.byref(st)))
        return st

    def stream_ssim(self, bit_depth=-1) -> None:
        """Arm a compare-armed ring for SSIM too (bit_depth -1: the ring's own; a compare-only ring needs it given)."""
        self._check(self.lib.h2y_stream_ssim(self.h, bit_depth))

    def stream_regions(self, flat_var, radius=1) -> None:
        """Arm a compare-armed ring to measure flat and busy areas, over- and undershoot too (h2y_stream_regions)."""
        self._check(self.lib.h2y_stream_regions(self.h, flat_var, radius))

    def stream_regions_result(self) -> H2YRegionsStats:
        """The H2YRegionsStats of the frame stream_output returned last."""
        st = H2YRegionsStats()
        self._check(self.lib.h2y_stream_regions_result(self.h, C.byref(st)))
        return st

    def stream_deltae(self, d: H2YCodelightDesc, threshold=1.0) -> None:
        """Arm a compare-armed ring for Delta E ITP too: d describes the ring's frames as PQ code planes."""
        self._check(self.lib.h2y_stream_deltae(self.h, C.byref(d), float(threshold)))

    def stream_deltae_result(self) -> H2YDeltaeStats:
        """The H2YDeltaeStats of the frame stream_output returned last."""
        st = H2YDeltaeStats()
        self._check(self.lib.h2y_stream_deltae_result(self.h, C.byref(st)))
        return st

    def stream_light(self) -> None:
        """Arm an open forward ring (plain, DPX, TIFF or EXR) to measure every frame's content light (h2y_stream_light)."""
        self._check(self.lib.h2y_stream_light(self.h))

    def stream_lightdist(self) -> None:
        """Arm an open forward ring to measure every frame's light distribution (h2y_stream_lightdist)."""
        self._check(self.lib.h2y_stream_lightdist(self.h))

    def stream_gamutcheck(self, file_primaries: int, sets, ratio: float = GAMUTCHECK_RATIO, floor: float = GAMUTCHECK_FLOOR) -> None:
        """Arm an open light-only ring to check every frame's gamut containment (h2y_stream_gamutcheck)."""
        arr, ns = _int_array(sets)
        self._check(self.lib.h2y_stream_gamutcheck(self.h, int(file_primaries), ns, arr, float(ratio), float(floor)))

    def stream_gamutcheck_result(self) -> H2YGamutcheckStats:
        """The gamut containment check of the frame stream_output returned last (h2y_stream_gamutcheck_result)."""
        st = H2YGamutcheckStats()
        self._check(self.lib.h2y_stream_gamutcheck_result(self.h, C.byref(st)))
        return st

    def stream_scenesig(self) -> None:
        """Arm an open forward ring or light-only ring to measure every frame's scene signature (h2y_stream_scenesig)."""
        self._check(self.lib.h2y_stream_scenesig(self.h))

    def stream_scenesig_result(self) -> H2YScenesig:
        """The scene signature of the frame stream_output() returned last."""
        st = H2YScenesig()
        self._check(self.lib.h2y_stream_scenesig_result(self.h, C.byref(st)))
        return st

    def stream_lightdist_bins(self) -> np.ndarray:
        """The LIGHTDIST_BINS bins (uint32) of the frame stream_output() returned last, on a ring that measures the distribution."""
        b = np.zeros(LIGHTDIST_BINS, dtype=np.uint32)
        self._check(self.lib.h2y_stream_lightdist_bins(self.h, b.ctypes.data))
        return b

    def stream_lightdist_result(self) -> H2YLightdistStats:
        """The light distribution of the frame stream_output returned last."""
        st = H2YLightdistStats()
        self._check(self.lib.h2y_stream_lightdist_result(self.h, C.byref(st)))
        return st

    def stream_light_result(self) -> H2YLightStats:
        """The H2YLightStats of the frame stream_output returned last."""
        st = H2YLightStats()
        self._check(self.lib.h2y_stream_light_result(self.h, C.byref(st)))
        return st

    def stream_ssim_result(self) -> H2YSsimStats:
        """The H2YSsimStats of the frame stream_output returned last."""
        st = H2YSsimStats()
        self._check(self.lib.h2y_stream_ssim_result(self.h, C.byref(st)))
        return st

    def compare_stream_open(self, width, height, chroma, sigma, depth=3) -> None:
        """A ring that only compares: stream_input lends A's three planes, stream_reference B's frame in the same layout."""
        self._check(self.lib.h2y_compare_stream_open(self.h, width, height, chroma, sigma, depth))
        nc = (width >> 1) * (height >> 1) if chroma == CHROMA_420 else width * height
        self._stream_inverse = None
        self._stream_dpx = None
        self._stream_rgb = False
        self._stream_cmp_planes = (width * height, nc, nc)
        self._stream_in_geom = (width, height, chroma)
        self._stream_ref_shape = (width * height + 2 * nc,)

    def stream_open(self, d, depth=3) -> None:
        self._check(self.lib.h2y_stream_open(self.h, C.byref(d), depth))
        self._stream_desc = d
        self._stream_out_geom = (d.width, d.height, d.dst_chroma_format_idc)
        self._stream_inverse = None
        self._stream_dpx = None
        self._stream_rgb = False

    def tiff_stream_open(self, d, info: H2YTiffInfo, clamp_video_range, depth=3) -> None:
        """The forward ring on TIFF rows: stream_input gives one uint8 view of the pinned slot (info.payload_bytes) to fill with
        the decoded rows; stream_output gives the .yuv frame as on a forward stream."""
        self._check(self.lib.h2y_tiff_stream_open(self.h, C.byref(d), C.byref(info), int(clamp_video_range), depth))
        self._stream_desc = d
        self._stream_out_geom = (d.width, d.height, d.dst_chroma_format_idc)
        self._stream_inverse = None
        self._stream_dpx = int(info.payload_bytes)
        self._stream_rgb = False

    def exr_stream_open(self, d, info: H2YExrInfo, depth=3) -> None:
        """The forward ring on EXR payloads: stream_input gives one uint8 view of the pinned slot (info.payload_bytes) to fill
        with exr_unpack; stream_output gives the .yuv frame as on a forward stream."""
        self._check(self.lib.h2y_exr_stream_open(self.h, C.byref(d), C.byref(info), depth))
        self._stream_desc = d
        self._stream_out_geom = (d.width, d.height, d.dst_chroma_format_idc)
        self._stream_inverse = None
        self._stream_dpx = int(info.payload_bytes)
        self._stream_rgb = False

    def tiff_inverse_stream_open(self, width, height, in_chroma, in_depth, in_full_range, in_matrix, out_depth, algorithm,
                                 depth=3) -> None:
        """The inverse ring with write_tiff's interleave: stream_input gives Y, Cb/Dz, Cr/Dx, stream_output a (height, width, 3)
        u16 view, R, G, B per pixel (the samples between tiff_layout's head and tail)."""
        self._check(self.lib.h2y_tiff_inverse_stream_open(self.h, width, height, in_chroma, in_depth, in_full_range, in_matrix,
                                                          out_depth, algorithm, depth))
        self._stream_inverse = (width, height, in_chroma)
        self._stream_in_geom = (width, height, in_chroma)
        self._stream_dpx = None
        self._stream_rgb = True

    def dpx_stream_open(self, d, info: H2YDpxInfo, depth=3) -> None:
        """The forward ring on DPX payloads: stream_input gives one uint8 view of the pinned payload (info.payload_bytes) to fill
        with the file's bytes from info.data_offset on; stream_output gives the .yuv frame as on a forward stream."""
        self._check(self.lib.h2y_dpx_stream_open(self.h, C.byref(d), C.byref(info), depth))
        self._stream_desc = d
        self._stream_out_geom = (d.width, d.height, d.dst_chroma_format_idc)
        self._stream_inverse = None
        self._stream_dpx = int(info.payload_bytes)
        self._stream_rgb = False

    def inverse_stream_open(self, width, height, in_chroma, in_depth, in_full_range, in_matrix, out_depth, algorithm, depth=3) -> None:
        """The pinned ring for the .yuv -> G,B,R flow: stream_input gives Y, Cb/Dz, Cr/Dx, stream_output G, B, R."""
        self._check(self.lib.h2y_inverse_stream_open(self.h, width, height, in_chroma, in_depth, in_full_range, in_matrix, out_depth,
                                                     algorithm, depth))
        self._stream_inverse = (width, height, in_chroma)
        self._stream_in_geom = (width, height, in_chroma)
        self._stream_dpx = None
        self._stream_rgb = False

    def stream_input(self):
        """The three pinned input planes of the next slot, as numpy views to fill in place (on a DPX, TIFF or EXR stream:
        [payload], uint8)."""
        import numpy as np

        ptrs = (C.c_void_p * 3)()
        self._check(self.lib.h2y_stream_input(self.h, ptrs))
        if getattr(self, "_stream_unpack_bytes", None):
            return [np.ctypeslib.as_array(C.cast(ptrs[0], C.POINTER(C.c_uint8)), shape=(self._stream_unpack_bytes,))]
        if getattr(self, "_stream_cmp_planes", None):
            return [np.ctypeslib.as_array(C.cast(ptrs[c], C.POINTER(C.c_uint16)), shape=(n,)) for c, n in enumerate(self._stream_cmp_planes)]
        if getattr(self, "_stream_dpx", None):
            return [np.ctypeslib.as_array(C.cast(ptrs[0], C.POINTER(C.c_uint8)), shape=(self._stream_dpx,))]
        if getattr(self, "_stream_inverse", None):
            w, h, chroma = self._stream_inverse
            nc = (w // 2) * (h // 2) if chroma == CHROMA_420 else w * h
            return [np.ctypeslib.as_array(C.cast(ptrs[c], C.POINTER(C.c_uint16)), shape=(nc if c else w * h,)) for c in range(3)]
        d = self._stream_desc
        n = d.width * d.height
        dt = np.float32 if d.in_sample_type == SAMPLE_F32 else np.uint16
        return [np.ctypeslib.as_array(C.cast(ptrs[c], C.POINTER(C.c_float if dt is np.float32 else C.c_uint16)), shape=(n,)) for c in range(3)]

    def stream_submit(self) -> None:
        self._check(self.lib.h2y_stream_submit(self.h))

    def stream_output(self):
        """The oldest frame in flight (a numpy view of pinned memory, valid until the next stream_output).  On an inverse
        stream: shape (3, width*height), rows G, B, R (``.reshape(-1)`` for the three planes as one)."""
        import numpy as np

        p = C.POINTER(C.c_uint16)()
        self._check(self.lib.h2y_stream_output(self.h, C.byref(p)))
        if not p:  # an armed ring with keep_output 0, or a compare-only ring: the frame stayed on the device
            return None
        if getattr(self, "_stream_pack_bytes", None):  # a ring that packs
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(self._stream_pack_bytes,))
        if getattr(self, "_stream_out_words", None):  # a ring that scales
            return np.ctypeslib.as_array(p, shape=(self._stream_out_words,))
        if getattr(self, "_stream_inverse", None):
            w, h, _ = self._stream_inverse
            if getattr(self, "_stream_rgb", False):
                return np.ctypeslib.as_array(p, shape=(h, w, 3))
            return np.ctypeslib.as_array(p, shape=(3, w * h))
        return np.ctypeslib.as_array(p, shape=(frame_bytes(self._stream_desc) // 2,))

    def stream_close(self) -> None:
        self._check(self.lib.h2y_stream_close(self.h))
        self._stream_cmp_planes = None
        self._stream_out_words = None
        self._stream_pack_bytes = None
        self._stream_unpack_bytes = None
        self._stream_in_geom = None
        self._stream_out_geom = None
        self._stream_inverse = None
        self._stream_dpx = None
        self._stream_rgb = False

    def last_kernel_name(self) -> str:
        return (self.lib.h2y_last_kernel_name(self.h) or b"").decode()

    def last_kernel_variant(self) -> str:
        return (self.lib.h2y_last_kernel_variant(self.h) or b"").decode()
