"""hdr2yuv_amd -- MI355X (gfx950) implementation of hdr2yuv's in-memory convert
path (linear RGB/XYZ -> PQ -> colour-difference matrix -> quantise -> 4:2:0).

The product is ``libhdr2yuv_hip.so`` (hand-written HIP kernels behind the C-ABI
in ``include/hdr2yuv_hip.h``).  This package is the thin Python host mirror of
that ABI used by the tests and ``bench.py``: ctypes only, plus torch for device
memory / streams.  There is no CPU fallback: importing works anywhere, creating
a :class:`Context` needs a HIP device and the built library.
"""
from .api import (  # noqa: F401
    CHROMA_420,
    CHROMA_444,
    CODELIGHT_FRAMES_PER_LAUNCH,
    H2YCodelightDesc,
    H2YCompareStats,
    H2YDesc,
    H2YDpxInfo,
    H2YError,
    H2YExrChunk,
    H2YExrInfo,
    H2YHistogramStats,
    H2YLightStats,
    H2YLightdistStats,
    LIGHTDIST_BINS,
    LIGHTDIST_FIRST_BITS,
    LIGHTDIST_PCT,
    H2YSsimStats,
    H2YTiffInfo,
    MATRIX_BT2020NC,
    MATRIX_BT709,
    MATRIX_GBR,
    MATRIX_Y100,
    MATRIX_Y500,
    MATRIX_YDZDX,
    MATRIX_YUVPRIME2,
    SAMPLE_F16,
    SAMPLE_F32,
    SAMPLE_U16,
    TRANSFER_LINEAR,
    TRANSFER_PQ,
    Context,
    build_library,
    desc_check,
    exr_unpack,
    frame_bytes,
    gamut_matrix,
    library_path,
    lightdist_json,
    load_library,
    make_codelight_desc,
    make_desc,
    parse_dpx,
    parse_exr,
    parse_tiff,
    scale_frame_bytes,
    scale_taps,
    set_library_path,
    tiff_layout,
)
