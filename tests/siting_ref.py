"""Top-left co-sited 4:2:0 chroma (chroma_sample_loc_type 2) restated in numpy, as include/hdr2yuv_hip.h ("chroma siting") defines it.

A plain module: numpy only.  A chroma plane T of W x H codes (matrix_convert's output: not shifted, not clamped to the output's
range), maxCV the FIR's clip:
  1. stage1(): Subsample444to420_FIR's horizontal stage (convert.cpp:305-317) at every row and every even column, in binary32, every
     product and sum rounded by itself in the reference's order (h2y_math.h's fir_h), + 0.5, clamped to [0, maxCV], truncated;
  2. stage2_top_left(): the same seven taps down the column at every even row, in exact integers:
     S = 21 (M[j-5] + M[j+5]) - 52 (M[j-3] + M[j+3]) + 159 (M[j-1] + M[j+1]) + 256 M[j], V = clamp((S + 256) >> 9, 0, maxCV);
  3. write_yuv(): the shift and the per-plane range clamp (tiff.cpp:457-550).
stage2_reference() is the reference's own vertical stage (the even 12-tap filter, half a row lower: centre sited; convert.cpp:365-374)
in binary32 the same way (h2y_math.h's fir_v): with stage1() it restates Subsample444to420_FIR, which pins this file's stage 1 to the
oracle at every bit depth.  Edges replicate by index clamping in both directions."""
import numpy as np

F32 = np.float32
TAPS7 = ((-5, 21), (-3, -52), (-1, 159), (0, 256), (1, 159), (3, -52), (5, 21))


def _c(k):
    return F32(k) / F32(512.0)  # k / 512 is exact in binary32


def _clamp_trunc(t, maxcv):
    """clamp to [0, maxCV] and truncate (convert.cpp:314-317, :372-374); t is a float32 array"""
    return np.minimum(np.maximum(t, F32(0.0)), F32(maxcv)).astype(np.int64)


def fir_h(m5, m3, m1, c, p1, p3, p5, maxcv):
    """h2y_math.h's fir_h on float32 arrays: the sums left to right, each operation rounded to binary32"""
    m5, m3, m1, c, p1, p3, p5 = (np.asarray(a, F32) for a in (m5, m3, m1, c, p1, p3, p5))
    acc = _c(21) * (m5 + p5) - _c(52) * (m3 + p3)
    acc = acc + _c(159) * (m1 + p1)
    acc = acc + _c(256) * c
    return _clamp_trunc(acc + F32(0.5), maxcv)


def fir_v(rows, maxcv):
    """h2y_math.h's fir_v: rows = the twelve float32 arrays of 4:2:2 rows j-5 .. j+6"""
    m5, m4, m3, m2, m1, m0, p1, p2, p3, p4, p5, p6 = (np.asarray(a, F32) for a in rows)
    acc = _c(228) * (m0 + p1) + _c(70) * (m1 + p2)
    acc = acc - _c(37) * (m2 + p3)
    acc = acc - _c(21) * (m3 + p4)
    acc = acc + _c(11) * (m4 + p5)
    acc = acc + _c(5) * (m5 + p6)
    return _clamp_trunc(acc + F32(0.5), maxcv)


def stage1(t, maxcv):
    """(H, W) codes -> the 4:2:2 intermediate (H, W/2), int64"""
    t = np.asarray(t).astype(F32)
    h, w = t.shape
    assert h % 2 == 0 and w % 2 == 0
    cols = np.arange(0, w, 2)
    return fir_h(*[t[:, np.clip(cols + off, 0, w - 1)] for off, _ in TAPS7], maxcv)


def vertical_sums(m):
    """S of the top-left vertical stage at every even row of the (H, W/2) intermediate, int64, not rounded and not clamped"""
    m = np.asarray(m).astype(np.int64)
    h = m.shape[0]
    rows = np.arange(0, h, 2)
    s = np.zeros((rows.size, m.shape[1]), np.int64)
    for off, k in TAPS7:
        s += k * m[np.clip(rows + off, 0, h - 1), :]
    return s


def stage2_top_left(m, maxcv):
    """(H, W/2) -> (H/2, W/2): the integer 7-tap at the even rows"""
    return np.clip((vertical_sums(m) + 256) >> 9, 0, maxcv)


def stage2_reference(m, maxcv):
    """(H, W/2) -> (H/2, W/2): the reference's 12-tap between rows 2r and 2r + 1, binary32"""
    m = np.asarray(m).astype(F32)
    h = m.shape[0]
    rows = np.arange(0, h, 2)
    return fir_v([m[np.clip(rows + off, 0, h - 1), :] for off in range(-5, 7)], maxcv)


def subsample_top_left(t, depth):
    """One (H, W) plane of codes below 2^depth -> (H/2, W/2) uint16, maxCV = 2^depth - 1, no write_yuv step: what
    h2y_subsample_420_sited(.., chroma_sample_loc_type 2, ..) writes"""
    maxcv = (1 << depth) - 1
    return stage2_top_left(stage1(t, maxcv), maxcv).astype(np.uint16)


def subsample_reference(t, depth):
    """Subsample444to420_FIR restated: stage 1, then the reference's vertical stage"""
    maxcv = (1 << depth) - 1
    return stage2_reference(stage1(t, maxcv), maxcv).astype(np.uint16)


def clip_limits(depth, full):
    """set_pic_clip() (common.cpp:262-327): (minVR, maxVR, minVRC, maxVRC, maxCV)"""
    maxcv = (1 << depth) - 1
    if full:
        return 0, maxcv, 0, maxcv, maxcv
    d = 1 << (depth - 8)
    return 16 * d, 235 * d, 16 * d, 240 * d, maxcv


def write_yuv(plane, down_shift, full, lo, hi, maxcv):
    """write_yuv's shift, then its clamp: [lo, hi] in video range, maxCV in full range"""
    v = np.asarray(plane).astype(np.int64) >> down_shift
    return (np.minimum(v, maxcv) if full else np.clip(v, lo, hi)).astype(np.uint16)


def tmp_depth(d):
    """tmp_pic's depth (hdr2yuv.cpp:803-812): the input's when the input is U16 too, else the output's"""
    return d.src_bit_depth if d.in_sample_type == 1 else d.dst_bit_depth


def tmp_planes(oracle, d, planes):
    """The oracle's matrix_convert(d, planes, floor, ceil, tmp depth) with pic_stats' floor and ceiling (the descriptor's when it
    overrides them; none are read when the transfers are equal): (3, H, W) uint16.  Half planes (their bits) are widened first."""
    flat = [np.ascontiguousarray(p).reshape(-1) for p in planes]
    if d.in_sample_type == 3:  # F16, exr.cpp:233
        flat = [p.view(np.float16).astype(np.float32) for p in flat]
    if d.stats_override:
        fl, ce = [d.floor[c] for c in range(3)], [d.ceiling[c] for c in range(3)]
    elif d.src_transfer == d.dst_transfer:
        fl, ce = [0, 0, 0], [1, 1, 1]
    else:
        assert d.in_sample_type != 1, "u16 input with a transfer conversion: not restated here"
        _, fl, ce = oracle.stats_f32(flat)
    di = type(d).from_buffer_copy(bytes(d))
    if d.in_sample_type == 3:
        di.in_sample_type = 2
    return oracle.matrix_convert(di, flat, fl, ce, tmp_depth(d)).reshape(3, d.height, d.width)


def frame_top_left(oracle, d, planes):
    """The .yuv frame (flat uint16: Y | Cb | Cr) of a 4:2:0 FIR descriptor with chroma siting 2"""
    assert d.dst_chroma_format_idc == 1 and d.chroma_resampler_type != 0
    t = tmp_planes(oracle, d, planes)
    td = tmp_depth(d)
    shift = td - d.dst_bit_depth
    assert shift >= 0
    lo, hi, loc, hic, maxcv = clip_limits(d.dst_bit_depth, d.dst_full_range)
    out = [write_yuv(t[0], shift, d.dst_full_range, lo, hi, maxcv).reshape(-1)]
    for c in (1, 2):
        out.append(write_yuv(subsample_top_left(t[c], td), shift, d.dst_full_range, loc, hic, maxcv).reshape(-1))
    return np.concatenate(out)
