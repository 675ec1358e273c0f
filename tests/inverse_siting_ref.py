"""4:2:0 -> 4:4:4 chroma upsampling restated in numpy: the reference's Subsample420to444 (FIR branch, convert.cpp:1882-1983), whose
source is centred between two luma rows (chroma_sample_loc_type 0), and the project's top-left form (loc type 2) as
include/hdr2yuv_hip.h ("inverse chroma siting") defines it.

A plain module: numpy only.  A chroma plane C of w2 x h2 codes, the clip [lo, hi]:
  1. the vertical stage into the U16 intermediate M of w2 x 2 h2, rows clamped into 0..h2-1:
       vertical_reference(): up_fir6, (3 -16 67 227 -32 7)/256 of rows r-3..r+2 for row 2r and, mirrored, of rows r+3..r-2 for row
         2r+1, in binary32, every product and sum rounded by itself, + 0.5, the clamp, truncation (h2y_math.h's up_fir6);
       vertical_top_left(): row 2r is med3(C[r], lo, hi); row 2r+1 is med3((S + 128) >> 8, lo, hi) with
         S = 21 (C[r-2] + C[r+3]) - 52 (C[r-1] + C[r+2]) + 159 (C[r] + C[r+1]) in exact integers;
  2. horizontal(): the reference's stage for both: out[y][2c] = M[y][c], out[y][2c+1] = up_fir_odd of M[y][c-2..c+3], columns
     clamped, in binary32 the same way (h2y_math.h's up_fir_odd).
tests/test_inverse_siting_host.py pins upsample_reference() to the oracle's Subsample420to444, and with it the shared stage 2."""
import numpy as np

F32 = np.float32


def _c(k):
    return F32(k) / F32(256.0)  # k / 256 is exact in binary32


def _clamp_trunc(t, lo, hi):
    """clamp to [lo, hi] and truncate (convert.cpp:1932-1934); t is a float32 array"""
    return np.maximum(np.minimum(t, F32(hi)), F32(lo)).astype(np.int64)


def up_fir6(a, b, c, d, e, f, lo, hi):
    """h2y_math.h's up_fir6 on float32 arrays: products and sums left to right, each rounded to binary32"""
    a, b, c, d, e, f = (np.asarray(x, F32) for x in (a, b, c, d, e, f))
    acc = _c(3) * a - _c(16) * b
    acc = acc + _c(67) * c
    acc = acc + _c(227) * d
    acc = acc - _c(32) * e
    acc = acc + _c(7) * f
    return _clamp_trunc(acc + F32(0.5), lo, hi)


def up_fir_odd(m0, m1, m2, m3, m4, m5, lo, hi):
    """h2y_math.h's up_fir_odd on float32 arrays"""
    m0, m1, m2, m3, m4, m5 = (np.asarray(x, F32) for x in (m0, m1, m2, m3, m4, m5))
    acc = _c(21) * (m0 + m5) - _c(52) * (m1 + m4)
    acc = acc + _c(159) * (m2 + m3)
    return _clamp_trunc(acc + F32(0.5), lo, hi)


def _rows(c, off):
    """rows r + off of the (h2, w2) plane for every r, clamped into the plane"""
    h2 = c.shape[0]
    return c[np.clip(np.arange(h2) + off, 0, h2 - 1), :]


def vertical_reference(c, lo, hi):
    """(h2, w2) -> the intermediate (2 h2, w2), int64: the reference's quarter-phase pair"""
    c = np.asarray(c).astype(F32)
    m = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    m[0::2] = up_fir6(*[_rows(c, o) for o in (-3, -2, -1, 0, 1, 2)], lo, hi)
    m[1::2] = up_fir6(*[_rows(c, o) for o in (3, 2, 1, 0, -1, -2)], lo, hi)
    return m


def top_left_sums(c):
    """S of the odd rows, int64, not rounded and not clamped"""
    c = np.asarray(c).astype(np.int64)
    return (21 * (_rows(c, -2) + _rows(c, 3)) - 52 * (_rows(c, -1) + _rows(c, 2)) + 159 * (_rows(c, 0) + _rows(c, 1)))


def vertical_top_left(c, lo, hi):
    """(h2, w2) -> the intermediate (2 h2, w2), int64: even rows copied, odd rows the integer half-phase six-tap"""
    c = np.asarray(c).astype(np.int64)
    m = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    m[0::2] = np.clip(c, lo, hi)
    m[1::2] = np.clip((top_left_sums(c) + 128) >> 8, lo, hi)  # >> on int64: arithmetic, the floor
    return m


def horizontal(m, lo, hi):
    """(H, w2) -> (H, 2 w2) uint16: the reference's horizontal stage"""
    m = np.asarray(m).astype(np.int64)
    w2 = m.shape[1]
    cols = np.arange(w2)
    out = np.empty((m.shape[0], 2 * w2), np.uint16)
    out[:, 0::2] = m
    mf = m.astype(F32)
    out[:, 1::2] = up_fir_odd(*[mf[:, np.clip(cols + o, 0, w2 - 1)] for o in (-2, -1, 0, 1, 2, 3)], lo, hi)
    return out


def upsample_top_left(c, lo, hi):
    """what h2y_upsample_444_sited(.., chroma_sample_loc_type 2, lo, hi, ..) writes: (h2, w2) -> (2 h2, 2 w2) uint16"""
    return horizontal(vertical_top_left(c, lo, hi), lo, hi)


def upsample_reference(c, lo, hi):
    """Subsample420to444's FIR branch restated"""
    return horizontal(vertical_reference(c, lo, hi), lo, hi)
