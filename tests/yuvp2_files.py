"""dst_matrix_coeffs 15 ("YUVPrime2") restated in numpy, and the pictures the Y'u'v' tests run.

What the reference does (hdr2yuv.cpp:797-928 as oracle/ref_shim.cpp drives it):
  - matrix_convert() into the U16 4:4:4 tmp_pic: G, B, R passed through (convert.cpp:1191-1194); unless the source matrix is
    15 too (with equal primaries), Half - 1 added to the two chroma planes (:1200-1201); everything clamped to tmp_pic's maxCV.
    The scale step and the transfer chain are the other matrices' (the oracle's C restatement supplies them: its identity
    case is the same arithmetic, and min(min(u, maxCV) + Half - 1, maxCV) == min(u + Half - 1, maxCV)).
  - convert(): 4:4:4 copies the planes.  4:2:0 (convert.cpp:533-800): Y' copied; lin(Y'), Z = Cb and X = Cr subsampled by
    the box or the FIR with tmp_pic's clip; per site, in binary64, X, Y, Z divided by 65535 whatever the depth,
    u' = 4X / (X + 15Y + 3Z), v' = 9Y / (X + 15Y + 3Z) (0 where the sum is not positive), clipped to [0, 1], times 65535.0
    and truncated.  (The reference computes u''v'' and overwrites them with u'v', convert.cpp:732-734.)
  - write_yuv(): the down shift and the output range clamp.
lin(c) = (unsigned short)(RHO_GAMMA_f((float)(c / 65535.0)) * 65535.0), with RHO_GAMMA_f's two pow calls made through this
host's libm exactly as the reference makes them (powf(25.0f, V), then pow in binary64)."""
import ctypes
import ctypes.util
import functools

import numpy as np

from oracle import binding as ob

MATRIX_YUVPRIME2 = 15

_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.powf.restype, _libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
_libm.pow.restype, _libm.pow.argtypes = ctypes.c_double, [ctypes.c_double, ctypes.c_double]


@functools.lru_cache(maxsize=1)
def lin_table() -> np.ndarray:
    """convert.cpp:586-592 for every u16 code (RHO_GAMMA_f: convert.cpp:12-27)"""
    gamma = float(np.float32(2.4))
    out = np.empty(65536, np.uint16)
    for c in range(65536):
        v = float(np.float32(c / 65535.0))
        p = _libm.powf(25.0, v)
        lf = float(np.float32(_libm.pow((p - 1.0) / 24.0, gamma)))
        out[c] = int(lf * 65535.0)
    return out


def tmp_depth(d) -> int:
    return d.src_bit_depth if d.in_sample_type == ob.SAMPLE_U16 else d.dst_bit_depth


def tmp_pic(oracle, d, planes) -> np.ndarray:
    """matrix_convert()'s output for dst_matrix 15: (3, H*W) uint16"""
    u16 = d.in_sample_type == ob.SAMPLE_U16
    flat = [np.ascontiguousarray(p).reshape(-1) for p in planes]
    if d.in_sample_type == ob.SAMPLE_F16:  # half bits as u16 (the C-ABI's layout), widened to float first (exr.cpp:233)
        flat = [p.astype(np.uint16).view(np.float16).astype(np.float32) for p in flat]
    fl, ce = [0, 0, 0], [1, 1, 1]
    if d.src_transfer != d.dst_transfer:
        if d.stats_override:
            fl, ce = list(d.floor), list(d.ceiling)
        elif u16:
            raise NotImplementedError("u16 input with a transfer conversion")
        else:
            _, fl, ce = oracle.stats_f32(flat)
    di = ob.H2YDesc.from_buffer_copy(bytes(d))
    di.src_matrix = di.dst_matrix = MATRIX_YUVPRIME2
    di.src_primaries = di.dst_primaries = d.dst_primaries
    if not u16:
        di.in_sample_type = ob.SAMPLE_F32
    td = tmp_depth(d)
    t = oracle.matrix_convert(di, flat, fl, ce, td).astype(np.int64)
    if not (d.src_matrix == d.dst_matrix and d.src_primaries == d.dst_primaries):
        max_cv, half_m1 = (1 << td) - 1, (1 << (td - 1)) - 1
        t[1:] = np.minimum(t[1:] + half_m1, max_cv)
    return t.astype(np.uint16)


def uv(sx, sy, sz):
    """u', v' of 4:2:0 sites from their subsampled X, linear Y and Z (convert.cpp:674-745)"""
    X = sx.astype(np.float64) / 65535.0
    Z = sz.astype(np.float64) / 65535.0
    Y = sy.astype(np.float64) / 65535.0
    s = (X + 15.0 * Y) + 3.0 * Z
    pos = s > 0.0
    safe = np.where(pos, s, 1.0)
    up = np.where(pos, (4.0 * X) / safe, 0.0)
    vp = np.where(pos, (9.0 * Y) / safe, 0.0)
    up = np.clip(up, 0.0, 1.0)
    vp = np.clip(vp, 0.0, 1.0)
    return (up * 65535.0).astype(np.uint32), (vp * 65535.0).astype(np.uint32)


def _box(p):
    p = p.astype(np.uint32)
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) // 4


def _write_yuv(v, shift, full, lo, hi, max_cv):
    v = v.astype(np.uint32) >> shift
    return np.minimum(v, max_cv) if full else np.clip(v, lo, hi)


def convert(oracle, d, planes) -> np.ndarray:
    """The .yuv frame the reference writes for a descriptor with dst_matrix 15"""
    W, H = d.width, d.height
    t = tmp_pic(oracle, d, planes)
    td = tmp_depth(d)
    if d.dst_chroma_format_idc == ob.CHROMA_444:
        y, cb, cr = t[0], t[1], t[2]
    else:
        yp = t[0].reshape(H, W)
        lin = lin_table()[yp]
        zp, xp = t[1].reshape(H, W), t[2].reshape(H, W)
        if d.chroma_resampler_type == 0:
            sy, sz, sx = _box(lin), _box(zp), _box(xp)
        else:
            sy, sz, sx = (oracle.sub420(p, td, True) for p in (lin, zp, xp))
        u, v = uv(sx, sy, sz)
        y, cb, cr = t[0], u.reshape(-1), v.reshape(-1)
    dd = d.dst_bit_depth
    shift, full, max_cv = td - dd, d.dst_full_range, (1 << dd) - 1
    D = 1 << (dd - 8)
    out = [_write_yuv(y, shift, full, 16 * D, 235 * D, max_cv), _write_yuv(cb, shift, full, 16 * D, 240 * D, max_cv),
           _write_yuv(cr, shift, full, 16 * D, 240 * D, max_cv)]
    return np.concatenate(out).astype(np.uint16)


# ---- pictures -------------------------------------------------------------------------------------------------------------
def desc(w, h, *, sample=ob.SAMPLE_U16, src_depth=16, dst_depth=16, src_matrix=MATRIX_YUVPRIME2, resampler=0, full=0,
         chroma=ob.CHROMA_420, transfer=(16, 16), primaries=(9, 9)):
    return ob.make_desc(w, h, sample=sample, src_depth=src_depth, dst_depth=dst_depth, src_transfer=transfer[0],
                        dst_transfer=transfer[1], src_matrix=src_matrix, dst_matrix=MATRIX_YUVPRIME2, src_primaries=primaries[0],
                        dst_primaries=primaries[1], full_range=full, chroma=chroma, resampler=resampler)


def u16_planes(rng, w, h, depth):
    """random code values below 2^depth, with black (X + 15Y + 3Z = 0) and white 2x2 blocks planted"""
    p = [rng.integers(0, 1 << depth, size=(h, w), dtype=np.uint16) for _ in range(3)]
    for c in range(3):
        p[c][0:2, 0:2] = 0
        p[c][0:2, 2:4] = (1 << depth) - 1
    p[1][2:4, 0:2] = 0  # Z = 0 under a random Y'/X
    return [x.reshape(-1) for x in p]


def every_code_planes(rng):
    """256 x 256: the Y' plane holds every u16 code once (shuffled), Z and X random"""
    y = rng.permutation(65536).astype(np.uint16)
    return [y, rng.integers(0, 65536, 65536, dtype=np.uint16), rng.integers(0, 65536, 65536, dtype=np.uint16)]


def float_planes(rng, w, h, f16=False):
    """linear light in [0, 1.2) with zeros and ones planted"""
    p = [(rng.random((h * w,), dtype=np.float32) * np.float32(1.2)).astype(np.float32) for _ in range(3)]
    for c in range(3):
        p[c][:3] = np.float32(0.0)
        p[c][3] = np.float32(1.0)
    return [x.astype(np.float16).view(np.uint16) for x in p] if f16 else p  # half: its bits, as the C-ABI takes them


def grid():
    """(name, descriptor, planes) of the single-frame cases, deterministic"""
    rng = np.random.default_rng(1515)
    out = []
    F = ob.SAMPLE_F32
    for src_m in (MATRIX_YUVPRIME2, 0):
        for res in (0, 1):
            for depth, dst in ((16, 16), (16, 12), (16, 10), (12, 12), (12, 10), (10, 10)):
                for full in (0, 1):
                    w, hh = (24, 12) if res == 0 else (22, 10)
                    d = desc(w, hh, src_depth=depth, dst_depth=dst, src_matrix=src_m, resampler=res, full=full)
                    out.append((f"u16_{src_m}_{res}_{depth}to{dst}_{full}", d, u16_planes(rng, w, hh, depth)))
            # float LINEAR -> PQ, the temporary picture at the output's depth
            for dst in (10, 12, 16):
                for full in (0, 1):
                    d = desc(32, 16, sample=F, src_depth=32, dst_depth=dst, src_matrix=src_m, resampler=res, full=full, transfer=(8, 16))
                    out.append((f"f32_{src_m}_{res}_{dst}_{full}", d, float_planes(rng, 32, 16)))
            d = desc(32, 8, sample=ob.SAMPLE_F16, src_depth=32, dst_depth=12, src_matrix=src_m, resampler=res, transfer=(8, 16))
            out.append((f"f16_{src_m}_{res}", d, float_planes(rng, 32, 8, f16=True)))
        # every 16-bit code of Y'
        for res in (0, 1):
            d = desc(256, 256, src_matrix=src_m, resampler=res, full=1)
            out.append((f"every_code_{src_m}_{res}", d, every_code_planes(rng)))
    # sizes: the smallest box, FIR edge sizes (narrow widths, a few rows), odd tile counts
    for w, hh, res in ((8, 4, 0), (4, 4, 0), (2, 2, 1), (6, 4, 1), (10, 6, 1), (14, 12, 1), (8, 4, 1), (68, 36, 1), (72, 36, 0),
                       (130, 34, 1), (132, 36, 0)):
        for src_m in (MATRIX_YUVPRIME2, 0):
            d = desc(w, hh, src_depth=16, dst_depth=12, src_matrix=src_m, resampler=res)
            out.append((f"size_{w}x{hh}_{src_m}_{res}", d, u16_planes(rng, w, hh, 16)))
    # 4:4:4 (the matrix step alone) and 15 -> 15 with other primaries (not the identity)
    for src_m in (MATRIX_YUVPRIME2, 0):
        d = desc(24, 8, src_depth=12, dst_depth=10, src_matrix=src_m, chroma=ob.CHROMA_444)
        out.append((f"444_{src_m}", d, u16_planes(rng, 24, 8, 12)))
    d = desc(24, 8, src_depth=16, dst_depth=16, primaries=(9, 1), resampler=1)
    out.append(("15to15_primaries", d, u16_planes(rng, 24, 8, 16)))
    return out


# ---- what the GPU tests run besides grid(): descriptors and planes, deterministic ----------------------------------------
def batch_case(res):
    """40 frames (two sub-batches of the scratch ring: 32 + 8), 0 -> 15, 64 x 32"""
    rng = np.random.default_rng(40 + res)
    d = desc(64, 32, src_depth=16, dst_depth=12, src_matrix=0, resampler=res)
    return d, [u16_planes(rng, 64, 32, 16) for _ in range(40)]


def ring_case():
    """six frames through the pinned ring, 15 -> 15 FIR (the identity matrix step)"""
    rng = np.random.default_rng(66)
    d = desc(128, 64, src_depth=16, dst_depth=10, resampler=1)
    return d, [u16_planes(rng, 128, 64, 16) for _ in range(6)]


def uhd_case(res):
    """one 3840 x 2160 frame, 0 -> 15, 16 -> 12 bits"""
    rng = np.random.default_rng(2160 + res)
    d = desc(3840, 2160, src_depth=16, dst_depth=12, src_matrix=0, resampler=res)
    return d, [rng.integers(0, 65536, 3840 * 2160, dtype=np.uint16) for _ in range(3)]


def cli_yuv_case():
    """two frames of a 16-bit 4:4:4 .yuv holding Y', Z, X -> 4:2:0 .yuv, FIR, video range (15 -> 15)"""
    rng = np.random.default_rng(4444)
    d = desc(96, 48, src_depth=16, dst_depth=10, resampler=1, primaries=(1, 1), transfer=(1, 1))
    return d, [u16_planes(rng, 96, 48, 16) for _ in range(2)]


def cli_tiff_rgb():
    """the samples of a 16-bit .tiff (R, G, B per pixel), 64 x 32"""
    rng = np.random.default_rng(7777)
    return rng.integers(0, 65536, size=(32, 64, 3), dtype=np.uint16)


def cli_tiff_desc():
    """what the command line makes of the .tiff line in test_yuvp2.py: read_tiff forces GBR, so 0 -> 15; box, full range"""
    return desc(64, 32, src_depth=16, dst_depth=16, src_matrix=0, resampler=0, full=1, primaries=(1, 1), transfer=(1, 1))
