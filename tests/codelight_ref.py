"""A numpy restatement of the light of PQ code planes of include/hdr2yuv_hip.h ("light of PQ code planes"), for the tests: the
4:2:0 chroma upsampled by the .yuv -> RGB flow's upsampler (oracle.up444 for replication and the reference's FIR pair,
inverse_siting_ref.py for the top-left form), the normalisation (binary32: one subtraction, one IEEE division), the matrix (every
product and sum rounded by itself), the clamp, PQ10000_f (the oracle's to_linear(v, 16)), and from there light_ref.py's and
lightdist_ref.py's per-frame figures.  A plain module: numpy, plus the oracle the caller hands in."""
from fractions import Fraction

import numpy as np

import inverse_siting_ref as isr
import light_ref as lr
import lightdist_ref as ldr

F32 = np.float32
PQ = 16
GBR, BT709, BT2020NC = 0, 1, 9
REPLICATE, FIR, FIR_TL = "replicate", "fir", "fir_tl"  # the upsampling forms: algorithm 0; algorithm 1 under siting 0; under siting 2


def f32_of(decimal: str) -> np.float32:
    """the decimal value rounded once to binary32 (not through binary64)"""
    x = Fraction(decimal)
    c = F32(float(x))  # a candidate; its neighbours decide
    best = min((np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))), key=lambda v: abs(Fraction(float(v)) - x))
    return F32(best)


# rv, bu, gu, gv:  R' = y + rv cr;  B' = y + bu cb;  G' = (y - gu cb) - gv cr
COEF = {
    BT2020NC: tuple(f32_of(s) for s in ("1.4746", "1.8814", "0.16455313", "0.57135313")),
    BT709: tuple(f32_of(s) for s in ("1.5748", "1.8556", "0.18732427", "0.46812427")),
}


def upsample(oracle, c, width, height, depth, form):
    """one (height / 2, width / 2) chroma plane -> (height, width) codes, with the clip [0, 2^depth - 1]"""
    hi = (1 << depth) - 1
    c = np.asarray(c, np.uint16).reshape(height >> 1, width >> 1)
    if form == FIR_TL:
        return isr.upsample_top_left(c, 0, hi)
    return oracle.up444(c, width, height, 0 if form == REPLICATE else 1, 0, hi)


def normalise(code, depth, full_range, chroma):
    """a plane's codes -> binary32: (code - sub) / div"""
    s = 1 << (depth - 8)
    if full_range:
        sub, div = ((1 << (depth - 1)) if chroma else 0), (1 << depth) - 1
    else:
        sub, div = (128 * s, 224 * s) if chroma else (16 * s, 219 * s)
    return ((np.asarray(code).astype(F32) - F32(sub)) / F32(div)).astype(F32)


def primes(planes444, depth, full_range, matrix):
    """(G', B', R') of three 4:4:4 code planes (flat binary32), before the clamp"""
    p = [np.asarray(x).reshape(-1) for x in planes444]
    y = normalise(p[0], depth, full_range, False)
    if matrix == GBR:
        return y, normalise(p[1], depth, full_range, False), normalise(p[2], depth, full_range, False)
    rv, bu, gu, gv = COEF[matrix]
    cb, cr = normalise(p[1], depth, full_range, True), normalise(p[2], depth, full_range, True)
    r = (y + (rv * cr).astype(F32)).astype(F32)
    b = (y + (bu * cb).astype(F32)).astype(F32)
    g = ((y - (gu * cb).astype(F32)).astype(F32) - (gv * cr).astype(F32)).astype(F32)
    return g, b, r


def clamp01(v):
    return np.where(v > 0, np.minimum(v, F32(1.0)), F32(0.0)).astype(F32)


def lights(oracle, planes444, depth, full_range, matrix):
    """[L_G, L_B, L_R] of three 4:4:4 code planes (flat binary32)"""
    return [clamp01(oracle.to_linear(clamp01(v), PQ)) for v in primes(planes444, depth, full_range, matrix)]


def planes444(oracle, planes, width, height, chroma, depth, form=FIR):
    """the frame's three planes at every pixel: 4:4:4 as they are, 4:2:0 chroma upsampled"""
    y = np.asarray(planes[0], np.uint16).reshape(-1)
    if chroma == 3:
        return [y, np.asarray(planes[1], np.uint16).reshape(-1), np.asarray(planes[2], np.uint16).reshape(-1)]
    return [y] + [upsample(oracle, planes[c], width, height, depth, form).reshape(-1) for c in (1, 2)]


def stats(oracle, planes, width, height, chroma, depth, full_range, matrix, form=FIR):
    """(h2y_light_stats' figures, h2y_lightdist_stats' figures with the bins) of one frame, as dicts"""
    ls = lights(oracle, planes444(oracle, planes, width, height, chroma, depth, form), depth, full_range, matrix)
    dist = ldr.stats_of_planes(ls)
    m = np.maximum(np.maximum(ls[0], ls[1]), ls[2]).astype(F32)
    return lr.stats_of_m(m, width), dist


def split(frame, width, height, chroma):
    """a frame's contiguous codes -> its three planes"""
    n = width * height
    nc = (width >> 1) * (height >> 1) if chroma == 1 else n
    frame = np.asarray(frame).reshape(-1)
    return [frame[:n], frame[n:n + nc], frame[n + nc:n + 2 * nc]]


def upsampler_name(chroma, siting, resampler):
    """the CLI's name of the upsampling form (the light_only_from: banner line)"""
    if chroma == 3:
        return "none"
    return "replicate" if not resampler else ("fir_top_left" if siting == 2 else "fir")
