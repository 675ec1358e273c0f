"""The light of SDR code planes (include/hdr2yuv_hip.h, "light of SDR code planes"), restated in numpy: codelight_ref's planes444 and
primes (steps 1-3), the clamp (4s), light_ref's to_linear for a BT.1886 source -- float64 np.power with (double)2.4f, rounded once to
binary32 (5s) -- and the binary32 product with kappa (6s).  A plain module: numpy, plus the oracle the caller hands in for 4:2:0
frames."""
import numpy as np

import codelight_ref as clr
import light_ref as lr

F32 = np.float32
WHITE_MIN, WHITE_MAX, WHITE_DEFAULT = 80, 1000, 203
BT709_TF = 1  # a transfer code of the BT.1886 class


def kappa_of(white):
    """W / 10000 in binary64, rounded once to binary32"""
    return F32(white / 10000.0)


def clean(v):
    """step 4s: what is not above 0 (NaN, -0.0, negatives) becomes +0.0, what is above 1 becomes 1"""
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        return np.where(v > 0, np.minimum(v, F32(1.0)), F32(0.0)).astype(F32)


def apply(primes, white):
    """steps 4s-6s: [G', B', R'] (float32, clamped or not) -> [L_G, L_B, L_R] as float32, 1.0 = 10000 cd/m2"""
    assert WHITE_MIN <= white <= WHITE_MAX
    kappa = kappa_of(white)
    return [(lr.to_linear(clean(v), BT709_TF) * kappa).astype(F32) for v in primes]


def planes(oracle, frame_planes, width, height, chroma, depth, full_range, matrix, white=WHITE_DEFAULT, form=clr.FIR):
    """[G, B, R]: flat binary32 planes of width x height in [+0, kappa] of one frame's three SDR code planes"""
    p444 = clr.planes444(oracle, frame_planes, width, height, chroma, depth, form)
    return [np.ascontiguousarray(x, F32) for x in apply(list(clr.primes(p444, depth, full_range, matrix)), white)]
