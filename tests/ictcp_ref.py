"""A numpy restatement of both ICtCp sections of include/hdr2yuv_hip.h, for the tests.  "ICtCp": display light -> code-valued I, Ct, Cp
planes (deltae_ref.py's lms and pq_r for steps 2-3, then the matrix and H.273's scale, one float32 operation per statement).  "light
of ICtCp code planes": codelight_ref.py's planes444 and normalise for steps 1-2, the inverse matrix, the clamp, PQ10000_f (the
oracle's to_linear(v, 16)), the inverse LMS matrix; from there light_ref.py's, lightdist_ref.py's and deltae_ref.py's figures.  And
BT.2100's formulas in binary64, to hold the restatement against.  A plain module: numpy, plus the oracle the caller hands in."""
from fractions import Fraction

import numpy as np

import codelight_ref as clr
import deltae_ref as der
import light_ref as lr
import lightdist_ref as ldr
import linearize_ref as lzr  # noqa: F401  (the planes this module's `planes` stands beside)

F32 = np.float32
ICTCP = 14
HALF = F32(0.5)

# the forward matrix over (l', m', s'), k / 4096: exact in binary32
I_NUM, CT_NUM, CP_NUM, DEN = (2048, 2048, 0), (6610, -13613, 7003), (17933, -17390, -543), 4096
CT = tuple(der.const(abs(k), DEN) for k in CT_NUM)  # Ct = (c0 l' - c1 m') + c2 s'
CP = tuple(der.const(abs(k), DEN) for k in CP_NUM)  # Cp = (p0 l' - p1 m') - p2 s'


def _inverse3(m):
    """the exact inverse of a 3 x 3 matrix of Fractions"""
    (a, b, c), (d, e, f), (g, h, i) = m
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f], [d * h - e * g, b * g - a * h, a * e - b * d]]
    return [[x / det for x in row] for row in adj]


def f32_of(x: Fraction) -> np.float32:
    """the rational rounded once to binary32"""
    c = F32(float(x))
    return F32(min((np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))), key=lambda v: abs(Fraction(float(v)) - x)))


FORWARD = [[Fraction(k, DEN) for k in row] for row in (I_NUM, CT_NUM, CP_NUM)]
INVERSE = _inverse3(FORWARD)                                            # rows L', M', S' over (I, Ct, Cp)
LMS_INVERSE = _inverse3([[Fraction(k, der.LMS_DEN) for k in row] for row in der.LMS_NUM])  # rows R, G, B over (l, m, s)
KA, KB, KC, KD = (f32_of(abs(x)) for x in (INVERSE[0][1], INVERSE[0][2], INVERSE[2][1], INVERSE[2][2]))
RGB_OF_LMS = [[f32_of(abs(x)) for x in row] for row in LMS_INVERSE]


def scale(depth, full_range):
    """(oY, aY, oC, aC, top): H.273's scale of a depth and range, as float32"""
    s, top = 1 << (depth - 8), (1 << depth) - 1
    if full_range:
        return F32(top), F32(0), F32(top), F32(1 << (depth - 1)), F32(top)
    return F32(219 * s), F32(16 * s), F32(224 * s), F32(128 * s), F32(top)


def clean(planes):
    """step 1: [G, B, R] of float32 or float16 -> float32 in [+0, 1]"""
    with np.errstate(invalid="ignore"):
        return [clr.clamp01(np.asarray(p).astype(F32)) for p in planes]


def ictcp_of_primes(lp, mp, sp):
    """step 4: (I, Ct, Cp) of l', m', s'"""
    i = ((HALF * lp).astype(F32) + (HALF * mp).astype(F32)).astype(F32)
    ct = ((CT[0] * lp).astype(F32) - (CT[1] * mp).astype(F32)).astype(F32)
    ct = (ct + (CT[2] * sp).astype(F32)).astype(F32)
    cp = ((CP[0] * lp).astype(F32) - (CP[1] * mp).astype(F32)).astype(F32)
    cp = (cp - (CP[2] * sp).astype(F32)).astype(F32)
    return i, ct, cp


def ictcp(oracle, planes):
    """steps 1-4: (I, Ct, Cp) of planes [G, B, R] of display light, unscaled float32"""
    lp, mp, sp = (der.pq_r(oracle, v) for v in der.lms(clean(planes)))
    return ictcp_of_primes(lp, mp, sp)


def to_codes(v, mul, add, top):
    v = ((v * mul).astype(F32) + add).astype(F32)
    v = (v + HALF).astype(F32)
    return np.minimum(np.maximum(v, F32(0)), top).astype(F32)


def apply(oracle, planes, depth, full_range):
    """the whole pixel: three float32 planes of code-valued I, Ct, Cp samples, the rounding half added"""
    oy, ay, oc, ac, top = scale(depth, full_range)
    i, ct, cp = ictcp(oracle, planes)
    return [to_codes(i, oy, ay, top), to_codes(ct, oc, ac, top), to_codes(cp, oc, ac, top)]


def codes(oracle, planes, depth, full_range):
    """the integer codes the conversion's cast makes of apply()'s planes (4:4:4, before any chroma clamp)"""
    return [np.trunc(p).astype(np.uint16) for p in apply(oracle, planes, depth, full_range)]


# ---- the way back ---------------------------------------------------------------------------------------------------------

def lms_primes(planes444, depth, full_range):
    """(L', M', S') of three 4:4:4 code planes (flat binary32), before the clamp"""
    p = [np.asarray(x).reshape(-1) for x in planes444]
    i = clr.normalise(p[0], depth, full_range, False)
    ct, cp = clr.normalise(p[1], depth, full_range, True), clr.normalise(p[2], depth, full_range, True)
    a, b, c, d = (KA * ct).astype(F32), (KB * cp).astype(F32), (KC * ct).astype(F32), (KD * cp).astype(F32)
    lp = ((i + a).astype(F32) + b).astype(F32)
    mp = ((i - a).astype(F32) - b).astype(F32)
    sp = ((i + c).astype(F32) - d).astype(F32)
    return lp, mp, sp


def lights_of_lms(l, m, s):
    """[L_G, L_B, L_R] of l, m, s"""
    (rl, rm, rs), (gl, gm, gs), (bl, bm, bs) = RGB_OF_LMS
    r = (((rl * l).astype(F32) - (rm * m).astype(F32)).astype(F32) + (rs * s).astype(F32)).astype(F32)
    g = (((gm * m).astype(F32) - (gl * l).astype(F32)).astype(F32) - (gs * s).astype(F32)).astype(F32)
    b = (((bs * s).astype(F32) - (bl * l).astype(F32)).astype(F32) - (bm * m).astype(F32)).astype(F32)
    return [clr.clamp01(g), clr.clamp01(b), clr.clamp01(r)]


def lights(oracle, planes444, depth, full_range):
    """[L_G, L_B, L_R] of three 4:4:4 ICtCp code planes (flat binary32)"""
    l, m, s = (clr.clamp01(oracle.to_linear(clr.clamp01(v), clr.PQ)) for v in lms_primes(planes444, depth, full_range))
    return lights_of_lms(l, m, s)


def planes(oracle, frame_planes, width, height, chroma, depth, full_range, form=clr.FIR):
    """linearize_ref.planes for matrix 14: [G, B, R], flat binary32 planes of display light of one frame's three code planes"""
    p444 = clr.planes444(oracle, frame_planes, width, height, chroma, depth, form)
    return [np.ascontiguousarray(x, F32) for x in lights(oracle, p444, depth, full_range)]


def stats(oracle, frame_planes, width, height, chroma, depth, full_range, form=clr.FIR):
    """codelight_ref.stats for matrix 14"""
    ls = planes(oracle, frame_planes, width, height, chroma, depth, full_range, form)
    m = np.maximum(np.maximum(ls[0], ls[1]), ls[2]).astype(F32)
    return lr.stats_of_m(m, width), ldr.stats_of_planes(ls)


def pixel_d(oracle, planes_a, planes_b, width, height, chroma, depth, full_range, form=clr.FIR):
    """deltae_ref.pixel_d for matrix 14"""
    sides = [der.itp_of_lms(oracle, der.lms(planes(oracle, p, width, height, chroma, depth, full_range, form))) for p in (planes_a, planes_b)]
    return der.distance(*sides)


# ---- BT.2100 in binary64 --------------------------------------------------------------------------------------------------

M1, M2, C1, C2, C3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32


def pq_exact(y):
    """the PQ inverse EOTF of y = light / 10000 cd/m2"""
    ym = np.power(np.asarray(y, np.float64), M1)
    return np.power((C1 + C2 * ym) / (1.0 + C3 * ym), M2)


def pq_eotf_exact(e):
    ep = np.power(np.clip(np.asarray(e, np.float64), 0.0, None), 1.0 / M2)
    return np.power(np.maximum(ep - C1, 0.0) / (C2 - C3 * ep), 1.0 / M1)


def ictcp_exact(gbr):
    """(I, Ct, Cp) of display light [G, B, R] (binary64, each in [0, 1]) by BT.2100"""
    g, b, r = (np.asarray(x, np.float64) for x in gbr)
    lms = [pq_exact((kr * r + kg * g + kb * b) / der.LMS_DEN) for kr, kg, kb in der.LMS_NUM]
    return tuple(sum(k * v for k, v in zip(row, lms)) / DEN for row in (I_NUM, CT_NUM, CP_NUM))
