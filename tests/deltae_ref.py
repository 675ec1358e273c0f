"""A numpy restatement of the Delta E ITP of PQ code planes of include/hdr2yuv_hip.h ("Delta E ITP of PQ code planes"), for the tests:
codelight_ref.py's planes444 and lights for steps 1-4 of the light of PQ code planes, then BT.2100 LMS, PQ10000_r (the oracle's
vector export from_linear(v, 16), one C call a plane: a picture may be as large as a sweep needs), I, T, P and d, in float32 arrays
with one operation per statement, and the per-frame figures of h2y_deltae_stats.  A plain module: numpy, plus the oracle the caller
hands in."""
from fractions import Fraction

import numpy as np

import codelight_ref as clr

F32 = np.float32

# numerators over (R, G, B) and the denominators: every quotient is exact in binary32
LMS_NUM = ((1688, 2146, 262), (683, 2951, 462), (99, 309, 3688))
LMS_DEN = 4096
T_NUM, T_DEN = (6610, 13613, 7003), 8192      # T = (t0 l' - t1 m') + t2 s'  (= Ct / 2)
P_NUM, P_DEN = (17933, 17390, 543), 4096      # P = (p0 l' - p1 m') - p2 s'  (= Cp)
HALF = F32(0.5)
SCALE = F32(720.0)
SUM_SHIFT = 20                                # sum_q adds rint(d x 2^20)


def const(num, den) -> np.float32:
    c = F32(num / den)
    assert Fraction(float(c)) == Fraction(num, den), (num, den)
    return c


LMS = tuple(tuple(const(k, LMS_DEN) for k in row) for row in LMS_NUM)
TC = tuple(const(k, T_DEN) for k in T_NUM)
PC = tuple(const(k, P_DEN) for k in P_NUM)


def pq_r(oracle, x):
    """PQ10000_r of a float32 array through the oracle's vector statement (h2y_oracle_from_linear: a plain loop over the scalar one)"""
    return oracle.from_linear(np.ascontiguousarray(x, F32), clr.PQ)


def lms(lights):
    """[l, m, s] of [L_G, L_B, L_R], before PQ10000_r"""
    g, b, r = lights
    out = []
    for kr, kg, kb in LMS:
        t0 = (kr * r).astype(F32)
        t1 = (kg * g).astype(F32)
        t2 = (kb * b).astype(F32)
        v = (t0 + t1).astype(F32)
        v = (v + t2).astype(F32)
        out.append(clr.clamp01(v))
    return out


def itp_of_lms(oracle, lms3):
    lp, mp, sp = (pq_r(oracle, v) for v in lms3)
    i0 = (HALF * lp).astype(F32)
    i1 = (HALF * mp).astype(F32)
    i = (i0 + i1).astype(F32)
    t0 = (TC[0] * lp).astype(F32)
    t1 = (TC[1] * mp).astype(F32)
    t2 = (TC[2] * sp).astype(F32)
    t = (t0 - t1).astype(F32)
    t = (t + t2).astype(F32)
    p0 = (PC[0] * lp).astype(F32)
    p1 = (PC[1] * mp).astype(F32)
    p2 = (PC[2] * sp).astype(F32)
    p = (p0 - p1).astype(F32)
    p = (p - p2).astype(F32)
    return i, t, p


def itp(oracle, planes444, depth, full_range, matrix):
    """(I, T, P) of three 4:4:4 code planes (flat binary32)"""
    return itp_of_lms(oracle, lms(clr.lights(oracle, planes444, depth, full_range, matrix)))


def radicand(a, b):
    """q = (dI dI + dT dT) + dP dP of two (I, T, P) triples: what the square root is taken of"""
    di = (a[0] - b[0]).astype(F32)
    dt = (a[1] - b[1]).astype(F32)
    dp = (a[2] - b[2]).astype(F32)
    ii = (di * di).astype(F32)
    tt = (dt * dt).astype(F32)
    pp = (dp * dp).astype(F32)
    q = (ii + tt).astype(F32)
    return (q + pp).astype(F32)


def d_of_radicand(q):
    root = np.sqrt(q).astype(F32)
    return (SCALE * root).astype(F32)


def distance(a, b):
    """d of two (I, T, P) triples"""
    return d_of_radicand(radicand(a, b))


def pixel_d(oracle, planes_a, planes_b, width, height, chroma, depth, full_range, matrix, form=clr.FIR):
    """d at every pixel of two frames (lists of three planes), flat binary32 in raster order"""
    a = itp(oracle, clr.planes444(oracle, planes_a, width, height, chroma, depth, form), depth, full_range, matrix)
    b = itp(oracle, clr.planes444(oracle, planes_b, width, height, chroma, depth, form), depth, full_range, matrix)
    return distance(a, b)


def stats_of_d(d, width, threshold=1.0):
    """h2y_deltae_stats' figures of one frame's d, as a dict"""
    d = np.asarray(d, F32).reshape(-1)
    bits = d.view(np.uint32)
    first = int(np.argmax(bits))  # d >= +0 orders as its bits; argmax returns the first
    sum_q = int(np.rint(d.astype(np.float64) * float(1 << SUM_SHIFT)).astype(np.uint64).sum(dtype=np.uint64))
    thr = F32(threshold)
    return dict(max_bits=int(bits[first]), max_x=first % width, max_y=first // width, threshold=float(thr), sum_q=sum_q, pixels=int(d.size),
                over=int(np.count_nonzero(d > thr)), mean=(float(sum_q) * 2.0 ** -SUM_SHIFT) / float(d.size), max=float(d[first]))


def stats(oracle, planes_a, planes_b, width, height, chroma, depth, full_range, matrix, form=clr.FIR, threshold=1.0):
    return stats_of_d(pixel_d(oracle, planes_a, planes_b, width, height, chroma, depth, full_range, matrix, form), width, threshold)


KEYS = ("max_bits", "max_x", "max_y", "threshold", "sum_q", "pixels", "over", "mean", "max")
