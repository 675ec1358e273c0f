"""Tone mapping (include/hdr2yuv_hip.h, the tone mapping section), restated in numpy: the BT.2390 curve in binary64 on the nodes of
the light distribution's bins, each gain rounded once to binary32, and the per-pixel arithmetic in binary32 with every product,
difference and sum rounded on its own."""
import numpy as np

BINS = 8706
FIRST_BITS = 0x37000000  # 2^-17: the lower edge of bin 1
LAST = BINS - 1

M1, M2 = 2610 / 16384, 2523 / 4096 * 128
C1, C2, C3 = 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32


def pq_n(l):
    """the ST 2084 inverse EOTF, binary64"""
    p = np.power(np.asarray(l, np.float64), M1)
    return np.power((C1 + C2 * p) / (1.0 + C3 * p), M2)


def pq_n_inv(v):
    p = np.power(np.asarray(v, np.float64), 1.0 / M2)
    return np.power(np.maximum(p - C1, 0.0) / (C2 - C3 * p), 1.0 / M1)


def params(s, d):
    """W, maxLum, KS of a pair of peaks in cd/m2"""
    w = float(pq_n(s / 10000.0))
    max_lum = float(pq_n(d / 10000.0)) / w
    return w, max_lum, 1.5 * max_lum - 0.5


def knee(s, d):
    """where the curve leaves the identity, in cd/m2"""
    w, _, ks = params(s, d)
    return 10000.0 * float(pq_n_inv(ks * w))


def nodes():
    """the float64 values of the 8705 nodes above entry 0: the floats of bits FIRST_BITS + ((k - 1) << 14), k = 1..8705"""
    bits = (FIRST_BITS + (np.arange(LAST, dtype=np.uint32) << np.uint32(14))).astype(np.uint32)
    return bits.view(np.float32).astype(np.float64)


def tone(e, s, d):
    """T(e) in binary64 and whether e lies below the knee"""
    w, max_lum, ks = params(s, d)
    e1 = np.minimum(pq_n(e) / w, 1.0)
    t = (e1 - ks) / (1.0 - ks)
    t2, t3 = t * t, t * t * t
    e2 = (2.0 * t3 - 3.0 * t2 + 1.0) * ks + (t3 - 2.0 * t2 + t) * (1.0 - ks) + (-2.0 * t3 + 3.0 * t2) * max_lum
    below = e1 < ks
    return np.where(below, e, pq_n_inv(np.where(below, e1, e2) * w)), below


def gain_exact(e, s, d, relative):
    """g(e) in binary64"""
    e = np.asarray(e, np.float64)
    u, inv_u = (d / 10000.0, 10000.0 / d) if relative else (1.0, 1.0)
    t, below = tone(e, s, d)
    with np.errstate(all="ignore"):
        return np.where(below, inv_u, t / (e * u))


def curve(s, d, relative):
    """(the BINS float32 gains, the float32 cap)"""
    assert 100 <= d < s <= 10000 and relative in (0, 1)
    g = np.empty(BINS, np.float64)
    g[0] = 10000.0 / d if relative else 1.0
    g[1:] = gain_exact(nodes(), s, d, relative)
    return g.astype(np.float32), np.float32(1.0) if relative else np.float32(d / 10000.0)


def bin_of(e):
    e = np.asarray(e, np.uint32).astype(np.int64)
    return np.minimum(np.where(e < FIRST_BITS, 0, ((e - FIRST_BITS) >> 14) + 1), LAST)


def apply(planes, gains, cap, half=None):
    """planes [G, B, R] (float32, or float16) -> the mapped [G, B, R] of the same dtype and shape; half: assert the dtype is (not)
    float16"""
    f32 = np.float32
    gains, cap = np.asarray(gains, f32), f32(cap)
    dt = planes[0].dtype
    assert dt in (np.float32, np.float16) and gains.shape == (BINS,)
    assert half is None or bool(half) == (dt == np.float16)
    with np.errstate(all="ignore"):
        c = [np.asarray(p).astype(f32) for p in planes]
        c = [np.where(x > 0, np.minimum(x, f32(1.0)), f32(0.0)).astype(f32) for x in c]  # NaN, -0.0, negatives: +0.0; inf: 1
        m = np.maximum(np.maximum(c[0], c[1]), c[2])
        e = m.view(np.uint32)
        k = bin_of(e)
        lo, hi = gains[k], gains[np.minimum(k + 1, LAST)]
        t = (e & np.uint32(0x3FFF)).astype(f32) * f32(2.0 ** -14)  # exact
        diff = (hi - lo).astype(f32)
        prod = (diff * t).astype(f32)
        interp = (lo + prod).astype(f32)
        gain = np.where((k == 0) | (k == LAST), lo, interp).astype(f32)
        out = [np.minimum((x * gain).astype(f32), cap) for x in c]
        assert all(o.dtype == f32 for o in out)
        return [o.astype(dt) for o in out]
