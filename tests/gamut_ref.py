"""The conversion between colour primaries (include/hdr2yuv_hip.h, the gamut section), restated in numpy: the matrix in exact
rationals, rounded once per entry, and the per-pixel arithmetic in binary32 with every product and sum rounded on its own."""
from fractions import Fraction as Fr

import numpy as np

# CIE 1931 x, y of R, G, B; every RGB set has the D65 white
PRIMARIES = {
    1: ((".640", ".330"), (".300", ".600"), (".150", ".060")),   # BT.709
    9: ((".708", ".292"), (".170", ".797"), (".131", ".046")),   # BT.2020
    12: ((".680", ".320"), (".265", ".690"), (".150", ".060")),  # P3-D65
}
PRIMARIES[8] = PRIMARIES[9]
WHITE = (".3127", ".3290")
XYZ = 10


def _mul(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _inv(a):
    cof = [[a[(i + 1) % 3][(j + 1) % 3] * a[(i + 2) % 3][(j + 2) % 3] - a[(i + 1) % 3][(j + 2) % 3] * a[(i + 2) % 3][(j + 1) % 3]
            for j in range(3)] for i in range(3)]
    det = sum(a[0][j] * cof[0][j] for j in range(3))
    return [[cof[j][i] / det for j in range(3)] for i in range(3)]


def npm(code):
    """the normalised primary matrix of SMPTE RP 177, in Fractions: columns = XYZ of R, G, B, scaled so that (1, 1, 1) gives the
    white with Y = 1; the identity for XYZ"""
    if code == XYZ:
        return [[Fr(int(i == j)) for j in range(3)] for i in range(3)]
    xy = [(Fr(x), Fr(y)) for x, y in PRIMARIES[code]]
    p = [[x / y for x, y in xy], [Fr(1)] * 3, [(1 - x - y) / y for x, y in xy]]
    xw, yw = Fr(WHITE[0]), Fr(WHITE[1])
    w = [xw / yw, Fr(1), (1 - xw - yw) / yw]
    pi = _inv(p)
    s = [sum(pi[i][k] * w[k] for k in range(3)) for i in range(3)]
    return [[p[i][j] * s[j] for j in range(3)] for i in range(3)]


def round_f32(q):
    """a Fraction rounded to nearest binary32, ties to even (normal results only); an exact 0 is +0.0"""
    if q == 0:
        return np.float32(0.0)
    a, e = abs(q), 0
    while a >= 2:
        a, e = a / 2, e + 1
    while a < 1:
        a, e = a * 2, e - 1
    assert -126 <= e <= 127
    scaled = a * (1 << 23)  # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fr(1, 2) or (rem == Fr(1, 2) and n & 1):
        n += 1
    v = np.float32(np.ldexp(np.float64(n), e - 23))  # n <= 2^24: exact
    return -v if q < 0 else v


def matrix_exact(s, d):
    return _mul(_inv(npm(d)), npm(s))


def matrix(s, d):
    """NPM(d)^-1 NPM(s): float32 (3, 3), row-major, on (R, G, B) columns"""
    return np.array([[round_f32(x) for x in row] for row in matrix_exact(s, d)], dtype=np.float32)


def convert(planes, m, clip):
    """planes [G, B, R] (float32, or float16) -> the converted [G, B, R] of the same dtype and shape"""
    m = np.asarray(m, np.float32).reshape(3, 3)
    dt = planes[0].dtype
    assert dt in (np.float32, np.float16)
    v = [np.asarray(planes[c]).astype(np.float32) for c in (2, 0, 1)]  # R, G, B
    out = []
    with np.errstate(all="ignore"):
        for i in range(3):
            o = ((m[i][0] * v[0]) + (m[i][1] * v[1])) + (m[i][2] * v[2])
            assert o.dtype == np.float32
            if clip:
                o = np.where(o > 0, o, np.float32(0.0))
            out.append(o.astype(dt))
    return [out[1], out[2], out[0]]
