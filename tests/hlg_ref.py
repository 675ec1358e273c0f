"""HLG (include/hdr2yuv_hip.h, the HLG section), restated in numpy: the two tables in binary64 on the nodes of the light distribution's
bins, each entry rounded once to binary32; the per-pixel arithmetic in binary32 with every product, difference and sum rounded on its
own; and the BT.2100 formulas themselves in binary64 (the inverse OOTF, the OETF and their inverses), which the accuracy condition
is measured against."""
import numpy as np

BINS = 8706
FIRST_BITS = 0x37000000  # 2^-17: the lower edge of bin 1
LAST = BINS - 1
LOW = np.float32(256.0)  # what a luminance below the first node is multiplied by before the gain table is read
OETF_FIRST = 13 * 512 + 1  # the node of 2^-4, thirteen binades above 2^-17: the lowest entry of `oetf` that is ever read

A = 0.17883277
B = 1.0 - 4.0 * A
C = 0.5 - A * np.log(4.0 * A)
TWELFTH = np.float32(1.0 / 12.0)  # the binary32 nearest to 1/12: the OETF's branch point
KR, KG, KB = np.float32(0.2627), np.float32(0.6780), np.float32(0.0593)


def gamma_of(peak):
    return 1.2 + 0.42 * np.log10(peak / 1000.0)


def k_of(peak, relative):
    """what a sample is multiplied by before the pass works in units of the peak: 10000 / L_W rounded once, or 1"""
    return np.float32(1.0) if relative else np.float32(10000.0 / peak)


def nodes():
    """the float64 values of the 8705 nodes above entry 0: the floats of bits FIRST_BITS + ((j - 1) << 14), j = 1..8705"""
    bits = (FIRST_BITS + (np.arange(LAST, dtype=np.uint32) << np.uint32(14))).astype(np.uint32)
    return bits.view(np.float32).astype(np.float64)


def tables(peak, relative):
    """(gain, oetf, k, gamma): the two float32 tables of BINS entries, the float32 factor and the binary64 system gamma"""
    assert 400 <= peak <= 2000 and relative in (0, 1)
    g = gamma_of(peak)
    p = (1.0 - g) / g
    x = nodes()
    gain = np.empty(BINS, np.float64)
    gain[1:] = np.power(x, p)
    gain[0] = np.power(256.0, -p)  # the factor that goes with LOW: Y^p = (256 Y)^p 256^-p
    oetf = np.zeros(BINS, np.float64)
    up = x >= 2.0 ** -4
    oetf[1:][up] = A * np.log(12.0 * x[up] - B) + C
    return gain.astype(np.float32), oetf.astype(np.float32), k_of(peak, relative), g


def scale(dst_bit_depth, dst_full_range, dst_matrix):
    """(mulY, addY, mulC, addC) as the conversion derives them for a float source: the clip limits of the destination depth, the
    chroma pair only for a Y'CbCr destination in video range"""
    f32 = np.float32
    if dst_full_range:
        m = f32((1 << dst_bit_depth) - 1)
        return m, f32(0), m, f32(0)
    d = 1 << (dst_bit_depth - 8)
    lo, hi, hic = 16 * d, 219 * d + 16 * d, 224 * d + 16 * d
    if dst_matrix == 0:
        return f32(hi), f32(lo), f32(hi), f32(lo)
    return f32(hi), f32(lo), f32(hic), f32(lo)


def bin_of(e):
    e = np.asarray(e, np.uint32).astype(np.int64)
    return np.minimum(np.where(e < FIRST_BITS, 0, ((e - FIRST_BITS) >> 14) + 1), LAST)


def _interp(table, x):
    """the table read at x's bits as tone mapping's steps 2-3 read theirs: entry 0 below the first node, entry 8705 at 1.0 and
    above, otherwise lo + (hi - lo) t, each operation rounded to binary32"""
    f32 = np.float32
    e = x.view(np.uint32)
    k = bin_of(e)
    lo, hi = table[k], table[np.minimum(k + 1, LAST)]
    t = (e & np.uint32(0x3FFF)).astype(f32) * f32(2.0 ** -14)  # exact
    diff = (hi - lo).astype(f32)
    prod = (diff * t).astype(f32)
    return np.where((k == 0) | (k == LAST), lo, (lo + prod).astype(f32)).astype(f32)


def gain_of(gain, y):
    """step 3: the gain at the luminance y (float32).  From the first node up the table is read at y; below it at 256 y (exact), and
    the result is multiplied by entry 0, the factor 256^-p; below 2^-25 the gain is held at entry 1 times entry 0"""
    f32 = np.float32
    low = y.view(np.uint32) < np.uint32(FIRST_BITS)
    y2 = np.where(low, (y * LOW).astype(f32), y).astype(f32)
    held = y2.view(np.uint32) < np.uint32(FIRST_BITS)
    g = np.where(held, gain[1], _interp(gain, np.where(held, f32(2.0 ** -17), y2).astype(f32))).astype(f32)
    return np.where(low, (g * gain[0]).astype(f32), g).astype(f32)


def scene(planes, gain, k):
    """steps 1-4: planes [G, B, R] (float32 or float16) of display light -> ([E_G, E_B, E_R], Y) as float32: the scene light a
    signal can carry, and the luminance the gain was read at"""
    f32 = np.float32
    gain, k = np.asarray(gain, f32), f32(k)
    assert planes[0].dtype in (np.float32, np.float16) and gain.shape == (BINS,)
    with np.errstate(all="ignore"):
        c = [np.asarray(p).astype(f32) for p in planes]
        c = [np.where(x > 0, np.minimum(x, f32(1.0)), f32(0.0)).astype(f32) for x in c]  # NaN, -0.0, negatives: +0.0; inf: 1
        s = [np.minimum((x * k).astype(f32), f32(1.0)) for x in c]
        y = ((KR * s[2]).astype(f32) + (KG * s[0]).astype(f32)).astype(f32)
        y = (y + (KB * s[1]).astype(f32)).astype(f32)
        g = gain_of(gain, y)
        return [np.minimum((x * g).astype(f32), f32(1.0)) for x in s], y


def signal(planes, gain, oetf, k):
    """steps 1-5: planes [G, B, R] (float32 or float16) of display light -> [E'_G, E'_B, E'_R] as float32, each in [+0, 1]"""
    f32 = np.float32
    oetf = np.asarray(oetf, f32)
    assert oetf.shape == (BINS,)
    with np.errstate(all="ignore"):
        out = []
        for e in scene(planes, gain, k)[0]:
            low = np.sqrt((f32(3.0) * e).astype(f32)).astype(f32)  # correctly rounded
            ep = np.where(e <= TWELFTH, low, _interp(oetf, e)).astype(f32)
            out.append(np.minimum(ep, f32(1.0)))
        assert all(o.dtype == f32 for o in out)
        return out


def apply(planes, gain, oetf, k, sc):
    """the whole pixel: signal(), then step 6 with sc = (mulY, addY, mulC, addC): product, then sum; float32 planes G, B, R"""
    f32 = np.float32
    my, ay, mc, ac = (f32(v) for v in sc)
    e = signal(planes, gain, oetf, k)
    return [((e[0] * my).astype(f32) + ay).astype(f32), ((e[1] * mc).astype(f32) + ac).astype(f32),
            ((e[2] * mc).astype(f32) + ac).astype(f32)]


SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 2.0 ** -17, float(np.nextafter(np.float32(2.0 ** -17), np.float32(0))), 1.0,
            float(np.nextafter(np.float32(1), np.float32(0))), float(np.nextafter(np.float32(1), np.float32(2))), 4.0, np.inf, -np.inf, np.nan, 65504.0, -1.0]


def specials_row():
    """every special value as G, as B, as R and as all three, and three tail pixels: a row of 67"""
    sp = np.array(SPECIALS, np.float32)
    n = len(sp)
    planes = [np.full(4 * n + 3, 0.004, np.float32) for _ in range(3)]
    for c in range(3):
        planes[c][c * n:(c + 1) * n] = sp
        planes[c][3 * n:4 * n] = sp
        planes[c][4 * n:] = sp[[13, 11, 1]]  # NaN, inf, -0.0 in the tail pixels
    return planes, n


# ---- BT.2100 in binary64 --------------------------------------------------------------------------------------------------

def oetf_exact(e):
    e = np.asarray(e, np.float64)
    with np.errstate(all="ignore"):
        return np.where(e <= 1.0 / 12.0, np.sqrt(3.0 * e), A * np.log(np.maximum(12.0 * e - B, 1e-300)) + C)


def oetf_inverse_exact(ep):
    ep = np.asarray(ep, np.float64)
    return np.where(ep <= 0.5, ep * ep / 3.0, (np.exp((ep - C) / A) + B) / 12.0)


def signal_exact(gbr, peak):
    """display light [G, B, R] in units of the peak (binary64, each in [0, 1]) -> E' by BT.2100: the inverse OOTF with the system
    gamma of the peak and no black lift, the scene light clipped to what a signal can carry, then the OETF"""
    g = gamma_of(peak)
    gbr = [np.asarray(x, np.float64) for x in gbr]
    y = 0.2627 * gbr[2] + 0.6780 * gbr[0] + 0.0593 * gbr[1]
    with np.errstate(all="ignore"):
        gain = np.where(y > 0, np.power(y, (1.0 - g) / g), 0.0)
    return [oetf_exact(np.minimum(x * gain, 1.0)) for x in gbr]


def display_exact(ep_gbr, peak):
    """the inverse: E' [G, B, R] -> display light in units of the peak (the OETF's inverse, then the OOTF)"""
    g = gamma_of(peak)
    e = [oetf_inverse_exact(x) for x in ep_gbr]
    ys = 0.2627 * e[2] + 0.6780 * e[0] + 0.0593 * e[1]
    with np.errstate(all="ignore"):
        gain = np.where(ys > 0, np.power(ys, g - 1.0), 0.0)
    return [x * gain for x in e]
