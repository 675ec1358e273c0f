"""The light of HLG code planes (include/hdr2yuv_hip.h, "light of HLG code planes"), restated in numpy: the two tables in binary64 on
hlg_ref's nodes, each entry rounded once to binary32; steps 4h-7h in binary32 with every product, sum and difference rounded on its
own, reading the tables with hlg_ref's _interp and gain_of; and in front of them codelight_ref's planes444, normalise and primes
(steps 1-3).  A plain module: numpy, plus the oracle the caller hands in for 4:2:0 frames."""
import numpy as np

import codelight_ref as clr
import hlg_ref as hr

F32 = np.float32
INV_FIRST = 16 * 512 + 1  # the node of 2^-1: the lowest entry of `inv` that is ever read
INV_NODES = hr.BINS - INV_FIRST  # 513
HOLD = 2.0 ** -25  # below this Y_s the OOTF's gain is held
THREE = F32(3.0)


def kappa_of(peak):
    """L_W / 10000 rounded once to binary32"""
    return F32(peak / 10000.0)


def tables(peak):
    """(ootf, inv, kappa, gamma): the two float32 tables of BINS entries, the float32 factor and the binary64 system gamma"""
    assert 400 <= peak <= 2000
    g = hr.gamma_of(peak)
    q = g - 1.0
    x = hr.nodes()
    ootf = np.empty(hr.BINS, np.float64)
    ootf[1:] = np.power(x, q)
    ootf[0] = np.power(256.0, -q)  # the factor that goes with the reads at 256 Y_s: Y^q = (256 Y)^q 256^-q
    inv = np.zeros(hr.BINS, np.float64)
    up = x >= 0.5
    inv[1:][up] = (np.exp((x[up] - hr.C) / hr.A) + hr.B) / 12.0
    return ootf.astype(F32), inv.astype(F32), kappa_of(peak), g


def clean(v):
    """step 4h: NaN, -0.0 and negatives become +0.0, what is above 1 becomes 1"""
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        return np.where(v > 0, np.minimum(v, F32(1.0)), F32(0.0)).astype(F32)


def scene(primes, inv):
    """steps 4h-5h: [G', B', R'] (float32) -> [E_G, E_B, E_R], the OETF's inverse"""
    inv = np.asarray(inv, F32)
    assert inv.shape == (hr.BINS,)
    out = []
    for v in primes:
        v = clean(v)
        low = ((v * v).astype(F32) / THREE).astype(F32)  # the product, then the IEEE division
        high = hr._interp(inv, np.maximum(v, F32(0.5)))  # (read only where v > 0.5)
        out.append(np.where(v <= F32(0.5), low, high).astype(F32))
    return out


def apply(primes, ootf, inv, kappa):
    """steps 4h-7h: [G', B', R'] (float32, clamped or not) -> ([L_G, L_B, L_R] as float32, 1.0 = 10000 cd/m2, and Y_s)"""
    ootf, kappa = np.asarray(ootf, F32), F32(kappa)
    e = scene(primes, inv)
    y = ((hr.KR * e[2]).astype(F32) + (hr.KG * e[0]).astype(F32)).astype(F32)
    y = (y + (hr.KB * e[1]).astype(F32)).astype(F32)
    g = hr.gain_of(ootf, y)
    return [((x * g).astype(F32) * kappa).astype(F32) for x in e], y


def planes(oracle, frame_planes, width, height, chroma, depth, full_range, matrix, peak, form=clr.FIR):
    """[G, B, R]: flat binary32 planes of width x height in [+0, kappa] of one frame's three HLG code planes"""
    p444 = clr.planes444(oracle, frame_planes, width, height, chroma, depth, form)
    ootf, inv, kappa, _ = tables(peak)
    out, _ = apply(list(clr.primes(p444, depth, full_range, matrix)), ootf, inv, kappa)
    return [np.ascontiguousarray(x, F32) for x in out]
