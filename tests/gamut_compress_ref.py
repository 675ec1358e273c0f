"""Gamut compression (include/hdr2yuv_hip.h, "gamut compression"), restated in numpy: the limits, the curve and its tables in
binary64, the per-pixel arithmetic in binary32 with every operation rounded on its own, and the test picture that the host and the
device tests share.  The header is normative; this follows it step by step and has none of the kernel's shortcuts."""
import math

import numpy as np

NODES = 1025
F32 = np.float32
FMAX = np.finfo(np.float32).max
CORNERS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0))
IDENTITY, CURVE, BEYOND, CLIP, DARK = range(5)  # the branch a channel of a pixel takes


def limits(m):
    """the binary32 limits R, G, B of the matrix m (float32 (3, 3)), from the six corners of the source cube, in binary64"""
    m = np.asarray(m, np.float32).reshape(3, 3).astype(np.float64)
    lim = [0.0, 0.0, 0.0]
    for x in CORNERS:
        o = [(m[i][0] * x[0] + m[i][1] * x[1]) + m[i][2] * x[2] for i in range(3)]
        a = max(o)
        lim = [max(lim[i], (a - o[i]) / a) for i in range(3)]
    return np.array(lim, np.float64).astype(np.float32)


def curve_s(l, t, p):
    w = l - t
    return w / math.pow(math.pow((1.0 - t) / w, -p) - 1.0, 1.0 / p)


def curve_at(u, l, t, p):
    """C at the distance t + u, in binary64 (python floats)"""
    s = curve_s(l, t, p)
    return t + u / math.pow(1.0 + math.pow(u / s, p), 1.0 / p)


def curve(m, threshold, power):
    """dict of limit, scale (float32 (3,)) and table (float32 (3, NODES)) for a matrix and the two binary32 parameters"""
    t32, p32 = F32(threshold), F32(power)
    t, p = float(t32), float(p32)
    lim = limits(m)
    scale = np.zeros(3, F32)
    table = np.zeros((3, NODES), F32)
    for i in range(3):
        if not lim[i] > F32(1):
            continue
        l = float(lim[i])
        w = l - t
        scale[i] = F32(1024.0 / w)
        for k in range(1, NODES - 1):
            table[i][k] = F32(curve_at((w * k) / 1024.0, l, t, p))
        table[i][0] = t32
        table[i][NODES - 1] = F32(1)
    return {"matrix": np.asarray(m, F32).reshape(3, 3), "threshold": t32, "limit": lim, "scale": scale, "table": table}


def sums(planes, m):
    """the matrix step alone: float32 R', G', B' of planes [G, B, R], as k_gamut's pixel computes them, unclipped"""
    m = np.asarray(m, np.float32).reshape(3, 3)
    v = [np.asarray(planes[c]).astype(np.float32) for c in (2, 0, 1)]
    with np.errstate(all="ignore"):
        return [((m[i][0] * v[0]) + (m[i][1] * v[1])) + (m[i][2] * v[2]) for i in range(3)]


def compress(planes, cv, branches=None):
    """planes [G, B, R] (float32 or float16) -> the compressed [G, B, R] of the same dtype and shape; cv: curve()'s dict.
    branches: a list that receives three uint8 arrays (R, G, B) of the branch every sample took"""
    dt = planes[0].dtype
    assert dt in (np.float32, np.float16)
    t = F32(cv["threshold"])
    with np.errstate(all="ignore"):
        o = sums(planes, cv["matrix"])
        o = [np.where(np.isnan(x), F32(0), np.where(x > FMAX, FMAX, x)).astype(F32) for x in o]
        a = np.maximum(np.maximum(o[0], o[1]), o[2])
        dark = ~(a > 0)
        out = []
        for i in range(3):
            s = o[i]
            d = (a - s) / a
            assert d.dtype == np.float32
            l, k, T = F32(cv["limit"][i]), F32(cv["scale"][i]), cv["table"][i]
            ident = d <= t
            if l > F32(1):
                beyond = ~ident & (d >= l)
                x = (d - t) * k
                xs = np.where(ident | beyond | dark | ~np.isfinite(x), F32(0), x)
                n = np.minimum(xs.astype(np.int32), NODES - 2)
                f = xs - n.astype(F32)
                cd = T[n] + (T[n + 1] - T[n]) * f
                v = a - cd * a
                assert v.dtype == np.float32
                v = np.where(v > 0, v, F32(0))
                r = np.where(ident, s, np.where(beyond, F32(0), v))
                br = np.where(ident, IDENTITY, np.where(beyond, BEYOND, CURVE))
            else:
                r = np.where(ident, s, np.where(s > 0, s, F32(0)))
                br = np.where(ident, IDENTITY, CLIP)
            r = np.where(dark, F32(0), r).astype(F32)
            out.append(r.astype(dt))
            if branches is not None:
                branches.append(np.where(dark, DARK, br).astype(np.uint8))
    return [out[1], out[2], out[0]]


def _solve(m, targets):
    """source pixels (n, 3) R, G, B whose converted pixels are about `targets` (n, 3), in binary64"""
    return np.linalg.solve(np.asarray(m, np.float64).reshape(3, 3), np.asarray(targets, np.float64).T).T


def picture(m, cv, npix, dtype=np.float32, seed=20250613):
    """The seeded test picture for a matrix: planes [G, B, R] of npix samples (npix >= 3000).  Uniform random source pixels; the six
    corners at scales 2^-20 .. 1; greys; pixels with negative and above-1 channels; +-0, subnormals, NaN and +-inf; pixels built so
    that a channel's d lands on the threshold, on the limit, on table nodes and past the limit; pixels that are not above 0."""
    rng = np.random.default_rng(seed)
    t = float(cv["threshold"])
    px = [rng.random((1200, 3))]
    px.append(np.array([[c * 2.0 ** -e for c in x] for x in CORNERS for e in range(21)]))
    g = rng.random(64)
    px.append(np.stack([g, g, g], 1))
    px.append(rng.random((300, 3)) * 3.0 - 1.0)
    sp = [0.0, -0.0, 1e-40, -1e-40, 1e-45, np.nan, np.inf, -np.inf, 1.0, 65504.0, 3e38, -3e38, 0.25]
    px.append(np.array([[sp[i % 13], sp[(i // 13) % 13], sp[(i // 169) % 13]] for i in rng.permutation(13 ** 3)[:260]]))
    built = []
    for i in range(3):  # channel i at a chosen distance d from the pixel's largest channel
        l = float(cv["limit"][i])
        if l > 1.0:
            ds = np.concatenate([[t, l] * 12, [np.nextafter(F32(t), F32(2)), np.nextafter(F32(t), F32(0)), np.nextafter(F32(l), F32(0))],
                                 t + (l - t) * rng.integers(0, 1025, 40) / 1024.0, t + (l - t) * rng.random(60),
                                 l + rng.random(50) * 0.5, t * rng.random(20)])
        else:
            ds = np.concatenate([[t, np.nextafter(F32(t), F32(2)), np.nextafter(F32(t), F32(0)), 1.0], t + (1.0 - t) * rng.random(60),
                                 1.0 + rng.random(60), t * rng.random(40)])
        for d in ds:
            a = 2.0 ** rng.integers(-12, 2) * (1.0 + rng.random())
            tgt = a * (0.2 + 0.8 * rng.random(3))
            tgt[(i + 1) % 3] = a
            tgt[i] = a * (1.0 - float(d))
            built.append(tgt)
    px.append(_solve(m, built))
    neg = -rng.random((40, 3)) * 2.0 ** rng.integers(-10, 1, (40, 1))  # every converted channel below 0
    px.append(_solve(m, neg))
    px = np.concatenate(px)
    assert len(px) <= npix, (len(px), npix)
    px = np.concatenate([px, rng.random((npix - len(px), 3)) * 1.2 - 0.1])
    px = px[rng.permutation(npix)]
    with np.errstate(all="ignore"):
        return [np.ascontiguousarray(px[:, c].astype(np.float32).astype(dtype)) for c in (1, 2, 0)]
