"""The Lanczos resampler of include/hdr2yuv_hip.h ("scaling"), restated in numpy from the header's text: the tap table of one
axis in binary64, and the frame in integers.  Nothing here calls the library."""
import math

import numpy as np

TAPS = 32
ONE = 16384


def _sinc(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0.0, 1.0, np.sin(np.pi * x) / (np.pi * x))


def taps(s, d, a):
    """(first int32[d], count int32[d], coef int16[d, 32]) of s source samples -> d output samples with a lobes."""
    first = np.zeros(d, dtype=np.int32)
    count = np.zeros(d, dtype=np.int32)
    coef = np.zeros((d, TAPS), dtype=np.int16)
    f = max(1.0, s / d)
    r = a * f
    for o in range(d):
        c = ((o + 0.5) * s) / d - 0.5
        i = np.arange(math.ceil(c - r), math.floor(c + r) + 1, dtype=np.int64)
        i = i[np.abs(i - c) < r]
        t = (i - c) / f
        w = _sinc(t) * _sinc(t / a)
        S = 0.0
        for x in w:  # left to right
            S += float(x)
        q = np.rint(w * 16384.0 / S).astype(np.int64)
        q[int(np.argmax(q))] += ONE - int(q.sum())  # argmax: the first one on ties
        ci = np.clip(i, 0, s - 1)
        row = np.zeros(TAPS, dtype=np.int64)
        np.add.at(row, ci - ci[0], q)
        assert int(np.abs(row).sum()) <= 32767, (s, d, a, o)
        first[o] = ci[0]
        count[o] = ci[-1] - ci[0] + 1
        coef[o] = row
    return first, count, coef


def clip_range(bit_depth, full_range, gbr, plane):
    """set_pic_clip()'s range of a plane: write_yuv()'s per-plane clamp."""
    if full_range:
        return 0, (1 << bit_depth) - 1
    D = 1 << (bit_depth - 8)
    if plane == 0 or gbr:
        return 16 * D, 235 * D
    return 16 * D, 240 * D


def scale_plane(src, th, tv, lo, hi):
    """src (sh, sw) u16 -> (dh, dw) u16 with the tables th = (first, count, coef) of the width and tv of the height."""
    sh, sw = src.shape
    s = src.astype(np.int64)
    fh, nh, qh = (np.asarray(x).astype(np.int64) for x in th)
    fv, nv, qv = (np.asarray(x).astype(np.int64) for x in tv)
    H = np.zeros((sh, len(fh)), dtype=np.int64)
    for i in range(int(nh.max())):  # a coefficient past a row's count is 0: the clamped index reads a sample that does not count
        H += qh[:, i][None, :] * s[:, np.minimum(fh + i, sw - 1)]
    assert np.abs(H).max() < 2 ** 31
    V = np.zeros((len(fv), len(fh)), dtype=np.int64)
    for j in range(int(nv.max())):
        V += qv[:, j][:, None] * H[np.minimum(fv + j, sh - 1), :]
    return np.clip((V + (1 << 27)) >> 28, lo, hi).astype(np.uint16)


def plane_shapes(w, h, chroma):
    """[(height, width)] of the three planes; chroma 1 (4:2:0) or 3 (4:4:4)."""
    return [(h, w)] + [(h >> 1, w >> 1) if chroma == 1 else (h, w)] * 2


def frame_words(w, h, chroma):
    return sum(a * b for a, b in plane_shapes(w, h, chroma))


def scale_frame(frame, sw, sh, dw, dh, chroma, bit_depth, full_range, gbr, a, taps_fn=taps):
    """A frame (flat u16, three planes one after the other) resampled plane by plane; taps_fn(s, d, a) gives an axis' table."""
    frame = np.asarray(frame, dtype=np.uint16).reshape(-1)
    out, at, cache = [], 0, {}

    def tab(s, d):
        if (s, d) not in cache:
            cache[(s, d)] = taps_fn(s, d, a)[:3]
        return cache[(s, d)]

    for p, ((ph, pw), (qh, qw)) in enumerate(zip(plane_shapes(sw, sh, chroma), plane_shapes(dw, dh, chroma))):
        src = frame[at:at + ph * pw].reshape(ph, pw)
        at += ph * pw
        lo, hi = clip_range(bit_depth, full_range, gbr, p)
        out.append(scale_plane(src, tab(pw, qw), tab(ph, qh), lo, hi).reshape(-1))
    assert at == frame.size
    return np.concatenate(out)
