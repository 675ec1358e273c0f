"""A numpy restatement of the SSIM that k_ssim computes (include/hdr2yuv_hip.h, h2y_ssim_stats): 4x4 blocks, 8x8 windows at a
stride of 4, exact int64 block and window sums, binary64 in exactly the stated order, rint(s x 2^32) summed in int64."""
import math

import numpy as np


def constants(depth):
    """c1, c2 of bit depth `depth`, in binary64, left to right"""
    m = float((1 << depth) - 1)
    c1 = ((0.01 * 0.01) * m) * m * 64.0
    c2 = (((0.03 * 0.03) * m) * m * 64.0) * 63.0
    return c1, c2


def plane(a, b, depth):
    """(windows, sum_q, ssim) of one plane: a, b 2-D arrays (rows, columns) of codes"""
    ph, pw = a.shape
    bw, bh = pw >> 2, ph >> 2
    assert bw >= 2 and bh >= 2, "a plane needs at least 8x8 samples"
    x = a[:4 * bh, :4 * bw].astype(np.int64).reshape(bh, 4, bw, 4)
    y = b[:4 * bh, :4 * bw].astype(np.int64).reshape(bh, 4, bw, 4)
    s1, s2 = x.sum(axis=(1, 3)), y.sum(axis=(1, 3))
    ss = (x * x).sum(axis=(1, 3)) + (y * y).sum(axis=(1, 3))
    s12 = (x * y).sum(axis=(1, 3))

    def win(v):  # the four blocks of every 2x2 group
        return v[:-1, :-1] + v[:-1, 1:] + v[1:, :-1] + v[1:, 1:]

    fs1, fs2, fss, fs12 = (win(v).astype(np.float64) for v in (s1, s2, ss, s12))
    c1, c2 = constants(depth)
    vars_ = ((fss * 64.0) - (fs1 * fs1)) - (fs2 * fs2)
    covar = (fs12 * 64.0) - (fs1 * fs2)
    num = (((2.0 * fs1) * fs2) + c1) * ((2.0 * covar) + c2)
    den = (((fs1 * fs1) + (fs2 * fs2)) + c1) * (vars_ + c2)
    q = np.rint((num / den) * 4294967296.0).astype(np.int64)
    windows = (bw - 1) * (bh - 1)
    sum_q = int(q.sum())
    return windows, sum_q, (float(sum_q) * 2.0 ** -32) / float(windows)


def split(frame, w, hh, chroma):
    """the three planes (2-D) of a flat frame, planes one after the other (chroma 1: 4:2:0, 3: 4:4:4)"""
    cw, ch = (w >> 1, hh >> 1) if chroma == 1 else (w, hh)
    n, nc = w * hh, cw * ch
    return [frame[:n].reshape(hh, w), frame[n:n + nc].reshape(ch, cw), frame[n + nc:n + 2 * nc].reshape(ch, cw)]


def frame(a, b, w, hh, chroma, depth):
    """dict(windows, sum_q, ssim, all) of flat frames a against b"""
    pa, pb = split(a, w, hh, chroma), split(b, w, hh, chroma)
    r = [plane(x, y, depth) for x, y in zip(pa, pb)]
    n = [float(x.size) for x in pa]
    s = [v[2] for v in r]
    return dict(windows=[v[0] for v in r], sum_q=[v[1] for v in r], ssim=s,
                all=((s[0] * n[0] + s[1] * n[1]) + s[2] * n[2]) / ((n[0] + n[1]) + n[2]))


def db(x):
    return math.inf if x >= 1.0 else -10.0 * math.log10(1.0 - x)


def db_str(x):
    return "inf" if x >= 1.0 else "%.4f" % db(x)


def report(figures, names):
    """the command line's ssim lines for a list of frame() dicts"""
    def line(v, al):
        return (" ".join("%s %.6f" % (names[p], v[p]) for p in range(3)) + " all %.6f db " % al
                + " ".join("%s %s" % (names[p], db_str(v[p])) for p in range(3)) + " all %s" % db_str(al))

    out = ["ssim frame %d %s" % (k, line(f["ssim"], f["all"])) for k, f in enumerate(figures)]
    mean, mean_all = [0.0, 0.0, 0.0], 0.0
    worst = 0
    for k, f in enumerate(figures):
        for p in range(3):
            mean[p] += f["ssim"][p]
        mean_all += f["all"]
        if f["all"] < figures[worst]["all"]:
            worst = k
    n = float(len(figures))
    out.append("ssim summary frames %d %s" % (len(figures), line([m / n for m in mean], mean_all / n)))
    out.append("ssim worst frame %d all %.6f" % (worst, figures[worst]["all"]))
    return out
