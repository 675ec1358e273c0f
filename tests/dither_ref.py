"""The numpy restatement of include/hdr2yuv_hip.h's section "dither": the mixer, the ordered matrix, the offsets t of one plane and
the reduction of a frame of three u16 planes from depth W to depth D.  Written from the definition's text, in uint32 arithmetic
with wrap-around; it shares no line with the library."""
import numpy as np

M32 = 0xFFFFFFFF


def mix(a):
    """mix() of a uint32 scalar or array"""
    a = np.asarray(a, dtype=np.uint64) & M32
    a ^= a >> 16
    a = (a * 0x7FEB352D) & M32
    a ^= a >> 15
    a = (a * 0x846CA68B) & M32
    a ^= a >> 16
    return a  # uint64 holding a uint32: sums below are masked again


def bayer(x, y):
    """B(x, y) for x, y in 0..15 (scalars or arrays)"""
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    a = x ^ y
    b = np.zeros(np.broadcast(x, y).shape, dtype=np.int64)
    for i in range(4):
        b |= ((a >> i) & 1) << (2 * (3 - i) + 1)
        b |= ((y >> i) & 1) << (2 * (3 - i))
    return b


def plane_key(temporal, seed, frame, plane):
    fi = (frame & M32) if temporal else 0
    kf = int(mix(((seed & M32) ^ 0x9E3779B9) + fi))
    return int(mix(kf + plane))


def offsets(mode, s, temporal, seed, frame, plane, w, h):
    """t of every sample of one plane: int64[h, w]"""
    kp = plane_key(temporal, seed, frame, plane)
    yy, xx = np.mgrid[0:h, 0:w]
    if mode == 0:
        return np.zeros((h, w), np.int64)
    if mode == 1:
        ox, oy = kp & 15, (kp >> 4) & 15
        return bayer((xx + ox) & 15, (yy + oy) & 15) >> (8 - s)
    assert mode == 2
    row = mix((kp + yy.astype(np.uint64)) & M32)
    return (mix((row + xx.astype(np.uint64)) & M32) & ((1 << s) - 1)).astype(np.int64)


def plane_shapes(w, h, chroma):
    """(rows, columns) of the three planes"""
    c = (h >> 1, w >> 1) if chroma == 1 else (h, w)
    return [(h, w), c, c]


def frame_words(w, h, chroma):
    return sum(a * b for a, b in plane_shapes(w, h, chroma))


def clip_range(depth, full, gbr, plane):
    """write_yuv's per-plane clamp at `depth`"""
    if full:
        return 0, (1 << depth) - 1
    return 16 << (depth - 8), (235 if plane == 0 or gbr else 240) << (depth - 8)


def reduce(frame, w, h, chroma, W, D, full, gbr, mode, temporal, seed, frame_no):
    """a flat u16 frame of three planes at depth W -> the same frame at depth D"""
    s = W - D
    assert 1 <= s <= 8 and 8 <= D < W <= 16
    frame = np.asarray(frame, dtype=np.uint16).reshape(-1)
    assert frame.size == frame_words(w, h, chroma)
    out, at = [], 0
    for p, (ph, pw) in enumerate(plane_shapes(w, h, chroma)):
        v = frame[at:at + ph * pw].astype(np.int64).reshape(ph, pw)
        at += ph * pw
        t = offsets(mode, s, temporal, seed, frame_no, p, pw, ph)
        lo, hi = clip_range(D, full, gbr, p)
        out.append(np.clip((v + t) >> s, lo, hi).astype(np.uint16).reshape(-1))
    return np.concatenate(out)
