"""The numpy restatement of h2y_regions_stats (include/hdr2yuv_hip.h): 8x8 tiles by padding and reshaping, the windows' smallest and
largest sample by shifted minima and maxima.  Plain integers throughout; the figures come back in H2YRegionsStats.as_dict()'s
shape, so a test compares two dictionaries."""
import numpy as np

import h2y_testing as ht


def default_flat_var(depth):
    """the command line's default V at bit depth d: a standard deviation of two 8-bit steps, squared"""
    return 4 * 4 ** (depth - 8)


def planes_of(frame, w, h, chroma):
    """the three 2-D planes of a frame whose planes lie one after the other"""
    cw, ch = (w >> 1, h >> 1) if chroma == 1 else (w, h)
    f = np.asarray(frame).reshape(-1)
    assert f.size == w * h + 2 * cw * ch
    return [f[:w * h].reshape(h, w), f[w * h:w * h + cw * ch].reshape(ch, cw), f[w * h + cw * ch:].reshape(ch, cw)]


def _tile_sums(x):
    """the sum of x over every 8x8 tile at (8i, 8j), the last row and column of tiles cut to the plane"""
    h, w = x.shape
    th, tw = -(-h // 8), -(-w // 8)
    padded = np.zeros((8 * th, 8 * tw), dtype=np.int64)
    padded[:h, :w] = x
    return padded.reshape(th, 8, tw, 8).sum(axis=(1, 3))


def plane_stats(a, b, flat_var, r):
    a, b = a.astype(np.int64), b.astype(np.int64)
    h, w = b.shape
    n, s, ss = _tile_sums(np.ones_like(b)), _tile_sums(b), _tile_sums(b * b)
    d = a - b
    sse, sad = _tile_sums(d * d), _tile_sums(np.abs(d))
    act = n * ss - s * s
    flat = act <= int(flat_var) * n * n
    out = {}
    for key, v in (("tiles", np.ones_like(n)), ("samples", n), ("sse", sse), ("sad", sad)):
        out[key] = [int(v[flat].sum()), int(v[~flat].sum())]
    # the window is a square: the rows' shifted minima and maxima first, then the columns' of those
    m = np.pad(b, ((0, 0), (r, r)), constant_values=1 << 16)  # past the plane: never the smallest
    M = np.pad(b, ((0, 0), (r, r)), constant_values=-1)       # nor the largest
    m = np.minimum.reduce([m[:, d:d + w] for d in range(2 * r + 1)])
    M = np.maximum.reduce([M[:, d:d + w] for d in range(2 * r + 1)])
    m = np.pad(m, ((r, r), (0, 0)), constant_values=1 << 16)
    M = np.pad(M, ((r, r), (0, 0)), constant_values=-1)
    m = np.minimum.reduce([m[d:d + h] for d in range(2 * r + 1)])
    M = np.maximum.reduce([M[d:d + h] for d in range(2 * r + 1)])
    o, u = np.maximum(a - M, 0), np.maximum(m - a, 0)
    out.update(over=int((o > 0).sum()), over_sum=int(o.sum()), over_max=int(o.max()),
               under=int((u > 0).sum()), under_sum=int(u.sum()), under_max=int(u.max()))
    return out


def frame_stats(w, h, chroma, flat_var, r, a, b):
    """h2y_regions_stats of frame a against frame b (each: three planes one after the other), as H2YRegionsStats.as_dict() gives it"""
    per = [plane_stats(pa, pb, flat_var, r) for pa, pb in zip(planes_of(a, w, h, chroma), planes_of(b, w, h, chroma))]
    out = {k: [p[k] for p in per] for k in ("tiles", "samples", "sse", "sad", "over", "over_sum", "under", "under_sum", "over_max", "under_max")}
    out.update(flat_var=int(flat_var), radius=int(r))
    return out


def picture(w, h, chroma, depth, rng):
    """A reference frame in which both classes and both excursions occur: tiles of a constant with noise of at most one code (tile
    (i, j) with i + j even, so every plane's first tile) alternate with tiles of full-range noise."""
    maxv = (1 << depth) - 1
    planes = []
    for ph, pw in ((h, w),) + (((h >> 1, w >> 1),) * 2 if chroma == 1 else ((h, w),) * 2):
        ty, tx = np.arange(ph)[:, None] // 8, np.arange(pw)[None, :] // 8
        const = (maxv // 4 + (maxv // 16) * ((ty * 5 + tx * 3) % 7)) + rng.integers(0, 2, (ph, pw))
        noise = rng.integers(0, maxv + 1, (ph, pw))
        planes.append(np.where((ty + tx) % 2 == 0, const, noise).astype(np.uint16).reshape(-1))
    return np.concatenate(planes)


def both_occur(st):
    """do a frame's restated figures hold both classes (on every plane of more than one tile) and both excursions on every plane?"""
    for p in range(3):
        flat, busy = st["tiles"][p]
        if flat + busy > 1 and not (flat > 0 and busy > 0):
            return False
        if st["over"][p] == 0 or st["under"][p] == 0:
            return False
    return True


# ---- the tests' pictures ---------------------------------------------------------------------------------------------------

def pair(w, hh, chroma, depth):
    """(A, B) of the size: B regions_ref.picture, A = B with every code moved by up to 3; the same pair for the same arguments"""
    rng = np.random.default_rng(1000 * w + 10 * hh + chroma + 100 * depth)
    b = picture(w, hh, chroma, depth, rng)
    return ht.noisy(b, depth, rng), b


def step_edge():
    """B 32x16: the left half 100, the right half 900; A = B but for column 15 at 90 and column 16 at 930 (10 bits, 4:4:4)"""
    b = np.full((16, 32), 100, np.uint16)
    b[:, 16:] = 900
    a = b.copy()
    a[:, 15], a[:, 16] = 90, 930
    return np.tile(a.reshape(-1), 3), np.tile(b.reshape(-1), 3)


STEP_EDGE = dict(under=16, under_sum=160, under_max=10, over=16, over_sum=480, over_max=30)


def check_step_edge(st):
    for key, v in STEP_EDGE.items():
        assert st[key][0] == v, (key, st)
    # every tile is constant, so flat, at any V: also the two columns of tiles the edge lies between
    assert st["tiles"][0] == [8, 0] and st["sse"][0] == [16 * 100 + 16 * 900, 0] and st["sad"][0] == [16 * 10 + 16 * 30, 0]


def bounds_16(w, hh):
    """the two 16-bit extremes (4:4:4): (A, B, V, the figures of every plane)"""
    n, tiles = w * hh, -(-w // 8) * -(-hh // 8)
    white, black = np.full(3 * n, 65535, np.uint16), np.zeros(3 * n, np.uint16)
    yy, xx = np.mgrid[:hh, :w]
    board = np.tile((((xx + yy) & 1) * 65535).astype(np.uint16).reshape(-1), 3)
    all_over = dict(tiles=[tiles, 0], samples=[n, 0], sse=[n * 65535 ** 2, 0], sad=[n * 65535, 0], over=n, over_sum=n * 65535, over_max=65535,
                    under=0, under_sum=0, under_max=0)
    busy = dict(tiles=[0, tiles], samples=[0, n], sse=[0, 0], sad=[0, 0], over=0, over_sum=0, over_max=0, under=0, under_sum=0, under_max=0)
    flat = dict(busy, tiles=[tiles, 0], samples=[n, 0])
    return [(white, black, default_flat_var(16), all_over), (board, board, default_flat_var(16), busy), (board, board, 2 ** 32 - 1, flat)]


def check_bounds(st, want):
    for key, v in want.items():
        assert st[key] == [v] * 3, (key, st[key], v)


# ---- the command line's report ---------------------------------------------------------------------------------------------

def _psnr(maxv, n, sse):
    import math

    if n == 0:
        return "-"
    return "inf" if sse == 0 else "%.4f" % (10.0 * math.log10(float(maxv) * maxv * n / sse))


def _ratio(num, den, fmt):
    return "-" if den == 0 else fmt % (float(num) / float(den))


def _classes(st, names, maxv, flat, busy):
    s = " flat_share" + "".join(f" {names[p]} {_ratio(st['samples'][p][0], sum(st['samples'][p]), '%.6f')}" for p in range(3))
    for c, key in ((0, flat), (1, busy)):
        s += f" {key}" + "".join(f" {names[p]} {_psnr(maxv, st['samples'][p][c], st['sse'][p][c])}" for p in range(3))
    return s


def report(stats, names, depth):
    """the `regions frame` and `regions summary` lines hdr2yuv prints for the frames' figures (frame_stats dictionaries)"""
    maxv = (1 << depth) - 1
    trip = lambda key, v: f" {key} {v[0]} {v[1]} {v[2]}"
    lines = []
    for k, st in enumerate(stats):
        lines.append(f"regions frame {k}" + _classes(st, names, maxv, "psnr_flat", "psnr_busy") + trip("over", st["over"]) +
                     trip("over_max", st["over_max"]) + trip("under", st["under"]) + trip("under_max", st["under_max"]))
    t = {k: [[sum(st[k][p][c] for st in stats) for c in range(2)] for p in range(3)] for k in ("samples", "sse")}
    for k in ("over", "over_sum", "under", "under_sum"):
        t[k] = [sum(st[k][p] for st in stats) for p in range(3)]
    for k in ("over_max", "under_max"):
        t[k] = [max(st[k][p] for st in stats) for p in range(3)]
    mean = lambda key, s, n: f" {key}" + "".join(f" {names[p]} {_ratio(t[s][p], t[n][p], '%.4f')}" for p in range(3))
    lines.append(f"regions summary frames {len(stats)}" + _classes(t, names, maxv, "global_psnr_flat", "global_psnr_busy") +
                 trip("over", t["over"]) + mean("over_mean", "over_sum", "over") + trip("over_max", t["over_max"]) +
                 trip("under", t["under"]) + mean("under_mean", "under_sum", "under") + trip("under_max", t["under_max"]))
    return lines
