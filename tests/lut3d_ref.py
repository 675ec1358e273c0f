"""The 3D LUT pass of include/hdr2yuv_hip.h ("3D LUT") restated in numpy, operation by operation: every product, difference and sum
is one float32 operation (numpy rounds each array operation on its own).  k_lut3d and h2y_lut3d_planes are held to it bit for bit.
Also the binary64 evaluations the float64 bound is checked against."""
import numpy as np

f32 = np.float32


def scales(n, lo, hi):
    """s_c = (N - 1) / (hi_c - lo_c) in binary64, rounded once to binary32"""
    lo, hi = np.asarray(lo, f32).astype(np.float64), np.asarray(hi, f32).astype(np.float64)
    return ((n - 1) / (hi - lo)).astype(f32)


def cell(planes, n, lo, hi):
    """steps 1-2 for planes G, B, R: (i, j, f), each indexed by channel r, g, b"""
    lo, s, last = np.asarray(lo, f32), scales(n, lo, hi), f32(n - 1)
    x = [np.asarray(planes[p]).astype(f32).reshape(-1) for p in (2, 0, 1)]  # r, g, b; a half widens exactly
    i, j, f = [], [], []
    with np.errstate(all="ignore"):
        for c in range(3):
            t = (x[c] - lo[c]) * s[c]
            t = np.where(t > 0, np.minimum(t, last), f32(0)).astype(f32)
            ic = t.astype(np.int64)
            i.append(ic)
            j.append(np.minimum(ic + 1, n - 1))
            f.append(t - ic.astype(f32))
    return i, j, f


def _node(flat, n, r, g, b):
    return flat[r + n * (g + n * b)]


def tetrahedral(flat, n, i, j, f):
    fr, fg, fb = f
    c1, c2, c3, c4, c5 = fr > fg, fg > fb, fr > fb, fb > fg, fb > fr
    paths = [(c1 & c2, (0, 1, 2)), (c1 & ~c2 & c3, (0, 2, 1)), (c1 & ~c2 & ~c3, (2, 0, 1)),
             (~c1 & c4, (2, 1, 0)), (~c1 & ~c4 & c5, (1, 2, 0)), (~c1 & ~c4 & ~c5, (1, 0, 2))]
    a = np.zeros((3, fr.size), np.int64)
    for mask, path in paths:
        for k in range(3):
            a[k][mask] = path[k]
    assert sum(m.astype(int) for m, _ in paths).min() == 1 and sum(m.astype(int) for m, _ in paths).max() == 1
    I, J, F = np.stack(i), np.stack(j), np.stack(f)
    ax = np.arange(3)[:, None]
    m1 = ax == a[0][None]
    m2 = m1 | (ax == a[1][None])
    I1, I2 = np.where(m1, J, I), np.where(m2, J, I)
    p0, p1, p2, p3 = (_node(flat, n, *X) for X in (I, I1, I2, J))
    w = [np.take_along_axis(F, a[k][None], 0)[0][:, None] for k in range(3)]
    return ((p0 + (p1 - p0) * w[0]) + (p2 - p1) * w[1]) + (p3 - p2) * w[2]


def trilinear(flat, n, i, j, f):
    (ir, ig, ib), (jr, jg, jb) = i, j
    fr, fg, fb = (x[:, None] for x in f)

    def lerp(a, b, w):
        return a + (b - a) * w

    c00 = lerp(_node(flat, n, ir, ig, ib), _node(flat, n, jr, ig, ib), fr)
    c10 = lerp(_node(flat, n, ir, jg, ib), _node(flat, n, jr, jg, ib), fr)
    c01 = lerp(_node(flat, n, ir, ig, jb), _node(flat, n, jr, ig, jb), fr)
    c11 = lerp(_node(flat, n, ir, jg, jb), _node(flat, n, jr, jg, jb), fr)
    return lerp(lerp(c00, c10, fg), lerp(c01, c11, fg), fb)


def interpolate(planes, nodes, lo, hi, interp=1):
    """steps 1-3: the float32 (npix, 3) values v_r, v_g, v_b"""
    nodes = np.asarray(nodes, f32)
    n = nodes.shape[0]
    i, j, f = cell(planes, n, lo, hi)
    with np.errstate(all="ignore"):
        v = (tetrahedral if interp else trilinear)(nodes.reshape(-1, 3), n, i, j, f)
    assert v.dtype == f32
    return v


def apply(planes, nodes, lo=(0, 0, 0), hi=(1, 1, 1), interp=1, signal=0, scale=None):
    """the whole pixel for planes G, B, R of float32 or float16: the three planes the pass leaves.  nodes: float32 (n, n, n, 3)
    indexed [b][g][r][channel].  signal 1: scale = (mulY, addY, mulC, addC) as float32 (hlg_ref.scale), the planes are float32."""
    dt, shape = np.asarray(planes[0]).dtype, np.asarray(planes[0]).shape
    v = interpolate(planes, nodes, lo, hi, interp)
    vr, vg, vb = v[:, 0], v[:, 1], v[:, 2]
    if signal:
        mulY, addY, mulC, addC = (f32(x) for x in scale)
        with np.errstate(all="ignore"):
            vr, vg, vb = (np.where(x > 0, np.minimum(x, f32(1)), f32(0)).astype(f32) for x in (vr, vg, vb))
        out = [vg * mulY + addY, vb * mulC + addC, vr * mulC + addC]
        assert all(o.dtype == f32 for o in out)
        return [o.reshape(shape) for o in out]
    with np.errstate(over="ignore"):
        return [o.astype(dt).reshape(shape) for o in (vg, vb, vr)]  # float16: to nearest even


# ---- binary64 --------------------------------------------------------------------------------------------------------------

def position64(planes, n, lo, hi):
    """the exact position t_c in [0, N - 1] of every pixel in binary64, indexed by channel r, g, b (inputs are finite)"""
    lo, hi = np.asarray(lo, f32).astype(np.float64), np.asarray(hi, f32).astype(np.float64)
    x = [np.asarray(planes[p]).astype(np.float64).reshape(-1) for p in (2, 0, 1)]
    return [np.clip((x[c] - lo[c]) * ((n - 1) / (hi[c] - lo[c])), 0, n - 1) for c in range(3)]


def tetrahedral64(nodes, t):
    """the barycentric evaluation on the tetrahedron of the sorted fractions, in binary64: (npix, 3)"""
    N = np.asarray(nodes, np.float64)
    n = N.shape[0]
    i = [np.minimum(np.floor(x).astype(np.int64), n - 2) for x in t]
    F = np.stack([x - k for x, k in zip(t, i)])          # (3, npix), in [0, 1]
    order = np.argsort(-F, axis=0, kind="stable")        # the largest fraction moves first
    I = np.stack(i)
    cur = I.copy()
    prev = N[cur[2], cur[1], cur[0]]
    out = prev.copy()
    for k in range(3):
        a = order[k]
        cur = cur + (np.arange(3)[:, None] == a[None]).astype(np.int64)
        nxt = N[cur[2], cur[1], cur[0]]
        out += (nxt - prev) * np.take_along_axis(F, a[None], 0)[0][:, None]
        prev = nxt
    return out


def bound(nodes):
    """2^-24 (16 M + 12 (N - 1) D): M = max |node|, D = the largest difference between neighbouring nodes"""
    N = np.asarray(nodes, np.float64)
    n = N.shape[0]
    M = np.abs(N).max()
    D = max(np.abs(np.diff(N, axis=a)).max() for a in range(3))
    return 2.0 ** -24 * (16 * M + 12 * (n - 1) * D)
