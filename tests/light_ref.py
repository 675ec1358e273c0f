"""A numpy restatement of the content light level of include/hdr2yuv_hip.h (h2y_light_stats), for the tests: pic_stats' floor and
ceiling (common.cpp:91-139), the normalisation of matrix_convert() (convert.cpp:939-1019, binary32), the source transfer functions
(convert.cpp:12-75: binary64 np.power, RHO_GAMMA's inner pow being binary32 powf) and the per-frame figures."""
import numpy as np

SAMPLE_U16, SAMPLE_F32, SAMPLE_F16 = 1, 2, 3  # H2Y_SAMPLE_*
LINEAR, PQ, RHO_GAMMA_TF, BT1886 = 8, 16, 18, (1, 6, 14, 15)
GAMMA24 = float(np.float32(2.4))  # (double)2.4f of bt1886_f and RHO_GAMMA_f


def pic_stats(planes, sample, src_depth=16):
    """[floor] * 3, [ceiling] * 3 of pic_stats(): min / max over the non-NaN samples, truncated to int (floats) or snapped to the
    video-range ceiling (u16)"""
    fl, ce = [], []
    for p in planes:
        x = p.astype(np.float32).reshape(-1)
        x = x[~np.isnan(x)]
        lo, hi = np.float32(x.min()), np.float32(x.max())
        if sample == SAMPLE_U16:
            f, c = int(lo), int(hi)
            d = 1 << (src_depth - 8)
            ymax, cmax = 219 * d + 16 * d, 224 * d + 16 * d
            if ymax * 3 // 4 < c < ymax:
                c = ymax
            if cmax * 3 // 4 < c < cmax:
                c = cmax
        else:
            lim = (np.float32(-2147483648.0), np.float32(2147483520.0))
            f, c = int(np.clip(lo, *lim)), int(np.clip(hi, *lim))
        fl.append(f)
        ce.append(c)
    return fl, ce


def _wrap32(v):
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def powf25(v):
    """powf(25.0f, v) of this host's libm, element by element (RHO_GAMMA_f's inner pow is powf; numpy's float32 power is not
    libm's)"""
    import ctypes
    import ctypes.util

    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.powf.restype, libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    u, inv = np.unique(v.view(np.uint32), return_inverse=True)
    out = np.array([libm.powf(25.0, float(x)) for x in u.view(np.float32)], np.float32)
    return out[inv.reshape(-1)].reshape(v.shape)


def to_linear(v, src_transfer, to_linear_fn=None):
    """tf_to_linear(class of src_transfer, v) on binary32 v: a binary32 result.  to_linear_fn(v, src_transfer), when given,
    computes it instead (the oracle's vector export, for lists too long for powf25's loop; test_light_sweeps.py pins it to the
    numpy + libm form below)"""
    if to_linear_fn is not None and src_transfer != LINEAR:
        return to_linear_fn(v, src_transfer)
    with np.errstate(all="ignore"):
        if src_transfer == LINEAR:
            return v
        if src_transfer in BT1886:
            x = (v + np.float32(0.0)).astype(np.float64)
            x = np.where(x > 0.0, x, 0.0)  # a NaN too
            return np.power(x, GAMMA24).astype(np.float32)
        if src_transfer == RHO_GAMMA_TF:
            p = powf25(v.astype(np.float32))
            x = (p.astype(np.float64) - 1.0) / 24.0
            r = np.where(x >= 0.0, np.power(np.where(x >= 0.0, x, 0.0), GAMMA24), np.nan)
            return r.astype(np.float32)
    raise ValueError(f"no linear light for src_transfer {src_transfer}")


def light_m(planes, floor, ceiling, src_transfer, to_linear_fn=None):
    """m per pixel (binary32, flat): max over G, B, R of the normalised, linearised sample, NaN as 0, clamped to [0, 1]"""
    out = None
    for c, p in enumerate(planes):
        v = p.astype(np.float32).reshape(-1)
        with np.errstate(all="ignore"):
            x = (v - np.float32(floor[c])) / np.float32(_wrap32(ceiling[c] - floor[c]))
        x = to_linear(x.astype(np.float32), src_transfer, to_linear_fn)
        x = np.where(x > 0, np.minimum(x, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        out = x if out is None else np.maximum(out, x)
    return out


def light_stats(planes, width, sample, src_transfer, src_depth=16, override=None, to_linear_fn=None):
    """the figures of h2y_light_stats for one frame (planes: G, B, R arrays as uploaded); override: (floor, ceiling) lists"""
    fl, ce = override if override is not None else pic_stats(planes, sample, src_depth)
    return stats_of_m(light_m(planes, fl, ce, src_transfer, to_linear_fn), width)


def stats_of_m(m, width):
    """the figures of one frame from its pixels' m (flat binary32)"""
    i = int(np.argmax(m))  # the first index of the maximum
    mx = m[i]
    sum_q = int(np.rint(m.astype(np.float64) * 2.0 ** 32).astype(np.uint64).sum(dtype=np.uint64))
    n = m.size
    return dict(max_bits=int(mx.view(np.uint32)), x=i % width, y=i // width, sum_q=sum_q, pixels=n, cll=10000.0 * float(mx),
                fall=((10000.0 * float(sum_q)) * 2.0 ** -32) / float(n))


def report_lines(stats):
    """the CLI's light lines (hdr2yuv.cpp) for a list of light_stats dicts"""
    lines = [f"light frame {k} peak {s['cll']:.4f} at {s['x']} {s['y']} average {s['fall']:.4f}" for k, s in enumerate(stats)]
    kc = max(range(len(stats)), key=lambda k: (stats[k]["cll"], -k))
    kf = max(range(len(stats)), key=lambda k: (stats[k]["fall"], -k))
    cll, fall = round_half_away(stats[kc]["cll"]), round_half_away(stats[kf]["fall"])
    lines.append(f"light summary frames {len(stats)} maxcll {cll} frame {kc} maxfall {fall} frame {kf}")
    lines.append(f'light x265 --max-cll "{cll},{fall}"')
    lines.append(f"light svt-av1 --content-light {cll},{fall}")
    return lines


def round_half_away(x):
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))
