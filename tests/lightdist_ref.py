"""A numpy restatement of the light distribution of include/hdr2yuv_hip.h (h2y_lightdist_stats), for the tests: the per-sample light
is light_ref.py's (the normalisation, the source transfer, NaN as 0, the clamp); here the per-frame figures, the logarithmic bins, the
percentiles, the HDR10+ JSON of h2y_lightdist_json and the command line's lines."""
import numpy as np

import light_ref as lr

BINS = 8706
FIRST_BITS = 0x37000000  # 2^-17
PCT = (100, 500, 1000, 2500, 5000, 7500, 9000, 9500, 9900, 9998)  # hundredths of a percent
BITS_100 = 0x3C23D70A  # 0.01f: 100 cd/m2


def bin_of(e):
    """the bin of m by its binary32 bit pattern e (an int or a uint32 array)"""
    e = np.asarray(e, np.int64)
    return np.where(e < FIRST_BITS, 0, ((e - FIRST_BITS) >> 14) + 1)


def edge_bits(k):
    """the lower edge of bin k as binary32 bits"""
    return 0 if k == 0 else FIRST_BITS + ((k - 1) << 14)


def light_planes(planes, floor, ceiling, src_transfer, to_linear_fn=None):
    """L_c of every sample, per plane (binary32, flat)"""
    return [lr.light_m([p], [floor[c]], [ceiling[c]], src_transfer, to_linear_fn) for c, p in enumerate(planes)]


def stats_of_planes(ls):
    """the figures of one frame from its three planes' L (flat binary32, G, B, R), with the bins"""
    m = np.maximum(np.maximum(ls[0], ls[1]), ls[2]).astype(np.float32)
    n = m.size
    bins = np.bincount(bin_of(m.view(np.uint32)), minlength=BINS).astype(np.uint32)
    cum = np.cumsum(bins.astype(np.uint64))  # cum(k): the count in bins 0..k
    pct = [edge_bits(int(np.argmax(cum * np.uint64(10000) >= np.uint64(p * n)))) for p in PCT]  # the smallest such k
    base = lr.stats_of_m(m, n)
    return dict(maxscl_bits=[int(x.max().view(np.uint32)) for x in ls], max_bits=base["max_bits"], sum_q=base["sum_q"], pixels=n,
                below_100=int(np.count_nonzero(m <= np.float32(0.01))), pct_bits=pct, bins=bins)


def lightdist_stats(planes, sample, src_transfer, src_depth=16, override=None, to_linear_fn=None):
    """the figures of h2y_lightdist_stats for one frame (planes: G, B, R arrays as uploaded); override: (floor, ceiling) lists"""
    fl, ce = override if override is not None else lr.pic_stats(planes, sample, src_depth)
    return stats_of_planes(light_planes(planes, fl, ce, src_transfer, to_linear_fn))


def _f(bits):
    return float(np.uint32(bits).view(np.float32))


def units(bits):
    """0.1 cd/m2 of a light given as bits: rint(100000 x (double)L), half to even"""
    return int(np.rint(100000.0 * _f(bits)))


def json_text(stats, first=0):
    """h2y_lightdist_json's text for a list of stats dicts"""
    out = ['{"JSONInfo": {"HDR10plusProfile": "A", "Version": "1.0"},\n"SceneInfo": [\n']
    for k, s in enumerate(stats):
        p = s["pct_bits"]
        avg = int(np.rint(((100000.0 * float(s["sum_q"])) * 2.0 ** -32) / float(s["pixels"])))
        values = [units(p[0]), units(p[9]), 100 * s["below_100"] // s["pixels"]] + [units(x) for x in p[3:9]]
        scl = s["maxscl_bits"]
        out.append('{"LuminanceParameters": {"AverageRGB": %d, "LuminanceDistributions": {"DistributionIndex": [1, 5, 10, 25, 50, 75, 90, '
                   '95, 99], "DistributionValues": [%s]}, "MaxScl": [%d, %d, %d]}, "NumberOfWindows": 1, '
                   '"TargetedSystemDisplayMaximumLuminance": 400, "SceneFrameIndex": %d, "SceneId": 0, "SequenceFrameIndex": %d}%s\n'
                   % (avg, ", ".join(str(v) for v in values), units(scl[2]), units(scl[0]), units(scl[1]), k, first + k,
                      "," if k + 1 < len(stats) else ""))
    out.append('],\n"SceneInfoSummary": {"SceneFirstFrameIndex": [%d], "SceneFrameNumbers": [%d]},\n'
               '"ToolInfo": {"Tool": "hdr2yuv", "Version": "1.0"}}\n' % (first, len(stats)))
    return "".join(out)


def report_lines(stats):
    """the CLI's per-frame dynamic_metadata: lines (hdr2yuv.cpp) for a list of stats dicts"""
    lines = []
    for k, s in enumerate(stats):
        scl = s["maxscl_bits"]
        avg = ((10000.0 * float(s["sum_q"])) * 2.0 ** -32) / float(s["pixels"])
        lines.append("dynamic_metadata: frame %d maxscl %.4f %.4f %.4f average %.4f percentiles %s below_100 %.4f"
                     % (k, 10000.0 * _f(scl[2]), 10000.0 * _f(scl[0]), 10000.0 * _f(scl[1]), avg,
                        " ".join("%.4f" % (10000.0 * _f(b)) for b in s["pct_bits"]), 100.0 * float(s["below_100"]) / float(s["pixels"])))
    return lines
