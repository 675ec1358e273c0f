"""A numpy restatement of the gamut containment check of include/hdr2yuv_hip.h ("gamut containment of PQ code planes"), for the
tests: steps 2-5 in binary32 on three light planes -- codelight_ref.lights' for a code frame -- with gamut_ref's exact matrices, every
product and sum rounded by itself.  A plain module: numpy, plus the oracle the caller hands to codelight_ref."""
import numpy as np

import codelight_ref as clr
import gamut_ref as gr

F32 = np.float32
RATIO, FLOOR = 0.02, 0.02  # the defaults: T, and A in cd/m2
NAMES = {1: "BT.709", 8: "BT.2020", 9: "BT.2020", 12: "P3-D65"}


def constants(ratio=RATIO, floor=FLOOR):
    """(t, a): t = (float)T; a = (float)(A / 10000.0), the division in binary64"""
    return F32(ratio), F32(np.float64(floor) / np.float64(10000.0))


def excursion(lights, file_primaries, check_set):
    """e of every pixel (flat binary32) of light planes [L_G, L_B, L_R] against one set"""
    m = gr.matrix(file_primaries, check_set)
    lg, lb, lr = (np.asarray(p, F32).reshape(-1) for p in lights)
    v = []
    for i in range(3):
        row = ((m[i][0] * lr) + (m[i][1] * lg)) + (m[i][2] * lb)
        assert row.dtype == F32
        v.append(row)
    lo = np.minimum(np.minimum(v[0], v[1]), v[2])
    return np.where(lo < 0, -lo, F32(0.0)).astype(F32)


def stats_of_lights(lights, width, file_primaries, sets, ratio=RATIO, floor=FLOOR):
    """h2y_gamutcheck_stats of one frame's light planes, as a dict: pixels, n_sets, and per set the integers of step 5"""
    t, a = constants(ratio, floor)
    lg, lb, lr = (np.asarray(p, F32).reshape(-1) for p in lights)
    mx = np.maximum(np.maximum(lg, lb), lr)
    npix = lg.size
    out = []
    for c in sets:
        e = excursion([lg, lb, lr], file_primaries, c)
        tm = t * mx
        assert tm.dtype == F32
        outside = int(np.count_nonzero(e > 0))
        beyond = int(np.count_nonzero((e > tm) & (e > a)))
        bits = e.view(np.uint32)
        key = (bits.astype(np.uint64) << np.uint64(32)) | (~np.arange(npix, dtype=np.uint32)).astype(np.uint64)
        top = int(key.max())
        index = (~top) & 0xFFFFFFFF
        sum_q = int(np.rint(e.astype(np.float64) * 4294967296.0).astype(np.uint64).sum(dtype=np.uint64))
        out.append(dict(primaries=int(c), max_bits=top >> 32, max_x=index % width if outside else -1, max_y=index // width if outside else -1,
                        outside=outside, beyond=beyond, sum_q=sum_q))
    return dict(pixels=npix, n_sets=len(out), sets=out)


def stats(oracle, planes, width, height, chroma, depth, full_range, matrix, file_primaries, sets, ratio=RATIO, floor=FLOOR, form=clr.FIR):
    """the same of one code frame's three planes (matrices 0, 1, 9: codelight_ref's lights; 14: ictcp_ref's)"""
    p444 = clr.planes444(oracle, planes, width, height, chroma, depth, form)
    if matrix == 14:
        import ictcp_ref

        ls = ictcp_ref.lights(oracle, p444, depth, full_range)
    else:
        ls = clr.lights(oracle, p444, depth, full_range, matrix)
    return stats_of_lights(ls, width, file_primaries, sets, ratio, floor)


def ints_of(st):
    """an H2YGamutcheckStats' integers, in stats_of_lights' form"""
    return dict(pixels=int(st.pixels), n_sets=int(st.n_sets),
                sets=[dict(primaries=int(s.primaries), max_bits=int(s.max_bits), max_x=int(s.max_x), max_y=int(s.max_y), outside=int(s.outside),
                           beyond=int(s.beyond), sum_q=int(s.sum_q)) for s in list(st.set)[:st.n_sets]])


def doubles_of(ints):
    """the host's doubles of step 5 from the integers: per set (max_cdm2, mean_cdm2, beyond_share)"""
    out = []
    for s in ints["sets"]:
        e = np.array([s["max_bits"]], np.uint32).view(F32)[0]
        out.append((10000.0 * float(e), ((10000.0 * float(s["sum_q"])) * 2.0 ** -32) / float(ints["pixels"]), float(s["beyond"]) / float(ints["pixels"])))
    return out


# ---- pictures the tests share ---------------------------------------------------------------------------------------------

PATCHES = {"red": (1, 0, 0), "green": (0, 1, 0), "blue": (0, 0, 1), "cyan": (0, 1, 1), "magenta": (1, 0, 1), "yellow": (1, 1, 0)}  # (R, G, B)


def patch_lights(name, level=0.01, n=64):
    """[L_G, L_B, L_R] of a patch of n pixels of a BT.2020 primary or secondary at `level` (0.01: 100 cd/m2), exact binary32 planes"""
    r, g, b = PATCHES[name]
    return [np.full(n, F32(level) * F32(c), F32) for c in (g, b, r)]


def patch_excursion_exact(name, file_primaries, check_set, level=0.01):
    """the patch's excursion in binary64 with the exact-fraction matrix, on the binary32 level"""
    m = gr.matrix_exact(file_primaries, check_set)
    v = [float(F32(level)) * c for c in PATCHES[name]]
    lo = min(sum(float(m[i][j]) * v[j] for j in range(3)) for i in range(3))
    return -lo if lo < 0 else 0.0


def boundary_lights(check_set, n, seed):
    """n colours on the boundary of check_set (one channel 0, the largest 1, the third uniform; peak log-uniform in 0.05 .. 1000 cd/m2),
    expressed in BT.2020 primaries: binary64 rows (R, G, B), in units of 10000 cd/m2"""
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    zero = rng.integers(0, 3, n)
    one = (zero + 1 + rng.integers(0, 2, n)) % 3
    rgb = rng.uniform(0.0, 1.0, (3, n))
    rgb[zero, idx] = 0.0
    rgb[one, idx] = 1.0
    rgb *= np.exp(rng.uniform(np.log(0.05), np.log(1000.0), n)) / 10000.0
    m = np.array([[float(x) for x in row] for row in gr.matrix_exact(check_set, 9)], np.float64)
    return np.clip(m @ rgb, 0.0, 1.0)


def pq_inverse_eotf(y):
    """BT.2100's PQ inverse EOTF of y = light / 10000 cd/m2, in binary64"""
    m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
    ym = np.power(np.asarray(y, np.float64), m1)
    return np.power((c1 + c2 * ym) / (1.0 + c3 * ym), m2)


def code_2020nc_10bit(rgb):
    """binary64 light rows (R, G, B) -> [Y, Cb, Cr] 10-bit video-range BT.2020nc PQ codes, 4:4:4, rounded to nearest"""
    r, g, b = (pq_inverse_eotf(v) for v in rgb)
    y = 0.2627 * r + 0.6780 * g + 0.0593 * b
    cb, cr = (b - y) / 1.8814, (r - y) / 1.4746
    q = lambda v: np.clip(np.rint(v), 0, 1023).astype(np.uint16)
    return [q(876.0 * y + 64.0), q(896.0 * cb + 512.0), q(896.0 * cr + 512.0)]


def patch_codes_16bit_full(name, level=0.01, n=64):
    """the patch as 16-bit full-range G, B, R PQ codes"""
    on = int(np.rint(pq_inverse_eotf(level) * 65535.0))
    r, g, b = PATCHES[name]
    return [np.full(n, on * c, np.uint16) for c in (g, b, r)]
