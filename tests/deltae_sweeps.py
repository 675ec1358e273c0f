"""Delta E sweeps: every code of a domain through k_deltae, whose figures (a sum, a maximum, a count per frame) are compared with the
restatement's (deltae_ref.py, ictcp_ref.py for matrix 14) figure for figure.  What the frames hold, the restatement over them, the
conditions that keep a sweep from passing by hiding, the comparison that names a row of codes, and BT.2124 in binary64 to hold the
restatement against; plain numpy.  tests/test_deltae_sweeps.py checks this file without a GPU, tests/test_deltae_value_sweeps.py runs
the rows through h2y_deltae_batch.

A row is a side A and the partners B it is run against, one pair per partner, all 4:4:4 at threshold 1.0:

E0  BT.709, BT.2020nc, 10 bits, video range.  A: every (Y, Cb) pair at Cr = 512 ("cb"), every (Y, Cr) pair at Cb = 512 ("cr"), as
    1024 x 1024 frames (Y the row, the swept chroma the column).  B: Y + 1 held at 1023 ("y+1"); the swept chroma + 1 held at 1023
    ("c+1"); A transposed, luma and the swept chroma trading places ("transposed": large differences, d up to 656 here and to 720 in E3).
E1  BT.709, BT.2020nc, 16 bits, both ranges.  A: every Y as a 256 x 256 frame at one of five chroma settings.  B: Y + 1 held at
    65535 ("y+1"); 65535 - Y ("mirror").
E2  G,B,R, 16 bits, both ranges.  A: G = B = R = every code ("grey"), or plane c the codes rotated by c thirds ("rot",
    sweep_values.Sweep's).  B: every code + 1 held at 65535 ("code+1"); every plane in reverse raster order ("reversed").
E3  ICtCp (matrix 14): E0's two grids over (I, Ct) and (I, Cp) with E0's partners; every 16-bit I at three chroma settings, both
    ranges, with E1's partners."""
from __future__ import annotations

import time
from fractions import Fraction

import numpy as np

import deltae_ref as der
import ictcp_ref as ir
import sweep_values as sv

GBR, BT709, BT2020NC, ICTCP = 0, 1, 9, 14
NAMES = {GBR: "GBR", BT709: "BT709", BT2020NC: "BT2020NC", ICTCP: "ICTCP"}
THRESHOLD = 1.0
CHUNKS = 16  # pieces of a frame the restatement takes one at a time (one per thread of the pool)
U16 = np.uint16


def variant(matrix: int) -> str:
    return f"k_deltae<{NAMES[matrix]},444>"


# ---- frames ---------------------------------------------------------------------------------------------------------------
def _held(p, top):
    return np.minimum(p.astype(np.uint32) + 1, top).astype(U16)


def grid10(swept: str):
    """E0's A: Y (I) the row, the swept chroma plane the column, the other chroma plane 512"""
    n = 1024
    y = np.repeat(np.arange(n, dtype=U16), n)
    c = np.tile(np.arange(n, dtype=U16), n)
    mid = np.full(n * n, 512, U16)
    return [y, c, mid] if swept == "cb" else [y, mid, c]


def grid10_partners(a, swept: str):
    k = 1 if swept == "cb" else 2
    up_y = [_held(a[0], 1023), a[1], a[2]]
    up_c = [a[c] if c != k else _held(a[k], 1023) for c in range(3)]
    trans = [a[k] if c == 0 else a[0] if c == k else a[c] for c in range(3)]
    return [("y+1", up_y), ("c+1", up_c), ("transposed", trans)]


def chroma_settings(depth: int):
    """test_sweep_every_luma's five (Cb, Cr)"""
    mid, top, s = 1 << (depth - 1), (1 << depth) - 1, 1 << (depth - 8)
    return [(mid, mid), (mid - 40 * s, mid + 60 * s), (16 * s, 240 * s), (0, top), (mid + 1, mid - 1)]


ICTCP_SETTINGS = (0, 1, 4)  # E3: the grey axis, a colour inside the gamut, and one code either side of the axis


def luma16(setting: int):
    y = np.arange(1 << 16, dtype=np.uint32).astype(U16)
    cb, cr = chroma_settings(16)[setting]
    return [y, np.full(y.size, cb, U16), np.full(y.size, cr, U16)]


def luma16_partners(a):
    return [("y+1", [_held(a[0], 65535), a[1], a[2]]), ("mirror", [(65535 - a[0]).astype(U16), a[1], a[2]])]


def gbr16(arrangement: str):
    return [p.copy() for p in sv.Sweep(sv.all_codes(16), arrangement, 256, 256).planes(0)]


def gbr16_partners(a):
    return [("code+1", [_held(p, 65535) for p in a]), ("reversed", [np.ascontiguousarray(p[::-1]) for p in a])]


def _row(row_id, matrix, depth, full, w, h, make):
    return dict(id=row_id, matrix=matrix, depth=depth, full=full, w=w, h=h, make=make, variant=variant(matrix))


def _grid_row(row_id, matrix, swept):
    def make():
        a = grid10(swept)
        return a, grid10_partners(a, swept)
    return _row(row_id, matrix, 10, 0, 1024, 1024, make)


def _luma_row(row_id, matrix, full, setting):
    def make():
        a = luma16(setting)
        return a, luma16_partners(a)
    return _row(row_id, matrix, 16, full, 256, 256, make)


def _gbr_row(row_id, full, arrangement):
    def make():
        a = gbr16(arrangement)
        return a, gbr16_partners(a)
    return _row(row_id, GBR, 16, full, 256, 256, make)


def rows():
    out = []
    for m in (BT709, BT2020NC):
        out += [_grid_row(f"E0/{NAMES[m]}/{s}", m, s) for s in ("cb", "cr")]
    for m in (BT709, BT2020NC):
        for full in (0, 1):
            out += [_luma_row(f"E1/{NAMES[m]}/{'full' if full else 'video'}/{k}", m, full, k) for k in range(5)]
    for full in (0, 1):
        out += [_gbr_row(f"E2/{'full' if full else 'video'}/{arr}", full, arr) for arr in ("grey", "rot")]
    out += [_grid_row(f"E3/grid/{s}", ICTCP, s) for s in ("cb", "cr")]
    for full in (0, 1):
        out += [_luma_row(f"E3/{'full' if full else 'video'}/{k}", ICTCP, full, k) for k in ICTCP_SETTINGS]
    return out


ROWS = {r["id"]: r for r in rows()}
PLUS_ONE = ("y+1", "c+1", "code+1")


# ---- the restatement ------------------------------------------------------------------------------------------------------
def side_itp(oracle, planes444, depth, full, matrix):
    """(I, T, P) of one side's three flat code planes"""
    if matrix == ICTCP:
        return der.itp_of_lms(oracle, der.lms(ir.lights(oracle, planes444, depth, full)))
    return der.itp(oracle, planes444, depth, full, matrix)


def restate(oracle, row, a, partners, pool=None, radicand=der.radicand, root=der.d_of_radicand):
    """{partner: (q, d)}: the radicand and d at every pixel of each pair, flat binary32, and the core-seconds it took.  radicand and
    root are deltae_ref's; the CPU tests hand in broken ones to see that the figures notice."""
    n = a[0].size
    chunks = max(1, min(CHUNKS, n // 4096))
    cuts = [n * k // chunks for k in range(chunks + 1)]

    def piece(k):
        t0 = time.thread_time()
        lo, hi = cuts[k], cuts[k + 1]
        ia = side_itp(oracle, [p[lo:hi] for p in a], row["depth"], row["full"], row["matrix"])
        out = []
        for _, b in partners:
            q = radicand(ia, side_itp(oracle, [p[lo:hi] for p in b], row["depth"], row["full"], row["matrix"]))
            out.append((q, root(q)))
        return out, time.thread_time() - t0

    pieces = list(pool.map(piece, range(chunks))) if pool is not None else [piece(k) for k in range(chunks)]
    res = {name: tuple(np.concatenate([pc[j][i] for pc, _ in pieces]) for i in range(2)) for j, (name, _) in enumerate(partners)}
    return res, sum(dt for _, dt in pieces)


def figures(q, d):
    """what the conditions are asked of: distinct radicand bit patterns, the share of pixels with d == 0, the pixels over the threshold"""
    return dict(distinct_q=int(np.unique(q.view(np.uint32)).size), zero_share=float(np.count_nonzero(d == 0)) / d.size,
                over=int(np.count_nonzero(d > np.float32(THRESHOLD))), pixels=int(d.size))


# ---- the conditions -------------------------------------------------------------------------------------------------------
# Share of a "+1" pair's pixels with d == 0, at most.  Codes below black and above white clamp to the same light on both sides: at
# video range that is 14.45 % of the luma codes (the grey rows' share), and a chroma far from the axis puts more of the three primes
# outside [0, 1] on both sides.  Every row's own arithmetic meets the bound (the restatement's shares stand beside DISTINCT_Q; the
# largest is 19.43 %, E1/BT2020NC/video/3, Cb = 0 and Cr = 65535), so no row has a bound of its own.
MAX_ZERO = 0.20
# distinct radicand bit patterns of every pair, as the restatement gives them: a sweep's count may fall 2 % short
DISTINCT_Q = {  # row: partner: count  (the share of pixels with d == 0 beside every "+1" pair)
    "E0/BT709/cb": {"y+1": 772720, "c+1": 872299, "transposed": 519361},  # y+1 3.39 %, c+1 4.46 %
    "E0/BT709/cr": {"y+1": 792471, "c+1": 873299, "transposed": 519994},  # y+1 1.56 %, c+1 2.98 %
    "E0/BT2020NC/cb": {"y+1": 768446, "c+1": 862684, "transposed": 518690},  # y+1 3.86 %, c+1 4.90 %
    "E0/BT2020NC/cr": {"y+1": 799336, "c+1": 877200, "transposed": 520393},  # y+1 1.38 %, c+1 2.80 %
    "E1/BT709/video/0": {"y+1": 427, "mirror": 28672},  # y+1 14.45 %
    "E1/BT709/video/1": {"y+1": 18307, "mirror": 32768},  # y+1 0.00 %
    "E1/BT709/video/2": {"y+1": 10864, "mirror": 32768},  # y+1 7.22 %
    "E1/BT709/video/3": {"y+1": 9261, "mirror": 32768},  # y+1 18.23 %
    "E1/BT709/video/4": {"y+1": 830, "mirror": 28674},  # y+1 14.45 %
    "E1/BT709/full/0": {"y+1": 374, "mirror": 32768},  # y+1 0.00 %
    "E1/BT709/full/1": {"y+1": 13424, "mirror": 32768},  # y+1 0.00 %
    "E1/BT709/full/2": {"y+1": 8297, "mirror": 32768},  # y+1 1.50 %
    "E1/BT709/full/3": {"y+1": 7119, "mirror": 32768},  # y+1 9.35 %
    "E1/BT709/full/4": {"y+1": 864, "mirror": 32768},  # y+1 0.00 %
    "E1/BT2020NC/video/0": {"y+1": 427, "mirror": 28672},  # y+1 14.45 %
    "E1/BT2020NC/video/1": {"y+1": 18460, "mirror": 32768},  # y+1 0.00 %
    "E1/BT2020NC/video/2": {"y+1": 9700, "mirror": 32768},  # y+1 8.19 %
    "E1/BT2020NC/video/3": {"y+1": 7967, "mirror": 32767},  # y+1 19.43 %
    "E1/BT2020NC/video/4": {"y+1": 1040, "mirror": 28674},  # y+1 14.45 %
    "E1/BT2020NC/full/0": {"y+1": 374, "mirror": 32768},  # y+1 0.00 %
    "E1/BT2020NC/full/1": {"y+1": 13586, "mirror": 32768},  # y+1 0.00 %
    "E1/BT2020NC/full/2": {"y+1": 7229, "mirror": 32768},  # y+1 1.93 %
    "E1/BT2020NC/full/3": {"y+1": 6092, "mirror": 32768},  # y+1 10.50 %
    "E1/BT2020NC/full/4": {"y+1": 930, "mirror": 32768},  # y+1 0.00 %
    "E2/video/grey": {"code+1": 427, "reversed": 28672},  # code+1 14.45 %
    "E2/video/rot": {"code+1": 10679, "reversed": 32634},  # code+1 0.00 %
    "E2/full/grey": {"code+1": 374, "reversed": 32768},  # code+1 0.00 %
    "E2/full/rot": {"code+1": 6643, "reversed": 32604},  # code+1 0.00 %
    "E3/grid/cb": {"y+1": 486127, "c+1": 406474, "transposed": 364490},  # y+1 7.96 %, c+1 8.07 %
    "E3/grid/cr": {"y+1": 527589, "c+1": 565280, "transposed": 414654},  # y+1 8.46 %, c+1 8.62 %
    "E3/video/0": {"y+1": 853, "mirror": 28672},  # y+1 14.45 %
    "E3/video/1": {"y+1": 20017, "mirror": 32762},  # y+1 3.84 %
    "E3/video/4": {"y+1": 927, "mirror": 28673},  # y+1 14.45 %
    "E3/full/0": {"y+1": 758, "mirror": 32768},  # y+1 0.00 %
    "E3/full/1": {"y+1": 15051, "mirror": 32768},  # y+1 0.00 %
    "E3/full/4": {"y+1": 826, "mirror": 32768},  # y+1 0.00 %
}


def check_conditions(row, figs) -> None:
    """figs: {partner: figures()} of one row, from the restatement"""
    for name, f in figs.items():
        key = (row["id"], name)
        if name in PLUS_ONE:
            assert f["zero_share"] <= MAX_ZERO, (key, f)
        assert f["distinct_q"] >= DISTINCT_Q[row["id"]][name] * 0.98, (key, f, DISTINCT_Q[row["id"]][name])
        if row["id"].startswith("E0") and name in PLUS_ONE:
            assert 0 < f["over"] < f["pixels"], (key, f)
    # the threshold both ways: the row has d below and above it
    assert any(f["over"] > 0 for f in figs.values()) and any(f["over"] < f["pixels"] for f in figs.values()), (row["id"], figs)


# ---- the comparison -------------------------------------------------------------------------------------------------------
def _span(p):
    p = np.asarray(p)
    if p.size and (p == p[0]).all():
        return str(int(p[0]))
    step = "" if p.size < 2 or (np.diff(p.astype(np.int64)) == 1).all() else " (not consecutive)"
    return f"{int(p[0])}..{int(p[-1])}{step}"


def describe_row(a, b, w, r) -> str:
    """the codes row r of a pair holds"""
    sl = slice(r * w, (r + 1) * w)
    return "A (" + ", ".join(_span(p[sl]) for p in a) + ") against B (" + ", ".join(_span(p[sl]) for p in b) + ")"


def differing(got: dict, want: dict) -> dict:
    return {k: (got[k], want[k]) for k in der.KEYS if got[k] != want[k]}


def measure_pairs(measure, pairs, w, h):
    return [g for k in range(0, len(pairs), 4) for g in measure(pairs[k:k + 4], w, h)]


def compare(row, a, partners, rest, measure, got=None):
    """The figures of every pair of the row from `measure` against the restatement's.  measure(pairs, w, h): a list of
    h2y_deltae_stats as dicts, one per (planes A, planes B) of w x h; it takes at most four pairs a call (got: the whole pairs' figures,
    where the caller has measured them already).  Returns (figures
    compared, figures that differ, message); on a difference the first differing pair is measured once more as its rows, w x 1
    pairs, and the message names the first row whose figures differ, the codes it holds, and the got and want of each figure."""
    w, h = row["w"], row["h"]
    pairs = [(a, b) for _, b in partners]
    if got is None:
        got = measure_pairs(measure, pairs, w, h)
    want = [der.stats_of_d(rest[name][1], w, THRESHOLD) for name, _ in partners]
    diffs = [differing(g, x) for g, x in zip(got, want)]
    bad = sum(len(x) for x in diffs)
    if not bad:
        return len(der.KEYS) * len(pairs), 0, ""
    j = next(i for i, x in enumerate(diffs) if x)
    name, b = partners[j]
    msg = f"{row['id']} ({row['variant']}): pair '{name}' differs in {diffs[j]} (got, want)"
    d = rest[name][1]
    rows_ab = [([p[r * w:(r + 1) * w] for p in a], [p[r * w:(r + 1) * w] for p in b]) for r in range(h)]
    for r0 in range(0, h, 4):  # once more, row by row: the failure names the codes
        got_rows = measure(rows_ab[r0:r0 + 4], w, 1)
        for r, g in enumerate(got_rows, r0):
            x = differing(g, der.stats_of_d(d[r * w:(r + 1) * w], w, THRESHOLD))
            if x:
                return len(der.KEYS) * len(pairs), bad, f"{msg}; first differing row {r}: {describe_row(a, b, w, r)}: {x} (got, want)"
    return len(der.KEYS) * len(pairs), bad, msg + "; no single row differs"


def sweep_line(row, pixels, oracle_s, wall, compared, bad, figs) -> str:
    fig = "; ".join(f"{n}: distinct q {f['distinct_q']}, zero share {f['zero_share']:.4f}, over {f['over']}" for n, f in figs.items())
    return (f"SWEEP {row['id']} | pixels {pixels} | {row['variant']} | oracle {oracle_s:.1f} core-s, wall {wall:.1f} s | "
            f"figures compared {compared} | mismatches {bad} | {fig}")


# ---- BT.2124 in binary64 --------------------------------------------------------------------------------------------------
DECIMAL = {BT2020NC: ("1.4746", "1.8814", "0.16455313", "0.57135313"), BT709: ("1.5748", "1.8556", "0.18732427", "0.46812427")}


def normalise_exact(code, depth, full, chroma):
    """(code - sub) / div, the quotient of two integers rounded once to binary64"""
    s = 1 << (depth - 8)
    if full:
        sub, div = ((1 << (depth - 1)) if chroma else 0), (1 << depth) - 1
    else:
        sub, div = (128 * s, 224 * s) if chroma else (16 * s, 219 * s)
    return (np.asarray(code).astype(np.int64) - sub).astype(np.float64) / float(div)


def itp_exact(planes444, depth, full, matrix):
    """(I, T, P) of three flat code planes by BT.2100 and BT.2124 in binary64: the primes clipped to [0, 1], the PQ EOTF, LMS, the PQ
    inverse EOTF, I, T = Ct / 2, P = Cp"""
    y = normalise_exact(planes444[0], depth, full, False)
    if matrix == GBR:
        g, b, r = y, normalise_exact(planes444[1], depth, full, False), normalise_exact(planes444[2], depth, full, False)
    else:
        rv, bu, gu, gv = (float(Fraction(s)) for s in DECIMAL[matrix])
        cb, cr = normalise_exact(planes444[1], depth, full, True), normalise_exact(planes444[2], depth, full, True)
        r, b, g = y + rv * cr, y + bu * cb, y - gu * cb - gv * cr
    g, b, r = (ir.pq_eotf_exact(np.clip(v, 0.0, 1.0)) for v in (g, b, r))
    lp, mp, sp = (ir.pq_exact((kr * r + kg * g + kb * b) / der.LMS_DEN) for kr, kg, kb in der.LMS_NUM)
    t = (der.T_NUM[0] * lp - der.T_NUM[1] * mp + der.T_NUM[2] * sp) / der.T_DEN
    p = (der.P_NUM[0] * lp - der.P_NUM[1] * mp - der.P_NUM[2] * sp) / der.P_DEN
    return 0.5 * lp + 0.5 * mp, t, p


def d_exact(a, b, depth, full, matrix):
    """a plain Euclidean distance of the two sides' (I, T, P), times 720, in binary64"""
    ia, ib = itp_exact(a, depth, full, matrix), itp_exact(b, depth, full, matrix)
    return 720.0 * np.sqrt(sum((x - y) ** 2 for x, y in zip(ia, ib)))


def accuracy(d32, d64):
    """(largest |d - d64|, largest |d - d64| / d64 over the pixels with d64 >= the threshold)"""
    err = np.abs(d32.astype(np.float64) - d64)
    big = d64 >= THRESHOLD
    return float(err.max()), float((err[big] / d64[big]).max()) if big.any() else 0.0


# The restatement's per-pixel d against d_exact over every pair of E0 and E1, as measured (never against the kernel): (absolute,
# relative).  The tests assert 1.25 times these; the quarter allows for another libm.
MEASURED = {  # row: (absolute, relative), the largest over the row's pairs
    "E0/BT709/cb": (7.278e-04, 5.476e-04),
    "E0/BT709/cr": (8.654e-04, 6.357e-04),
    "E0/BT2020NC/cb": (7.729e-04, 6.338e-04),
    "E0/BT2020NC/cr": (8.094e-04, 6.403e-04),
    "E1/BT709/video/0": (7.525e-05, 2.713e-05),
    "E1/BT709/video/1": (7.216e-04, 4.446e-05),
    "E1/BT709/video/2": (6.669e-04, 3.250e-04),
    "E1/BT709/video/3": (7.089e-04, 4.609e-04),
    "E1/BT709/video/4": (1.054e-04, 6.838e-05),
    "E1/BT709/full/0": (7.312e-05, 1.526e-05),
    "E1/BT709/full/1": (6.808e-04, 4.805e-05),
    "E1/BT709/full/2": (6.825e-04, 3.528e-04),
    "E1/BT709/full/3": (7.429e-04, 3.959e-04),
    "E1/BT709/full/4": (7.999e-05, 1.526e-05),
    "E1/BT2020NC/video/0": (7.525e-05, 2.713e-05),
    "E1/BT2020NC/video/1": (6.650e-04, 5.811e-05),
    "E1/BT2020NC/video/2": (7.288e-04, 4.689e-04),
    "E1/BT2020NC/video/3": (7.150e-04, 5.001e-04),
    "E1/BT2020NC/video/4": (7.765e-05, 2.713e-05),
    "E1/BT2020NC/full/0": (7.312e-05, 1.526e-05),
    "E1/BT2020NC/full/1": (6.564e-04, 5.646e-05),
    "E1/BT2020NC/full/2": (6.082e-04, 4.219e-04),
    "E1/BT2020NC/full/3": (6.069e-04, 4.412e-04),
    "E1/BT2020NC/full/4": (1.098e-04, 3.582e-05),
}
