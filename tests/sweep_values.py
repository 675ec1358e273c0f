"""Value sweeps: lists of input values (as bit patterns), their arrangement into frames, and the conditions a sweep must
meet to count.  Plain numpy; tests/test_sweep_values.py checks this file without a GPU, tests/test_value_sweeps.py runs
the sweeps through the forward kernels.

A value list is a 1-D array of bit patterns: uint32 for binary32 input, uint16 for half and for integer input.  An
arrangement (Sweep) lays a list out into frames of W x H; frame k is made when asked for, so a sweep of 2^28 values never
holds more than the list itself and one batch of frames."""
from __future__ import annotations

import numpy as np

FULL_W, FULL_H = 4096, 2048  # 2^23 pixels: one binade of binary32 per frame

T1_LO, T1_HI = 0x33000000, 0x40800000    # [2^-25, 4): the first tier's domain and a binade either side
T1N_LO, T1N_HI = 0x33800000, 0x41000000  # [2^-24, 8): the same after (x - 0) / 2


# ---- value lists -----------------------------------------------------------------------------------------------------
def float_range(lo_bits: int, hi_bits: int, stride: int = 1) -> np.ndarray:
    """The binary32 bit patterns lo_bits, lo_bits + stride, ... below hi_bits."""
    if hi_bits <= 0xFFFFFFFF:
        return np.arange(lo_bits, hi_bits, stride, dtype=np.uint32)
    return np.arange(lo_bits, hi_bits, stride, dtype=np.int64).astype(np.uint32)


def all_halves() -> np.ndarray:
    return np.arange(65536, dtype=np.uint32).astype(np.uint16)


def all_codes(depth: int) -> np.ndarray:
    return np.arange(1 << depth, dtype=np.uint32).astype(np.uint16)


def f32_bits(x: float) -> int:
    return int(np.float32(x).view(np.uint32))


def around(bits: int, ulps: int) -> np.ndarray:
    """Every pattern within `ulps` of `bits` on the integer line of patterns (wrapping below 0 into the other sign)."""
    return ((np.arange(-ulps, ulps + 1, dtype=np.int64) + bits) & 0xFFFFFFFF).astype(np.uint32)


def special_floats(stride: int = 1021, ulps: int = 64) -> np.ndarray:
    """F7: every stride-th of all 2^32 patterns (both signs, subnormals, infinities, quiet and signalling NaNs) and every
    float within `ulps` of 0, +-2^-126, 2^-25, 2^-24, 1, 1 + 2^-8, 2, 4, +-inf (below +0 the patterns wrap to the largest
    negative NaNs, below -0 they are the largest positive NaNs: both belong to the list)."""
    parts = [float_range(0, 1 << 32, stride)]
    for x in (0.0, 2.0 ** -126, -(2.0 ** -126), 2.0 ** -25, 2.0 ** -24, 1.0, 1.0 + 2.0 ** -8, 2.0, 4.0, np.inf, -np.inf):
        parts.append(around(f32_bits(x), ulps))
    parts.append(around(0x80000000, ulps))  # -0
    return np.concatenate(parts)


PQ_F_KINK = 0.8359375 ** 78.84375  # PQ10000_f: max(V^(1/m2) - c1, 0) leaves zero here


def pair_source_values(src_transfer: int, stride: int = 3, near: int = 1 << 16) -> np.ndarray:
    """P: the source domain of a transfer pair.  PQ source (16): every float of [2^-12, 1].  Others: [2^-25, 2) at the odd
    `stride`, plus every float within `near` patterns of each power of two of the domain and of PQ10000_f's kink."""
    if src_transfer == 16:
        return float_range(f32_bits(2.0 ** -12), f32_bits(1.0) + 1)
    assert stride % 2 == 1
    parts = [float_range(f32_bits(2.0 ** -25), f32_bits(2.0), stride)]
    for e in range(-25, 2):
        parts.append(around(f32_bits(2.0 ** e), near))
    parts.append(around(f32_bits(PQ_F_KINK), near))
    return np.concatenate(parts)


# ---- arrangements ----------------------------------------------------------------------------------------------------
ARRANGEMENTS = ("grey", "rot", "blocks", "thirds")


def frame_shape(n_pixels: int):
    """W x H for a list that fills n_pixels: the full frame where the list is long, else 256 wide and as high as it takes."""
    if n_pixels >= FULL_W * FULL_H:
        return FULL_W, FULL_H
    w = 256 if n_pixels <= 256 * FULL_H else FULL_W
    rows = -(-n_pixels // w)
    return w, max(4, rows + (-rows) % 4)


class Sweep:
    """A value list laid out into frames.

    grey:   all three planes are the list (planes() returns one array three times).
    rot:    plane c is the list rotated by c thirds of its length.
    blocks: rot at half the width and height, every pixel repeated over a 2 x 2 block.
    thirds: plane c is the c-th third of the list (an identity matrix keeps the planes apart, so one frame carries three
            values per pixel; the list's length must be a multiple of 3).
    The last frame is padded by repeating the last value of each plane's (rotated) list."""

    def __init__(self, values: np.ndarray, arrangement: str, width: int | None = None, height: int | None = None):
        assert arrangement in ARRANGEMENTS and values.ndim == 1 and values.size > 0
        self.values, self.arrangement = values, arrangement
        n = values.size
        self.length = n // 3 if arrangement == "thirds" else n  # entries of one plane's list
        if arrangement == "thirds":
            assert n % 3 == 0
        px = 4 if arrangement == "blocks" else 1
        if width is None:
            width, height = frame_shape(self.length * px)
        if arrangement == "blocks":
            assert width % 4 == 0 and height % 4 == 0
        self.width, self.height = width, height
        self.per_frame = width * height // px  # list entries one frame holds
        self.n_frames = -(-self.length // self.per_frame)
        if arrangement == "grey":
            self.starts = (0, 0, 0)
        elif arrangement == "thirds":
            self.starts = (0, self.length, 2 * self.length)
        else:
            self.starts = (0, n // 3, 2 * (n // 3))

    def _run(self, c: int, first: int, count: int) -> np.ndarray:
        """Entries [first, first + count) of plane c's list, padded with its last entry."""
        v, n = self.values, self.values.size
        real = max(0, min(count, self.length - first))
        if self.arrangement == "thirds":
            out = v[self.starts[c] + first:self.starts[c] + first + real]
        else:
            a = (self.starts[c] + first) % n
            out = v[a:a + real] if a + real <= n else np.concatenate((v[a:], v[:a + real - n]))
        if real < count:
            last = v[(self.starts[c] + self.length - 1) % n]
            out = np.concatenate((out, np.full(count - real, last, dtype=v.dtype)))
        return np.ascontiguousarray(out)

    def planes(self, k: int):
        """Frame k: three flat arrays of width x height bit patterns (grey: the same array three times)."""
        assert 0 <= k < self.n_frames
        first = k * self.per_frame
        if self.arrangement == "grey":
            p = self._run(0, first, self.per_frame)
            return [p, p, p]
        out = [self._run(c, first, self.per_frame) for c in range(3)]
        if self.arrangement == "blocks":
            w2, h2 = self.width // 2, self.height // 2
            out = [np.ascontiguousarray(np.repeat(np.repeat(p.reshape(h2, w2), 2, axis=0), 2, axis=1)).reshape(-1) for p in out]
        return out

    def pixel(self, k: int, y: int, x: int):
        """The three input bit patterns of pixel (x, y) of frame k."""
        if self.arrangement == "blocks":
            i = k * self.per_frame + (y // 2) * (self.width // 2) + x // 2
        else:
            i = k * self.per_frame + y * self.width + x
        n = self.values.size
        i = min(i, self.length - 1)
        if self.arrangement == "thirds":
            return tuple(int(self.values[s + i]) for s in self.starts)
        return tuple(int(self.values[(s + i) % n]) for s in self.starts)

    def real_pixels(self, k: int) -> int:
        """Pixels of frame k before the padding."""
        px = 4 if self.arrangement == "blocks" else 1
        return max(0, min(self.per_frame, self.length - k * self.per_frame)) * px


def plane_sizes(width: int, height: int, chroma_420: bool):
    nc = (width >> 1) * (height >> 1) if chroma_420 else width * height
    return width * height, nc, nc


def report(sweep: Sweep, chroma_420: bool, got, want, first_frame: int = 0) -> str:
    """got, want: one output frame each per entry (Y | Cb | Cr, flat u16), for frames first_frame, first_frame + 1, ...
    Empty string when they agree; else the count and the first eight differing samples as plane, frame, index, the input
    bit patterns (G, B, R) of the pixel (4:2:0 chroma: of the top left pixel of the sample's 2 x 2 block), got, want."""
    ny, nc, _ = plane_sizes(sweep.width, sweep.height, chroma_420)
    total, lines = 0, []
    hexw = 8 if sweep.values.dtype == np.uint32 else 4
    for j, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g).reshape(-1), np.asarray(w).reshape(-1)
        assert g.size == w.size == ny + 2 * nc, (g.size, w.size, ny, nc)
        if np.array_equal(g, w):
            continue
        bad = np.flatnonzero(g != w)
        total += bad.size
        for s in bad[:max(0, 8 - len(lines))]:
            s = int(s)
            plane = 0 if s < ny else 1 if s < ny + nc else 2
            idx = s - (0, ny, ny + nc)[plane]
            if plane and chroma_420:
                y, x = 2 * (idx // (sweep.width >> 1)), 2 * (idx % (sweep.width >> 1))
            else:
                y, x = idx // sweep.width, idx % sweep.width
            pix = sweep.pixel(first_frame + j, y, x)
            lines.append(f"plane {plane} frame {first_frame + j} index {idx} input (" + ", ".join(f"0x{b:0{hexw}x}" for b in pix) +
                         f") got {int(g[s])} want {int(w[s])}")
    if not total:
        return ""
    return f"{total} samples differ ({sweep.arrangement}, {sweep.values.size} values); first:\n  " + "\n  ".join(lines)


# ---- conditions ------------------------------------------------------------------------------------------------------
def luma_limits(depth: int, full_range: int):
    """The ends of the luma range write_yuv clamps to (reference: video range 16 D .. 235 D, full range 0 .. 2^depth - 1)."""
    if full_range:
        return 0, (1 << depth) - 1
    return 16 << (depth - 8), 235 << (depth - 8)


def chroma_top(depth: int, full_range: int) -> int:
    return (1 << depth) - 1 if full_range else 240 << (depth - 8)


MAX_CLAMPED_LUMA = 0.12  # share of luma samples on either end of the range


def max_clamped_cr(full_range: int, matrix: int) -> float:
    """Share of Cr / Dx samples a rot or blocks sweep may hold at the top of the chroma range: 8 % (the oracle gives 2.9 %
    for BT.2020nc at full range, 7.5 % at video range, 5.1 % for YDzDx at full range).  YDzDx at video range: 10 %.  The
    reference scales chroma by 240 D there as it scales luma by 235 D, Dx = (R' - G') / 2 has no divisor above one to pull
    it back as Cr has (1.4746), and so it clips from R' - G' = 0.93 up instead of never: the oracle gives 9.3 %, a share
    that is a property of the pairing of magnitudes in rot, not of the kernel."""
    return 0.10 if matrix == 11 and not full_range else 0.08


def min_codes(depth: int, full_range: int, matrix: int, arrangement: str):
    """Distinct luma codes a sweep of [2^-25, 4) must reach (None: no figure set for this form).

    16-bit: 65 000 for a full-range grey, YDzDx (11) or GBR (0) sweep (the oracle gives 65 329 - 65 330); 49 000 for the
    others (BT.2020nc / BT.709 rot: 54 052 full, 49 749 video; grey at video range: 55 874).
    12-bit: 3 300 (3 378 rot, 4 083 grey at full range; YDzDx blocks at video range, whose luma is G' alone: 3 494, and
    13 970 of 14 bits).  A BT.2020nc or BT.709 rot or blocks sweep at video range cannot reach it: luma clips from x = 0.53
    up there, such a sweep reaches 49 749 codes of 16 bits and so 49 749 / 16 = 3 109 of 12 (F6: 3 110, F3: 3 147) whatever
    the kernel does; for those forms alone the bound is the 16-bit one in 12-bit codes, 49 000 / 16 = 3 062.
    14-bit: four times the 12-bit bound less 2 %.  10-bit: 780."""
    if depth == 16:
        return 65000 if full_range and (arrangement == "grey" or matrix in (0, 11)) else 49000
    twelve = 3300 if full_range or arrangement == "grey" or matrix in (0, 11) else 49000 // 16
    return {14: int(4 * twelve * 0.98), 12: twelve, 10: 780}.get(depth)


def _to_linear(tf: int, v):
    """Textbook transfer functions in binary64 (8 linear, 16 PQ, 18 rho-gamma with rho 25 and gamma 2.4, 1 BT.1886)."""
    v = np.asarray(v, np.float64)
    if tf == 16:
        p = v ** (1.0 / 78.84375)
        return (np.maximum(p - 0.8359375, 0.0) / (18.8515625 - 18.6875 * p)) ** (1.0 / 0.1593017578125)
    if tf == 18:
        return ((25.0 ** v - 1.0) / 24.0) ** 2.4
    return v ** 2.4 if tf == 1 else v


# P: what the conditions ask of each transfer pair's two forms, (largest bottom share of luma, fewest distinct luma codes).
# The issue's figures -- 12 % on either end; 65 000 codes of a 16-bit full-range grey sweep, 3 300 of a 12-bit one -- stand
# wherever the pair's own arithmetic lets them: the comment beside each other figure is what the oracle gives on the
# stride-64 subsample of the list (the full list gives the same shares and at least as many codes), and the bound is that
# share plus one point, or that count less 2 %.  PQ -> LINEAR sends every PQ value below 0.15 under 10000 / 65535 nit, the
# first 16-bit code; x^2.4 (BT.1886, rho-gamma) of a float below 2^-12 is below PQ's first code; and a 12-bit video-range rot
# sweep has 3 504 luma codes in all, of which a pair whose output crowds towards one end reaches fewer than LINEAR -> PQ does.
P_BOUNDS = {
    (16, 8): dict(grey=(0.66, 50600), rot=(0.51, 2499)),    # grey 64.8 %, 51 679 (full list: 65 536); rot 49.4 %, 2 550
    (8, 1): dict(grey=(0.12, 65000), rot=(0.12, 3300)),     # 65 500; 3 457
    (1, 16): dict(grey=(0.29, 65000), rot=(0.12, 2944)),    # grey 28.0 %, 65 536; rot 0 %, 3 005
    (16, 1): dict(grey=(0.12, 65000), rot=(0.12, 2503)),    # 65 527; 2 555
    (18, 16): dict(grey=(0.40, 65000), rot=(0.12, 3300)),   # grey 39.2 %, 65 536; rot 0.6 %, 3 505
    (8, 18): dict(grey=(0.12, 65000), rot=(0.12, 2856)),    # 65 182; 2 915
    (16, 18): dict(grey=(0.12, 65000), rot=(0.12, 2526)),   # 65 479; 2 578
}


def cast_undefined_halves() -> np.ndarray:
    """Mask over all_halves(): the PQ code values V in (1, 1.992) whose linear light PQ10000_f(V), scaled to 16-bit codes,
    is 2^31 or more.  PQ10000_f has a pole at V = 1.99206 (18.8515625 - 18.6875 V^(1/m2) = 0); below it the value grows past
    every integer, and the reference's (unsigned int) cast of a float of 2^31 or more is undefined in C (its x86-64 build
    keeps the low word of a 64-bit conversion: zero from 2^55 up; the kernels' converts saturate).  260 patterns,
    0x3EF4 .. 0x3FF7.  Beyond the pole the quotient is negative, pow() gives NaN, and NaN is compared like any value."""
    v = all_halves().view(np.float16).astype(np.float64)
    with np.errstate(all="ignore"):
        lin = _to_linear(16, v)
    return (v > 1.0) & np.isfinite(lin) & (lin * 65535.0 >= 2.0 ** 31)


class Conditions:
    """Accumulates over the frames of `want` what the conditions need; check() asserts them."""

    def __init__(self, sweep: Sweep, depth: int, full_range: int, matrix: int, chroma_420: bool, codes=True, label: str = "",
                 max_low: float = MAX_CLAMPED_LUMA):
        """codes: True -- min_codes() of the form; an integer -- that many (the transfer pairs' own floors, P_BOUNDS)."""
        self.sweep, self.depth, self.full, self.matrix, self.c420 = sweep, depth, full_range, matrix, chroma_420
        self.seen = np.zeros(1 << 16, dtype=bool)
        self.n_luma = self.at_lo = self.at_hi = self.n_cr = self.cr_top = 0
        self.codes, self.label, self.max_low = codes, label, max_low

    def add(self, k: int, frame: np.ndarray) -> None:
        ny, nc, _ = plane_sizes(self.sweep.width, self.sweep.height, self.c420)
        real = self.sweep.real_pixels(k)  # padding repeats one value: it would only inflate a share
        luma = frame[:real]
        lo, hi = luma_limits(self.depth, self.full)
        if self.matrix == 0:  # GBR: all three planes are "luma"
            luma = np.concatenate([frame[c * ny:c * ny + real] for c in range(3)])
        self.seen[luma] = True
        self.n_luma += luma.size
        self.at_lo += int(np.count_nonzero(luma <= lo))
        self.at_hi += int(np.count_nonzero(luma >= hi))
        if self.matrix != 0 and self.sweep.arrangement != "grey":
            cr = frame[ny + nc:ny + nc + (real // 4 if self.c420 else real)]
            self.n_cr += cr.size
            self.cr_top += int(np.count_nonzero(cr >= chroma_top(self.depth, self.full)))

    def figures(self) -> dict:
        return {"luma": self.n_luma, "at_low": self.at_lo / max(self.n_luma, 1), "at_high": self.at_hi / max(self.n_luma, 1),
                "cr_top": self.cr_top / max(self.n_cr, 1), "codes": int(np.count_nonzero(self.seen))}

    def check(self) -> dict:
        f = self.figures()
        assert f["at_low"] <= self.max_low and f["at_high"] <= MAX_CLAMPED_LUMA, (self.label, f)
        assert f["cr_top"] <= max_clamped_cr(self.full, self.matrix), (self.label, f)
        need = min_codes(self.depth, self.full, self.matrix, self.sweep.arrangement) if self.codes is True else self.codes
        if need is not None:
            assert f["codes"] >= need, (self.label, f, need)
        return f


# ---- the sweeps of tests/test_value_sweeps.py ------------------------------------------------------------------------
# A row: id, descriptor keywords (make_desc's; "depths": the candidates of a "deepest" row, tried in turn on the device),
# the value list (lo, hi, and the stride of each arrangement), and the kernel forms that must each be reached:
# (context options, kernel name, substrings of the variant).  One oracle result serves every form of a row.
GBR, BT709, BT2020NC, YDZDX = 0, 1, 9, 11
IDENT, HALF = [(0, 1)] * 3, [(0, 2)] * 3
DEEPEST = (16, 14, 12)
F_SWEEPS = [
    dict(id="F1", kw=dict(dst_matrix=BT2020NC, full_range=1, chroma=1, resampler=0, stats=IDENT), depths=DEEPEST,
         bits=(T1_LO, T1_HI), arrangements=dict(grey=1, blocks=3),
         forms=[(dict(t1="always"), "k_fused_t1", ("PQ_IDENT",)), (dict(t1="0"), "k_fused2", ("PQ_IDENT",))]),
    dict(id="F2full", kw=dict(dst_matrix=BT2020NC, dst_depth=16, full_range=1, chroma=3, resampler=0, stats=IDENT),
         bits=(T1_LO, T1_HI), arrangements=dict(grey=1, rot=1), forms=[(dict(), "k_fused2", ("PQ_IDENT",))]),
    dict(id="F2video", kw=dict(dst_matrix=BT2020NC, dst_depth=16, full_range=0, chroma=3, resampler=0, stats=IDENT),
         bits=(T1_LO, T1_HI), arrangements=dict(grey=1, rot=1), forms=[(dict(), "k_fused2", ("PQ_IDENT",))]),
    dict(id="F3", kw=dict(dst_matrix=BT709, full_range=0, chroma=1, resampler=1, stats=IDENT), depths=DEEPEST,
         bits=(T1_LO, T1_HI), arrangements=dict(rot=1),
         forms=[(dict(t1="always", fir="fused"), "k_fir_fused", ("PQ_IDENT",)),
                (dict(t1="always", fir="twopass"), "k_fused_t1", ("PQ_IDENT", "+k_fir420"))]),
    dict(id="F4full", kw=dict(dst_matrix=YDZDX, dst_depth=16, full_range=1, chroma=3, resampler=0, stats=IDENT),
         bits=(T1_LO, T1_HI), arrangements=dict(rot=1), forms=[(dict(), "k_fused2", ("YDZDX", "PQ_IDENT"))]),
    dict(id="F4video", kw=dict(dst_matrix=YDZDX, full_range=0, chroma=1, resampler=0, stats=IDENT), depths=DEEPEST,
         bits=(T1_LO, T1_HI), arrangements=dict(blocks=3), forms=[(dict(t1="always"), "k_fused_t1", ("YDZDX", "PQ_IDENT"))]),
    dict(id="F6", kw=dict(dst_matrix=BT2020NC, dst_depth=12, full_range=0, chroma=1, resampler=0, stats=HALF),
         bits=(T1N_LO, T1N_HI), arrangements=dict(rot=1),
         forms=[(dict(t1="always"), "k_fused_t1", ("PQ_NORM",)), (dict(t1="0"), "k_fused2", ("PQ_NORM",))]),
]
# F5: the GBR identity, the three planes holding three different thirds of the list; the geometries pick the kernel
F5_KW = dict(dst_matrix=GBR, dst_depth=16, full_range=1, chroma=3, resampler=0, stats=IDENT)
F5_GEOMETRIES = [(FULL_W, FULL_H, "k_fused"), (FULL_W, FULL_H - 1, "k_fused"), (FULL_W - 6, FULL_H, "k_fused_narrow")]
# P: the other transfer pairs, each grey at 16-bit full range 4:4:4 and rot at 12-bit video range 4:2:0 box
P_PAIRS = [(16, 8), (8, 1), (1, 16), (16, 1), (18, 16), (8, 18), (16, 18)]
P_FORMS = [("grey", dict(dst_matrix=BT2020NC, dst_depth=16, full_range=1, chroma=3, resampler=0, stats=IDENT)),
           ("rot", dict(dst_matrix=BT2020NC, dst_depth=12, full_range=0, chroma=1, resampler=0, stats=IDENT))]
P_STRIDE = 3  # the odd stride of the non-PQ sources: the only figure the time rule may raise


def f_cases():
    """(row, arrangement, stride) for every F1-F4, F6 sweep."""
    return [(row, arr, stride) for row in F_SWEEPS for arr, stride in row["arrangements"].items()]


def subsample(values: np.ndarray, step: int = 64) -> np.ndarray:
    """Every step-th value, cut to a multiple of 3 so that every arrangement takes it."""
    v = values[::step]
    return v[:v.size - v.size % 3]


# ---- the oracle over a sweep -----------------------------------------------------------------------------------------
def workers() -> int:
    import os

    return min(16, int(os.environ.get("OMP_NUM_THREADS", "8")))


def as_input(planes, f32: bool):
    """Bit patterns -> what convert_frame takes (binary32 planes keep every payload: a view, no arithmetic)."""
    return [p.view(np.float32) for p in planes] if f32 else planes


def oracle_frames(convert, desc_for, sweep: Sweep, frames, f32: bool = True, pool=None):
    """[convert(desc_for(sweep), planes of frame k) for k in frames], on `pool` (a ThreadPoolExecutor; ctypes releases the
    GIL) when given."""
    d = desc_for(sweep.width, sweep.height)

    def one(k):
        return convert(d, as_input(sweep.planes(k), f32))

    return list(pool.map(one, frames)) if pool is not None else [one(k) for k in frames]
