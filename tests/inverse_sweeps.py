"""Inverse sweeps: code triples (Y, Cb, Cr) for the .yuv -> RGB kernels, their arrangement into frames, and the conditions a
sweep must meet to count.  Plain numpy; tests/test_inverse_sweeps.py checks this file without a GPU,
tests/test_inverse_value_sweeps.py runs the sweeps through inverse_pixel (k_inverse, k_inverse_batch, k_inverse420<REPLICATE>,
k_inverse420_batch<REPLICATE>).

Why 12-bit planes and not 8- or 10-bit cubes.  matrix_inverse keeps Half = 2048 and Full = 4096 at every bit depth, so its
arithmetic is made for 12-bit codes.  Over ALL 2^24 triples of 8-bit input and ALL 2^30 of 10-bit input, B and R come out as
one single code, for matrix 1 and for Y'DzDx, and the BT.709 G sits on a limit for 100 % (8-bit), 96.6 % (10-bit video) and
93.0 % (10-bit full) of the cube; 10-bit video G reaches 269 of its 877 legal codes.  With uniform 16-bit codes 99.6 % of B is
clamped at 4095, and at video range minVR = 4096 then lifts every BT.709 output to one constant.  Only 12-bit input (24.5 % of
uniform triples pass without any clamp) shows the matrix.  An exhaustive 8- or 10-bit cube would be 2^24 / 2^30 comparisons
of clamps and shifts: do not add one as "coverage".

A plane frame is 4096 x 4096: pixel (r, c) holds Y = r, one chroma plane holds c, the other a constant of S.  Eight frames
with Cr fixed hold every (Y, Cb), eight with Cb fixed every (Y, Cr): B depends on (Y, Cb) alone and R on (Y, Cr) alone, so
the sixteen frames are exhaustive for B and R at 12 bits, and sixteen dense cuts through the cube for G.  The blocks layout is
the same set of triples as 4:2:0 input (luma 4096 x 4096, chroma 2048 x 2048) whose replication makes every pixel a function
of one triple."""
from __future__ import annotations

import numpy as np

N = 4096
S = (0, 256, 1024, 2047, 2048, 3072, 3760, 4095)
BT709, BT2020NC, YDZDX = 1, 9, 11
PLANE_NAMES = ("G", "B", "R")


def limits(depth: int, full_range: int):
    """minVR, maxVR of matrix_inverse's clamp: the INPUT picture's (a full-range input: 0 and maxCV)."""
    if full_range:
        return 0, (1 << depth) - 1
    return 16 << (depth - 8), 235 << (depth - 8)


# ---- arrangements ----------------------------------------------------------------------------------------------------
def plane_frames(consts=S):
    """The sixteen frames of a 12-bit row: (which chroma plane varies, the other's constant, a, b)."""
    return [("cb", s, 0, 0) for s in consts] + [("cr", s, 0, 0) for s in consts]


class PlaneSweep:
    """Frames of N x N pixels over (Y, C) planes.

    layout "plane":  Y[r, c] = scale r + a, the varying chroma plane = scale c + b, the fixed one = scale s.
    layout "blocks": 4:2:0.  Chroma sample (i, j) of the varying plane = j + 2048 (i mod 2); the four luma pixels of block
                     (i, j) hold Y = 4 (i div 2) + 0 .. 3; the fixed plane is s.  Every (Y, C) pair occurs exactly once.
    A plane is made once per key (what it holds) and shared by the frames that use it: planes() of two frames may return
    the same array, nothing writes to them."""

    def __init__(self, frames, layout: str = "plane", scale: int = 1, rows=None):
        assert layout in ("plane", "blocks") and (layout == "plane" or scale == 1)
        self.frames, self.layout, self.scale = list(frames), layout, scale
        self.n_frames = len(self.frames)
        self.c420 = layout == "blocks"
        # rows: the luma rows kept (a subsample for the CPU tests); whole 4-row groups for blocks, so that chroma rows pair up
        self.rows = np.arange(N) if rows is None else np.asarray(rows)
        self.width, self.height = N, self.rows.size
        assert not self.c420 or (self.height % 4 == 0 and np.all(self.rows.reshape(-1, 4) % 4 == np.arange(4)))
        self._cache = {}

    def subsampled(self, step: int = 16) -> "PlaneSweep":
        """Every step-th row (blocks: every step-th group of four luma rows, two chroma rows), still full rows."""
        rows = np.arange(N)
        rows = rows[(rows // 4) % step == 0] if self.c420 else rows[::step]
        return PlaneSweep(self.frames, self.layout, self.scale, rows)

    def keys(self, k: int):
        """What the three planes (Y, Cb, Cr) of frame k hold."""
        fam, s, a, b = self.frames[k]
        var, fix = ("C", b), ("K", s)
        return [("Y", a), var, fix] if fam == "cb" else [("Y", a), fix, var]

    def plane(self, key) -> np.ndarray:
        if key not in self._cache:
            kind, v = key
            r = self.rows
            if self.layout == "plane":
                if kind == "Y":
                    p = np.repeat((self.scale * r + v).astype(np.uint16), N)
                elif kind == "C":
                    p = np.tile((self.scale * np.arange(N) + v).astype(np.uint16), r.size)
                else:
                    p = np.full(r.size * N, self.scale * v, np.uint16)
            else:
                if kind == "Y":
                    p = (4 * (r // 4) + 2 * (r % 2))[:, None] + (np.arange(N) % 2)[None, :]
                elif kind == "C":
                    i = r[::2] // 2
                    p = np.arange(N // 2)[None, :] + (N // 2) * (i % 2)[:, None]
                else:
                    p = np.full((r.size // 2) * (N // 2), v)
                p = np.ascontiguousarray(p, dtype=np.uint16).reshape(-1)
            p.setflags(write=False)
            self._cache[key] = p
        return self._cache[key]

    def planes(self, k: int):
        return [self.plane(key) for key in self.keys(k)]

    def triple(self, k: int, idx: int):
        """(Y, Cb, Cr) that output sample idx of frame k is a function of."""
        r, c = divmod(idx, self.width)
        ci = (r // 2) * (self.width // 2) + c // 2 if self.c420 else idx
        y, cb, cr = self.planes(k)
        return int(y[idx]), int(cb[ci]), int(cr[ci])


def i5_frames():
    """I5: 16-bit codes Y = 16 i + a, C = 16 j + b for three (a, b), three constants 16 s each, the varying plane alternating."""
    picks = {(0, 0): (0, 2048, 4095), (15, 15): (256, 2047, 3760), (7, 8): (1024, 3072, 2048)}
    out = []
    for (a, b), consts in picks.items():
        for s in consts:
            out.append(("cb" if len(out) % 2 == 0 else "cr", s, a, b))
    return out


def report(triple_of, got, want, first_frame: int = 0, frames=None) -> str:
    """got, want: per frame three planes (G, B, R), for frames first_frame, first_frame + 1, ... (or those listed in `frames`).
    Empty when equal, else the count and the first eight differing samples as frame, plane, index, the triple (Y, Cb, Cr),
    got, want.  triple_of(frame, index) names the triple."""
    total, lines = 0, []
    for j, (g3, w3) in enumerate(zip(got, want)):
        k = first_frame + j if frames is None else frames[j]
        for c in range(3):
            g, w = np.asarray(g3[c]).reshape(-1), np.asarray(w3[c]).reshape(-1)
            assert g.size == w.size, (g.size, w.size)
            if np.array_equal(g, w):
                continue
            bad = np.flatnonzero(g != w)
            total += bad.size
            for s in bad[:max(0, 8 - len(lines))]:
                y, cb, cr = triple_of(k, int(s))
                lines.append(f"frame {k} plane {PLANE_NAMES[c]} index {int(s)} triple (Y {y}, Cb {cb}, Cr {cr}) got {int(g[s])} want {int(w[s])}")
    if not total:
        return ""
    return f"{total} samples differ; first:\n  " + "\n  ".join(lines)


# ---- conditions ------------------------------------------------------------------------------------------------------
def histograms(planes3) -> np.ndarray:
    """(3, 65536) counts of the codes of one frame's G, B, R."""
    return np.stack([np.bincount(np.asarray(p).reshape(-1), minlength=65536) for p in planes3])


class Conditions:
    """Accumulates the histograms of the EXPECTED output (the oracle's, never the GPU's); check() asserts that every plane
    reaches every code of `codes` (counted before the left shift) and holds at most caps[plane] of its samples on minVR or
    maxVR (after the clamp)."""

    def __init__(self, in_depth: int, full_range: int, out_depth: int, codes, caps, label: str = ""):
        assert out_depth >= in_depth  # a right shift folds codes together: such a row is asked no conditions
        self.shift = out_depth - in_depth
        self.lo, self.hi = limits(in_depth, full_range)
        self.codes, self.caps, self.label = codes, caps, label
        self.hist = np.zeros((3, 65536), np.int64)

    def add(self, hist3) -> None:
        self.hist += hist3

    def figures(self) -> dict:
        total = self.hist.sum(axis=1)
        at = self.hist[:, self.lo << self.shift] + (self.hist[:, self.hi << self.shift] if self.hi != self.lo else 0)
        want = np.arange(self.codes[0], self.codes[1] + 1) << self.shift
        return {"at_limit": [round(float(a) / max(int(t), 1), 4) for a, t in zip(at, total)],
                "codes": [int(np.count_nonzero(self.hist[c, want])) for c in range(3)], "of": int(want.size)}

    def check(self) -> dict:
        f = self.figures()
        assert f["codes"] == [f["of"]] * 3, (self.label, f)
        assert all(a <= cap for a, cap in zip(f["at_limit"], self.caps)), (self.label, f, self.caps)
        return f


# The share of samples on a limit that the ORACLE gives for the sixteen frames of a row as built above (G, B, R), derived by
# tests/test_inverse_sweeps.py::test_conditions_of_the_plane_rows, which fails if a figure here is not the oracle's to the
# fourth decimal.  Half of a (Y, C) square is out of gamut by construction, so no fixed small cap is possible: the cap is the
# oracle's own share plus one point (the margin rule of sweep_values.P_BOUNDS).
ORACLE_SHARE = {
    "709_video": (0.2573, 0.5874, 0.5118),
    "709_full": (0.1524, 0.5054, 0.4289),
    "ydzdx_video": (0.1448, 0.6168, 0.6168),
    "ydzdx_full": (0.0005, 0.5447, 0.5447),
    "709_14_full": (0.0675, 0.2539, 0.2155),  # I4: limits 0 and 16383 / 65535, so only the samples at 0 count
    "709_16_full": (0.0675, 0.2539, 0.2155),
}
MARGIN = 0.01
CAPS = {k: tuple(round(x + MARGIN, 4) for x in v) for k, v in ORACLE_SHARE.items()}

# ---- the rows of tests/test_inverse_value_sweeps.py ----------------------------------------------------------------
# id -> matrix, in depth, in full range, out depth, layout, entry ("batch": h2y_inverse_batch, "single": h2y_matrix_inverse),
# the key of ORACLE_SHARE / CAPS, the codes every plane must reach (before the left shift)
ROWS = {
    "I1v": dict(matrix=BT709, ind=12, full=0, outd=16, layout="plane", entry="batch", share="709_video", codes=(256, 3760)),
    "I1f": dict(matrix=BT709, ind=12, full=1, outd=12, layout="plane", entry="batch", share="709_full", codes=(0, 4095)),
    "I1s": dict(matrix=BT709, ind=12, full=0, outd=16, layout="plane", entry="single", share=None, codes=None, frames=(4, 11)),
    "I2v": dict(matrix=BT709, ind=12, full=0, outd=16, layout="blocks", entry="batch", share="709_video", codes=(256, 3760)),
    "I2f": dict(matrix=BT709, ind=12, full=1, outd=12, layout="blocks", entry="batch", share="709_full", codes=(0, 4095)),
    "I3v": dict(matrix=YDZDX, ind=12, full=0, outd=16, layout="plane", entry="batch", share="ydzdx_video", codes=(256, 3760), same_as=BT2020NC),
    "I3f": dict(matrix=YDZDX, ind=12, full=1, outd=12, layout="plane", entry="batch", share="ydzdx_full", codes=(0, 4095), same_as=BT2020NC),
    "I4a": dict(matrix=BT709, ind=14, full=1, outd=16, layout="plane", entry="batch", share="709_14_full", codes=(0, 4095)),
    "I4b": dict(matrix=BT709, ind=16, full=1, outd=16, layout="plane", entry="batch", share="709_16_full", codes=(0, 4095)),
    "I5": dict(matrix=YDZDX, ind=16, full=0, outd=10, layout="plane", entry="batch", share=None, codes=None, scale=16),
}
VARIANT = {("plane", "batch"): ("k_inverse_batch", "k_inverse_batch"), ("plane", "single"): ("k_inverse", "k_inverse"),
           ("blocks", "batch"): ("k_inverse420_batch", "k_inverse420_batch<REPLICATE>"),
           ("blocks", "single"): ("k_inverse420", "k_inverse420<REPLICATE>")}


def row_sweep(row_id: str) -> PlaneSweep:
    row = ROWS[row_id]
    if row_id == "I5":
        return PlaneSweep(i5_frames(), "plane", 16)
    frames = plane_frames()
    if "frames" in row:
        frames = [frames[k] for k in row["frames"]]
    return PlaneSweep(frames, row["layout"])


def oracle_frame(oracle, row, sweep: PlaneSweep, planes, matrix=None):
    """The oracle's G, B, R for one frame of a row: up444 (replication) of both chroma planes first for the blocks layout."""
    w, hh = sweep.width, sweep.height
    if sweep.c420:
        maxcv = (1 << row["ind"]) - 1
        planes = [planes[0]] + [oracle.up444(p, w, hh, 0, 0, maxcv).reshape(-1) for p in planes[1:]]
    return oracle.matrix_inverse(w, hh, row["ind"], row["full"], row["matrix"] if matrix is None else matrix, row["outd"], planes)


# ---- guard triples (tests/golden/inverse_guard_triples.npz) ----------------------------------------------------------
GUARD_CATEGORIES = ("inside", "edge", "tiny", "ceil", "shows")  # make_inverse_guard_triples.py says what each is
GUARD_CONFIGS = {"12v16": (12, 0, 16), "12f12": (12, 1, 12), "14f16": (14, 1, 16), "16f16": (16, 1, 16)}  # in depth, full, out depth


def padded(triples: np.ndarray, width: int, multiple: int = 1) -> np.ndarray:
    """The list padded with its last triple to a whole number of rows of `width` (and rows to a multiple)."""
    rows = -(-len(triples) // width)
    rows += (-rows) % multiple
    return np.concatenate((triples, np.repeat(triples[-1:], rows * width - len(triples), axis=0)))


def g1_cut(triples: np.ndarray, width: int = 67) -> np.ndarray:
    """The longest head of the list that fills whole rows of `width` with npix % 4 == 3."""
    rows = len(triples) // width
    while (rows * width) % 4 != 3:
        rows -= 1
    assert rows > 0
    return triples[:rows * width]


def blocks_420(triples: np.ndarray, w2: int = 64):
    """Each triple over a 2 x 2 block: (luma (2 h2, 2 w2), Cb (h2, w2), Cr (h2, w2)) flat, the padded list, width, height."""
    t = padded(triples, w2)
    h2 = len(t) // w2
    luma = np.repeat(np.repeat(t[:, 0].reshape(h2, w2), 2, axis=0), 2, axis=1)
    return [np.ascontiguousarray(luma).reshape(-1), np.ascontiguousarray(t[:, 1]), np.ascontiguousarray(t[:, 2])], t, 2 * w2, 2 * h2
