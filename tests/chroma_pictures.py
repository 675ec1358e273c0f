"""Saturated, high-contrast pictures for the chroma resamplers, and Subsample444to420_FIR restated in integers.

The suite's other pictures are iid uniform linear light (after PQ a narrow chroma band round mid-grey) or consecutive floats
(chroma over its whole range, but smooth: the FIR of a flat area is the identity).  Neither brings a sum of the 4:4:4 -> 4:2:0
FIR, or a sample of the 4:2:0 -> 4:4:4 one, near a clamp.  The pictures here hold only corners of the RGB cube, changing every
one to three pixels: the 7-tap and 12-tap sums leave [0, maxCV] and the output range in 3 - 17 % of the samples of either
stage (tests/test_chroma_pictures.py holds the census).

A plain module: numpy only, nothing of the library or the oracle is called.  Every picture is a map of corner indices
(bit 0 = G, bit 1 = B, bit 2 = R: the planes' order), from which come the float planes, their halves, their 16-bit codes and
the two-level chroma planes of the inverse direction."""
import numpy as np

BLUE, CYAN, RED, YELLOW = 2, 3, 4, 5  # corner indices: bit 0 = G, bit 1 = B, bit 2 = R

# k_fir_fused's strips are 240 columns wide with two halo lanes (eight columns) either side; the picture-edge substitutions act
# on the first and the last four columns; a 260-row frame is cut into two segments at chroma row 65 (rows 130).
STEP_COLUMNS = (4, 8, 236, 240, 244, 476, 480, 484)  # and w - 4
STEP_ROWS = (2, 6, 124, 130, 136)  # and h - 2

PICTURES = ("corners1", "corners2", "corners3", "checker3_by", "checker3_rc", "cols3_by", "rows6_by", "rows4_rc", "steps_by", "steps_rc")
_SEEDS = {"corners1": 101, "corners2": 102, "corners3": 103}


def _parity(edges, n):
    """0 / 1 along an axis of n samples, changing at every edge inside (0, n)"""
    out = np.zeros(n, np.int64)
    for e in sorted({int(e) for e in edges if 0 < e < n}):
        out[e:] ^= 1
    return out


def corner_map(name, w, h):
    """The picture `name` at w x h as an (h, w) array of corner indices 0 .. 7."""
    yy, xx = np.mgrid[0:h, 0:w]
    if name.startswith("corners"):
        b = int(name[len("corners"):])
        rng = np.random.default_rng(_SEEDS[name] + 1000 * w + h)
        cells = rng.integers(0, 8, (-(-h // b), -(-w // b)))
        # black, white and one more pair of opposite corners in the first cells: every plane holds 0.0 and 1.0 at any size
        cells.flat[:min(4, cells.size)] = [0, 7, BLUE, YELLOW][:min(4, cells.size)]
        return np.repeat(np.repeat(cells, b, 0), b, 1)[:h, :w]
    kind, _, colours = name.partition("_")
    a, b = {"by": (BLUE, YELLOW), "rc": (RED, CYAN)}[colours]
    if kind == "checker3":
        m = ((xx // 3) + (yy // 3)) & 1
    elif kind == "cols3":
        m = (xx // 3) & 1
    elif kind == "rows6":
        m = (yy // 6) & 1
    elif kind == "rows4":
        m = (yy // 4) & 1
    elif kind == "steps":  # a field of b with bars of a; every listed column and row is an edge over the whole frame
        m = _parity(STEP_COLUMNS + (w - 4,), w)[None, :] ^ _parity(STEP_ROWS + (h - 2,), h)[:, None]
    else:
        raise KeyError(name)
    return np.where(m == 1, a, b)


def planes_f32(name, w, h):
    """G, B, R float32 planes (flat) holding 0.0 and 1.0 only, both in every plane (a size too small for the picture to show both
    of its colours is refused: rows6 needs seven rows)."""
    c = corner_map(name, w, h).reshape(-1)
    out = [((c >> k) & 1).astype(np.float32) for k in range(3)]
    assert all(p.min() == 0.0 and p.max() == 1.0 for p in out), name
    return out


def planes_f16(name, w, h):
    """The same picture as halves (their bits, as the C-ABI takes them): 0x0000 and 0x3C00, both exact."""
    return [p.astype(np.float16).view(np.uint16) for p in planes_f32(name, w, h)]


def planes_u16(name, w, h, depth=16):
    """The same picture as integer codes 0 and 2^depth - 1."""
    return [(p.astype(np.uint32) * ((1 << depth) - 1)).astype(np.uint16) for p in planes_f32(name, w, h)]


# ---- the inverse direction ------------------------------------------------------------------------------------------------
def inside_levels(min_cv, max_cv):
    """Two levels strictly inside [min_cv, max_cv], a sixteenth of the range from either end: (maxCV / 16, 15 maxCV / 16) for
    the full clamp.  An upsampled sample equal to min_cv or max_cv can then only come from a clamp."""
    span = max_cv - min_cv
    return min_cv + span // 16, min_cv + (15 * span) // 16


# The 4:2:0 -> 4:4:4 FIR on the two-level planes at the inside levels, 264 x 40, all pictures and both planes together, measured
# with the oracle: 9.43 % of the upsampled samples equal min_cv and 9.54 % max_cv, the same to 0.01 at 10, 12 and 16 bits and
# for the full and the video clamp (levels a sixteenth of the clamp's range inside it).  Required: the figure less a fifth.
INVERSE_AT_AN_END = 0.075


def chroma_planes(name, cw, ch, low, high):
    """Two u16 chroma planes (ch, cw) of the picture's pattern: Cb / Dz follows the corner's B bit, Cr / Dx its R bit."""
    c = corner_map(name, cw, ch)
    return [np.where((c >> k) & 1, high, low).astype(np.uint16) for k in (1, 2)]


def luma_plane(w, h, depth, seed=7):
    return np.random.default_rng(seed + 100 * depth).integers(0, 1 << depth, w * h).astype(np.uint16)


# ---- Subsample444to420_FIR in integers --------------------------------------------------------------------------------------
H_TAPS = ((-5, 21), (-3, -52), (-1, 159), (0, 256), (1, 159), (3, -52), (5, 21))
V_TAPS = (5, 11, -21, -37, 70, 228, 228, 70, -37, -21, 11, 5)  # rows 2j - 5 .. 2j + 6


def fir_sums(src, depth):
    """The two stages of Subsample444to420_FIR on an (h, w) plane of codes below 2^depth, in numpy int64:
    (hraw, vraw) = floor((S + 256) / 512) of the horizontal 7-tap sums at the even columns, (h, w/2), and of the vertical 12-tap
    sums over the horizontal results clamped to [0, maxCV], (h/2, w/2); neither is clamped.  Edges replicate by index clamping.

    Exact for depths up to 14: every coefficient is k/512 and every sample an integer below 2^14, so every product, partial
    sum and the final + 0.5 of the reference's binary32 expression is a multiple of 2^-9 below 2^15 in magnitude -- exact in
    binary32 -- and clamp-then-truncate of that float is the clamp of this floor (the argument of h2y_math.h's fir_h_int /
    fir_v_int).  At 15 and 16 bits the float sums round, and in which order they are added decides bytes: refused."""
    if not 1 <= depth <= 14:
        raise ValueError(f"fir_sums is the reference's arithmetic only up to 14 bits, not at {depth}")
    s = np.asarray(src).astype(np.int64)
    assert s.ndim == 2 and s.min() >= 0 and s.max() < (1 << depth)
    hh, w = s.shape
    cols = np.arange(0, w - 1, 2)
    hs = np.zeros((hh, cols.size), np.int64)
    for off, k in H_TAPS:
        hs += k * s[:, np.clip(cols + off, 0, w - 1)]
    hraw = (hs + 256) >> 9
    mid = np.clip(hraw, 0, (1 << depth) - 1)
    rows = np.arange(0, hh - 1, 2)
    vs = np.zeros((rows.size, cols.size), np.int64)
    for t, k in enumerate(V_TAPS):
        vs += k * mid[np.clip(rows - 5 + t, 0, hh - 1), :]
    return hraw, (vs + 256) >> 9


EVENTS = ("h<0", "h>max", "v<lo", "v>hi")


def census(src, depth, lo, hi):
    """Shares of the samples of either stage whose sum a clamp acts on: horizontal sums below 0 and above maxCV, vertical
    sums below lo and above hi (the plane's output range), in EVENTS' order."""
    hraw, vraw = fir_sums(src, depth)
    return (float((hraw < 0).mean()), float((hraw > (1 << depth) - 1).mean()), float((vraw < lo).mean()), float((vraw > hi).mean()))


def chroma_range(depth, full):
    """write_yuv's range of a chroma plane"""
    return (0, (1 << depth) - 1) if full else (16 << (depth - 8), 240 << (depth - 8))


# ---- configurations ---------------------------------------------------------------------------------------------------------
# descriptor keywords (numbers only: 1 = BT.709, 9 = BT.2020nc, 11 = Y'DzDx) of the FIR configurations at which the integer
# restatement is the reference's arithmetic; the GPU tests (tests/test_chroma_extremes.py) run these and the 16-bit ones
FIR_INT_CONFIGS = {
    "2020_12b_video": dict(dst_matrix=9, dst_depth=12, full_range=0),
    "2020_12b_full": dict(dst_matrix=9, dst_depth=12, full_range=1),
    "709_10b_video": dict(dst_matrix=1, dst_depth=10, full_range=0),
    "709_12b_video": dict(dst_matrix=1, dst_depth=12, full_range=0),
    "ydzdx_14b_video": dict(dst_matrix=11, dst_depth=14, full_range=0),
}
FRAME = (496, 260)  # three strips of 240, 240 and 16 columns; 130 chroma rows: two segments; 496 = 7 x 64 + 48, 260 = 8 x 32 + 4
