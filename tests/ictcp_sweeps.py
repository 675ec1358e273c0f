"""ICtCp sweeps: every source value through k_ictcp (h2y_ictcp_batch, F32 out of place, and F16 for the halves), every output sample
against ictcp_ref.apply, bit for bit.  Lists, frames, the restatement over them and the conditions, in plain numpy;
tests/test_ictcp_sweeps.py checks this file without a GPU, tests/test_ictcp_value_sweeps.py runs the sweeps.

I0  grey: every binary32 of [2^-27, 1), one binade per case, as 256 x 256 frames of 2^16 consecutive patterns, all three plane
    pointers on one plane; the scale alternates between (16, 0) and (16, 1) by binade.  One more case, the specials: +0, every
    1021st pattern below 2^-27 (denormals included), 1.0 and the 64 patterns above it (the clamp), at (16, 1).
I1  one channel lit, G, B and R in turn, the other two planes +0: every 8th pattern of [2^-27, 1) with a seeded offset per group of
    eight, and the specials.
I2  grey, every half as one 256 x 256 F16 frame per scale of SCALES."""
from __future__ import annotations

import numpy as np

import ictcp_ref as ir
import sweep_values as sv

W = H = 256
PER = W * H
LO_E = -27
LO, ONE = sv.f32_bits(2.0 ** LO_E), sv.f32_bits(1.0)
BINADES = list(range(LO_E, 0))  # e: the floats of [2^e, 2^(e + 1))
FRAMES_PER_BINADE = (1 << 23) // PER
SCALES = [(8, 0), (8, 1), (10, 0), (10, 1), (12, 0), (12, 1), (16, 0), (16, 1)]  # test_ictcp.py's: (dst_bit_depth, dst_full_range)
SPECIALS_SCALE = (16, 1)
CHANNELS = ("G", "B", "R")
I1_SCALE = {"G": (16, 0), "B": (16, 1), "R": (16, 0)}
I1_STEP = 8
VARIANT = {"F32": "k_ictcp<F32>", "F16": "k_ictcp<F16>"}


def scale_of(e: int):
    return 16, (e - LO_E) % 2


def binade_starts(e: int) -> np.ndarray:
    """the first pattern of each of the 128 frames of [2^e, 2^(e + 1))"""
    return (sv.f32_bits(2.0 ** e) + PER * np.arange(FRAMES_PER_BINADE, dtype=np.int64)).astype(np.uint32)


def frame_bits(starts: np.ndarray) -> np.ndarray:
    """(frames, 2^16) consecutive bit patterns"""
    return starts.astype(np.uint32)[:, None] + np.arange(PER, dtype=np.uint32)[None, :]


def specials() -> np.ndarray:
    """(frames, 2^16) patterns: +0 and every 1021st pattern below 2^-27, 1.0, the 64 patterns above it; the last frame is filled up
    with the last pattern"""
    v = np.concatenate([sv.float_range(0, LO, 1021), np.arange(ONE, ONE + 65, dtype=np.uint32)])
    v = np.concatenate([v, np.full(-v.size % PER, v[-1], np.uint32)])
    return v.reshape(-1, PER)


def lit_bits(channel: str) -> np.ndarray:
    """I1's (frames, 2^16) patterns of the lit plane: of every eight consecutive patterns of [2^-27, 1) one, drawn by a seeded
    generator; then the specials"""
    rng = np.random.default_rng(2100 + CHANNELS.index(channel))
    n = (ONE - LO) // I1_STEP
    v = (LO + I1_STEP * np.arange(n, dtype=np.int64) + rng.integers(0, I1_STEP, n)).astype(np.uint32)
    assert v.size % PER == 0
    return np.concatenate([v.reshape(-1, PER), specials()])


def planes_of(bits: np.ndarray, which: str):
    """[G, B, R] float32 of flat patterns: grey, or one channel lit and the others +0"""
    v = bits.reshape(-1).view(np.float32)
    z = np.zeros_like(v)
    return [v if which in ("grey", c) else z for c in CHANNELS]


def want(oracle, bits: np.ndarray, which: str, scale):
    """ictcp_ref.apply of the frames: (3, frames, 2^16) float32"""
    return np.stack([p.reshape(bits.shape) for p in ir.apply(oracle, planes_of(bits, which), *scale)])


def lms_reach(bits: np.ndarray, which: str):
    """per l, m, s of the restatement: does it hold 0, a value of (0, 2^-24), a value above 2^-6"""
    lms = ir.der.lms(ir.clean(planes_of(bits, which)))
    return [((v == 0).any(), ((v > 0) & (v < 2.0 ** -24)).any(), (v > 2.0 ** -6).any()) for v in lms]


def i_codes(want_planes: np.ndarray) -> np.ndarray:
    """the distinct integer I codes of restated frames"""
    return np.unique(np.trunc(want_planes[0]).astype(np.uint16))


def name_samples(bits, got, want_planes, limit: int = 8) -> str:
    """Empty when the device's samples are the restatement's bit for bit; else the count and the first differing samples.
    got, want_planes: (3, frames, 2^16) float32; bits: (frames, 2^16) patterns of the swept plane."""
    g, w = got.view(np.uint32), want_planes.view(np.uint32)
    bad = np.argwhere(g != w)
    if not bad.size:
        return ""
    hexw = 8 if bits.dtype == np.uint32 else 4
    lines = [f"plane {'I Ct Cp'.split()[c]} frame {f} sample {i} input 0x{int(bits[f, i]):0{hexw}x}: got 0x{int(g[c, f, i]):08x} ({got[c, f, i]!r}), "
             f"restated 0x{int(w[c, f, i]):08x} ({want_planes[c, f, i]!r})" for c, f, i in bad[:limit]]
    return f"{len(bad)} samples differ; first:\n  " + "\n  ".join(lines)


# Distinct I codes of the I0 cases at (16, 1), as the restatement gives them: a case's count may fall 2 % short.  PQ is steep near
# black and flat near the peak on this scale of exponents: a binade of light spans 70 codes of 16 bits at 2^-26 and 4 946 at 2^-4.
I_CODES = {"specials": 94, -26: 70, -24: 149, -22: 298, -20: 559, -18: 966, -16: 1534, -14: 2238, -12: 3007, -10: 3746, -8: 4355,
           -6: 4765, -4: 4946, -2: 4906}
